"""The float64 whole-hand Cartesian reference (tests/cartesian_multi_ref.py) against the single-link reference, its
algebraic properties, the precision emulations that make the GPU bounds of tests/test_gpu_cartesian_multi.py
meaningful, and the ABI declaration of ha_cartesian_multi_targets. No GPU.

Bounds:
* identities between float64 evaluations of the same step (T = 1 against cartesian_step, weights and damping doubled
  together, a position-only task against a full task without its angular rows, the posture term's leak): both sides are
  a handful of float64 operations on the same J and e, steps below 1 rad, condition of A at most a few thousand: 1e-12.
* precision emulations, for every one-step case of the GPU test, J and e rounded to float32:
  (a) the rest of the step in float64 stays within 1e-6 rad of the float64 step, one tenth of the GPU bound. Measured
      here: 1.7e-7 rad at most over all cases (the weighted inconsistent arm cases 1.3e-7 and 1.7e-7, the AllegroHand
      at lambda 0.01 1.5e-8).
  (b) the rest of the step in float32 (numpy's float32 Cholesky, float32 substitutions and products) exceeds 2e-5 rad in
      the weighted inconsistent arm cases: 3.9e-5 rad (Ur5Sih, 21 rows on 17 DOFs) and 6.4e-5 rad (AllegroKuka) in the
      worst of each robot's six envs, so the 1e-5 GPU bound tells the two designs apart. (The single env of the N = 1
      cases gives 1.7e-5 and 2.7e-5.)
* reference closed loop, 40 iterations on consistent goals: the AllegroHand (lambda 0.01) ends below 1e-8 m; the arms'
  stacked loop converges slowly (1e-4 to 5e-4 m left), so it is held to cutting the largest position error 10x."""
import ctypes as C

import numpy as np
import pytest

from handarm_hip import _lib
from handarm_hip import model as HM
from tests import cartesian_multi_ref as MR
from tests import cartesian_ref as CR
from tests.kinematics import Chain
from tests.test_independent_dynamics import ROBOTS

ASSET = dict(ROBOTS)
ARMS = [HM.TASK_UR5SIH, HM.TASK_ALLEGRO_KUKA]
NS = (5, 1)


def case_seed(task, n):
    """The seed of the (robot, N) case the CPU and the GPU tests share."""
    return 500 + 10 * task + n


def _chain(task):
    return Chain(HM.load_scene(ASSET[task]))


@pytest.mark.parametrize("task,asset", ROBOTS)
def test_one_task_is_the_single_link_step(task, asset):
    ch = _chain(task)
    c = MR.robot_multi_case(ch, task, 3, case_seed(task, 3))
    lo, up = CR.limits(ch)
    rest = (lo + up) / 2
    for e in range(3):
        q = c["q"][e].astype(np.float64)
        for t, tk in enumerate(c["tasks"]):
            for extra in (dict(), dict(max_step=0.05), dict(q_rest=rest, null_gain=0.5)):
                kw = dict(damping=c["damping"], lower=lo, upper=up, **extra)
                a, ea = MR.multi_step(ch, q, c["inconsistent"][e][t:t + 1], [tk], **kw)
                b, eb = CR.cartesian_step(ch, q, c["inconsistent"][e][t], tk["link"], offset=tk["offset"],
                                          position_only=tk["position_only"], **kw)
                assert np.abs(a - b).max() <= 1e-12 and np.abs(ea[0] - eb).max() <= 1e-12
                assert np.abs(a - q).max() > 1e-3


@pytest.mark.parametrize("task,asset", ROBOTS)
def test_weights_are_row_scalings(task, asset):
    ch = _chain(task)
    c = MR.robot_multi_case(ch, task, 3, case_seed(task, 3))
    tasks = MR.weighted(c["tasks"], 1.0, 3.0)
    twice = [dict(t, weight=2.0 * t["weight"]) for t in tasks]
    for e in range(3):
        q = c["q"][e].astype(np.float64)
        a, ea = MR.multi_step(ch, q, c["inconsistent"][e], tasks, damping=0.05)
        b, eb = MR.multi_step(ch, q, c["inconsistent"][e], twice, damping=0.10)
        assert np.abs(a - b).max() <= 1e-12 and np.array_equal(ea, eb), "e is the unweighted error"
        # the weights matter: inconsistent goals weighted differently give another step
        u, _ = MR.multi_step(ch, q, c["inconsistent"][e], c["tasks"], damping=0.05)
        assert np.abs(a - u).max() > 1e-4


@pytest.mark.parametrize("task,asset", ROBOTS)
def test_position_only_task_is_a_full_task_without_its_angular_rows(task, asset):
    ch = _chain(task)
    c = MR.robot_multi_case(ch, task, 3, case_seed(task, 3))
    full = [dict(t, position_only=False) for t in c["tasks"]][:4]      # four full tasks: 24 rows
    keep = np.concatenate([np.arange(6 * t, 6 * t + (3 if tk["position_only"] else 6))
                           for t, tk in enumerate(c["tasks"][:4])])
    for e in range(3):
        q = c["q"][e].astype(np.float64)
        g = c["inconsistent"][e][:4].astype(np.float64)
        J, err, w, _, U = MR.stacked(ch, q, g, full)
        J, err = J[keep], err[keep]
        dq = J.T @ np.linalg.solve(J @ J.T + 0.05 ** 2 * np.eye(len(keep)), err)
        t, e6 = MR.multi_step(ch, q, g, c["tasks"][:4], damping=0.05)
        assert np.abs((t - q) - dq).max() <= 1e-12
        for k, tk in enumerate(c["tasks"][:4]):
            assert (not e6[k, 3:6].any()) == tk["position_only"]
        rest = [d for d in range(ch.D) if d not in U]
        assert np.array_equal(t[rest], q[rest])


def test_step_limit_limits_and_posture_term():
    task = HM.TASK_ALLEGRO_KUKA
    ch = _chain(task)
    c = MR.robot_multi_case(ch, task, 2, case_seed(task, 2))
    lo, up = CR.limits(ch)
    tasks, T = c["tasks"], len(c["tasks"])
    q = c["q"][0].astype(np.float64)
    far = np.tile(np.array([0, 0, 5.0, 0, 0, 0]), (T, 1))
    t, _ = MR.multi_step(ch, q, far, tasks, mode=MR.DELTA, max_step=0.2, lower=lo - 10, upper=up + 10)
    assert abs(np.abs(t - q).max() - 0.2) < 1e-12
    t2, _ = MR.multi_step(ch, q, far, tasks, mode=MR.DELTA)
    d = t2 - q
    assert np.abs(d).max() > 0.2 and np.allclose(d * (0.2 / np.abs(d).max()), t - q, atol=1e-12)
    t3, _ = MR.multi_step(ch, q, far, tasks, mode=MR.DELTA, lower=q - 0.01, upper=q + 0.01)
    assert np.abs(t3 - q).max() <= 0.01 + 1e-15
    # posture term: what the damped projector leaks into task space is lambda^2 A^-1 Jw z
    p, _ = HM.build_params(task=task)
    rest = np.array(list(p.reset_pose)[:ch.D])
    g = c["consistent"][0]
    with_, _ = MR.multi_step(ch, q, g, tasks, q_rest=rest, null_gain=0.5)
    without, _ = MR.multi_step(ch, q, g, tasks)
    J, _, w, _, U = MR.stacked(ch, q, g.astype(np.float64), tasks)
    z = np.zeros(ch.D)
    z[U] = 0.5 * (rest[U] - q[U])
    A = J @ J.T + 0.05 ** 2 * np.eye(len(w))
    assert np.abs(J @ (with_ - without) - 0.05 ** 2 * np.linalg.solve(A, J @ z)).max() <= 1e-12
    assert np.abs(with_ - without).max() > 1e-3


def _emulation_errors(task, n):
    ch = _chain(task)
    c, variants = MR.one_step_variants(ch, task, n, case_seed(task, n))
    out = {}
    for name, var in variants.items():
        kw = {k: x for k, x in MR.variant_kwargs(var).items() if k != "max_step"}
        a = b = 0.0
        for e in range(n):
            q = c["q"][e].astype(np.float64)
            exact = MR.exact_dq(ch, q, var["goals"][e], **kw)
            a = max(a, np.abs(MR.emulated_dq(ch, q, var["goals"][e], rest="float64", **kw) - exact).max())
            b = max(b, np.abs(MR.emulated_dq(ch, q, var["goals"][e], rest="float32", **kw) - exact).max())
        out[name] = (a, b)
    return out


@pytest.mark.parametrize("task,asset", ROBOTS)
def test_precision_emulations(task, asset):
    worst32 = 0.0
    for n in NS:
        for name, (a, b) in _emulation_errors(task, n).items():
            print(f"task {task} N {n} {name}: float32 J and e, rest float64 {a:.2e} rad, rest float32 {b:.2e} rad")
            assert a <= 1e-6, f"{name}, N {n}: the float64 solve on float32 rows is {a:.2e} rad off"
            if name == "weighted_inconsistent":
                worst32 = max(worst32, b)
    if task in ARMS:
        assert worst32 > 2e-5, f"a float32-only solve is only {worst32:.2e} rad off: the GPU bound would not tell"


@pytest.mark.parametrize("task,asset", ROBOTS)
def test_one_step_cases_move_and_have_the_stated_rows(task, asset):
    ch = _chain(task)
    lo, up = CR.limits(ch)
    rows = {HM.TASK_UR5SIH: 21, HM.TASK_ALLEGRO_KUKA: 18, HM.TASK_ALLEGRO_HAND: 12}[task]
    for n in NS:
        c, variants = MR.one_step_variants(ch, task, n, case_seed(task, n))
        assert c["rows"] == rows and c["q"].dtype == np.float32 and c["consistent"].dtype == np.float32
        assert c["consistent"].shape == (n, len(c["tasks"]), 7)
        assert 0 < np.abs(c["inconsistent"] - c["consistent"])[:, :, 0:3].max() <= 0.01 + 1e-6
        assert ("posture" in variants) == (task == HM.TASK_ALLEGRO_KUKA)
        for name, var in variants.items():
            for e in range(n):
                q = c["q"][e].astype(np.float64)
                t, _ = MR.multi_step(ch, q, var["goals"][e], lower=lo, upper=up, **MR.variant_kwargs(var))
                step = np.abs(t - q).max()
                assert step > 1e-3, f"{name} env {e} does not move"
                if name == "step_binding":
                    assert abs(step - 0.02) < 1e-12


@pytest.mark.parametrize("task,asset", ROBOTS)
def test_reference_closed_loop(task, asset):
    ch = _chain(task)
    n = 5
    c, variants = MR.one_step_variants(ch, task, n, case_seed(task, n))
    var = variants["consistent"]
    for e in range(n):
        q0 = c["q"][e].astype(np.float64)
        before = MR.position_residual(ch, q0, var["goals"][e], var["tasks"])
        hist = MR.closed_loop(ch, q0, var["goals"][e], iters=40, **MR.variant_kwargs(var))
        after = MR.position_residual(ch, hist[-1], var["goals"][e], var["tasks"])
        print(f"task {task} env {e}: largest position error {before:.2e} -> {after:.2e} m")
        if task == HM.TASK_ALLEGRO_HAND:
            assert after <= 1e-8
        else:
            assert after * 10.0 <= before


def test_header_declares_and_lib_binds_cartesian_multi_targets():
    assert "ha_cartesian_multi_targets" in _lib.header_symbols()
    args, res = _lib.SIGNATURES["ha_cartesian_multi_targets"]
    assert args[1]._type_ is _lib.HaCartesianMulti and res is C.c_int
    assert [f[0] for f in _lib.HaCartTask._fields_] == ["link", "position_only", "offset", "weight"]
    assert [f[0] for f in _lib.HaCartesianMulti._fields_] == [
        "goal", "targets", "err_out", "q_rest", "env_ids", "n_envs", "n_tasks", "mode", "dof_mask", "damping",
        "max_step", "null_gain", "task"]
    assert C.sizeof(_lib.HaCartTask) == 2 * 4 + 4 * 4
    assert C.sizeof(_lib.HaCartesianMulti) == 5 * 8 + 4 * 4 + 3 * 4 + 6 * 24 + 4     # tail padding to 8
    assert HM.CART_MAX_TASKS == 6 and HM.CART_MAX_ROWS == 24
    with open(_lib.HEADER) as f:
        txt = f.read()
    assert "#define HA_ABI_VERSION 16" in txt
    assert "#define HA_CART_MAX_TASKS 6" in txt and "#define HA_CART_MAX_ROWS  24" in txt
    # ha_cartesian_t stays as it was
    assert C.sizeof(_lib.HaCartesian) == 5 * 8 + 5 * 4 + 6 * 4 + 4
