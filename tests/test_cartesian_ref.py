"""The float64 Cartesian controller reference (tests/cartesian_ref.py) against Chain.fk itself, its closed-loop
convergence for the three robots, and the ABI declaration of ha_cartesian_targets. No GPU.

Bounds:
* Jacobian against central differences of the task error: with the goal at the current tool pose the error is 0 and
  de/dq_d = -J[:, d] exactly; a central difference with step h = 1e-5 has a truncation error of h^2 |e'''| / 6, about
  2e-11 for metre-sized arms, and a rounding error of eps / h = 2e-11: 1e-8 leaves two orders.
* arms (lambda 0.05, max_step 0.2, goals 5 cm + 0.2 rad away): the loop was prototyped at < 5e-8 m and rad after 10
  iterations, held here with a factor 10 (5e-7); after 20 iterations it sits on float64 rounding of a metre-sized FK
  with about 15 chained products (1e-16..1e-15), held at 1e-12.
* thumb tip (position only, 1 cm, 4 DOFs): the tool Jacobian's smallest singular value at the mid-range pose is 0.017,
  so a goal along that direction contracts slowly; over 40 random goals the lambda 0.01 loop was between 0 and 5e-6 m
  after 30 iterations (most at the float64 floor). Held at 1e-5 m, a decade under the 1e-4 m the device loop is held
  to. Lambda 0.05 leaves more than 1e-4 m after 40 iterations, which is why the finger cases use 0.01.
* the all-zero pose is singular for both arms (the tool Jacobian's sixth singular value is below 1e-9 of its first,
  against more than 0.05 at every case pose; from there the loop can stall centimetres off), so no case starts there.
* posture term (AllegroKuka, null_gain 0.5): the damped projector leaks lambda^2 A^-1 J z into task space, and the
  loop settles off the goal and stays (two consecutive iterates within 1e-9): how far depends on the goal, 0.08 to
  2 mm here; every env more than 1e-6 m (the loop without the term is at 1e-16), the worst more than 1 mm, none 1 cm."""
import numpy as np
import pytest

from handarm_hip import _lib
from handarm_hip import model as HM
from tests import cartesian_ref as CR
from tests.kinematics import Chain
from tests.test_independent_dynamics import ROBOTS

ASSET = dict(ROBOTS)


def _setup(task, n=4, seed=None):
    ch = Chain(HM.load_scene(ASSET[task]))
    p, _ = HM.build_params(task=task)
    rest = np.array(list(p.reset_pose)[:ch.D])
    return ch, rest, CR.robot_case(ch, task, rest, n, seed=100 + task if seed is None else seed)


def _errors(ch, c, q, e):
    err = CR.task_error(ch, q, c["goal"][e].astype(np.float64), c["link"], offset=CR.OFFSET,
                        position_only=c["position_only"])
    return np.abs(err[0:3]).max(), np.abs(err[3:6]).max()


@pytest.mark.parametrize("task,asset", ROBOTS)
def test_error_vector_matches_central_differences_of_fk(task, asset):
    ch, _, c = _setup(task)
    h = 1e-5
    for e in range(len(c["q"])):
        q = c["q"][e].astype(np.float64)
        pt, Rl = CR.tool_pose(ch, q, c["link"], CR.OFFSET)
        goal = np.concatenate([pt, CR.matrix_quat(Rl)])
        assert np.abs(CR.task_error(ch, q, goal, c["link"], offset=CR.OFFSET)).max() < 1e-12
        J = CR.tool_jacobian(ch, q, c["link"], offset=CR.OFFSET)
        for d in range(ch.D):
            dq = np.zeros(ch.D)
            dq[d] = h
            fd = (CR.task_error(ch, q + dq, goal, c["link"], offset=CR.OFFSET) -
                  CR.task_error(ch, q - dq, goal, c["link"], offset=CR.OFFSET)) / (2 * h)
            assert np.abs(fd + J[:, d]).max() < 1e-8, f"task {task} env {e} DOF {d}"
            if d not in c["dofs"]:
                assert not J[:, d].any() and np.abs(fd).max() < 1e-10
    # a 0.2 rad goal rotation comes back as a rotation vector of that length, a delta goal as itself
    q = c["q"][0].astype(np.float64)
    e6 = CR.task_error(ch, q, c["goal"][0].astype(np.float64), c["link"], offset=CR.OFFSET)
    assert abs(np.linalg.norm(e6[3:6]) - 0.2) < 1e-6 and abs(np.linalg.norm(e6[0:3]) - c["dist"]) < 1e-6
    assert np.array_equal(CR.task_error(ch, q, np.arange(6.0), c["link"], mode=CR.DELTA), np.arange(6.0))


@pytest.mark.parametrize("task", [HM.TASK_UR5SIH, HM.TASK_ALLEGRO_KUKA])
def test_arm_loop_converges(task):
    ch, _, c = _setup(task)
    worst10 = worst20 = 0.0
    for e in range(len(c["q"])):
        hist = CR.closed_loop(ch, c["q"][e], c["goal"][e], c["link"], 20, dofs=c["dofs"], **c["gains"])
        worst10 = max(worst10, *_errors(ch, c, hist[9], e))
        worst20 = max(worst20, *_errors(ch, c, hist[19], e))
        q64 = c["q"][e].astype(np.float64)
        J = CR.tool_jacobian(ch, q64, c["link"], offset=CR.OFFSET)
        assert np.linalg.cond(J @ J.T + 0.05 ** 2 * np.eye(6)) <= 370
        # only the selected DOFs ever move
        rest = [d for d in range(ch.D) if d not in c["dofs"]]
        assert np.array_equal(hist[-1][rest], q64[rest])
    print(f"task {task}: error after 10 iterations {worst10:.2e}, after 20 {worst20:.2e}")
    assert worst10 < 5e-7 and worst20 < 1e-12


def test_thumb_tip_needs_the_smaller_damping():
    task = HM.TASK_ALLEGRO_HAND
    ch, _, c = _setup(task)
    assert c["position_only"] and c["damping"] == 0.01
    left = []
    for e in range(len(c["q"])):
        hist = CR.closed_loop(ch, c["q"][e], c["goal"][e], c["link"], 30, dofs=c["dofs"], **c["gains"])
        pos, rot = _errors(ch, c, hist[-1], e)
        print(f"env {e}: {pos:.2e} m left with lambda 0.01")
        assert pos < 1e-5 and rot == 0.0, f"env {e}: {pos:.2e} m left with lambda 0.01"
        slow = CR.closed_loop(ch, c["q"][e], c["goal"][e], c["link"], 40, dofs=c["dofs"],
                              **dict(c["gains"], damping=0.05))
        left.append(_errors(ch, c, slow[-1], e)[0])
    print("lambda 0.05 leaves after 40 iterations:", " ".join(f"{x:.1e}" for x in left))
    assert max(left) > 1e-4


@pytest.mark.parametrize("task", [HM.TASK_UR5SIH, HM.TASK_ALLEGRO_KUKA])
def test_arms_are_singular_at_the_zero_pose(task):
    ch, _, c = _setup(task)
    s0 = np.linalg.svd(CR.tool_jacobian(ch, np.zeros(ch.D), c["link"], offset=CR.OFFSET), compute_uv=False)
    assert s0[5] < 1e-9 * s0[0], "the zero pose is expected to be singular"
    for e in range(len(c["q"])):
        J = CR.tool_jacobian(ch, c["q"][e].astype(np.float64), c["link"], offset=CR.OFFSET)
        assert np.linalg.svd(J, compute_uv=False)[5] > 0.05


def test_posture_term_settles_off_the_goal():
    task = HM.TASK_ALLEGRO_KUKA
    ch, rest, c = _setup(task)
    worst = 0.0
    for e in range(len(c["q"])):
        hist = CR.closed_loop(ch, c["q"][e], c["goal"][e], c["link"], 60, dofs=c["dofs"], q_rest=rest, null_gain=0.5,
                              **c["gains"])
        pos, rot = _errors(ch, c, hist[-1], e)
        print(f"env {e}: settles {pos:.2e} m, {rot:.2e} rad from the goal")
        assert np.abs(hist[-1] - hist[-2]).max() < 1e-9
        assert 1e-6 < pos < 1e-2 and rot < 1e-2
        worst = max(worst, pos)
    assert worst > 1e-3


def test_limits_clamp_and_step_limit():
    ch, _, c = _setup(HM.TASK_UR5SIH)
    lo, up = CR.limits(ch)
    q = c["q"][0].astype(np.float64)
    far = np.array([0, 0, 5.0, 0, 0, 0])
    t, _ = CR.cartesian_step(ch, q, far, c["link"], mode=CR.DELTA, max_step=0.2, lower=lo, upper=up)
    assert abs(np.abs(t - q).max() - 0.2) < 1e-12
    t2, _ = CR.cartesian_step(ch, q, far, c["link"], mode=CR.DELTA)
    d = t2 - q
    assert np.abs(d).max() > 0.2 and np.allclose(d * (0.2 / np.abs(d).max()), t - q, atol=1e-12)
    t3, _ = CR.cartesian_step(ch, q, far, c["link"], mode=CR.DELTA, lower=q - 0.01, upper=q + 0.01)
    assert np.abs(t3 - q).max() <= 0.01 + 1e-15


def test_header_declares_and_lib_binds_cartesian_targets():
    assert "ha_cartesian_targets" in _lib.header_symbols()
    args, res = _lib.SIGNATURES["ha_cartesian_targets"]
    assert args[1]._type_ is _lib.HaCartesian
    names = [f[0] for f in _lib.HaCartesian._fields_]
    assert names == ["goal", "targets", "err_out", "q_rest", "env_ids", "n_envs", "link", "mode", "position_only",
                     "dof_mask", "offset", "damping", "max_step", "null_gain"]
    import ctypes as C
    assert C.sizeof(_lib.HaCartesian) == 5 * 8 + 5 * 4 + 6 * 4 + 4      # 5 pointers, 5 ints, 6 floats, tail padding
    with open(_lib.HEADER) as f:
        txt = f.read()
    assert "#define HA_ABI_VERSION 16" in txt and "#define HA_CART_POSE 0" in txt and "#define HA_CART_DELTA 1" in txt
