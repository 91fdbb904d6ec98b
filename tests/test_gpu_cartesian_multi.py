"""The whole-hand Cartesian controller kernel (ha_cartesian_multi_kernel through HandArmSim.cartesian_multi_targets,
WholeHandController and gym_api) against the float64 tests/cartesian_multi_ref.py, for the three robots, N = 5 envs (no
multiple of the kernel's envs per workgroup) and N = 1. Sims as test_gpu_cartesian.py builds them: objects parked,
collisions off.

Cases (cartesian_multi_ref.robot_multi_case / one_step_variants): Ur5Sih flange pose + 5 fingertip positions (21 rows on
17 DOFs), AllegroKuka iiwa7_link_7 pose + 4 fingertip positions (18 rows), AllegroHand 4 fingertip positions (12 rows);
tool offset (0.02, -0.01, 0.05).

Bounds (from the reference's and the formats' precision, not from the kernel's output):
* one step: targets and err_out within 1e-5 of the float64 reference, the project's one-step bound. The CPU emulation of
  the kernel's arithmetic (float32 J and e, float64 from A on; tests/test_cartesian_multi_ref.py) is within 1.7e-7 rad,
  and the emulation of a float32-only solve misses the bound in the weighted inconsistent arm cases (3.9e-5, 6.4e-5).
* kinematic closed loop, 40 iterations on consistent goals: final q within 1e-4 rad of the reference loop; AllegroHand
  fingertip error left < 1e-4 m; arms (the stacked loop converges slowly, the reference itself leaves 1e-4 to 5e-4 m):
  the kernel loop's residual within 1e-5 of the reference loop's.
* closed loop with physics (AllegroKuka, N = 2, 60 steps) against a twin sim driven by the torch composition on
  acquire_jacobian_tensor(links=[...]) with a float64 solve: PHYS_TOL below.
The device reaches (MI355X, the cases below): one step, targets 2.0e-6 rad and err_out 3.4e-7 at most (the float32 FK is
what is left: T = 1 and ha_cartesian_targets are both 1.6e-6 rad at most from the reference); kinematic loop, final q
3.8e-6 rad from the reference loop, AllegroHand 8.2e-8 m left, the arms' residuals (9.5e-5 to 4.5e-4 m) equal to the
reference loop's to three digits; with physics, the two routes' link positions 2.6e-7 m apart, the farthest goal from
6.5 cm to 2.8 cm on both."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from handarm_hip import _lib
from handarm_hip import model as HM
from tests import cartesian_multi_ref as MR
from tests import cartesian_ref as CR
from tests.kinematics import Chain
from tests.test_cartesian_multi_ref import case_seed
from tests.test_gpu_cartesian import _make_sim, _qmul
from tests.test_independent_dynamics import ROBOTS

pytestmark = pytest.mark.gpu
ASSET = dict(ROBOTS)
CASES = [(task, n) for task, _ in ROBOTS for n in (5, 1)]
# final link-position gap between the kernel-driven and the torch-driven sim after 60 physics steps. Both routes compute
# the same step in different float orders (float32 rows, float64 solve) under a stable PD loop.
# PHYS_MEASURED is what the MI355X gave; PHYS_TOL is 10x that
PHYS_MEASURED = 2.608e-7
PHYS_TOL = None if PHYS_MEASURED is None else 10.0 * PHYS_MEASURED
NAMES = ["consistent", "weighted_inconsistent", "delta", "step_binding", "subset", "same_link_twice"]
ONE_STEP = [(task, n, name) for task, n in CASES
            for name in NAMES + (["posture"] if task == HM.TASK_ALLEGRO_KUKA else [])]


@functools.lru_cache(maxsize=None)
def _case(task, n):
    """One sim per (robot, N) at the case's joints, the float64 chain and the variants of the one-step test."""
    ch = Chain(HM.load_scene(ASSET[task]))
    c, variants = MR.one_step_variants(ch, task, n, case_seed(task, n))
    sim = _make_sim(task, n, c["q"])
    D = sim.num_dofs
    lo = np.array(list(sim.model.dof_lower)[:D], np.float32)
    up = np.array(list(sim.model.dof_upper)[:D], np.float32)
    return dict(sim=sim, chain=ch, c=c, lo=lo, up=up, variants=variants)


def _ref(cs, var, q, envs=None, lo=None, up=None):
    """Float64 targets (len(envs), D) and errors (len(envs), T, 6) of a variant; goal row k belongs to envs[k]."""
    envs = range(len(q)) if envs is None else envs
    lo = cs["lo"].astype(np.float64) if lo is None else lo
    up = cs["up"].astype(np.float64) if up is None else up
    out = [MR.multi_step(cs["chain"], q[e], var["goals"][k], lower=lo, upper=up, **MR.variant_kwargs(var))
           for k, e in enumerate(envs)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _union(cs, var):
    return sorted(set().union(*[CR.selected_dofs(cs["chain"], t["link"], var.get("dofs")) for t in var["tasks"]]))


def _launch(sim, var, targets, err_out=None, env_ids=None, goals=None):
    kw = {k: x for k, x in var.items() if k not in ("goals", "q_rest", "mode")}
    q_rest = var.get("q_rest")
    g = torch.as_tensor(var["goals"] if goals is None else goals).to(sim.device)
    return sim.cartesian_multi_targets(g, mode="pose" if var["mode"] == MR.POSE else "delta",
                                       q_rest=None if q_rest is None else torch.as_tensor(q_rest).to(sim.device),
                                       targets=targets, err_out=err_out, env_ids=env_ids, **kw)


@pytest.mark.parametrize("task,n,name", ONE_STEP)
def test_one_step_matches_float64_reference(task, n, name):
    cs = _case(task, n)
    sim, var, q = cs["sim"], cs["variants"][name], cs["c"]["q"]
    T = len(var["tasks"])
    tgt = torch.as_tensor(q).to(sim.device).clone()
    err = torch.full((n, T, 6), float("nan"), device=sim.device)
    # what the launch must not read is NaN on the device: a position-only task's goal quaternion / angular part
    g = var["goals"].copy()
    for t, tk in enumerate(var["tasks"]):
        if tk["position_only"]:
            g[:, t, 3:] = np.nan
    assert _launch(sim, var, tgt, err, goals=g) is tgt
    torch.cuda.synchronize()
    t_ref, e_ref = _ref(cs, var, q.astype(np.float64))
    t, e = tgt.cpu().numpy(), err.cpu().numpy()
    step = np.abs(t_ref - q).max(axis=1)
    dt, de = np.abs(t - t_ref).max(), np.abs(e - e_ref).max()
    print(f"task {task} N {n} {name}: steps {step.min():.3f}..{step.max():.3f} rad, targets max err {dt:.2e}, "
          f"err_out max err {de:.2e}")
    assert step.min() > 1e-3, "the case must move"
    if name == "step_binding":
        assert np.allclose(step, 0.02, atol=1e-12)
    assert np.isfinite(t).all() and np.isfinite(e).all()
    assert dt <= 1e-5 and de <= 1e-5, f"targets {dt:.2e}, err_out {de:.2e}"
    U = _union(cs, var)
    rest = [d for d in range(sim.num_dofs) if d not in U]
    assert np.array_equal(t[:, rest].view(np.uint32), q[:, rest].view(np.uint32))
    for k, tk in enumerate(var["tasks"]):
        if tk["position_only"]:
            assert not e[:, k, 3:6].any() and not np.signbit(e[:, k, 3:6]).any()


@pytest.mark.parametrize("task,n", CASES)
def test_one_task_matches_the_single_link_kernel(task, n):
    cs = _case(task, n)
    sim, c, q = cs["sim"], cs["c"], cs["c"]["q"]
    for t, tk in enumerate(c["tasks"][:2]):
        var = dict(tasks=[tk], goals=np.ascontiguousarray(c["inconsistent"][:, t:t + 1]), mode=MR.POSE,
                   damping=c["damping"], max_step=0.2)
        a = torch.as_tensor(q).to(sim.device).clone()
        b = a.clone()
        ea = torch.zeros((n, 1, 6), device=sim.device)
        eb = torch.zeros((n, 6), device=sim.device)
        _launch(sim, var, a, ea)
        sim.cartesian_targets(torch.as_tensor(var["goals"][:, 0]).to(sim.device), tk["link"], offset=tk["offset"],
                              position_only=tk["position_only"], damping=c["damping"], max_step=0.2, targets=b,
                              err_out=eb)
        torch.cuda.synchronize()
        t_ref, e_ref = _ref(cs, var, q.astype(np.float64))
        da, db = np.abs(a.cpu().numpy() - t_ref).max(), np.abs(b.cpu().numpy() - t_ref).max()
        print(f"task {task} N {n} link {tk['link']}: multi {da:.2e}, single {db:.2e} rad from the reference")
        assert np.abs(t_ref - q).max() > 1e-3
        assert da <= 1e-5 and db <= 1e-5
        assert np.abs(ea.cpu().numpy()[:, 0] - e_ref[:, 0]).max() <= 1e-5
        assert np.abs(eb.cpu().numpy() - e_ref[:, 0]).max() <= 1e-5


@pytest.mark.parametrize("task,n", CASES)
def test_write_discipline(task, n):
    cs = _case(task, n)
    sim, var, q = cs["sim"], cs["variants"]["consistent"], cs["c"]["q"]
    D, T = sim.num_dofs, len(var["tasks"])
    if task == HM.TASK_UR5SIH:
        var = dict(var, dofs=[d for d in range(D) if d not in (3, 8)])     # two DOFs of U held: they keep the sentinel
    U = [d for d in _union(cs, var)]
    ids = [3, n + 2, 0, -1] if n == 5 else [7, 0]
    listed = [(k, e) for k, e in enumerate(ids) if 0 <= e < n]
    sentinel = (1000.0 + np.arange(n * D, dtype=np.float32).reshape(n, D))
    tgt = torch.as_tensor(sentinel).to(sim.device).clone()
    err = torch.full((n, T, 6), float("nan"), device=sim.device)
    before = {k: v.clone() for k, v in sim.t.items()}
    goals = np.stack([var["goals"][max(0, min(e, n - 1))] for e in ids])      # row k is for the k-th listed env
    _launch(sim, var, tgt, err, env_ids=torch.tensor(ids, dtype=torch.int32, device=sim.device), goals=goals)
    torch.cuda.synchronize()
    for k, v in sim.t.items():
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), f"the launch changed {k}"
    t, e = tgt.cpu().numpy(), err.cpu().numpy()
    written = np.zeros((n, D), bool)
    t_ref, e_ref = _ref(cs, dict(var, goals=np.stack([goals[k] for k, _ in listed])), q.astype(np.float64),
                        envs=[e_ for _, e_ in listed])
    for j, (_, env) in enumerate(listed):
        written[env, U] = True
        assert np.abs(t[env, U] - t_ref[j][U]).max() <= 1e-5
        assert np.abs(e[env] - e_ref[j]).max() <= 1e-5
    assert np.isfinite(t[written]).all()
    assert np.array_equal(t[~written].view(np.uint32), sentinel[~written].view(np.uint32))
    if task == HM.TASK_UR5SIH:
        assert not written[:, [3, 8]].any()
    unlisted = [env for env in range(n) if env not in [e_ for _, e_ in listed]]
    assert np.isnan(e[unlisted]).all()
    # default targets: the bound sim_targets, and only U of it
    var = cs["variants"]["subset"]
    U = _union(cs, var)
    snap = sim.t["sim_targets"].clone()
    out = sim.cartesian_multi_targets(torch.as_tensor(var["goals"]).to(sim.device), var["tasks"],
                                      damping=var["damping"], max_step=var["max_step"])
    torch.cuda.synchronize()
    assert out is sim.t["sim_targets"]
    full, _ = _ref(cs, var, q.astype(np.float64))
    got = out.cpu().numpy().reshape(n, D)
    assert np.abs(got - full).max() <= 1e-5
    rest = [d for d in range(D) if d not in U]
    assert len(rest) > 0 and np.array_equal(got[:, rest], snap.cpu().numpy().reshape(n, D)[:, rest])
    sim.t["sim_targets"].copy_(snap)


def test_limits_give_exactly_the_limit():
    cs = _case(HM.TASK_UR5SIH, 5)
    sim, q, lo, up = cs["sim"], cs["c"]["q"], cs["lo"], cs["up"]
    n = len(q)
    tips = [t for t in cs["c"]["tasks"] if t["position_only"]]
    fingers = list(range(6, sim.num_dofs))
    inf = np.full(sim.num_dofs, np.inf)
    hit = 0
    for sign in (1.0, -1.0):        # a 1 m "error" along x and along -x on all five fingertips, the arm held
        g = np.tile(np.array([sign, 0, 0, 0, 0, 0], np.float32), (n, len(tips), 1))
        var = dict(tasks=tips, goals=g, mode=MR.DELTA, damping=0.01, dofs=fingers)
        free, _ = _ref(cs, var, q.astype(np.float64), lo=-inf, up=inf)
        tgt = torch.as_tensor(q).to(sim.device).clone()
        _launch(sim, var, tgt)
        torch.cuda.synchronize()
        t = tgt.cpu().numpy()
        for d in fingers:
            over, under = free[:, d] > up[d] + 1e-3, free[:, d] < lo[d] - 1e-3
            assert np.array_equal(t[over, d], np.full(over.sum(), up[d]))
            assert np.array_equal(t[under, d], np.full(under.sum(), lo[d]))
            hit += int(over.sum() + under.sum())
        assert (t >= lo).all() and (t <= up).all()
        assert np.array_equal(t[:, 0:6], q[:, 0:6])
    assert hit >= 5, "the case must drive finger joints to their limits"


@pytest.mark.parametrize("task,n", CASES)
def test_closed_loop_kinematic(task, n):
    """Kernel and reference side by side from the same float32 start: targets written back as dof positions."""
    cs = _case(task, n)
    sim, var, q0 = cs["sim"], cs["variants"]["consistent"], cs["c"]["q"]
    D = sim.num_dofs
    dof = sim.t["dof_state"].view(n, D, 2)
    keep = dof.clone()
    tgt = torch.as_tensor(q0).to(sim.device).clone()
    g = torch.as_tensor(var["goals"]).to(sim.device)
    for _ in range(40):
        sim.cartesian_multi_targets(g, var["tasks"], damping=var["damping"], max_step=var["max_step"], targets=tgt)
        dof[..., 0] = tgt
    torch.cuda.synchronize()
    q_dev = dof[..., 0].cpu().numpy().astype(np.float64)
    dof.copy_(keep)
    q_ref = q0.astype(np.float64)
    for _ in range(40):
        q_ref, _ = _ref(cs, var, q_ref)
    gap = np.abs(q_dev - q_ref).max()
    left = [[MR.position_residual(cs["chain"], qq[e], var["goals"][e], var["tasks"]) for e in range(n)]
            for qq in (q_dev, q_ref)]
    print(f"task {task} N {n}: final q gap to the reference loop {gap:.2e} rad, position error left "
          f"{max(left[0]):.2e} m (kernel), {max(left[1]):.2e} m (reference)")
    assert gap <= 1e-4, f"final q gap {gap:.2e}"
    if task == HM.TASK_ALLEGRO_HAND:
        assert max(left[0]) < 1e-4
    else:
        assert np.abs(np.array(left[0]) - np.array(left[1])).max() <= 1e-5


def _torch_whole_hand(sim, jac, links, goal, lo, up, damping, max_step):
    """The route that exists without the kernel: the same stacked step composed in torch on the refreshed Jacobian
    tensor of the tasks' links and their rigid-body rows (tool offset 0; task 0 a pose, the others positions), the
    R x R solve in float64."""
    n, D = sim.num_envs, sim.num_dofs
    sim.refresh_jacobian_tensors()
    rb = sim.t["rigid_body_state"].view(n, sim.num_bodies, 13)[:, [sim.model.body_robot0 + l for l in links]]
    qg = goal[:, 0, 3:7] / goal[:, 0, 3:7].norm(dim=1, keepdim=True)
    qe = _qmul(qg, rb[:, 0, 3:7] * torch.tensor([-1.0, -1.0, -1.0, 1.0], device=sim.device))
    qe = torch.where(qe[:, 3:4] < 0, -qe, qe)
    v = qe[:, 0:3]
    vn = v.norm(dim=1, keepdim=True)
    rot = torch.where(vn < 1e-6, 2.0 * v, v / vn.clamp_min(1e-12) * 2.0 * torch.atan2(vn, qe[:, 3:4]))
    e = torch.cat([goal[:, 0, 0:3] - rb[:, 0, 0:3], rot, (goal[:, 1:, 0:3] - rb[:, 1:, 0:3]).reshape(n, -1)], 1)
    J = torch.cat([jac[:, 0], jac[:, 1:, 0:3].reshape(n, -1, D)], 1).double()
    A = J @ J.transpose(1, 2) + damping ** 2 * torch.eye(J.shape[1], device=sim.device, dtype=torch.float64)
    dq = (J.transpose(1, 2) @ torch.linalg.solve(A, e.double().unsqueeze(-1))).squeeze(-1)
    mx = dq.abs().amax(dim=1, keepdim=True)
    dq = torch.where(mx > max_step, dq * (max_step / mx), dq)
    q = sim.t["dof_state"].view(n, D, 2)[:, :, 0]
    sim.t["sim_targets"].view(n, D)[:] = torch.minimum(torch.maximum((q.double() + dq).float(), lo), up)


def test_closed_loop_with_physics_matches_torch_route():
    from handarm_hip.controllers import WholeHandController
    from handarm_hip.gym_api import acquire_gym
    task, n = HM.TASK_ALLEGRO_KUKA, 2
    cs = _case(task, 1)
    ch = cs["chain"]
    rng = np.random.default_rng(case_seed(task, n) + 7)
    p, _ = HM.build_params(task=task)
    rest = np.array(list(p.reset_pose)[:ch.D], np.float64)
    lo64, up64 = CR.limits(ch)
    # the arm within 0.05 rad of the reset pose, where the hand hovers over the table (test_gpu_cartesian.py), goals
    # the tool poses 0.1 rad away, raised where the arm's goal lies below its start
    q = np.clip(rest + rng.uniform(-0.05, 0.05, (n, ch.D)), lo64 + 0.05, up64 - 0.05).astype(np.float32)
    tasks = [dict(t, offset=(0.0, 0.0, 0.0)) for t in cs["c"]["tasks"]]
    links = [t["link"] for t in tasks]
    qg = np.clip(q + rng.uniform(-0.1, 0.1, q.shape), lo64 + 0.05, up64 - 0.05)
    goal = np.stack([MR.tool_goals(ch, qg[e], tasks) for e in range(n)])
    for e in range(n):
        z0 = MR.tool_goals(ch, q[e].astype(np.float64), tasks[:1])[0, 2]
        goal[e, :, 2] += max(0.0, z0 - goal[e, 0, 2])
    goal = torch.as_tensor(goal.astype(np.float32)).to("cuda:0")
    a, b = _make_sim(task, n, q), _make_sim(task, n, q)
    gym = acquire_gym()
    ctrl = WholeHandController(a, [dict(t, link=ch.links[t["link"]]["name"]) for t in tasks], damping=0.05,
                               max_step=0.2)
    assert ctrl.links == links and ctrl.targets is a.t["sim_targets"] and ctrl.err.shape == (n, len(tasks), 6)
    jac = b.acquire_jacobian_tensor(links=links)
    lo, up = (torch.as_tensor(x).to("cuda:0") for x in (cs["lo"], cs["up"]))

    def link_pos(sim):
        rows = [sim.model.body_robot0 + l for l in links]
        return sim.t["rigid_body_state"].view(n, sim.num_bodies, 13)[:, rows, 0:3].clone()
    for sim in (a, b):
        sim.simulate(1)             # fills rigid_body_state for the first torch step
    d0 = (goal[:, :, 0:3] - link_pos(a)).norm(dim=2)
    for _ in range(60):
        assert gym.set_cartesian_pose_target(a, ctrl, goal)
        a.simulate(1)
        _torch_whole_hand(b, jac, links, goal, lo, up, 0.05, 0.2)
        b.simulate(1)
    torch.cuda.synchronize()
    pa, pb = link_pos(a), link_pos(b)
    gap = float((pa - pb).abs().max())
    da, db = (goal[:, :, 0:3] - pa).norm(dim=2), (goal[:, :, 0:3] - pb).norm(dim=2)
    print(f"link position gap kernel route / torch route after 60 steps {gap:.3e} m; largest distance to a goal "
          f"{float(d0.max()):.3e} -> {float(da.max()):.3e} (kernel), {float(db.max()):.3e} (torch); last task error "
          f"{float(ctrl.err.abs().max()):.3e}")
    assert torch.isfinite(pa).all() and torch.isfinite(pb).all()
    assert da.max() < d0.max() and db.max() < d0.max(), "both sims must end closer to the goals than they started"
    assert PHYS_TOL is not None and gap <= PHYS_TOL, f"gap {gap:.3e} m"


def test_argument_errors():
    cs = _case(HM.TASK_UR5SIH, 1)
    sim, var = cs["sim"], cs["variants"]["consistent"]
    lib, D, L = sim.lib, sim.num_dofs, sim.num_links
    T = len(var["tasks"])
    goal = torch.as_tensor(var["goals"]).to(sim.device)
    tgt = torch.zeros((1, D), device=sim.device)
    rest = torch.zeros(D, device=sim.device)
    ids = torch.zeros(1, dtype=torch.int32, device=sim.device)
    flange, thumb = var["tasks"][0]["link"], var["tasks"][-1]["link"]

    def tasks_of(spec):
        arr = (_lib.HaCartTask * HM.CART_MAX_TASKS)()
        for t, (link, ponly, w) in enumerate(spec):
            arr[t] = _lib.HaCartTask(link, ponly, (C.c_float * 3)(0.02, -0.01, 0.05), w)
        return arr
    good = [(flange, 0, 1.0)] + [(t["link"], 1, 1.0) for t in var["tasks"][1:]]

    def call(h=None, null=False, spec=None, **kw):
        spec = good if spec is None else spec
        f = dict(goal=goal.data_ptr(), targets=tgt.data_ptr(), err_out=None, q_rest=None, env_ids=None, n_envs=0,
                 n_tasks=len(spec), mode=HM.CART_POSE, dof_mask=(1 << D) - 1, damping=0.05, max_step=0.0,
                 null_gain=0.0, task=tasks_of(spec[:HM.CART_MAX_TASKS]))
        f.update(kw)
        s = _lib.HaCartesianMulti(**f)
        return lib.ha_cartesian_multi_targets(sim.h if h is None else h, None if null else C.byref(s), sim._stream())
    assert call() == 0
    E_ARG, E_STATE = -1, -3
    nan, inf = float("nan"), float("inf")
    bad = [dict(goal=None), dict(targets=None), dict(n_tasks=0), dict(n_tasks=-1), dict(n_tasks=7), dict(mode=2),
           dict(mode=-1), dict(damping=0.0), dict(damping=-0.1), dict(damping=nan), dict(damping=inf),
           dict(max_step=-1.0), dict(max_step=nan), dict(max_step=inf), dict(null_gain=-0.5), dict(null_gain=nan),
           dict(null_gain=inf), dict(null_gain=0.5), dict(dof_mask=0),
           dict(dof_mask=1 << 14),                              # a thumb DOF does not move the flange
           dict(env_ids=ids.data_ptr(), n_envs=0), dict(env_ids=ids.data_ptr(), n_envs=-2),
           dict(spec=[(0, 0, 1.0)]), dict(spec=[(L, 0, 1.0)]), dict(spec=[(-1, 0, 1.0)]),
           dict(spec=[(flange, 0, 1.0), (L, 1, 1.0)]), dict(spec=[(flange, 0, 1.0), (0, 1, 1.0)]),
           dict(spec=[(flange, 0, 1.0)] * 5),                   # 30 rows
           dict(spec=[(flange, 0, 1.0)] * 4 + [(thumb, 1, 1.0)]),   # 27 rows
           dict(spec=[(flange, 0, 0.0)]), dict(spec=[(flange, 0, -1.0)]), dict(spec=[(flange, 0, nan)]),
           dict(spec=[(flange, 0, inf)]), dict(spec=[(flange, 0, 1.0), (thumb, 1, nan)])]
    for kw in bad:
        assert call(**kw) == E_ARG, kw
    assert call(dof_mask=0x3F) == 0                             # the arm DOFs move every link
    assert call(dof_mask=0x3F | 1 << 14, spec=[(flange, 0, 1.0), (thumb, 1, 1.0)]) == 0
    assert call(dof_mask=1 << 14, spec=[(thumb, 1, 1.0)]) == 0
    assert call(spec=[(flange, 0, 1.0)] * 4) == 0               # 24 rows exactly
    assert call(spec=[(thumb, 1, 1.0)] * 6) == 0                # six tasks on one link
    assert call(null=True) == E_ARG
    assert lib.ha_cartesian_multi_targets(None, None, None) == E_ARG
    assert call(null_gain=0.5, q_rest=rest.data_ptr()) == 0 and call(env_ids=ids.data_ptr(), n_envs=1) == 0
    h2 = C.c_void_p()
    assert lib.ha_create(C.byref(sim.model), C.byref(sim.params), 1, C.byref(h2)) == 0
    try:
        assert call(h=h2) == E_STATE                                      # before ha_bind_state
    finally:
        lib.ha_destroy(h2)
    torch.cuda.synchronize()
    # the same through Python: every refusal raises HandArmError
    from handarm_hip.controllers import WholeHandController
    tasks = var["tasks"]
    five_poses = [dict(link="flange")] * 5
    for kw in (dict(mode="twist"), dict(mode=5), dict(damping=0.0), dict(damping=nan), dict(max_step=-1.0),
               dict(null_gain=-1.0), dict(null_gain=0.5), dict(dofs=[D]), dict(dofs=[]),
               dict(dofs=[14]),                                           # a thumb DOF moves no other task's link
               dict(env_ids=torch.zeros(0, dtype=torch.int32))):
        with pytest.raises(_lib.HandArmError):
            sim.cartesian_multi_targets(goal, tasks, targets=tgt, **kw)
    wrong = [None, goal[:, :, 0:6].contiguous(), goal[:, 0].contiguous(), goal[:, 0:T - 1].contiguous(),
             goal.transpose(1, 2)]
    for g in wrong:
        with pytest.raises(_lib.HandArmError):
            sim.cartesian_multi_targets(g, tasks, targets=tgt)
    g5 = torch.zeros((1, 5, 7), device=sim.device)
    for bad_tasks in ([dict(link="no_such_link")], five_poses, [], [dict(link="flange")] * 7, [dict(link=0)],
                      [dict(link="flange", weight=0.0)], [dict(link="flange", weight=nan)],
                      [dict(link="flange", gain=2.0)], [dict(offset=(0, 0, 0))]):
        with pytest.raises(_lib.HandArmError):
            sim.cartesian_multi_targets(g5[:, 0:max(1, len(bad_tasks))].contiguous(), bad_tasks, targets=tgt)
        with pytest.raises(_lib.HandArmError):
            WholeHandController(sim, bad_tasks)
    with pytest.raises(_lib.HandArmError):
        WholeHandController(sim, [dict(link="flange")], dofs=[14])
    with pytest.raises(_lib.HandArmError):
        sim.cartesian_multi_targets(goal, tasks, targets=tgt, err_out=torch.zeros((1, 6), device=sim.device))
    assert sim.cartesian_multi_targets(goal, [dict(t, link=cs["chain"].links[t["link"]]["name"]) for t in tasks],
                                       targets=tgt) is tgt
    torch.cuda.synchronize()


@pytest.mark.parametrize("task", [HM.TASK_UR5SIH, HM.TASK_ALLEGRO_HAND])
def test_gym_api_drives_the_whole_hand_controller(task):
    from handarm_hip.controllers import WholeHandController
    from handarm_hip.gym_api import acquire_gym
    n = 5
    cs = _case(task, n)
    sim, var, q = cs["sim"], cs["variants"]["weighted_inconsistent"], cs["c"]["q"]
    goal = torch.as_tensor(var["goals"]).to(sim.device)
    direct = torch.as_tensor(q).to(sim.device).clone()
    via = direct.clone()
    c1 = WholeHandController(sim, var["tasks"], damping=var["damping"], max_step=var["max_step"], targets=direct)
    c2 = WholeHandController(sim, var["tasks"], damping=var["damping"], max_step=var["max_step"], targets=via)
    assert c1.step(goal) is direct
    assert acquire_gym().set_cartesian_pose_target(sim, c2, goal) is True
    torch.cuda.synchronize()
    assert c1.err.shape == (n, len(var["tasks"]), 6) and c1.sim is sim and c1.targets is direct
    assert torch.equal(direct, via) and torch.equal(c1.err, c2.err)
    t_ref, e_ref = _ref(cs, var, q.astype(np.float64))
    assert np.abs(via.cpu().numpy() - t_ref).max() <= 1e-5 and np.abs(c2.err.cpu().numpy() - e_ref).max() <= 1e-5
    other = _case(task, 1)["sim"]
    with pytest.raises(ValueError):
        acquire_gym().set_cartesian_pose_target(other, c2, goal)
