"""The Cartesian controller kernel (ha_cartesian_kernel through HandArmSim.cartesian_targets, CartesianController and
gym_api) against the float64 tests/cartesian_ref.py, for the three robots, N = 5 envs (no multiple of the kernel's envs
per workgroup) and N = 1.

Inputs (cartesian_ref.robot_case): arms at reset_pose + U(-0.3, 0.3) kept 0.05 rad inside the limits, tool offset
(0.02, -0.01, 0.05), goals 5 cm and 0.2 rad away, lambda 0.05; the AllegroHand at its mid-range pose, thumb-tip goals
1 cm away, position only, lambda 0.01. Objects parked with collisions off (_fill of test_independent_dynamics).

Bounds (from the reference's and the formats' precision, not from the kernel's output):
* one step: targets within 1e-5 rad of the float64 reference and err_out within 1e-5, the Jacobian tensor's own bound
  (test_gpu_kinematics_tensors). A float32 numpy emulation of the same arithmetic differs from float64 by at most
  7.2e-7 on steps of 0.08-0.46 rad, so the bound has about 14x headroom.
* kinematic closed loop, 30 iterations: final q within 1e-4 rad of the reference loop (10 one-step bounds: the loop
  contracts), final tool error below 1e-4 m by Chain.fk (the bound of the torch DLS test). With the posture term the
  loop does not reach the goal (the damped projector leaks into task space): agreement with the reference only.
* closed loop with physics, 120 steps of cartesian_targets -> simulate(1), against a twin sim driven by the torch
  composition on acquire_jacobian_tensor(links=[link]): PHYS_TOL below.
The device reaches (MI355X, the cases below): one step, arms 7.9e-7 rad, the fingertip cases at lambda 0.01 3.4e-6 rad,
err_out 3.5e-7; kinematic loop, final q 1.4e-6 rad from the reference loop and 3.5e-7 m of tool error left, with the
posture term 7.8e-7 rad; with physics, the two routes' link positions 2.4e-7 m (Ur5Sih) and 5.1e-7 m (AllegroKuka)
apart, the flange 0.12 mm and the iiwa's last link (kp 40) 8.7 mm from goals that were 5 cm away."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from handarm_hip import _lib
from handarm_hip import model as HM
from tests import cartesian_ref as CR
from tests.kinematics import Chain
from tests.test_independent_dynamics import ROBOTS, _fill

pytestmark = pytest.mark.gpu
ASSET = dict(ROBOTS)
CASES = [(task, n) for task, _ in ROBOTS for n in (5, 1)]
# final link-position gap between the kernel-driven and the torch-driven sim after 120 physics steps. The two routes
# compute the same step in different float32 orders (their targets differ by about 1e-6 rad per step) and the PD-driven
# arm is a stable system, so the gap stays of that order times the arm's reach.
# PHYS_MEASURED is what the MI355X gave (2 and 4 float32 ulps of a metre); PHYS_TOL is 10x that
PHYS_MEASURED = {HM.TASK_UR5SIH: 2.384e-7, HM.TASK_ALLEGRO_KUKA: 5.066e-7}
PHYS_TOL = {k: None if v is None else 10.0 * v for k, v in PHYS_MEASURED.items()}


def _make_sim(task, n, q):
    """A sim of the task's robot at rest in the joint positions q (n, D) float32, targets = q."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from handarm_hip.sim import HandArmSim
    from oracle.oracle_lib import HostState
    sim = HandArmSim(n, "cuda:0", task_cfg=dict(task=task), task=task)
    m, p = sim.model, sim.params
    st = HostState(n, model=m, params=p)
    for k in HM.STATE_FIELDS:
        if k not in HM.null_fields(task) and k not in ("stats", "term_sums"):
            st[k][...] = sim.t[k].cpu().numpy().reshape(st[k].shape)
    _fill(st, m, p, q, np.zeros_like(q), q)
    for k in ("root_state", "dof_state", "sim_targets", "collision_enabled", "object_scale"):
        if k not in HM.null_fields(task):
            sim.t[k].copy_(torch.as_tensor(st[k]).reshape(sim.t[k].shape).to(sim.t[k].dtype))
    return sim


@functools.lru_cache(maxsize=None)
def _case(task, n):
    """One sim per (robot, N) with the case's joints, the float64 chain and the variants of the one-step test."""
    ch = Chain(HM.load_scene(ASSET[task]))
    p, _ = HM.build_params(task=task)
    rest = np.array(list(p.reset_pose)[:ch.D], np.float32)
    c = CR.robot_case(ch, task, rest, n, seed=200 + 10 * task + n)
    sim = _make_sim(task, n, c["q"])
    D = sim.num_dofs
    lo = np.array(list(sim.model.dof_lower)[:D], np.float32)
    up = np.array(list(sim.model.dof_upper)[:D], np.float32)
    names = [l["name"] for l in ch.links]
    rng = np.random.default_rng(300 + 10 * task + n)
    base = dict(link=c["link"], dofs=c["dofs"], mode="pose", goal=c["goal"], **c["gains"])
    v = {"pose": base,
         "step_off": dict(base, max_step=0.0),
         "step_binding": dict(base, max_step=0.02),
         "step_not_binding": dict(base, max_step=10.0),
         "no_offset": dict(base, offset=(0.0, 0.0, 0.0)),
         "delta": dict(base, mode="delta",
                       goal=(rng.uniform(-0.03, 0.03, (n, 6)) * ([1] * 3 + [4] * 3)).astype(np.float32))}
    if task == HM.TASK_ALLEGRO_KUKA:
        v["posture"] = dict(base, q_rest=rest, null_gain=0.5)
        tip = names.index("thumb_link_3")
        tg = CR.case_goals(ch, c["q"], tip, CR.OFFSET, rng, dist=0.01)
        v["thumb_tip"] = dict(base, link=tip, dofs=[19, 20, 21, 22], goal=tg, damping=0.01, position_only=True)
        v["thumb_tip_with_arm"] = dict(base, link=tip, dofs=sorted(ch.ancestors(tip)), goal=tg, position_only=True)
    if task == HM.TASK_UR5SIH:
        tip = names.index("thumb_fingertip")
        tg = CR.case_goals(ch, c["q"], tip, CR.OFFSET, rng, dist=0.01)
        v["thumb_tip"] = dict(base, link=tip, dofs=[14, 15, 16], goal=tg, damping=0.01, position_only=True)
    return dict(sim=sim, chain=ch, c=c, rest=rest, lo=lo, up=up, variants=v)


COMMON = ["pose", "step_off", "step_binding", "step_not_binding", "no_offset", "delta"]
EXTRA = {HM.TASK_UR5SIH: ["thumb_tip"], HM.TASK_ALLEGRO_HAND: [],
         HM.TASK_ALLEGRO_KUKA: ["posture", "thumb_tip", "thumb_tip_with_arm"]}
ONE_STEP = [(task, n, name) for task, n in CASES for name in COMMON + EXTRA[task]]


def _ref(cs, var, q, envs=None):
    """Float64 targets (len(envs), D) and errors (len(envs), 6) of a variant; goal row k belongs to envs[k]."""
    kw = {k: x for k, x in var.items() if k not in ("goal", "mode", "link")}
    mode = CR.POSE if var["mode"] == "pose" else CR.DELTA
    envs = range(len(q)) if envs is None else envs
    lo, up = cs["lo"].astype(np.float64), cs["up"].astype(np.float64)
    out = [CR.cartesian_step(cs["chain"], q[e], var["goal"][k], var["link"], mode=mode, lower=lo, upper=up, **kw)
           for k, e in enumerate(envs)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _launch(sim, var, targets, err_out=None, env_ids=None, goal=None):
    kw = {k: x for k, x in var.items() if k not in ("goal", "q_rest")}
    q_rest = var.get("q_rest")
    g = torch.as_tensor(var["goal"] if goal is None else goal).to(sim.device)
    return sim.cartesian_targets(g, q_rest=None if q_rest is None else torch.as_tensor(q_rest).to(sim.device),
                                 targets=targets, err_out=err_out, env_ids=env_ids, **kw)


@pytest.mark.parametrize("task,n,name", ONE_STEP)
def test_one_step_matches_float64_reference(task, n, name):
    cs = _case(task, n)
    sim, var, q = cs["sim"], cs["variants"][name], cs["c"]["q"]
    tgt = torch.as_tensor(q).to(sim.device).clone()
    err = torch.full((n, 6), float("nan"), device=sim.device)
    assert _launch(sim, var, tgt, err) is tgt
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
    if name == "step_not_binding":
        assert (step < 10.0).all()
        assert np.array_equal(t_ref, _ref(cs, cs["variants"]["step_off"], q.astype(np.float64))[0])
    if name == "pose":
        assert step.max() <= 0.2 + 1e-12
    assert np.isfinite(t).all() and np.isfinite(e).all()
    assert dt <= 1e-5 and de <= 1e-5, f"targets {dt:.2e}, err_out {de:.2e}"
    rest = [d for d in range(sim.num_dofs) if d not in var["dofs"]]
    assert np.array_equal(t[:, rest], q[:, rest])
    if var.get("position_only"):
        assert not e[:, 3:6].any()


@pytest.mark.parametrize("task,n", CASES)
def test_write_discipline(task, n):
    cs = _case(task, n)
    sim, var, q = cs["sim"], cs["variants"]["pose"], cs["c"]["q"]
    D = sim.num_dofs
    ids = [3, n + 2, 0, -1] if n == 5 else [7, 0]
    listed = [(k, e) for k, e in enumerate(ids) if 0 <= e < n]
    sentinel = (1000.0 + np.arange(n * D, dtype=np.float32).reshape(n, D))
    tgt = torch.as_tensor(sentinel).to(sim.device).clone()
    err = torch.full((n, 6), float("nan"), device=sim.device)
    before = {k: v.clone() for k, v in sim.t.items()}
    goal = np.stack([var["goal"][max(0, min(e, n - 1))] for e in ids])      # row k is for the k-th listed env
    _launch(sim, var, tgt, err, env_ids=torch.tensor(ids, dtype=torch.int32, device=sim.device), goal=goal)
    torch.cuda.synchronize()
    for k, v in sim.t.items():
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), f"the launch changed {k}"
    t, e = tgt.cpu().numpy(), err.cpu().numpy()
    written = np.zeros((n, D), bool)
    t_ref, e_ref = _ref(dict(cs), dict(var, goal=np.stack([goal[k] for k, _ in listed])), q.astype(np.float64),
                        envs=[e_ for _, e_ in listed])
    for j, (_, env) in enumerate(listed):
        written[env, var["dofs"]] = True
        assert np.abs(t[env, var["dofs"]] - t_ref[j][var["dofs"]]).max() <= 1e-5
        assert np.abs(e[env] - e_ref[j]).max() <= 1e-5
    assert np.isfinite(t[written]).all()
    assert np.array_equal(t[~written].view(np.uint32), sentinel[~written].view(np.uint32))
    unlisted = [env for env in range(n) if env not in [e_ for _, e_ in listed]]
    assert np.isnan(e[unlisted]).all()
    # default targets: the bound sim_targets, and only the selected DOFs of it
    snap = sim.t["sim_targets"].clone()
    out = sim.cartesian_targets(torch.as_tensor(var["goal"]).to(sim.device), var["link"], **cs["c"]["gains"])
    torch.cuda.synchronize()
    assert out is sim.t["sim_targets"]
    full, _ = _ref(cs, var, q.astype(np.float64))
    got = out.cpu().numpy().reshape(n, D)
    assert np.abs(got - full).max() <= 1e-5
    rest = [d for d in range(D) if d not in var["dofs"]]
    assert np.array_equal(got[:, rest], snap.cpu().numpy().reshape(n, D)[:, rest])
    sim.t["sim_targets"].copy_(snap)


def _limit_case(cs, link, dofs, goal6, **kw):
    sim, q = cs["sim"], cs["c"]["q"]
    n = len(q)
    var = dict(link=link, dofs=dofs, mode="delta", goal=np.tile(np.asarray(goal6, np.float32), (n, 1)), **kw)
    free, _ = _ref(dict(cs, lo=np.full_like(cs["lo"], -np.inf), up=np.full_like(cs["up"], np.inf)), var,
                   q.astype(np.float64))
    tgt = torch.as_tensor(q).to(sim.device).clone()
    _launch(sim, var, tgt)
    torch.cuda.synchronize()
    return free, tgt.cpu().numpy()


def test_limits_give_exactly_the_limit():
    cs = _case(HM.TASK_UR5SIH, 5)
    lo, up = cs["lo"], cs["up"]
    names = [l["name"] for l in cs["chain"].links]
    # a 10 m "error" along z with no step limit: joint 2 of the UR5 is driven several radians past its +-pi limit
    free, t = _limit_case(cs, cs["c"]["link"], cs["c"]["dofs"], [0, 0, 10.0, 0, 0, 0], damping=0.05)
    over, under = free[:, 2] > up[2] + 1e-3, free[:, 2] < lo[2] - 1e-3
    assert (over | under).all(), "the case must drive joint 2 past a limit in every env"
    assert np.array_equal(t[over, 2], np.full(over.sum(), up[2]))
    assert np.array_equal(t[under, 2], np.full(under.sum(), lo[2]))
    assert (t >= lo).all() and (t <= up).all()
    # an index-finger joint: 1 m along x and along -x, position only
    tip, dofs = names.index("index_fingertip"), [6, 7]
    hit = 0
    for sign in (1.0, -1.0):
        free, t = _limit_case(cs, tip, dofs, [sign, 0, 0, 0, 0, 0], damping=0.01, position_only=True)
        for d in dofs:
            over, under = free[:, d] > up[d] + 1e-3, free[:, d] < lo[d] - 1e-3
            assert np.array_equal(t[over, d], np.full(over.sum(), up[d]))
            assert np.array_equal(t[under, d], np.full(under.sum(), lo[d]))
            hit += int(over.sum() + under.sum())
        assert (t >= lo).all() and (t <= up).all()
    assert hit >= 5, "the finger case must reach a limit"


def _kin_loop(cs, var, iters):
    """Kernel and reference side by side from the same float32 start: targets written back as dof positions."""
    sim, q0 = cs["sim"], cs["c"]["q"]
    n, D = q0.shape
    dof = sim.t["dof_state"].view(n, D, 2)
    keep = dof.clone()
    tgt = torch.as_tensor(q0).to(sim.device).clone()
    g = torch.as_tensor(var["goal"]).to(sim.device)
    kw = {k: x for k, x in var.items() if k not in ("goal", "q_rest")}
    q_rest = None if var.get("q_rest") is None else torch.as_tensor(var["q_rest"]).to(sim.device)
    for _ in range(iters):
        sim.cartesian_targets(g, q_rest=q_rest, targets=tgt, **kw)
        dof[..., 0] = tgt
    torch.cuda.synchronize()
    q_dev = dof[..., 0].cpu().numpy().astype(np.float64)
    dof.copy_(keep)
    q_ref = q0.astype(np.float64)
    for _ in range(iters):
        q_ref, _ = _ref(cs, var, q_ref)
    return q_dev, q_ref


@pytest.mark.parametrize("task,n", CASES)
def test_closed_loop_kinematic(task, n):
    cs = _case(task, n)
    var = cs["variants"]["pose"]
    q_dev, q_ref = _kin_loop(cs, var, 30)
    gap = np.abs(q_dev - q_ref).max()
    left = max(np.abs(CR.task_error(cs["chain"], q_dev[e], var["goal"][e].astype(np.float64), var["link"],
                                    offset=var["offset"], position_only=var["position_only"])[0:3]).max()
               for e in range(n))
    print(f"task {task} N {n}: final q gap to the reference loop {gap:.2e} rad, tool error left {left:.2e} m")
    assert gap <= 1e-4, f"final q gap {gap:.2e}"
    assert left < 1e-4, f"final tool error {left:.2e} m"


@pytest.mark.parametrize("n", [5, 1])
def test_closed_loop_kinematic_with_posture_term(n):
    cs = _case(HM.TASK_ALLEGRO_KUKA, n)
    q_dev, q_ref = _kin_loop(cs, cs["variants"]["posture"], 30)
    gap = np.abs(q_dev - q_ref).max()
    print(f"AllegroKuka N {n} posture term: final q gap to the reference loop {gap:.2e} rad")
    assert gap <= 1e-4, f"final q gap {gap:.2e}"


def _qmul(a, b):
    x1, y1, z1, w1 = a.unbind(-1)
    x2, y2, z2, w2 = b.unbind(-1)
    return torch.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                        w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], -1)


def _torch_dls(sim, jac, link, dofs, goal, lo, up, damping, max_step):
    """The route that exists without the kernel: the same step composed in torch on the refreshed Jacobian tensor of the
    one link and the rigid-body row of the link (tool offset 0)."""
    n, D = sim.num_envs, sim.num_dofs
    sim.refresh_jacobian_tensors()
    rb = sim.t["rigid_body_state"].view(n, sim.num_bodies, 13)[:, sim.model.body_robot0 + link]
    qg = goal[:, 3:7] / goal[:, 3:7].norm(dim=1, keepdim=True)
    qe = _qmul(qg, rb[:, 3:7] * torch.tensor([-1.0, -1.0, -1.0, 1.0], device=sim.device))
    qe = torch.where(qe[:, 3:4] < 0, -qe, qe)
    v = qe[:, 0:3]
    vn = v.norm(dim=1, keepdim=True)
    rot = torch.where(vn < 1e-6, 2.0 * v, v / vn.clamp_min(1e-12) * 2.0 * torch.atan2(vn, qe[:, 3:4]))
    e = torch.cat([goal[:, 0:3] - rb[:, 0:3], rot], 1).unsqueeze(-1)
    J = jac[:, 0][:, :, dofs]
    A = J @ J.transpose(1, 2) + damping ** 2 * torch.eye(6, device=sim.device)
    dq = (J.transpose(1, 2) @ torch.linalg.solve(A, e)).squeeze(-1)
    mx = dq.abs().amax(dim=1, keepdim=True)
    dq = torch.where(mx > max_step, dq * (max_step / mx), dq)
    q = sim.t["dof_state"].view(n, D, 2)[:, dofs, 0]
    sim.t["sim_targets"].view(n, D)[:, dofs] = torch.minimum(torch.maximum(q + dq, lo[dofs]), up[dofs])


@pytest.mark.parametrize("task", [HM.TASK_UR5SIH, HM.TASK_ALLEGRO_KUKA])
def test_closed_loop_with_physics_matches_torch_route(task):
    from handarm_hip.controllers import CartesianController
    from handarm_hip.gym_api import acquire_gym
    n = 5
    cs = _case(task, n)
    ch, c = cs["chain"], cs["c"]
    link, dofs = c["link"], c["dofs"]
    rng = np.random.default_rng(400 + task)
    q = c["q"]
    if task == HM.TASK_ALLEGRO_KUKA:
        # at the case's poses (+-0.3 rad) the hand can start inside the table, whose contacts then move the arm whatever
        # the targets say. Here the arm stays within 0.05 rad of the reset pose, where the hand hovers 16 cm over the
        # table, and the goals lie level with the tool or above it
        q = np.clip(cs["rest"] + rng.uniform(-0.05, 0.05, c["q"].shape), cs["lo"] + 0.05, cs["up"] - 0.05)
        q = q.astype(np.float32)
    goal = CR.case_goals(ch, q, link, (0.0, 0.0, 0.0), rng)
    if task == HM.TASK_ALLEGRO_KUKA:
        z = np.array([CR.tool_pose(ch, q[e].astype(np.float64), link)[0][2] for e in range(n)], np.float32)
        goal[:, 2] = z + np.abs(goal[:, 2] - z)
    goal = torch.as_tensor(goal).to("cuda:0")
    a, b = _make_sim(task, n, q), _make_sim(task, n, q)
    gym = acquire_gym()
    ctrl = CartesianController(a, ch.links[link]["name"], damping=0.05, max_step=0.2)
    assert ctrl.link == link and ctrl.dofs == dofs and ctrl.targets is a.t["sim_targets"]
    jac = b.acquire_jacobian_tensor(links=[link])
    lo, up = (torch.as_tensor(x).to("cuda:0") for x in (cs["lo"], cs["up"]))

    def link_pos(sim):
        return sim.t["rigid_body_state"].view(n, sim.num_bodies, 13)[:, sim.model.body_robot0 + link, 0:3].clone()
    for sim in (a, b):
        sim.simulate(1)             # fills rigid_body_state for the first torch step
    d0 = (goal[:, 0:3] - link_pos(a)).norm(dim=1)
    for _ in range(120):
        assert gym.set_cartesian_pose_target(a, ctrl, goal)
        a.simulate(1)
        _torch_dls(b, jac, link, dofs, goal, lo, up, 0.05, 0.2)
        b.simulate(1)
    torch.cuda.synchronize()
    pa, pb = link_pos(a), link_pos(b)
    gap = float((pa - pb).abs().max())
    da, db = (goal[:, 0:3] - pa).norm(dim=1), (goal[:, 0:3] - pb).norm(dim=1)
    print(f"task {task}: link position gap kernel route / torch route after 120 steps {gap:.3e} m; distance to goal "
          f"{float(d0.max()):.3e} -> {float(da.max()):.3e} (kernel), {float(db.max()):.3e} (torch); last task error "
          f"{float(ctrl.err.abs().max()):.3e}")
    assert torch.isfinite(pa).all() and torch.isfinite(pb).all()
    assert (da < d0).all() and (db < d0).all(), "both sims must end closer to the goal than they started"
    assert PHYS_TOL[task] is not None and gap <= PHYS_TOL[task], f"gap {gap:.3e} m"


def test_argument_errors():
    cs = _case(HM.TASK_UR5SIH, 1)
    sim, var = cs["sim"], cs["variants"]["pose"]
    lib, D = sim.lib, sim.num_dofs
    goal = torch.as_tensor(var["goal"]).to(sim.device)
    tgt = torch.zeros((1, D), device=sim.device)
    rest = torch.zeros(D, device=sim.device)
    ids = torch.zeros(1, dtype=torch.int32, device=sim.device)
    mask = sum(1 << d for d in var["dofs"])

    def call(h=None, null=False, **kw):
        f = dict(goal=goal.data_ptr(), targets=tgt.data_ptr(), err_out=None, q_rest=None, env_ids=None, n_envs=0,
                 link=var["link"], mode=HM.CART_POSE, position_only=0, dof_mask=mask, offset=(C.c_float * 3)(0, 0, 0),
                 damping=0.05, max_step=0.0, null_gain=0.0)
        f.update(kw)
        s = _lib.HaCartesian(**f)
        return lib.ha_cartesian_targets(sim.h if h is None else h, None if null else C.byref(s), sim._stream())
    assert call() == 0
    E_ARG, E_STATE = -1, -3
    bad = [dict(goal=None), dict(targets=None), dict(link=0), dict(link=sim.num_links), dict(link=-1), dict(mode=2),
           dict(mode=-1), dict(damping=0.0), dict(damping=-0.1), dict(damping=float("nan")), dict(damping=float("inf")),
           dict(max_step=-1.0), dict(max_step=float("nan")), dict(max_step=float("inf")), dict(null_gain=-0.5),
           dict(null_gain=float("nan")), dict(null_gain=float("inf")), dict(null_gain=0.5),
           dict(dof_mask=0), dict(dof_mask=1 << 14),                    # a thumb DOF does not move the flange
           dict(env_ids=ids.data_ptr(), n_envs=0), dict(env_ids=ids.data_ptr(), n_envs=-2)]
    for kw in bad:
        assert call(**kw) == E_ARG, kw
    assert call(null=True) == E_ARG
    assert lib.ha_cartesian_targets(None, None, None) == E_ARG
    assert call(null_gain=0.5, q_rest=rest.data_ptr()) == 0 and call(env_ids=ids.data_ptr(), n_envs=1) == 0
    h2 = C.c_void_p()
    assert lib.ha_create(C.byref(sim.model), C.byref(sim.params), 1, C.byref(h2)) == 0
    try:
        assert call(h=h2) == E_STATE                                      # before ha_bind_state
    finally:
        lib.ha_destroy(h2)
    torch.cuda.synchronize()
    # the same through Python: every refusal raises HandArmError, an unknown link name KeyError
    gains = dict(damping=0.05)
    for kw in (dict(link=0), dict(link=sim.num_links), dict(mode="twist"), dict(mode=5), dict(damping=0.0),
               dict(damping=float("nan")), dict(max_step=-1.0), dict(null_gain=-1.0), dict(null_gain=0.5),
               dict(dofs=[14]), dict(dofs=[]), dict(dofs=[D]), dict(env_ids=torch.zeros(0, dtype=torch.int32))):
        args = dict(dict(link=var["link"], targets=tgt, **gains), **kw)
        with pytest.raises(_lib.HandArmError):
            sim.cartesian_targets(goal, **args)
    with pytest.raises(_lib.HandArmError):
        sim.cartesian_targets(None, var["link"], targets=tgt)
    with pytest.raises(_lib.HandArmError):
        sim.cartesian_targets(goal[:, 0:6].contiguous(), var["link"], targets=tgt)      # pose goals are 7 wide
    with pytest.raises(KeyError):
        sim.cartesian_targets(goal, "no_such_link", targets=tgt)
    from handarm_hip.controllers import CartesianController
    with pytest.raises(KeyError):
        CartesianController(sim, "no_such_link")
    with pytest.raises(_lib.HandArmError):
        CartesianController(sim, "flange", dofs=[14])
    assert sim.cartesian_targets(goal, "flange", targets=tgt) is tgt
    torch.cuda.synchronize()
