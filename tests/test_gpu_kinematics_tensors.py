"""Jacobian and mass-matrix tensors on the device (ha_kinematics_kernel through HandArmSim and gym_api) against the
float64 tests/kinematics.py Chain and tests/jacobian_ref.py, for the three robots.

Inputs of every case: q = reset_pose + U(-0.3, 0.3), qd = U(-1, 1), objects parked with collisions off (_fill of
test_independent_dynamics); N = 5 envs (no multiple of the kernel's envs per workgroup) and N = 1.

Bounds (from the reference's and the formats' precision, not from the kernel's output):
* Jacobian entries: atol 1e-5. An entry is a x r: positions hold to 3e-6 (test_oracle_fk_matches_independent_fk), axes
  after 15 quaternion levels to about 1e-6, |r| <= 1.5 m: 1.5e-6 + 3e-6, doubled. Exact zeros of the reference (the
  columns of DOFs that do not move the link, a x 0, zero axis components) must be exactly 0.0. Not counted: a zero
  the float64 reference gets by subtracting two equal NON-ZERO products (jacobian_ref.cancellation_mask), where a link
  origin lies on the joint axis: whether that difference is 0.0 or 1e-17 is rounding luck of the reference (its
  neighbours in the same column are ~1e-17), so no kernel can match it; AllegroKuka has 1 such entry per env here
  (for one, iiwa7_link_4 in joint 3's column, z row), where the device gives 8.4e-9, and the atol above still holds there.
* mass matrix: max|M - M_ref| / max|M_ref| <= 3e-5 (the closed-form bound of _check_step) and
  max_ij |M - M_ref|_ij / sqrt(M_ref,ii M_ref,jj) <= 2e-3 (4x what a float32 world-origin composite recursion loses
  on the Ur5Sih finger-tip entries); exactly symmetric; M[d, d] >= armature[d].
* J qd against the rigid-body rows: 1e-5 ||qd||_1 + 3e-6.
The device reaches (MI355X, the cases below): Jacobian max error 1.7e-6 (AllegroKuka; 5e-7 for the other two), M
1.2e-6 of max|M| and 6.9e-6 of sqrt(M_ii M_jj), J qd against the body rows 1.1% of its tolerance, the DLS loop
3.8e-8 m."""
import copy
import functools

import numpy as np
import pytest
import torch

from handarm_hip import _lib
from handarm_hip import model as HM
from tests.jacobian_ref import cancellation_mask, jacobian_tensor
from tests.kinematics import Chain
from tests.test_independent_dynamics import ROBOTS, _fill

pytestmark = pytest.mark.gpu
ASSET = dict(ROBOTS)
CASES = [(task, n) for task, _ in ROBOTS for n in (5, 1)]


def _make_sim(task, n, seed, cfg=None):
    """A sim of the task's robot with the case's joint state written into its tensors; (sim, q, qd) float32."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from handarm_hip.sim import HandArmSim
    from oracle.oracle_lib import HostState
    sim = HandArmSim(n, "cuda:0", task_cfg=dict(cfg or {}, task=task), task=task)
    m, p = sim.model, sim.params
    D = m.n_dofs
    st = HostState(n, model=m, params=p)
    for k in HM.STATE_FIELDS:
        if k not in HM.null_fields(task) and k not in ("stats", "term_sums"):
            st[k][...] = sim.t[k].cpu().numpy().reshape(st[k].shape)
    rng = np.random.default_rng(seed)
    q = (np.array(list(p.reset_pose)[:D]) + rng.uniform(-0.3, 0.3, (n, D))).astype(np.float32)
    qd = rng.uniform(-1, 1, (n, D)).astype(np.float32)
    _fill(st, m, p, q, qd, q)
    for k in ("root_state", "dof_state", "sim_targets", "collision_enabled", "object_scale"):
        if k not in HM.null_fields(task):
            sim.t[k].copy_(torch.as_tensor(st[k]).reshape(sim.t[k].shape).to(sim.t[k].dtype))
    return sim, q, qd


@functools.lru_cache(maxsize=None)
def _case(task, n):
    """One sim per (robot, N): both tensors acquired, overwritten with NaN, refreshed by ONE call; and the float64
    references, computed once."""
    sim, q, qd = _make_sim(task, n, seed=20 + task)
    jac, mm = sim.acquire_jacobian_tensor(), sim.acquire_mass_matrix_tensor()
    assert sim.acquire_jacobian_tensor() is jac and sim.acquire_mass_matrix_tensor() is mm
    first = jac.cpu().numpy().copy(), mm.cpu().numpy().copy()          # what the acquires themselves filled in
    jac.fill_(float("nan"))
    mm.fill_(float("nan"))
    sim.refresh_jacobian_tensors()                                     # both are acquired: one launch writes both
    torch.cuda.synchronize()
    ch = Chain(HM.load_scene(ASSET[task]))
    q64 = q.astype(np.float64)
    return dict(sim=sim, q=q, qd=qd, chain=ch, J=jac.cpu().numpy().copy(), M=mm.cpu().numpy().copy(), first=first,
                J_ref=np.stack([jacobian_tensor(ch, q64[e]) for e in range(n)]),
                lucky=np.stack([cancellation_mask(ch, q64[e]) for e in range(n)]),
                M_ref=np.stack([ch.mass_matrix(q64[e]) for e in range(n)]))


def _check_mass_matrix(M, M_ref, armature, tag):
    for e in range(M.shape[0]):
        err = np.abs(M[e] - M_ref[e])
        e_max = err.max() / np.abs(M_ref[e]).max()
        dg = np.sqrt(np.diag(M_ref[e]))
        e_rel = (err / np.outer(dg, dg)).max()
        print(f"{tag} env {e}: M err / max|M| {e_max:.2e}, err / sqrt(Mii Mjj) {e_rel:.2e}")
        assert e_max <= 3e-5 and e_rel <= 2e-3, f"{tag} env {e}: {e_max:.2e} of max|M|, {e_rel:.2e} of sqrt(Mii Mjj)"
        assert np.array_equal(M[e], M[e].T), f"{tag} env {e}: M is not exactly symmetric"
        assert (np.diag(M[e]) >= armature).all(), f"{tag} env {e}: diagonal below the armature"


@pytest.mark.parametrize("task,n", CASES)
def test_jacobian_matches_float64_reference(task, n):
    c = _case(task, n)
    sim, J, J_ref = c["sim"], c["J"], c["J_ref"]
    assert J.shape == (n, sim.num_links - 1, 6, sim.num_dofs) and J.dtype == np.float32
    assert np.isfinite(J).all(), "refresh left elements of the NaN-filled tensor unwritten"
    err = np.abs(J - J_ref).max()
    print(f"task {task} N {n}: Jacobian max abs err {err:.2e}")
    assert err <= 1e-5, f"task {task}: Jacobian max abs err {err:.2e}"
    zero = (J_ref == 0.0) & ~c["lucky"]
    luck = np.abs(J[c["lucky"] & (J_ref == 0.0)])
    print(f"task {task} N {n}: {zero.sum()} exact zeros of the reference, {luck.size} more by cancellation"
          f"{f' (device: up to {luck.max():.1e} there)' if luck.size else ''}")
    assert zero.any() and (J[zero] == 0.0).all(), "an exact zero of the reference is not exactly 0.0"
    np.testing.assert_array_equal(c["first"][0], J)                   # acquire filled it for the same dof_state


@pytest.mark.parametrize("task,n", CASES)
def test_mass_matrix_matches_chain(task, n):
    c = _case(task, n)
    sim, M = c["sim"], c["M"]
    assert M.shape == (n, sim.num_dofs, sim.num_dofs) and M.dtype == np.float32
    assert np.isfinite(M).all(), "refresh_jacobian_tensors left the acquired mass matrix unwritten"
    arm = np.array(list(sim.model.dof_armature)[:sim.num_dofs], np.float32)
    np.testing.assert_allclose(arm, c["chain"].armature, rtol=1e-7)
    _check_mass_matrix(M, c["M_ref"], arm, f"task {task} N {n}")
    np.testing.assert_array_equal(c["first"][1], M)


def _subset_links(chain):
    names = [l["name"] for l in chain.links]
    arm_end = next((names.index(k) for k in ("flange", "iiwa7_link_7") if k in names), 1)
    return [arm_end, chain.L - 1]


@pytest.mark.parametrize("task,asset", ROBOTS)
def test_link_subset_equals_full_tensor_slices(task, asset):
    c = _case(task, 5)
    links = _subset_links(c["chain"])
    sim, _, _ = _make_sim(task, 5, seed=20 + task)                     # the same joint state as the full-tensor sim
    sub = sim.acquire_jacobian_tensor(links=links)
    assert sub.shape == (5, 2, 6, sim.num_dofs) and sim.acquire_jacobian_tensor(links=links) is sub
    sub.fill_(float("nan"))
    sim.refresh_jacobian_tensors()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(sub.cpu().numpy(), c["J"][:, [i - 1 for i in links]])
    with pytest.raises(_lib.HandArmError):
        sim.acquire_jacobian_tensor()                                  # one Jacobian tensor per sim
    with pytest.raises(_lib.HandArmError):
        _make_sim(task, 1, seed=0)[0].acquire_jacobian_tensor(links=[0])


def test_dr_link_masses_scale_the_mass_matrix():
    task, n = HM.TASK_ALLEGRO_HAND, 5
    scene = HM.load_scene(ASSET[task])
    L = len(scene["robot"]["links"])
    fac = np.random.default_rng(7).uniform(0.5, 1.5, (n, L)).astype(np.float32)
    refs = []
    for e in range(n):
        s = copy.deepcopy(scene)
        for i, l in enumerate(s["robot"]["links"]):
            l["mass"] = float(l["mass"]) * float(fac[e, i])
            l["inertia"] = (np.asarray(l["inertia"], np.float64) * float(fac[e, i])).tolist()
        refs.append(Chain(s))
    for dr in (1, 0):
        sim, q, _ = _make_sim(task, n, seed=31, cfg={"dr_enable": dr})
        sim.t["dr_scale"][:, HM.DR_LINK_MASS:HM.DR_LINK_MASS + L] = torch.as_tensor(fac).to(sim.device)
        mm = sim.acquire_mass_matrix_tensor()
        mm.fill_(float("nan"))
        sim.refresh_mass_matrix_tensors()
        torch.cuda.synchronize()
        chains = refs if dr else [Chain(scene)] * n
        M_ref = np.stack([chains[e].mass_matrix(q[e].astype(np.float64)) for e in range(n)])
        arm = np.array(list(sim.model.dof_armature)[:sim.num_dofs], np.float32)
        _check_mass_matrix(mm.cpu().numpy(), M_ref, arm, f"dr_enable {dr}")


@pytest.mark.parametrize("task,asset", ROBOTS)
def test_jacobian_times_qd_equals_body_velocities(task, asset):
    """refresh_* of the state tensors copy nothing (the kernels write them at the end of a launch), so one gym.simulate
    brings rigid_body_state and dof_state to the same instant; the Jacobian refreshed from that dof_state must then
    reproduce the links' angular (10:13) and COM (7:10) velocities."""
    n = 5
    sim, _, _ = _make_sim(task, n, seed=40 + task)
    jac = sim.acquire_jacobian_tensor()
    sim.simulate(1)
    sim.refresh_rigid_body_state_tensor()
    sim.refresh_jacobian_tensors()
    torch.cuda.synchronize()
    m, D, L = sim.model, sim.num_dofs, sim.num_links
    J = jac.cpu().numpy().astype(np.float64)
    qd = sim.t["dof_state"].cpu().numpy().reshape(n, D, 2)[..., 1].astype(np.float64)
    rb = sim.t["rigid_body_state"].cpu().numpy().reshape(n, m.n_bodies, 13)[:, m.body_robot0:m.body_robot0 + L]
    rb = rb.astype(np.float64)
    from tests.kinematics import quat_matrix
    worst = 0.0
    for e in range(n):
        tol = 1e-5 * np.abs(qd[e]).sum() + 3e-6
        for i in range(1, L):
            w = J[e, i - 1, 3:6] @ qd[e]
            com = quat_matrix(rb[e, i, 3:7]) @ np.array(list(m.link_com[i]), np.float64)
            v = J[e, i - 1, 0:3] @ qd[e] + np.cross(w, com)
            err = max(np.abs(w - rb[e, i, 10:13]).max(), np.abs(v - rb[e, i, 7:10]).max())
            worst = max(worst, err / tol)
            assert err <= tol, f"task {task} env {e} link {i}: {err:.2e} > {tol:.2e}"
    print(f"task {task}: worst J qd error / tolerance {worst:.2e}")


def test_damped_least_squares_reach_through_gym_api():
    """A kinematic DLS loop on the Ur5Sih arm through gym_api: dq = J^T (J J^T + 0.05^2 I)^-1 e on the 6 arm DOFs with the
    flange's linear rows of gym.acquire_jacobian_tensor, dof_state written directly, no simulate (no joint limits).
    The refresh_* calls of the state tensors copy nothing here and only a launch of the physics rewrites
    rigid_body_state, so without simulate the flange position comes from the float64 Chain.fk of the dof_state just
    written: the loop converges only if the device Jacobian is the derivative of that independent FK. 5 cm goals, 30
    iterations, final error < 1e-4 m (the float64 reference loop reaches 2e-16 m)."""
    from handarm_hip.gym_api import acquire_gym
    n, task = 4, HM.TASK_UR5SIH
    sim, q, _ = _make_sim(task, n, seed=50)
    ch = Chain(HM.load_scene(ASSET[task]))
    flange = [l["name"] for l in ch.links].index("flange")
    D = sim.num_dofs
    rng = np.random.default_rng(51)
    q = np.tile(np.array(list(sim.params.reset_pose)[:D], np.float32), (n, 1))
    dirs = rng.standard_normal((n, 3))
    goal = np.stack([ch.fk(q[e].astype(np.float64))[1][flange] for e in range(n)]) + \
        0.05 * dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    gym = acquire_gym()
    dof = gym.acquire_dof_state_tensor(sim).view(n, D, 2)
    dof[..., 0] = torch.as_tensor(q).to(sim.device)
    dof[..., 1] = 0.0
    jac = gym.acquire_jacobian_tensor(sim, "robot")
    assert jac.shape == (n, sim.num_links - 1, 6, D)
    for _ in range(30):
        gym.refresh_rigid_body_state_tensor(sim)
        gym.refresh_jacobian_tensors(sim)
        qc = dof[..., 0].cpu().numpy()
        pos = np.stack([ch.fk(qc[e].astype(np.float64))[1][flange] for e in range(n)])
        e_ = torch.as_tensor(goal - pos, dtype=torch.float32, device=sim.device).unsqueeze(-1)
        Jl = jac[:, flange - 1, 0:3, 0:6]
        A = Jl @ Jl.transpose(1, 2) + 0.05 ** 2 * torch.eye(3, device=sim.device)
        dof[:, 0:6, 0] += (Jl.transpose(1, 2) @ torch.linalg.solve(A, e_)).squeeze(-1)
    qc = dof[..., 0].cpu().numpy()
    err = np.linalg.norm(goal - np.stack([ch.fk(qc[e].astype(np.float64))[1][flange] for e in range(n)]), axis=1)
    print(f"DLS final flange error {err.max():.2e} m")
    assert err.max() < 1e-4, f"DLS final flange error {err.max():.2e} m"


def test_refresh_before_acquire_raises():
    from handarm_hip.gym_api import acquire_gym
    sim, _, _ = _make_sim(HM.TASK_ALLEGRO_HAND, 1, seed=0)
    with pytest.raises(_lib.HandArmError):
        sim.refresh_jacobian_tensors()
    with pytest.raises(_lib.HandArmError):
        sim.refresh_mass_matrix_tensors()
    with pytest.raises(_lib.HandArmError):
        acquire_gym().refresh_mass_matrix_tensors(sim)
    sim.acquire_mass_matrix_tensor()
    sim.refresh_mass_matrix_tensors()
    with pytest.raises(_lib.HandArmError):
        sim.refresh_jacobian_tensors()                                 # only the mass matrix is acquired
