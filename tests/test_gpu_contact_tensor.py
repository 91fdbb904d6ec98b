"""The contact tensor (ha_refresh_contacts, one query kernel per family) on the GPU: bit identity with the C oracle's
contact list in all four kernel families, the query leaving the simulation untouched, the bounds of what it writes, the
body indices and local points against rigid_body_state, the independent float64 checker (tests/contact_ref.py) on the
kernel's rows, and the argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from handarm_hip import gym_api
from handarm_hip import model as HM
from tests import contact_ref as CR
from tests import scenes

pytestmark = pytest.mark.gpu


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def put(sim, name, arr):
    t = sim.t[name]
    t.copy_(torch.as_tensor(np.ascontiguousarray(arr)).reshape(t.shape).to(t.dtype))


def push(sim, st):
    for k in HM.STATE_FIELDS:
        if k in ("stats", "term_sums") or k in HM.null_fields(sim.task):
            continue
        put(sim, k, st[k])


def query(sim, env_ids=None):
    rows, counts = sim.acquire_contact_tensor()
    sim.refresh_contact_tensor(env_ids)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), counts.cpu().numpy()


def oracle_rows(sim, st):
    from oracle.oracle_lib import Oracle
    orc = Oracle(sim.model, sim.params, sim.num_envs)
    return [orc.contacts(st, e) for e in range(sim.num_envs)]


def assert_rows_match(sim, st, tag):
    """rows[:kept, :9] of every env bit-identical to the oracle's list, kept == its length; returns both."""
    rows, counts = query(sim)
    ref = oracle_rows(sim, st)
    assert counts.shape == (sim.num_envs, 2) and rows.shape == (sim.num_envs, sim.contact_capacity, 20)
    for e, r in enumerate(ref):
        assert counts[e, 0] == len(r), f"{tag} env {e}: kept {counts[e, 0]}, oracle {len(r)}"
        assert counts[e, 1] >= counts[e, 0]
        g = np.ascontiguousarray(rows[e, :len(r), :9])
        assert (g.view(np.uint32) == np.ascontiguousarray(r).view(np.uint32)).all(), f"{tag} env {e}: rows differ"
    return rows, counts, ref


# ----------------------------------------------------------------------------- the four families' states
def ur5sih_pile():
    """The pile-in-hand state (tests/contact_ref.py ur5sih_hand_pile) on a sim."""
    need_gpu()
    from handarm_hip.sim import HandArmSim
    n = 64
    st = CR.ur5sih_hand_pile(n)[3]
    sim = HandArmSim(n, "cuda:0")
    assert sim.contact_capacity == 84
    push(sim, st)
    return sim, st


def allegro_closing_hand():
    need_gpu()
    from handarm_hip.sim import HandArmSim
    n = 128
    st = CR.allegro_closing_hand(n)[3]
    sim = HandArmSim(n, "cuda:0", task=HM.TASK_ALLEGRO_HAND)
    assert sim.contact_capacity == 48
    push(sim, st)
    return sim, st


def kuka_closed_hand(n=128):
    need_gpu()
    from handarm_hip.sim import HandArmSim
    st = CR.kuka_closed_hand(n)[3]
    sim = HandArmSim(n, "cuda:0", task=HM.TASK_ALLEGRO_KUKA)
    assert sim.contact_capacity == 42
    assert (st["object_scale"] == sim.t["object_scale"].cpu().numpy().reshape(st["object_scale"].shape)).all()
    push(sim, st)
    return sim, st


def clutter_bin(n=16):
    need_gpu()
    from handarm_hip.sim import HandArmSim
    from oracle.oracle_lib import HostState
    sim = HandArmSim(n, "cuda:0", task_cfg={"n_objects": 8}, scene=HM.load_scene(HM.BIN_ASSET))
    assert sim.contact_capacity == 84
    st = HostState(n, model=sim.model, params=sim.params)
    scenes.fill_bin_scene(st, n, sim.scene, seed=0, n_obj=8)
    push(sim, st)
    return sim, st


def advance(sim, st, calls):
    from oracle.oracle_lib import Oracle
    sim.simulate(calls)
    Oracle(sim.model, sim.params, sim.num_envs).simulate(st, calls)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 1. bit identity with the oracle
def test_ur5sih_pile_rows_match_oracle_with_overflow_entries_and_give_way():
    sim, st = ur5sih_pile()
    rows, counts, ref = assert_rows_match(sim, st, "ur5sih pile")
    ln = np.array([len(r) for r in ref])
    print(f"ur5sih pile: oracle rows per env min {ln.min()} mean {ln.mean():.1f} max {ln.max()}, offered max "
          f"{counts[:, 1].max()}, envs over capacity {(counts[:, 1] > counts[:, 0]).sum()}")
    assert (ln > 21).all(), "every env must reach the overflow entries (past chunk 0's 21)"
    assert abs(ln.mean() - 76) < 1 and ln.max() == 84
    assert (counts[:, 1] > counts[:, 0]).any(), "some env must be over capacity (the give-way rule)"
    advance(sim, st, 2)
    assert_rows_match(sim, st, "ur5sih pile after 2 calls")


def test_allegro_hand_closing_hand_rows_match_oracle():
    sim, st = allegro_closing_hand()
    _, _, ref = assert_rows_match(sim, st, "allegro closing hand")
    ln = np.array([len(r) for r in ref])
    print(f"allegro closing hand: envs over 12 rows {(ln > 12).mean():.2f}, max {ln.max()}")
    assert (ln > 12).mean() >= 0.5 and ln.max() == 48


def test_kuka_closed_hand_rows_match_oracle_with_self_rows_and_scaled_cuboids():
    sim, st = kuka_closed_hand()
    _, _, ref = assert_rows_match(sim, st, "kuka closed hand")
    ln = np.array([len(r) for r in ref])
    self_rows = np.array([((r[:, 7] >= 100) & (r[:, 8] >= 100)).sum() for r in ref])
    print(f"kuka closed hand: rows per env max {ln.max()}, envs over 21 {(ln > 21).sum()}, envs with self rows "
          f"{(self_rows > 0).sum()}")
    assert (self_rows > 0).any(), "self-collision rows (both codes >= 100)"
    assert (ln > 21).any(), "some env past chunk 0's 21 entries"
    assert np.ptp(st["object_scale"].reshape(sim.num_envs, -1), axis=0).max() > 0, "per-env cuboid dimensions"
    advance(sim, st, 2)
    assert_rows_match(sim, st, "kuka closed hand after 2 calls")


def test_clutter_bin_rows_match_oracle():
    sim, st = clutter_bin()
    _, _, ref = assert_rows_match(sim, st, "clutter bin")
    codes = np.concatenate([r[:, 7:9] for r in ref])
    multi = [i for i, o in enumerate(sim.scene["objects"]) if len(o.get("hulls") or []) > 1]
    ids = st["object_indices"].reshape(sim.num_envs, 8)
    compound = 0
    for e, r in enumerate(ref):
        c = r[:, 7:9]
        compound += int(np.isin(ids[e, c[(c >= 0) & (c < 100)].astype(int)], multi).sum())
    print(f"clutter bin: {len(codes)} rows, {int((codes == -1).any(1).sum())} with a static, {compound} body entries "
          f"of compound objects")
    assert (codes == -1).any() and compound > 0, "tote statics and compound (multi-piece) objects"


# ----------------------------------------------------------------------------- 2. the query perturbs nothing
@pytest.mark.parametrize("family", ["clutter", "kuka"])
def test_query_between_simulate_calls_changes_nothing(family):
    make = (lambda: clutter_bin(16)) if family == "clutter" else (lambda: kuka_closed_hand(64))
    (A, _), (B, _) = make(), make()
    B.acquire_contact_tensor()
    force = "object_force" not in HM.null_fields(A.task)
    rng = np.random.default_rng(4)
    for step in range(3):
        if force:
            f = (0.5 * rng.standard_normal(tuple(A.t["object_force"].shape))).astype(np.float32)
            put(A, "object_force", f)
            put(B, "object_force", f)
        before = {k: v.clone() for k, v in B.t.items()}
        B.refresh_contact_tensor()
        torch.cuda.synchronize()
        for k, v in before.items():
            assert v.cpu().numpy().tobytes() == B.t[k].cpu().numpy().tobytes(), f"the query wrote {k} (step {step})"
        A.simulate(1)
        B.simulate(1)
        torch.cuda.synchronize()
        for k in scenes.PHYSICS_OUTPUTS + ("contact_stats",):
            if k in HM.null_fields(A.task):
                continue
            a, b = A.t[k].cpu().numpy(), B.t[k].cpu().numpy()
            assert (a.view(np.uint8) == b.view(np.uint8)).all(), f"{family} step {step}: {k} differs after a query"
        if force:       # handed in before the query, consumed by the simulate after it
            assert not B.t["object_force"].any()
    if force:
        free = make()[0]
        free.simulate(3)
        torch.cuda.synchronize()
        assert not torch.equal(free.t["root_state"], B.t["root_state"]), "the forces must have acted"


# ----------------------------------------------------------------------------- 3. bounds of the write
def test_write_bounds_env_ids_and_one_env():
    sim, st = ur5sih_pile()
    n, cap = sim.num_envs, sim.contact_capacity
    rows_t, counts_t = sim.acquire_contact_tensor()
    rows_t.fill_(float("nan"))
    counts_t.fill_(-7)
    full, fc = query(sim)
    slot = np.arange(cap)[None, :] < fc[:, 0:1]
    assert (fc[:, 0] >= 0).all() and (fc[:, 0] <= cap).all() and (fc[:, 0] < cap).any()
    assert np.isfinite(full[slot]).all(), "rows < kept"
    assert np.isnan(full[~slot]).all(), "rows >= kept must not be written"
    assert (full[slot][:, 17:20] == 0).all(), "reserved floats"
    # five unsorted envs of 64: the others keep the prefill
    rows_t.fill_(float("nan"))
    counts_t.fill_(-7)
    ids = [41, 3, 63, 17, 20]
    part, pc = query(sim, torch.tensor(ids, dtype=torch.int32, device=sim.device))
    listed = np.isin(np.arange(n), ids)
    assert (pc[listed] == fc[listed]).all() and (pc[~listed] == -7).all()
    assert np.isnan(part[~listed]).all()
    same = (part[listed].view(np.uint32) == full[listed].view(np.uint32)) | ~slot[listed][..., None]
    assert same.all() and np.isnan(part[listed][~slot[listed]]).all()
    # a single env
    from handarm_hip.sim import HandArmSim
    one = HandArmSim(1, "cuda:0")
    for k in ("root_state", "dof_state", "sim_targets", "object_indices", "collision_enabled"):
        put(one, k, np.asarray(st[k]).reshape(n, -1)[5:6])
    r1, c1 = query(one)
    assert (c1[0] == fc[5]).all()
    assert (r1[0, :c1[0, 0]].view(np.uint32) == full[5, :c1[0, 0]].view(np.uint32)).all()


# ----------------------------------------------------------------------------- 4. body indices and local points
def _rot(q):
    x, y, z, w = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


@pytest.mark.parametrize("family", ["ur5sih", "kuka", "clutter"])
def test_body_indices_and_local_points_against_rigid_body_state(family):
    """Link and object frames (ur5sih, kuka with per-env cuboid scales) and static rows, compound objects (clutter)."""
    sim, st = {"ur5sih": ur5sih_pile, "kuka": kuka_closed_hand, "clutter": clutter_bin}[family]()
    sim.simulate(1)                     # rigid_body_state is current after a simulate
    rows, counts = query(sim)
    body = sim.t["rigid_body_state"].cpu().numpy().reshape(sim.num_envs, sim.num_bodies, 13).astype(np.float64)
    m = sim.model
    env, slot = np.nonzero(np.arange(rows.shape[1])[None, :] < counts[:, 0:1])
    r = rows[env, slot].astype(np.float64)
    assert len(r) > (100 if family == "clutter" else 1000)

    def expect(code):
        return np.where(code < 0, -1, np.where(code >= 100, m.body_robot0 + code - 100, m.body_object0 + code))

    world = []
    for side, (cc, bc, lc) in enumerate(((7, 9, slice(11, 14)), (8, 10, slice(14, 17)))):
        code, b = r[:, cc].astype(int), r[:, bc].astype(int)
        np.testing.assert_array_equal(b, expect(code))
        assert (b < sim.num_bodies).all()
        pose = body[env, np.maximum(b, 0), 0:7]
        pose[b < 0] = [0, 0, 0, 0, 0, 0, 1]                 # a static's frame is the env frame
        world.append(np.einsum("kij,kj->ki", _rot(pose[:, 3:7]), r[:, lc]) + pose[:, 0:3])
    assert ((r[:, [7, 8]] >= 0) & (r[:, [7, 8]] < 100)).any()
    assert (r[:, 8] < 0).any() if family == "clutter" else (r[:, [7, 8]] >= 100).any(), "static rows / link rows"
    e1 = np.abs((world[0] - world[1]) - r[:, 3:6] * r[:, 6:7]).max()
    e2 = np.abs(0.5 * (world[0] + world[1]) - r[:, 0:3]).max()
    print(f"{family}: {len(r)} rows, |pa - pb - n sep| {e1:.2e}, |midpoint - x| {e2:.2e}")
    assert e1 <= 1e-5 and e2 <= 1e-5
    # gym.get_rigid_contacts: the same records
    g = gym_api.Gym()
    rc = g.get_rigid_contacts(sim)
    assert len(rc) == counts[:, 0].sum()
    np.testing.assert_array_equal(rc["env0"], env)
    np.testing.assert_array_equal(rc["body0"], r[:, 9].astype(np.int32))
    np.testing.assert_array_equal(rc["body1"], r[:, 10].astype(np.int32))
    np.testing.assert_array_equal(rc["minDist"], rows[env, slot][:, 6])
    np.testing.assert_array_equal(rc["normal"], rows[env, slot][:, 3:6])
    np.testing.assert_array_equal(rc["localPos0"], rows[env, slot][:, 11:14])
    np.testing.assert_array_equal(rc["localPos1"], rows[env, slot][:, 14:17])
    e = int(np.argmax(counts[:, 0]))
    one = g.get_env_rigid_contacts(sim, e)
    assert len(one) == counts[e, 0] and (one["env0"] == e).all()
    assert one.tobytes() == rc[rc["env0"] == e].tobytes()


# ----------------------------------------------------------------------------- 5. the float64 checker on the kernel
@pytest.fixture(scope="module")
def box_sim():
    need_gpu()
    from handarm_hip.sim import HandArmSim
    scene = scenes.box_pool_scene(scenes.EDGE_BOXES)
    sim = HandArmSim(256, "cuda:0", scene=scene)
    return sim, CR.SceneRef(scene)


@pytest.mark.parametrize("seed", CR.BOX_SEEDS)
def test_float64_checker_on_the_kernels_rows(box_sim, seed):
    from oracle.oracle_lib import HostState
    sim, ref = box_sim
    n = sim.num_envs
    st = CR.box_pile_state(HostState(n, model=sim.model, params=sim.params), n, seed)
    push(sim, st)
    rows, counts = query(sim)
    rep = CR.Report()
    for e in range(n):
        CR.check_env(ref, sim.model, sim.params, st, e, rows[e, :counts[e, 0]], rep)
    print(f"box pile seed {seed} (kernel rows): {rep}")
    assert rep.rows > 1000 and rep.pairs == 6 * n
    CR.assert_report(rep, margin=float(sim.params.contact_margin))


@pytest.mark.parametrize("name", list(CR.LINK_SCENES))
def test_float64_checker_on_the_kernels_link_rows(name):
    """Link-object, link-static and link-link rows of the kernel against the link hulls posed by the independent FK."""
    need_gpu()
    from handarm_hip.sim import HandArmSim
    make, n = CR.LINK_SCENES[name]
    scene, m, p, st = make(n)
    sim = HandArmSim(n, "cuda:0", task=int(p.task))
    push(sim, st)
    rows, counts = query(sim)
    CR.check_link_scene(name, scene, sim.model, sim.params, st, lambda e: rows[e, :counts[e, 0]], tag=" (kernel rows)")


# ----------------------------------------------------------------------------- 6. errors
def test_argument_errors():
    need_gpu()
    from handarm_hip import _lib
    from handarm_hip.sim import HandArmSim
    sim = HandArmSim(4, "cuda:0")
    with pytest.raises(RuntimeError):
        sim.refresh_contact_tensor()
    cap = sim.contact_capacity
    rows = torch.zeros((4, cap, 20), dtype=torch.float32, device=sim.device)
    counts = torch.zeros((4, 2), dtype=torch.int32, device=sim.device)
    lib = _lib.load()

    def call(k):
        return lib.ha_refresh_contacts(sim.h, C.byref(k), None)

    assert call(HM.HaContacts(rows.data_ptr(), counts.data_ptr(), cap - 1, None, 0)) == -1      # HA_E_ARG
    assert call(HM.HaContacts(None, counts.data_ptr(), cap, None, 0)) == -1
    assert call(HM.HaContacts(rows.data_ptr(), None, cap, None, 0)) == -1
    assert call(HM.HaContacts(rows.data_ptr(), counts.data_ptr(), cap, counts.data_ptr(), 0)) == -1
    assert lib.ha_refresh_contacts(sim.h, None, None) == -1
    assert call(HM.HaContacts(rows.data_ptr(), counts.data_ptr(), cap, None, 0)) == 0
    torch.cuda.synchronize()
    assert (counts.cpu().numpy()[:, 0] >= 0).all()
