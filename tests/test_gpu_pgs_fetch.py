"""The PGS fetch's per-contact descriptor (AllegroKuka), bit for bit against the C oracle.

A fetch of ak_step_kernel reads one descriptor word per contact, built once per substep: the byte offset of the
contact's object block and of its robot block, each with the place it lives in (LDS, the env's global area, or no
robot block at all). Lanes without an entry read a zero pad in LDS. ak_simulate_kernel keeps the link-slot register.
Both kernels must give the oracle's bits on scenes whose contact lists reach every descriptor case.

64 envs: tests/test_gpu_pgs_sweep.py kuka_sweep_scene (finger closure from open to closed, the cuboid in or over the
palm, three envs with the open hand clear of a cuboid that hangs, lies flat or stands on an edge on the table), and in
the last eight envs the closed hand keeps its self contacts while the cuboid lies on the table (flat: 4 contacts, on an
edge: 2). The oracle's own contact lists must show, before anything runs on the GPU,

* (a) a contact that touches no link (cuboid on table),
* (b) link contacts whose robot block is in an LDS slot (the first 9 link contacts of a substep),
* (c) an env with more than 9 link contacts (robot blocks from the global spill rows),
* (d) an env with more than 21 contacts (object blocks from the global row area), also one whose contacts past 21
  include spill-row robot blocks (both global sources in one fetch) and one with the full 42,
* (e) the cases changing inside one trip of three (the sweep's unroll): a trip that holds a no-link and an LDS-slot
  contact and a trip that holds an LDS-slot and a spill-row contact, in the same substep. A single trip with all
  three cannot occur in this family: detect lists the cuboid's table contacts before every link contact (pair_desc),
  and the slots follow the list's order, so nine LDS-slot contacts always lie between a no-link and a spill-row one;
* (f) no contact index reaches 64 (the capacity is 42): asserted, so that a larger capacity brings the case up.

The test fails if the scene does not give them. contact_stats must equal the oracle's after the run.
"""
import numpy as np
import pytest
import torch

from handarm_hip import model as HM
from oracle import kuka_oracle as KO
from tests import scenes, step_chains
from tests.test_gpu_fused_steps import exact, get, near, pull_all, push_all, put
from tests.test_gpu_pgs_sweep import TABLE_TOP, kuka_sweep_scene

pytestmark = pytest.mark.gpu
N = 64
KL, CHUNK, CAPACITY = 9, 21, 42       # LDS link slots, contacts of chunk 0 (object blocks in LDS), contact capacity


def fetch_scene(sim, hs, lo, up):
    """kuka_sweep_scene; in the last eight envs the cuboid leaves the (nearly closed) hand for the table: flat in the
    even envs, on one edge in the odd ones (the placements of that scene's envs 5 and 6)."""
    n, m = sim.num_envs, sim.model
    kuka_sweep_scene(sim, hs, lo, up)
    rs = hs["root_state"].reshape(n, m.n_actors, 13)
    obj = m.actor_object0
    half = 0.025 * hs["object_scale"].reshape(n, -1, 3)[:, 0]
    s = np.float32(np.sqrt(0.5))
    for e in range(n - 8, n):
        if e % 2 == 0:
            rs[e, obj, 0:3] = [0.12, -0.09, TABLE_TOP + half[e, 2] + 0.001]
            rs[e, obj, 3:7] = [0, 0, 0, 1]
        else:
            rs[e, obj, 0:3] = [0.12, -0.09, TABLE_TOP + (half[e, 1] + half[e, 2]) * s + 0.001]
            rs[e, obj, 3:7] = [np.sin(np.pi / 8), 0, 0, np.cos(np.pi / 8)]


def contact_kinds(orc, hs, e):
    """The descriptor case of each contact the env's first substep keeps: n (no link), l (LDS slot), s (spill row)."""
    c = orc.contacts(hs, e)[:CAPACITY]
    a, b = c[:, 7].astype(int), c[:, 8].astype(int)
    link = (a >= 100) | (b >= 100)
    slot = np.cumsum(link) - 1
    return "".join("n" if not k else ("l" if t < KL else "s") for k, t in zip(link, slot))


def check_descriptor_cases(orc, hs):
    kinds = [contact_kinds(orc, hs, e) for e in range(N)]
    offered = [len(orc.contacts(hs, e)) for e in range(N)]
    trips = [[k[i:i + 3] for i in range(0, len(k), 3)] for k in kinds]
    print("fetch scene, contact kinds per env:", kinds)
    assert any("n" in k for k in kinds), "(a) no contact without a link"
    assert any("l" in k for k in kinds), "(b) no link contact in an LDS slot"
    assert any("s" in k for k in kinds), "(c) no env with more than 9 link contacts"
    assert any(len(k) > CHUNK for k in kinds), "(d) no env with more than 21 contacts"
    assert any("s" in k[CHUNK:] for k in kinds), "(d) no spill-row robot block among the contacts past 21"
    assert any(len(k) == CAPACITY for k in kinds) and max(offered) >= CAPACITY, "(d) no env fills the capacity"
    assert any("n" in k and "l" not in k for k in kinds), "(a) no env with no-link contacts only"
    assert any(any("n" in t and "l" in t for t in ts) and any("l" in t and "s" in t for t in ts) for ts in trips), \
        "(e) no substep with a no-link / LDS-slot trip and an LDS-slot / spill-row trip"
    assert max(len(k) for k in kinds) <= 64, "(f) a contact index reaches 64: the second descriptor register is in use"


def _scene():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from handarm_hip.sim import HandArmSim
    from oracle.oracle_lib import HostState, Oracle
    sim = HandArmSim(N, "cuda:0", task_cfg={"task": HM.TASK_ALLEGRO_KUKA, "subtask": "regrasping"},
                     task=HM.TASK_ALLEGRO_KUKA)
    assert sim.contact_capacity == CAPACITY
    m, p = sim.model, sim.params
    lo = np.array(m.dof_lower[:23], np.float32)
    up = np.array(m.dof_upper[:23], np.float32)
    hs = HostState(N, model=m, params=p)
    pull_all(sim, hs)                   # object dims, task-state keypoints, scalars
    fetch_scene(sim, hs, lo, up)
    hs["object_force"][:] = 0
    hs["contact_stats"][:] = 0
    orc = Oracle(m, p, N)
    check_descriptor_cases(orc, hs)
    push_all(sim, hs)
    return sim, hs, orc, lo, up


def _stats_equal(sim, hs):
    g = get(sim, "contact_stats").reshape(hs["contact_stats"].shape)
    assert (g[:, :6] == hs["contact_stats"][:, :6]).all(), "contact statistics differ from the oracle's"
    assert g[:, 2].max() >= CAPACITY, "no substep of the run offered a full contact list"


@pytest.mark.parametrize("calls", [1, 4])
def test_fetch_scene_simulate_matches_oracle_bit_for_bit(calls):
    """ak_simulate_kernel, `calls` gym.simulate calls in one launch, every physics output bit-identical."""
    sim, hs, orc, _, _ = _scene()
    sim.simulate(calls)
    orc.simulate(hs, calls)
    scenes.assert_physics_bit_identical(sim, hs, N, tag=f"fetch scene, {calls} calls")
    _stats_equal(sim, hs)


def test_fetch_scene_fused_step_io_matches_oracle_chain():
    """ak_step_kernel (the descriptor fetch) through ha_task_step_io: two steps with the fingers driven further closed,
    against kuka_oracle.pre -> physics_oracle -> kuka_oracle.post. Physics outputs and the step's buffers bit-exact;
    observations and rewards within 1e-4 (the bound of tests/test_gpu_pgs_sweep.py: their float32 arithmetic differs
    in order from numpy's)."""
    sim, hs, orc, lo, up = _scene()
    p = sim.params
    rng = np.random.default_rng(29)
    hs["dof_position_targets"][:] = hs["sim_targets"]
    hs["reset_buf"][:] = 0
    hs["reset_goal_buf"][:] = 0
    hs["progress_buf"][:] = rng.integers(1, 50, N)
    hs["task_state"][:, HM.AK_FORCE_PROB] = 0.0
    scalars = hs["task_scalars"].copy()
    push_all(sim, hs)
    clip_act, clip_obs = 1.0, 5.0
    ds = KO.draw_slots(p)
    out = torch.zeros((N, p.num_obs), device="cuda:0")
    for t in range(2):
        act = np.zeros((N, 23), np.float32)
        act[:, 7:] = rng.uniform(0.6, 1.0, (N, 16))
        draws = rng.uniform(0, 1, (N, HM.DRAW_STRIDE)).astype(np.float32)
        draws[:, ds["FORCE_N"]:ds["FORCE_N"] + 3] = rng.standard_normal((N, 3))
        hs["actions"][:] = act
        hs["reset_draws"][:] = draws
        put(sim, "reset_draws", draws)
        sim.task_step_io(HM.FLAG_REPLAY_DRAWS, torch.from_numpy(act).cuda(), clip_act, out, clip_obs)
        obs, rew, timeout = step_chains.kuka_step(orc, hs, p, lo, up, scalars, draws)
        tag = f"fetch scene step_io {t}"
        scenes.assert_physics_bit_identical(sim, hs, N, tag=tag)
        exact(sim, hs, ["actions", "dof_position_targets", "sim_targets", "goal_state", "reset_buf", "reset_goal_buf",
                        "progress_buf", "successes"], tag)
        assert (get(sim, "timeout_buf").astype(bool) == timeout).all(), tag
        eo = near(get(sim, "obs"), obs, 1e-4, tag + " obs")
        er = near(get(sim, "rew"), rew, 1e-4, tag + " rew")
        torch.cuda.synchronize()
        near(out.cpu().numpy(), np.clip(obs, -clip_obs, clip_obs), 1e-4, tag + " returned obs")
        print(f"{tag}: obs max |d| {eo:.2e}, rew max |d| {er:.2e}")
    _stats_equal(sim, hs)
