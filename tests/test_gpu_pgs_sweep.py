"""The PGS sweep's loop structure, bit for bit against the C oracle.

The contact loop of a sweep is unrolled by three (a contact's row entries live in one of three register sets that
rotate by name, prefetched two contacts ahead), and the joint rows prefetch their row of M^-1. The bit-for-bit suites
pin the arithmetic; these scenes pin the structure: the unroll's remainder, the first and second prefetch with fewer
contacts than the look-ahead, and the rotation across the chunk edge.

AllegroKuka, 32 envs, from tests/test_gpu_fused_steps.py kuka_closed_hand_scene: finger closure and object height vary
per env, from the open hand with the cuboid lifted clear to the fully closed hand on the cuboid in its palm; three
envs keep the hand clear of the cuboid, which rests on the table flat, on an edge, or hangs in the air. The oracle's
own contact lists must show, before anything runs on the GPU,

* an env with 0 contacts, one with 1 or 2, one with 3 or 4 (the cuboid resting on the table),
* among the envs with at most 21 contacts (chunk 0) every residue of the contact count modulo 3, the unroll factor,
* among the envs with more than 21 contacts every residue too, and an env with more than 9 link contacts (robot blocks
  past the LDS link slots, fetched from the global spill rows),
* an env with a DOF within joint_limit_margin of its lower limit and one of its upper (the joint-limit rows);

the test fails if the scene does not give them. Then gym.simulate once and three times in one launch, and two fused
VecTask steps (ha_task_step_io) against the oracle chain, as tests/test_gpu_kuka_contact_solve.py does.

AllegroHand (dense rows, overflow chunks of 12), 32 envs, from the self-collision drives of
tests/test_gpu_self_collision.py: every env is stopped (on the oracle) after its own number of simulate calls on the
way into the finger-finger or thumb-palm press, so the first substep on the GPU offers from none to two chunks of
contacts, with every residue modulo 3 on both sides of the chunk size.
"""
import numpy as np
import pytest
import torch

from handarm_hip import model as HM
from oracle import kuka_oracle as KO
from tests import scenes, step_chains
from tests import self_collision_scenes as SC
from tests.test_gpu_fused_steps import exact, get, kuka_closed_hand_scene, near, pull_all, push_all, put

pytestmark = pytest.mark.gpu
N = 32
UNROLL = 3
TABLE_TOP = 0.53            # the AllegroKuka table's surface (tests/test_kuka_physics.py)


# ----------------------------------------------------------------------------- AllegroKuka
def kuka_sweep_scene(sim, hs, lo, up):
    """kuka_closed_hand_scene with the finger closure going from 0 (env 0: every finger DOF at its lower limit) to 1
    (env N - 1: at its upper limit), the cuboid lifted off the palm by 0 / 2 / 4 cm in turn, and three envs whose open
    hand touches nothing: the cuboid in the air (env 4), flat on the table (env 5), on one edge on the table (env 6)."""
    n, m = sim.num_envs, sim.model
    kuka_closed_hand_scene(sim, hs, lo, up)
    ds = hs["dof_state"].reshape(n, 23, 2)
    frac = (np.arange(n) / (n - 1)).astype(np.float32)
    ds[:, 7:, 0] = lo[7:] + (up[7:] - lo[7:]) * frac[:, None]
    ds[:, :, 1] = 0
    hs["sim_targets"][:] = ds[..., 0]
    hs["sim_targets"][:, 7:] = up[7:]
    rs = hs["root_state"].reshape(n, m.n_actors, 13)
    obj = m.actor_object0
    rs[:, obj, 2] += np.array([0.0, 0.02, 0.04], np.float32)[np.arange(n) % 3]
    half = 0.025 * hs["object_scale"].reshape(n, -1, 3)[:, 0]
    rs[4, obj, 0:3] = [0.12, -0.09, 1.2]
    rs[5, obj, 0:3] = [0.12, -0.09, TABLE_TOP + half[5, 2] + 0.001]
    rs[5, obj, 3:7] = [0, 0, 0, 1]
    s = np.float32(np.sqrt(0.5))
    rs[6, obj, 0:3] = [0.12, -0.09, TABLE_TOP + (half[6, 1] + half[6, 2]) * s + 0.001]
    rs[6, obj, 3:7] = [np.sin(np.pi / 8), 0, 0, np.cos(np.pi / 8)]          # 45 degrees about x
    rs[:, obj, 7:13] = 0


def check_kuka_lists(orc, hs, m, p, lo, up):
    """The first substep's contact lists (the oracle's detect on the scene as it stands) and joint positions hold
    every case of the loop structure."""
    counts, links = [], []
    for e in range(N):
        c = orc.contacts(hs, e)
        a, b = c[:, 7].astype(int), c[:, 8].astype(int)
        counts.append(len(c))
        links.append(int(((a >= 100) | (b >= 100)).sum()))
    counts, links = np.array(counts), np.array(links)
    q = hs["dof_state"].reshape(N, 23, 2)[..., 0]
    at_lo = ((q - lo) <= p.joint_limit_margin).any(1)
    at_up = ((up - q) <= p.joint_limit_margin).any(1)
    print(f"kuka sweep scene: contacts per env {counts.tolist()}, link contacts {links.tolist()}, "
          f"envs at a lower limit {int(at_lo.sum())}, at an upper limit {int(at_up.sum())}")
    assert (counts == 0).any(), "no env without contacts"
    assert ((counts == 1) | (counts == 2)).any(), "no env with 1 or 2 contacts"
    assert ((counts == 3) | (counts == 4)).any(), "no env with 3 or 4 contacts"
    small, big = counts[counts <= 21], counts[counts > 21]
    for r in range(UNROLL):
        assert (small % UNROLL == r).any(), f"no env with at most 21 contacts and count % {UNROLL} == {r}"
        assert (big % UNROLL == r).any(), f"no env with more than 21 contacts and count % {UNROLL} == {r}"
    assert ((counts > 21) & (links > 9)).any(), "no env over 21 contacts with more than 9 link contacts"
    assert at_lo.any(), "no DOF within joint_limit_margin of its lower limit"
    assert at_up.any(), "no DOF within joint_limit_margin of its upper limit"
    return counts


def _kuka():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from handarm_hip.sim import HandArmSim
    from oracle.oracle_lib import HostState, Oracle
    sim = HandArmSim(N, "cuda:0", task_cfg={"task": HM.TASK_ALLEGRO_KUKA, "subtask": "regrasping"},
                     task=HM.TASK_ALLEGRO_KUKA)
    assert sim.contact_capacity == 42
    m, p = sim.model, sim.params
    lo = np.array(m.dof_lower[:23], np.float32)
    up = np.array(m.dof_upper[:23], np.float32)
    hs = HostState(N, model=m, params=p)
    pull_all(sim, hs)                   # object dims, task-state keypoints, scalars
    kuka_sweep_scene(sim, hs, lo, up)
    hs["object_force"][:] = 0
    hs["contact_stats"][:] = 0
    orc = Oracle(m, p, N)
    check_kuka_lists(orc, hs, m, p, lo, up)
    push_all(sim, hs)
    return sim, hs, orc, lo, up


def _stats_equal(sim, hs):
    g = get(sim, "contact_stats").reshape(hs["contact_stats"].shape)
    assert (g[:, :6] == hs["contact_stats"][:, :6]).all(), "contact statistics differ from the oracle's"
    return g


@pytest.mark.parametrize("calls", [1, 3])
def test_kuka_sweep_scene_simulate_matches_oracle_bit_for_bit(calls):
    """ak_simulate_kernel, `calls` gym.simulate calls in one launch, every physics output bit-identical."""
    sim, hs, orc, _, _ = _kuka()
    sim.simulate(calls)
    orc.simulate(hs, calls)
    scenes.assert_physics_bit_identical(sim, hs, N, tag=f"kuka sweep scene, {calls} calls")
    _stats_equal(sim, hs)


def test_kuka_sweep_scene_fused_step_io_matches_oracle_chain():
    """ak_step_kernel through ha_task_step_io: two steps with the fingers driven further closed, against
    kuka_oracle.pre -> physics_oracle -> kuka_oracle.post. Physics outputs and the step's buffers bit-exact;
    observations, also the clamped copy the launch returns, and rewards within 1e-4."""
    sim, hs, orc, lo, up = _kuka()
    p = sim.params
    rng = np.random.default_rng(23)
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
        tag = f"kuka sweep scene step_io {t}"
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


# ----------------------------------------------------------------------------- AllegroHand
AH_CHUNK = 12
AH_CALLS = [0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 63, 64, 72, 77, 90]     # simulate calls before an env is stopped


def allegro_sweep_scene(m, p):
    """The self-collision drives of tests/test_gpu_self_collision.py (envs alternate between the two, targets jittered
    per env), run on the oracle; env e keeps the state it had after AH_CALLS[e // 2] simulate calls."""
    from oracle.oracle_lib import HostState, Oracle
    D = m.n_dofs
    lo, up = np.array(m.dof_lower[:D], np.float32), np.array(m.dof_upper[:D], np.float32)
    drives = SC.allegro_drives(lo, up)
    names = list(drives)
    rng = np.random.default_rng(5)
    targets = np.stack([drives[names[e % len(names)]] for e in range(N)])
    targets = np.clip(targets + rng.uniform(-0.05, 0.05, targets.shape).astype(np.float32), lo, up)
    hs = SC.drive_state(HostState(N, model=m, params=p), m, targets, N)
    orc = Oracle(m, p, N)
    for e in range(N):
        if AH_CALLS[e // 2]:
            orc.simulate(hs, AH_CALLS[e // 2], begin=e, end=e + 1)
    hs["contact_stats"][:] = 0
    return hs, orc


def check_allegro_lists(orc, hs):
    counts = np.array([len(orc.contacts(hs, e)) for e in range(N)])
    print(f"allegro sweep scene: contacts per env {counts.tolist()}")
    small, big = counts[counts <= AH_CHUNK], counts[counts > AH_CHUNK]
    assert (counts == 0).any(), "no env without contacts"
    for r in range(UNROLL):
        assert (small % UNROLL == r).any(), f"no env with at most {AH_CHUNK} contacts and count % {UNROLL} == {r}"
        assert (big % UNROLL == r).any(), f"no env with more than {AH_CHUNK} contacts and count % {UNROLL} == {r}"
    assert (counts > 2 * AH_CHUNK).any(), "no env reaches a third chunk"


@pytest.mark.parametrize("calls", [1, 3])
def test_allegro_sweep_scene_simulate_matches_oracle_bit_for_bit(calls):
    """ah_simulate_kernel on the stopped self-collision drives, `calls` gym.simulate calls in one launch."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from handarm_hip.sim import HandArmSim
    sim = HandArmSim(N, "cuda:0", task=HM.TASK_ALLEGRO_HAND)
    assert sim.contact_capacity == 48
    hs, orc = allegro_sweep_scene(sim.model, sim.params)
    check_allegro_lists(orc, hs)
    for k in HM.STATE_FIELDS:
        if k in ("stats", "term_sums", "task_state", "task_scalars") or k in HM.null_fields(sim.task):
            continue
        put(sim, k, hs[k])
    sim.simulate(calls)
    orc.simulate(hs, calls)
    scenes.assert_physics_bit_identical(sim, hs, N, tag=f"allegro sweep scene, {calls} calls")
    _stats_equal(sim, hs)
