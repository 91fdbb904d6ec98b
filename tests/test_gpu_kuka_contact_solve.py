"""AllegroKuka contact rows and contact solve on their heaviest paths, bit for bit against the C oracle.

The rows phase takes each link's ancestor DOFs from a per-lane bit mask (link_dof_masks) instead of walking the link
tree through memory, the PGS fetch reads a contact's link slot from a lane register and loads through typed LDS /
global paths, and the joint and contact forces are built only in a launch's final substep. One small scene drives
all of it at once: the half-closed hand closing on the cuboid in its palm (tests/test_gpu_fused_steps.py
kuka_closed_hand_scene, the scene of test_gpu_overflow.py's Kuka case) on 32 envs. The oracle's own contact lists
must show, before anything runs on the GPU,

* an env with more than 21 contacts (the second chunk, in the env's global area) of which more than 9 touch a link
  (robot blocks past the LDS link slots, in the global spill rows),
* a contact between two links (two ancestor chains in one row),
* a contact between a link and the object (robot and object blocks in one row),
* a contact on a fingertip link (the deepest chain: 11 DOFs);

the test fails if the scene does not give them. Then gym.simulate once and three times in one launch (only the third
call's last substep may build the forces, and they must be that substep's), and two fused VecTask steps
(ha_task_step_io) against the oracle chain.
"""
import numpy as np
import pytest
import torch

from handarm_hip import model as HM
from oracle import kuka_oracle as KO
from tests import scenes, step_chains
from tests.test_gpu_fused_steps import exact, get, kuka_closed_hand_scene, near, pull_all, push_all, put

pytestmark = pytest.mark.gpu
N = 32


def _scene():
    """The sim, the host state of the closed-hand scene (already pushed to the sim) and an oracle."""
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
    kuka_closed_hand_scene(sim, hs, lo, up)
    hs["object_force"][:] = 0
    hs["contact_stats"][:] = 0
    orc = Oracle(m, p, N)
    check_contact_lists(orc, hs, m)
    push_all(sim, hs)
    return sim, hs, orc, lo, up


def check_contact_lists(orc, hs, m):
    """The first substep's contact lists (the oracle's detect on the scene as it stands) hold every case."""
    level = np.array(m.link_level[:m.n_links])
    heavy = two_links = link_object = fingertip = 0
    for e in range(N):
        c = orc.contacts(hs, e)
        a, b = c[:, 7].astype(int), c[:, 8].astype(int)
        la, lb = a >= 100, b >= 100
        oa, ob = (a >= 0) & (a < 100), (b >= 0) & (b < 100)
        heavy += len(c) > 21 and int((la | lb).sum()) > 9
        two_links += int((la & lb).sum())
        link_object += int(((la & ob) | (lb & oa)).sum())
        tips = [int(x) - 100 for x in np.concatenate([a[la], b[lb]])]
        fingertip += sum(level[t] == m.max_level for t in tips)
    print(f"closed-hand scene, {N} envs: {heavy} envs over 21 contacts with over 9 link contacts, {two_links} link-link, "
          f"{link_object} link-object, {fingertip} fingertip contact sides")
    assert heavy > 0, "no env has more than 21 contacts and more than 9 link contacts in its first substep"
    assert two_links > 0, "no contact joins two links"
    assert link_object > 0, "no contact joins a link and the object"
    assert fingertip > 0, "no contact sits on a fingertip link"


@pytest.mark.parametrize("calls", [1, 3])
def test_kuka_closed_hand_simulate_matches_oracle_bit_for_bit(calls):
    """ak_simulate_kernel, `calls` gym.simulate calls in one launch: dof / root / rigid-body states, net contact forces,
    joint forces and the persistent manifolds bit-identical on every env."""
    sim, hs, orc, _, _ = _scene()
    sim.simulate(calls)
    orc.simulate(hs, calls)
    scenes.assert_physics_bit_identical(sim, hs, N, tag=f"kuka closed hand, {calls} calls")
    f = get(sim, "net_contact_force").reshape(N, sim.model.n_bodies, 3)
    assert (np.abs(f).sum(-1) > 0).sum(1).max() > 3, "contact forces on several bodies"
    g = get(sim, "contact_stats").reshape(hs["contact_stats"].shape)
    assert (g[:, :6] == hs["contact_stats"][:, :6]).all(), "contact statistics differ from the oracle's"


def test_kuka_closed_hand_fused_step_io_matches_oracle_chain():
    """ak_step_kernel through ha_task_step_io (the launch VecTask.step makes): two steps with the fingers driven
    further closed, against kuka_oracle.pre -> physics_oracle -> kuka_oracle.post. Physics outputs (net contact
    forces and joint forces among them) and the step's buffers bit-exact; observations, also the clamped copy the
    launch returns, and rewards within 1e-4."""
    sim, hs, orc, lo, up = _scene()
    p = sim.params
    rng = np.random.default_rng(21)
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
        tag = f"kuka closed hand step_io {t}"
        scenes.assert_physics_bit_identical(sim, hs, N, tag=tag)
        exact(sim, hs, ["actions", "dof_position_targets", "sim_targets", "goal_state", "reset_buf", "reset_goal_buf",
                        "progress_buf", "successes"], tag)
        assert (get(sim, "timeout_buf").astype(bool) == timeout).all(), tag
        eo = near(get(sim, "obs"), obs, 1e-4, tag + " obs")
        er = near(get(sim, "rew"), rew, 1e-4, tag + " rew")
        torch.cuda.synchronize()
        near(out.cpu().numpy(), np.clip(obs, -clip_obs, clip_obs), 1e-4, tag + " returned obs")
        print(f"{tag}: obs max |d| {eo:.2e}, rew max |d| {er:.2e}")
    g = get(sim, "contact_stats").reshape(hs["contact_stats"].shape)
    assert (g[:, :6] == hs["contact_stats"][:, :6]).all(), "contact statistics differ from the oracle's"
    assert (g[:, 2] > 21).any(), "some env went over chunk 0's 21 contacts"
