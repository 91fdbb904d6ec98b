"""The rows phase without a round trip per DOF (AllegroKuka), bit for bit against the C oracle.

rows_chunk (ha_solve.h) stores Y_r = M^-1 J_r^T in its loop over the DOFs and takes the diagonal term J_r . Y_r
afterwards, from J_r in registers and Y_r read back in one batch; delassus_chunk loads J once for both of a friction
row's sums and issues the loads of J, Y0 (and Y1) ahead of the two chains. Every chain keeps its index order, so both
AllegroKuka kernels must still give the oracle's bits where a chunk's lanes diverge between robot blocks in LDS slots
and in the env's global spill rows.

The scene is tests/test_gpu_pgs_fetch.py's (64 envs), imported; its own checks guarantee envs with more than 9 link
contacts, more than 21 contacts with spill-row robot blocks among them, and a full list of 42. On top of them the
oracle's contact lists of the first substep must show, before any kernel runs,

* a chunk (contacts 0..20 or 21..41) whose rows mix LDS-slot and spill-row robot blocks: the divergent case,
* a spilled contact with its friction rows k = 1 and k = 2 (a contact's rows come in threes: the rows of contact ci
  are 3 ci .. 3 ci + 2, so a spilled contact inside the list has both; asserted on the row count),
* spill rows in chunk 1 (the rows whose object blocks are global too).

Whether an env with exactly 9 and one with exactly 10 link contacts occur (the last LDS slot / the first spill row)
is printed, not required.

Then ak_simulate_kernel (1 and 4 calls) and two fused steps of ak_step_kernel run that test's bodies (the same
buffer lists, scenes.assert_physics_bit_identical, contact_stats equal to the oracle's) on the checked scene.

Paths: both AllegroKuka kernels run the batched read-back of Y_r, the batched row of M^-1 and the batched Delassus
sums. The AllegroHand and clutter kernels keep the per-DOF reload of J_r[i] (Family rows_y_batch = false: the second
array would cost the first scratch and measured slower in the second); they take the other two like every family.
"""
import pytest

from tests import test_gpu_pgs_fetch as PF

pytestmark = pytest.mark.gpu

PATHS = ("ak_simulate_kernel / ak_step_kernel: Y_r read back in one batch (rows_y_batch), batched M^-1 row and Delassus "
         "sums; ah_* / hb_* kernels (not run here): per-DOF reload of J_r[i] kept, batched M^-1 row and Delassus sums")


def check_rows_cases(orc, hs):
    kinds = [PF.contact_kinds(orc, hs, e) for e in range(PF.N)]
    chunks = [(k[:PF.CHUNK], k[PF.CHUNK:PF.CAPACITY]) for k in kinds]
    links = [sum(ch != "n" for ch in k) for k in kinds]
    print("rows scene, link contacts per env:", links)
    mixed = [(e, i) for e, cs in enumerate(chunks) for i, ch in enumerate(cs) if "l" in ch and "s" in ch]
    print("chunks with LDS-slot and spill-row robot blocks (env, chunk):", mixed)
    assert mixed, "no chunk whose rows mix LDS-slot and spill-row robot blocks"
    # rows 3 ci + 1 and 3 ci + 2 of a spilled contact ci: inside the env's 3 x contacts rows
    spilled = [(e, k.index("s")) for e, k in enumerate(kinds) if "s" in k]
    assert spilled, "no spilled contact"
    assert all(3 * ci + 2 < 3 * len(kinds[e]) for e, ci in spilled), "a spilled contact without both friction rows"
    assert any("s" in cs[1] for cs in chunks), "no spill row in chunk 1"
    print(f"an env with exactly {PF.KL} link contacts: {PF.KL in links}; with exactly {PF.KL + 1}: {PF.KL + 1 in links}")
    print("paths:", PATHS)


def _checked_scene():
    sim, hs, orc, lo, up = _fetch_scene()
    # (the scene is on the device, no kernel has run on it yet: the oracle lists the first substep's contacts from hs)
    check_rows_cases(orc, hs)
    return sim, hs, orc, lo, up


_fetch_scene = PF._scene


@pytest.fixture
def checked_scene(monkeypatch):
    monkeypatch.setattr(PF, "_scene", _checked_scene)


@pytest.mark.parametrize("calls", [1, 4])
def test_rows_scene_simulate_matches_oracle_bit_for_bit(checked_scene, calls):
    """ak_simulate_kernel, `calls` gym.simulate calls in one launch: every physics output bit-identical, contact_stats
    equal to the oracle's."""
    PF.test_fetch_scene_simulate_matches_oracle_bit_for_bit(calls)


def test_rows_scene_fused_steps_match_oracle_chain(checked_scene):
    """ak_step_kernel, two fused steps: physics outputs and the step's buffers bit-exact against the oracle chain,
    contact_stats equal to the oracle's."""
    PF.test_fetch_scene_fused_step_io_matches_oracle_chain()
