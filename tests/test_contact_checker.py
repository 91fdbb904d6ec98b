"""The independent float64 contact checker (tests/contact_ref.py) on the C oracle's contact rows: three
box piles (every property, including pair completeness and axis quality against a brute-force SAT) and two YCB-hull
piles (unit normals, depth and surface points), and the rows with a robot link of three hand scenes (the Ur5Sih pile in
the hand, the AllegroHand closing hand, the AllegroKuka closed hand) against the link hulls posed by the independent
FK. It pins the oracle; tests/test_gpu_contact_tensor.py runs the same checker on the kernel's rows."""
import numpy as np
import pytest

from handarm_hip import model as HM
from oracle.oracle_lib import HostState, Oracle
from tests import contact_ref as CR
from tests import scenes


@pytest.fixture(scope="module")
def box_setup():
    scene = scenes.box_pool_scene(scenes.EDGE_BOXES)
    m = HM.build_model(scene)
    p, _ = HM.build_params()
    return CR.SceneRef(scene), m, p


@pytest.mark.parametrize("seed", CR.BOX_SEEDS)
def test_box_piles_on_the_oracle(box_setup, seed):
    ref, m, p = box_setup
    n = 256
    st = CR.box_pile_state(HostState(n, model=m, params=p), n, seed)
    orc = Oracle(m, p, n)
    rep = CR.Report()
    deepest = 0.0
    for e in range(n):
        rows = orc.contacts(st, e)
        deepest = min(deepest, float(rows[:, 6].min()) if len(rows) else 0.0)
        CR.check_env(ref, m, p, st, e, rows, rep)
    print(f"box pile seed {seed}: {rep}; deepest row {deepest:.4f}")
    assert rep.rows > 1000 and deepest < -0.02 and rep.pairs == 6 * n, "the scene must be a deep pile"
    CR.assert_report(rep, margin=float(p.contact_margin))


@pytest.mark.parametrize("seed,near_hand", CR.YCB_CASES)
def test_ycb_piles_on_the_oracle(seed, near_hand):
    scene = HM.load_scene()
    m = HM.build_model(scene)
    p, _ = HM.build_params()
    ref = CR.SceneRef(scene, edges=False)
    n = 64
    st = CR.ycb_pile_state(HostState(n), n, seed, near_hand)
    orc = Oracle(m, p, n)
    rep = CR.Report()
    for e in range(n):
        CR.check_env(ref, m, p, st, e, orc.contacts(st, e), rep, pairs=False)
    print(f"ycb pile seed {seed}: {rep}")
    assert rep.rows > 300
    CR.assert_report(rep, margin=None, pairs=False)


@pytest.mark.parametrize("name", list(CR.LINK_SCENES))
def test_link_hull_rows_on_the_oracle(name):
    """Link-object, link-static and link-link rows of the three robots against the link hulls posed by the independent
    float64 FK: (a), (b), the lower bound of (c), no row of a link without a hull or of a filtered link pair."""
    make, n = CR.LINK_SCENES[name]
    scene, m, p, st = make(n)
    orc = Oracle(m, p, n)
    CR.check_link_scene(name, scene, m, p, st, lambda e: orc.contacts(st, e))
