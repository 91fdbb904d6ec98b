"""Replayed domain-randomization draws (sim.reference_rng + task.randomize), host side: handarm_hip/ref_rng.py DrDraws
makes the reference's numpy / torch draws in the reference's order, and handarm_hip/dr.py gate restates the device's
frequency gate so the host knows how many to make.

Pinned against the REFERENCE's recorded apply_randomizations runs (tests/golden/dr_reference.npz, made by
make_goldens_dr.py with np.random.default_rng(7) for AllegroKuka.yaml's schema and (8) for AllegroHand.yaml's):
* the draws DrDraws.apply consumes, per call of the golden's ten calls, are the reference's, in the reference's order,
  and each lands in the dr_draws slot of the quantity it randomizes (gravity in the gravity draws);
* the envs that draw and the non-env flag are the reference's;
* the values those slots give through oracle/dr_oracle.py are the values the reference set;
* on the real global generators, apply / noise consume the streams like a hand-written sequence of the same calls.
The device side is tests/test_gpu_dr_replay.py, which replays `golden_sequence`'s draws.
"""
import copy
from unittest import mock

import numpy as np
import pytest
import torch

from handarm_hip import dr as DR
from handarm_hip import model as HM
from handarm_hip import ref_rng as RR
from oracle import dr_oracle as DO
from tests.test_dr_schema import ATTRS, PK_SIM, _attr_of, _setup, ref  # noqa: F401  (ref: the golden fixture)

F = np.float32
SEEDS = {"kuka": 7, "hand": 8}
TASKS = {"kuka": (HM.TASK_ALLEGRO_KUKA, DR.ALLEGRO_KUKA_SCHEMA), "hand": (HM.TASK_ALLEGRO_HAND, DR.ALLEGRO_HAND_SCHEMA)}
MASS = (HM.DRA_LINK_MASS, HM.DRA_OBJ_MASS)


class Shim:
    """np.random.uniform / normal over the generator make_goldens_dr.py's Draws used, recording what is consumed."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.log = []

    def uniform(self, lo, hi, shape):
        q = self.rng.random(shape)
        self.log.extend(np.atleast_1d(q).tolist())
        return lo + (hi - lo) * q

    def normal(self, mu, var, shape):
        z = self.rng.standard_normal(shape)
        self.log.extend(np.atleast_1d(z).tolist())
        return mu + var * z


def make_draws(name, n):
    task, schema = TASKS[name]
    sc = copy.deepcopy(schema)
    sc["frequency"] = 3
    p, m = _setup(name)
    return p, m, RR.DrDraws(p, m, n, DR.draw_plan(sc, task))


_SEQ = {}


def golden_sequence(refz, name):
    """DrDraws.apply driven through the golden's ten calls with the recording shim; the shard-wide state between the
    calls is advanced by the oracle's global_update (a reset launch). Computed once per scenario and shared (the GPU
    test uploads the same draws). -> (params, model, [(dr_global before the call, DrApplied, consumed draws)])."""
    if name not in _SEQ:
        n = refz[f"{name}_reset"].shape[1]
        p, m, dd = make_draws(name, n)
        shim = Shim(SEEDS[name])
        g = DR.init_global(p)
        calls = []
        with mock.patch.object(np.random, "uniform", shim.uniform), mock.patch.object(np.random, "normal", shim.normal):
            for c in range(len(refz[f"{name}_frame"])):
                g.view(np.int32)[HM.DRG_FRAME_NEXT] = int(refz[f"{name}_frame"][c])
                reset = refz[f"{name}_reset"][c]
                shim.log = []
                res = dd.apply(g, reset, refz[f"{name}_rb_before"][c])
                calls.append((g.copy(), res, np.array(shim.log, np.float64)))
                DO.global_update(p, g, bool(reset.any()), 1)
        _SEQ[name] = (p, m, calls)
    return _SEQ[name]


def f32_draw(draw, kind):
    """The float32 the kernel is handed for a recorded double draw: a quantile stays below 1."""
    return min(F(draw), RR.U_BELOW_ONE) if kind == 0 else F(draw)


def value_og(refz, name, m, k, call, elem):
    """The nominal value the reference's sample applies to (tests/test_dr_schema.py's rule) and, for a mass, the
    body's own nominal mass."""
    if k == HM.DRA_LINK_MASS:
        own = F(m.link_mass[elem])
        return (F(m.pool_mass[0]) if call > 0 else own), own
    if k == HM.DRA_OBJ_MASS:
        return F(m.pool_mass[0]), F(m.pool_mass[0])
    if k == HM.DRA_GRAVITY:
        return (F([0.0, 0.0, -9.81][elem]) if call == 0 else F(refz[f"{name}_gravity"][0][elem])), None
    nominal = {HM.DRA_DOF_KD: m.dof_kd, HM.DRA_DOF_KP: m.dof_kp, HM.DRA_DOF_LOWER: m.dof_lower,
               HM.DRA_DOF_UPPER: m.dof_upper}
    return (F(nominal[k][elem]) if k in nominal else F(1.0)), None


def value_from_draw(a, frame, og, own, d, mass):
    """dr_value / dr_mass_ratio (csrc/ha_dr.h) from an explicit draw d, through the oracle's value(): what a dr_scale
    slot holds (a mass slot holds new / nominal mass)."""
    r0, r1 = DO.scheduled_range(a, frame)
    if not mass:
        return DO.value(a, r0, r1, og, d, d)
    og, own = np.asarray(og, F), np.asarray(own, F)
    with np.errstate(invalid="ignore", divide="ignore"):
        general = (DO.value(a, r0, r1, og, d, d) / own).astype(F)
    if not (a.op == DO.OP_SCALING and a.num_buckets == 0):
        return general
    return np.where(og == own, DO.value(a, r0, r1, F(1.0), d, d), general).astype(F)


def check_against_golden(refz, name, p, m, call, produced):
    """The golden's tolerance rule (tests/test_dr_schema.py::test_property_values_from_the_same_draws) for the rows of
    one call: produced(k, env, elem) is the dr_scale slot value (gravity: the gravity component). rtol 2e-6, atol 2e-7;
    a bucketed value may land one bucket off (returned count); masses compare as new / nominal."""
    edge = 0
    vals = refz[f"{name}_values"]
    for _, env, pk, actor, elem, attr, kind, draw, value in vals[vals[:, 0] == call]:
        k, env, elem = _attr_of(int(pk), int(actor), attr), int(env), int(elem)
        a = p.dr_attr[k]
        mine = float(produced(k, env, elem))
        if k in MASS:
            own = float(value_og(refz, name, m, k, call, elem)[1])
            if own == 0.0:
                assert value == 0.0                      # a massless body stays massless; its ratio is not compared
                continue
            value = value / own
        if a.num_buckets > 0 and abs(mine - value) > 1e-6:
            w = (a.range[1] - a.range[0]) / a.num_buckets
            assert abs(abs(mine - value) - w) < 1e-5, (ATTRS[int(attr)], call, env, mine, value)
            edge += 1
            continue
        np.testing.assert_allclose(mine, value, rtol=2e-6, atol=2e-7, err_msg=f"{ATTRS[int(attr)]} call {call}")
    return edge


@pytest.mark.parametrize("name", ["kuka", "hand"])
def test_draw_order_and_slots_against_the_reference(ref, name):  # noqa: F811
    p, m, calls = golden_sequence(ref, name)
    vals = ref[f"{name}_values"]
    total = 0
    for c, (g, res, consumed) in enumerate(calls):
        rows = vals[vals[:, 0] == c]
        np.testing.assert_array_equal(consumed, rows[:, 7], err_msg=f"call {c}: draws consumed, in order")
        total += len(rows)
        want = np.zeros_like(res.draws)
        grav = None
        for _, env, pk, actor, elem, attr, kind, draw, _v in rows:
            k = _attr_of(int(pk), int(actor), attr)
            assert (kind == 1) == (p.dr_attr[k].dist == DO.DIST_GAUSSIAN)
            if int(pk) == PK_SIM:
                grav = np.zeros(3, F) if grav is None else grav
                grav[int(elem)] = f32_draw(draw, kind)
            else:
                want[int(env), RR.DR_SLOT[k] + int(elem)] = f32_draw(draw, kind)
        np.testing.assert_array_equal(res.draws, want, err_msg=f"call {c}: every draw in its slot, nothing else")
        if grav is None:
            assert res.gravity is None
        else:
            np.testing.assert_array_equal(res.gravity, grav)
        np.testing.assert_array_equal(res.envs, ref[f"{name}_randomized"][c], err_msg=f"call {c}")
        assert res.nonenv == bool(ref[f"{name}_nonenv"][c]) and res.all == (c == 0), f"call {c}"
    assert total == len(vals) > 500


@pytest.mark.parametrize("name", ["kuka", "hand"])
def test_values_from_the_replayed_slots(ref, name):  # noqa: F811
    p, m, calls = golden_sequence(ref, name)
    edge = 0
    for c, (g, res, _) in enumerate(calls):
        frame = int(ref[f"{name}_frame"][c])

        def produced(k, env, elem):
            og, own = value_og(ref, name, m, k, c, elem)
            d = res.gravity[elem] if k == HM.DRA_GRAVITY else res.draws[env, RR.DR_SLOT[k] + elem]
            return value_from_draw(p.dr_attr[k], frame, og, own, d, k in MASS)
        edge += check_against_golden(ref, name, p, m, c, produced)
    assert edge <= 2


def test_gate_mirror_matches_the_oracle_step_mode(ref):  # noqa: F811
    """dr.gate on a step launch's inputs == the oracle's global_update / env_pre decisions (mode 0, counts + 1)."""
    p, m = _setup("kuka")
    n = 6
    g = DR.init_global(p)
    rb = np.zeros(n, np.int32)
    rng = np.random.default_rng(0)
    for step in range(12):
        reset = rng.random(n) < 0.4
        nonenv, all_, envs = DR.gate(g, p.dr_frequency, reset, rb)
        epoch = g.view(np.int32)[HM.DRG_EPOCH]
        DO.global_update(p, g, bool(reset.any()), 0)
        assert nonenv == (g.view(np.int32)[HM.DRG_EPOCH] != epoch) and all_ == bool(g.view(np.int32)[HM.DRG_ALL])
        smp = DO.env_pre(p, m, DR.default_rows(m, p, n), rb, np.zeros(n, np.uint32), np.zeros((n, 1), np.int64), reset,
                         g, True)
        np.testing.assert_array_equal(envs, smp)


def test_apply_on_the_real_numpy_generator():
    """After np.random.seed(3): the first randomization of AllegroHand.yaml's schema and a later one draw like a
    hand-written sequence of np.random.uniform / np.random.normal calls of the golden's kinds and counts."""
    n = 3
    p, m, dd = make_draws("hand", n)
    L, D = m.n_links, m.n_dofs
    g = DR.init_global(p)
    np.random.seed(3)
    first = dd.apply(g, np.ones(n), np.zeros(n, np.int32))
    DO.global_update(p, g, True, 1)
    g.view(np.int32)[HM.DRG_FRAME_NEXT] = 5
    later = dd.apply(g, np.array([0, 1, 0]), np.array([3, 3, 3], np.int32))
    assert first.all and later.nonenv and not later.all and later.envs.tolist() == [False, True, False]

    np.random.seed(3)
    u = lambda k: np.minimum(np.random.uniform(0.0, 1.0, k).astype(F), RR.U_BELOW_ONE)  # noqa: E731
    z = lambda k: np.random.normal(0.0, 1.0, k).astype(F)                               # noqa: E731
    want = np.zeros((n, HM.DR_SIZE), F)
    grav = z(3)
    for e in range(n):                                       # the hand actor: dof_properties, bodies, shapes
        want[e, HM.DR_DOF_KD:HM.DR_DOF_KD + D] = u(D)
        want[e, HM.DR_DOF_KP:HM.DR_DOF_KP + D] = u(D)
        want[e, HM.DR_DOF_LOWER:HM.DR_DOF_LOWER + D] = z(D)
        want[e, HM.DR_DOF_UPPER:HM.DR_DOF_UPPER + D] = z(D)
        for i in range(L):
            want[e, HM.DR_LINK_MASS + i] = u(1)[0]
        for i in range(L):
            want[e, HM.DR_LINK_FRIC + i] = u(1)[0]
    for e in range(n):                                       # the object actor: scale, body, shape
        want[e, HM.DR_OBJ_SCALE], want[e, HM.DR_OBJ_MASS], want[e, HM.DR_OBJ_FRIC] = u(1)[0], u(1)[0], u(1)[0]
    np.testing.assert_array_equal(first.gravity, grav)
    np.testing.assert_array_equal(first.draws, want)
    want2 = np.zeros((n, HM.DR_SIZE), F)
    grav2 = z(3)
    want2[1, HM.DR_DOF_KD:HM.DR_DOF_KD + D] = u(D)           # setup_only mass / scale: no draw after the first
    want2[1, HM.DR_DOF_KP:HM.DR_DOF_KP + D] = u(D)
    want2[1, HM.DR_DOF_LOWER:HM.DR_DOF_LOWER + D] = z(D)
    want2[1, HM.DR_DOF_UPPER:HM.DR_DOF_UPPER + D] = z(D)
    want2[1, HM.DR_LINK_FRIC] = u(1)[0]                      # later_elems: the first link only
    want2[1, HM.DR_OBJ_FRIC] = u(1)[0]
    np.testing.assert_array_equal(later.gravity, grav2)
    np.testing.assert_array_equal(later.draws, want2)


@pytest.mark.parametrize("dist", ["gaussian", "uniform"])
def test_noise_on_the_real_torch_generator(dist):
    """After torch.manual_seed(3): four steps' lambda draws equal a hand-written torch.randn / torch.rand sequence:
    the first randomization in step 1 (no action noise yet, obs corr drawn in that very step), no randomization in
    step 2 (act corr drawn now, obs corr kept), a randomization in step 3 (act corr kept, obs corr redrawn), step 4."""
    n = 5
    sc = {"frequency": 1, "observations": {"range": [0.1, 0.3], "range_correlated": [0, 0.1], "operation": "additive",
                                           "distribution": dist},
          "actions": {"range": [0.0, 0.05], "range_correlated": [0, 0.015], "operation": "additive",
                      "distribution": dist}}
    p, _ = HM.build_params({"dr_enable": 1, "randomization_params": sc}, task=HM.TASK_ALLEGRO_KUKA)
    m = HM.build_model(HM.load_scene(HM.KUKA_ASSET))
    dd = RR.DrDraws(p, m, n, DR.draw_plan(sc, HM.TASK_ALLEGRO_KUKA))
    no, na = p.num_obs, p.num_actions
    task = lambda: torch.rand(7)                             # noqa: E731  the task's own pre-physics draws
    torch.manual_seed(3)
    got = [dd.noise(nonenv, task) for nonenv in (True, False, True, False)]
    assert dd.noise(False, None, step=False) == dict.fromkeys(got[0])       # a bare reset_idx draws nothing

    torch.manual_seed(3)
    white = torch.randn if dist == "gaussian" else torch.rand
    w = lambda k: white((n, k))                              # noqa: E731
    c = lambda k: torch.randn((n, k))                        # noqa: E731
    want = []
    s = {"act_corr": None, "act_white": None, "task": task()}
    s["obs_corr"], s["obs_white"] = c(no), w(no)
    want.append(s)
    s = {"act_corr": c(na), "act_white": w(na), "task": task(), "obs_corr": None, "obs_white": w(no)}
    want.append(s)
    s = {"act_corr": None, "act_white": w(na), "task": task()}
    s["obs_corr"], s["obs_white"] = c(no), w(no)
    want.append(s)
    s = {"act_corr": c(na), "act_white": w(na), "task": task(), "obs_corr": None, "obs_white": w(no)}
    want.append(s)
    for step, (a, b) in enumerate(zip(got, want)):
        for key in b:
            if b[key] is None:
                assert a[key] is None, (step, key)
            else:
                assert a[key] is not None and torch.equal(a[key], b[key]), (step, key)


def test_ur5sih_has_no_reference_stream():
    """One object actor is what the reference's schemas randomize; the multi-object Ur5Sih schema is the build's own and
    stays on the device hash (handarm_hip/ref_rng.py docstring)."""
    p, _ = HM.build_params({"dr_enable": 1}, task=HM.TASK_UR5SIH)
    m = HM.build_model(HM.load_scene())
    with pytest.raises(NotImplementedError):
        RR.DrDraws(p, m, 4)
