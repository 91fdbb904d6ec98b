"""Replayed domain-randomization draws on the device (HA_FLAG_REPLAY_DR, ha_bind_dr_replay): the kernels take every DR
sample from the uploaded host draws (handarm_hip/ref_rng.py DrDraws) in place of the counter hash, with the gates,
schedules and arithmetic of csrc/ha_dr.h unchanged.

* The golden sequence (tests/golden/dr_reference.npz: the reference's ten apply_randomizations calls) on AllegroKuka and
  AllegroHand sims: dr_scale, randomize_buf and the gravity after every call, bit for bit against oracle/dr_oracle.py
  fed the same draws, and within the golden's tolerance of the values the reference set.
* Observation and action noise from uploaded corr / white tensors, bit for bit in numpy float32.
* Without the flag nothing reads the buffers; the flag without buffers is an error.
* AllegroKuka / AllegroHand with sim.reference_rng and task.randomize: same seed -> same run, another seed -> another.
"""
import copy

import numpy as np
import pytest
import torch

from handarm_hip import _lib
from handarm_hip import dr as DR
from handarm_hip import model as HM
from handarm_hip import ref_rng as RR
from oracle import dr_oracle as DO
from tests.test_dr_replay import MASS, TASKS, check_against_golden, golden_sequence, value_from_draw
from tests.test_dr_schema import ref  # noqa: F401  (the golden fixture)
from tests.test_gpu_fused_steps import get, need_gpu, put

pytestmark = pytest.mark.gpu
F = np.float32
REPLAY = HM.FLAG_NO_PHYSICS | HM.FLAG_REPLAY_DR


def _expected_rows(p, m, rows, res, frame):
    """dr_env_pre's samples (oracle/dr_oracle.py env_pre's walk) from the explicit draws of `res`, into `rows`."""
    L, D = m.n_links, m.n_dofs
    envs = np.nonzero(res.envs)[0]
    pool_mass = F(m.pool_mass[0])

    def put_(k, slot, n, og, own=None):
        d = res.draws[envs, RR.DR_SLOT[k]:RR.DR_SLOT[k] + n]
        rows[envs, slot:slot + n] = value_from_draw(p.dr_attr[k], frame, og, own, d, k in MASS)
    n = DO.elems(p, HM.DRA_LINK_MASS, res.all, L)
    if n:
        own = np.array(list(m.link_mass)[:n], F)[None]
        og = np.full_like(own, pool_mass) if (not res.all and p.dr_attr[HM.DRA_LINK_MASS].later_og_object) else own
        put_(HM.DRA_LINK_MASS, HM.DR_LINK_MASS, n, og, own)
    n = DO.elems(p, HM.DRA_LINK_FRIC, res.all, L)
    if n:
        put_(HM.DRA_LINK_FRIC, HM.DR_LINK_FRIC, n, F(p.friction))
    for k, slot, nm in ((HM.DRA_DOF_KD, HM.DR_DOF_KD, "dof_kd"), (HM.DRA_DOF_KP, HM.DR_DOF_KP, "dof_kp"),
                        (HM.DRA_DOF_LOWER, HM.DR_DOF_LOWER, "dof_lower"),
                        (HM.DRA_DOF_UPPER, HM.DR_DOF_UPPER, "dof_upper")):
        if DO.active(p, k, res.all):
            put_(k, slot, D, np.array(list(getattr(m, nm))[:D], F)[None])
    if DO.active(p, HM.DRA_OBJ_MASS, res.all):
        put_(HM.DRA_OBJ_MASS, HM.DR_OBJ_MASS, 1, np.full((1, 1), pool_mass), np.full((1, 1), pool_mass))
    if DO.active(p, HM.DRA_OBJ_FRIC, res.all):
        put_(HM.DRA_OBJ_FRIC, HM.DR_OBJ_FRIC, 1, F(p.friction))
    if DO.active(p, HM.DRA_OBJ_SCALE, res.all):
        put_(HM.DRA_OBJ_SCALE, HM.DR_OBJ_SCALE, 1, F(1.0))


@pytest.mark.parametrize("name", ["kuka", "hand"])
def test_golden_sequence_on_the_device(ref, name):  # noqa: F811
    need_gpu()
    from handarm_hip.sim import HandArmSim
    task, schema = TASKS[name]
    sc = copy.deepcopy(schema)
    sc["frequency"] = 3
    p, m, calls = golden_sequence(ref, name)
    n = ref[f"{name}_reset"].shape[1]
    sim = HandArmSim(n, "cuda:0", task_cfg={"task": task, "dr_enable": 1, "randomization_params": sc}, task=task)
    assert get(sim, "object_indices").max() == 0              # one object, pool entry 0, as _expected_rows takes it
    sim.bind_dr_replay()
    rows = get(sim, "dr_scale").copy()
    np.testing.assert_array_equal(rows, DR.default_rows(sim.model, sim.params, n))
    edge = 0
    gi = [HM.DRG_FIRST, HM.DRG_LAST_RAND, HM.DRG_EPOCH, HM.DRG_VALID]
    for c, (g_host, res, _) in enumerate(calls):
        frame = int(ref[f"{name}_frame"][c])
        g0 = get(sim, "dr_global").copy()
        g0.view(np.int32)[HM.DRG_FRAME_NEXT] = frame
        np.testing.assert_array_equal(g0.view(np.int32)[gi], g_host.view(np.int32)[gi], err_msg=f"call {c}: gate state")
        put(sim, "dr_global", g0)
        put(sim, "reset_buf", ref[f"{name}_reset"][c].astype(np.int64))
        put(sim, "randomize_buf", ref[f"{name}_rb_before"][c].astype(np.int32))
        sim.upload_dr_replay(res)
        sim.task_reset(REPLAY)
        _expected_rows(sim.params, sim.model, rows, res, frame)       # the other envs and slots: unchanged
        dev = get(sim, "dr_scale")
        np.testing.assert_array_equal(dev.view(np.int32), rows.view(np.int32), err_msg=f"call {c}: dr_scale")
        np.testing.assert_array_equal(get(sim, "randomize_buf"), ref[f"{name}_rb_after"][c], err_msg=f"call {c}")
        # the shard-wide state: the oracle's, with the gravity sampled from the uploaded draws
        g = DO.global_update(sim.params, g0.copy(), bool(ref[f"{name}_reset"][c].any()), 1)
        a = sim.params.dr_attr[HM.DRA_GRAVITY]
        if res.gravity is not None:
            og = np.array(list(sim.params.gravity), F) if res.all else g0[HM.DRG_GRAVITY_OG:HM.DRG_GRAVITY_OG + 3]
            g[HM.DRG_GRAVITY:HM.DRG_GRAVITY + 3] = value_from_draw(a, frame, og, None, res.gravity, False)
            if res.all:
                g[HM.DRG_GRAVITY_OG:HM.DRG_GRAVITY_OG + 3] = g[HM.DRG_GRAVITY:HM.DRG_GRAVITY + 3]
        gd = get(sim, "dr_global")
        np.testing.assert_array_equal(gd.view(np.int32), g.view(np.int32), err_msg=f"call {c}: dr_global")
        if name == "hand":
            np.testing.assert_allclose(gd[HM.DRG_GRAVITY:HM.DRG_GRAVITY + 3], ref["hand_gravity"][c], rtol=0, atol=2e-6)
        else:
            assert res.gravity is None
        edge += check_against_golden(
            ref, name, p, m, c, lambda k, env, elem: gd[HM.DRG_GRAVITY + elem] if k == HM.DRA_GRAVITY
            else dev[env, RR.DR_SLOT[k] + elem])
    assert edge <= 2


def _noise(x, corr, white, P, scaling=False):
    nz = (((corr * P[0] + P[1]).astype(F) + (white * P[2]).astype(F)).astype(F) + P[3]).astype(F)
    return (x * nz if scaling else x + nz).astype(F)


@pytest.mark.parametrize("dist", ["gaussian", "uniform"])
def test_observation_noise_from_uploaded_tensors(dist):
    """Ur5Sih, NO_PHYSICS steps at frame 150 of a constant 100-frame schedule: obs = teacher_obs + ((corr P0 + P1) +
    white P2) + P3 from the uploaded corr / white, bit for bit; a second step with a new white and the old corr."""
    need_gpu()
    from handarm_hip.sim import HandArmSim
    schema = {"frequency": 1, "observations": {"range": [0, 0.01] if dist == "gaussian" else [-0.02, 0.03],
                                               "range_correlated": [0, 0.005] if dist == "gaussian" else [-0.01, 0.02],
                                               "operation": "additive", "distribution": dist,
                                               "schedule": "constant", "schedule_steps": 100}}
    n = 64
    sim = HandArmSim(n, "cuda:0", task_cfg={"dr_enable": 1, "randomization_params": schema})
    bufs = sim.bind_dr_replay()
    g0 = get(sim, "dr_global").copy()
    g0.view(np.int32)[HM.DRG_FRAME_NEXT] = 150
    put(sim, "dr_global", g0)
    sim.t["reset_buf"][: n // 2] = 1
    rng = np.random.default_rng(1)
    no = sim.params.num_obs
    corr = rng.standard_normal((n, no)).astype(F)
    bufs["dr_obs_corr"].copy_(torch.from_numpy(corr))
    P = DO.noise_params(sim.params.dr_attr[HM.DRA_OBS], 150)
    assert P[2] != 0 and P[0] != 0
    for step in range(2):
        white = (rng.standard_normal((n, no)) if dist == "gaussian" else rng.random((n, no))).astype(F)
        bufs["dr_obs_white"].copy_(torch.from_numpy(white))
        sim.task_step(REPLAY)
        np.testing.assert_array_equal(get(sim, "dr_global")[HM.DRG_OBS:HM.DRG_OBS + 4], P)
        want = _noise(get(sim, "teacher_obs"), corr, white, P)
        np.testing.assert_array_equal(get(sim, "obs").view(np.int32), want.view(np.int32), err_msg=f"step {step}")
        assert np.abs(get(sim, "obs") - get(sim, "teacher_obs")).max() > 1e-3


def _kuka_sim(n, frame=35000):
    from handarm_hip.sim import HandArmSim
    sc = copy.deepcopy(DR.ALLEGRO_KUKA_SCHEMA)
    sim = HandArmSim(n, "cuda:0", task_cfg={"task": HM.TASK_ALLEGRO_KUKA, "dr_enable": 1, "randomization_params": sc},
                     task=HM.TASK_ALLEGRO_KUKA)
    g0 = get(sim, "dr_global").copy()
    g0.view(np.int32)[HM.DRG_FRAME_NEXT] = frame            # the 40000-frame noise schedules at 0.875
    put(sim, "dr_global", g0)
    return sim


def test_action_noise_from_uploaded_tensors():
    """AllegroKuka, ha_task_step_io, NO_PHYSICS: the stored actions are clamp(raw + noise) from the uploaded tensors; in
    the step that carries the first randomization (no noise lambda yet, vec_task.py:400-402) the clamped raw ones."""
    need_gpu()
    n = 64
    sim = _kuka_sim(n)
    bufs = sim.bind_dr_replay()
    na = sim.params.num_actions
    rng = np.random.default_rng(2)
    out = torch.zeros((n, sim.params.num_obs), device="cuda:0")
    for k in HM.DR_REPLAY_FIELDS[2:]:
        bufs[k].copy_(torch.from_numpy(rng.standard_normal(tuple(bufs[k].shape)).astype(F)))
    bufs["dr_draws"].copy_(torch.from_numpy(rng.random((n, HM.DR_SIZE)).astype(F)))
    corr, white = bufs["dr_act_corr"].cpu().numpy(), bufs["dr_act_white"].cpu().numpy()
    for step in range(2):
        raw = rng.uniform(-1.5, 1.5, (n, na)).astype(F)
        sim.task_step_io(REPLAY, torch.from_numpy(raw).to("cuda:0"), 1.0, out, 5.0)
        g = get(sim, "dr_global")
        assert g.view(np.int32)[HM.DRG_ACT_ON] == step
        x = raw if step == 0 else _noise(raw, corr, white, g[HM.DRG_ACT_USE:HM.DRG_ACT_USE + 4])
        np.testing.assert_array_equal(get(sim, "actions").view(np.int32), np.clip(x, F(-1), F(1)).view(np.int32),
                                      err_msg=f"step {step}")
    assert g[HM.DRG_ACT_USE + 2] > 0.04 and np.abs(x - raw).max() > 0.05


def test_flag_discipline():
    """Without the flag a sim whose replay buffers are bound (and full of huge values) steps bit-identically to one that
    never bound them; the flag without bound buffers is refused before anything launches."""
    need_gpu()
    from handarm_hip.sim import HandArmSim
    n = 64
    sims = [HandArmSim(n, "cuda:0", task_cfg={"dr_enable": 1}) for _ in range(2)]
    for b in sims[1].bind_dr_replay().values():
        b.fill_(1e30)
    for s in sims:
        s.t["reset_buf"][: n // 2] = 1
        for _ in range(2):
            s.task_step(HM.FLAG_NO_PHYSICS)
    assert np.abs(get(sims[0], "dr_scale")[:, HM.DR_LINK_MASS] - 1).max() > 0.1        # the hash path sampled
    for k in ("dr_scale", "obs", "dr_global", "randomize_buf"):
        np.testing.assert_array_equal(get(sims[0], k).view(np.int32), get(sims[1], k).view(np.int32), err_msg=k)
    before = {k: get(sims[0], k).copy() for k in ("dr_scale", "dr_global", "obs")}
    for launch in (sims[0].task_step, sims[0].task_reset, sims[0].task_observe):
        with pytest.raises(_lib.HandArmError):
            launch(HM.FLAG_NO_PHYSICS | HM.FLAG_REPLAY_DR)
    for k, v in before.items():
        np.testing.assert_array_equal(get(sims[0], k), v, err_msg=k)


def _run_task(cls, seed, steps, reference_rng=True, frame=None):
    cfg = {"env": {"numEnvs": 64}, "task": {"randomize": True}, "sim": {"reference_rng": reference_rng}}
    RR.set_seed(seed)
    env = cls(cfg, "cuda:0", "cuda:0")
    if frame is not None:
        g0 = get(env.sim, "dr_global").copy()
        g0.view(np.int32)[HM.DRG_FRAME_NEXT] = frame
        put(env.sim, "dr_global", g0)
    env.reset()
    gen = torch.Generator().manual_seed(0)                   # the policy's actions: not from the global generators
    for _ in range(steps):
        env.step((torch.rand((64, env.num_actions), generator=gen) * 2 - 1).to("cuda:0"))
    return {k: get(env.sim, k).copy() for k in ("dr_scale", "obs", "actions", "dr_global")}


@pytest.mark.parametrize("task", ["kuka", "hand"])
def test_identical_seeds_through_the_task_class(task):
    """sim.reference_rng + task.randomize: ref_rng.set_seed(5), reset() and a few steps, twice -> bit-identical
    dr_scale, obs and actions; seed 6 and reference_rng off give other samples. (AllegroKuka's schedules start at
    frame 0, where every range is a point: the run starts at frame 35000.)"""
    need_gpu()
    from handarm_hip.tasks import AllegroHand, AllegroKuka
    cls, steps, frame = (AllegroKuka, 4, 35000) if task == "kuka" else (AllegroHand, 2, None)
    a, b = _run_task(cls, 5, steps, frame=frame), _run_task(cls, 5, steps, frame=frame)
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.int32), b[k].view(np.int32), err_msg=k)
    used = slice(HM.DR_DOF_KD, HM.DR_DOF_KD + 16)
    assert np.abs(a["dr_scale"][:, used] - _run_task(cls, 6, steps, frame=frame)["dr_scale"][:, used]).max() > 1e-3
    assert np.abs(a["dr_scale"][:, used] - _run_task(cls, 5, steps, False, frame)["dr_scale"][:, used]).max() > 1e-3
    assert a["dr_global"].view(np.int32)[HM.DRG_EPOCH] >= 1 and np.abs(a["actions"]).max() > 0
