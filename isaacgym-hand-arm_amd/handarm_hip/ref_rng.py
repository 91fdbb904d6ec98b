"""Seed-faithful random draws: the reference's RNG stream, in the reference's order (cfg "reference_rng").

The reference draws its reset randomness from torch's GLOBAL generator of the sim device. On the path the
north_star names (sim_device=cpu, seeded by utils/utils.py:94 set_seed: random.seed, np.random.seed,
torch.manual_seed) that is the CPU generator. By default the fused kernels draw from a counter hash instead
(ha_task.h uniform01), which is fast and needs no host sync but matches nothing in the reference. With
``reference_rng`` on, the VecTask classes draw every reset value here, on the host, from that same global CPU
generator with the reference's calls (same functions, shapes and order), upload the values into
``ha_state_t.reset_draws`` and launch with HA_FLAG_REPLAY_DRAWS. A user who seeds like the reference then gets
the reference's reset indexing (target object, object configuration, goal, cube/hand resets).

The price is one device->host read of the reset flags per step (the reference reads them too, with
``nonzero()``) and one small upload.

Domain randomization (``task.randomize``) follows the same switch for AllegroKuka and AllegroHand: ``DrDraws`` makes
the reference's numpy draws of apply_randomizations (utils/dr_utils.py:98-130 through tasks/base/vec_task.py:756-864)
and the torch draws of its two noise lambdas (vec_task.py:700-754) on the host, in the reference's order, and the
kernels replay them (HA_FLAG_REPLAY_DR, the buffers of ha_bind_dr_replay). The device still decides which envs sample
(csrc/ha_dr.h); the host restates that decision (handarm_hip/dr.py gate) to know how many draws to make, which adds
one more small device->host read per step (randomize_buf and the 32-float dr_global, one copy) and a few uploads: the
white noise tensors every step, the correlated ones and the sampled envs' draw rows when they are redrawn. Nobody
has measured that cost; the default hash path pays none of it.
Ur5Sih keeps today's behaviour with both switches on: its schema is the build's own (handarm_hip/dr.py
UR5SIH_SCHEMA; the reference's Ur5Sih DR flag has no consumer), so there is no reference stream to follow and its
DR samples stay on the device counter hash.

Each function cites the reference lines whose draws it reproduces; the kernel-side slot layouts are documented
in csrc/ha_task.h (Ur5Sih), csrc/ak_task.h (AllegroKuka) and csrc/ah_task.h (AllegroHand).
"""
import math
import random

import numpy as np
import torch

from . import model as HM


def set_seed(seed, torch_deterministic=False):
    """utils/utils.py:88-110 set_seed: the seeding the reference's train.py does before building the task."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    return seed


def torch_rand_float(lower, upper, shape):
    """torch_jit_utils.py:216-218 on the CPU global generator."""
    return (upper - lower) * torch.rand(*shape, device="cpu") + lower


# --------------------------------------------------------------------------- HandArm (Ur5Sih)
def ur5sih_reset_draws(n, num_initial_poses, num_objects):
    """reset_idx of all envs (multi_object_manipulation.py:62-91,193-230): _reset_objects'
    torch.randint(num_initial_poses, (n,)), _reset_target_object's torch.randint(num_objects, (n,)), then
    _reset_goal -> _get_random_object_pos(..., 'goal')'s torch.rand((n, 3)).
    Returns (n, 5) float32 in the ha_task.h replay slots: [cfg index, target index, goal rand x3]."""
    cfg = torch.randint(num_initial_poses, (n,), dtype=torch.int64, device="cpu")
    tgt = torch.randint(num_objects, (n,), dtype=torch.int64, device="cpu")
    goal = torch.rand((n, 3), dtype=torch.float32, device="cpu")
    return torch.cat([cfg.float()[:, None], tgt.float()[:, None], goal], 1)


def ur5sih_drop_pose(n, pos, noise):
    """One drop of n objects (multi_object_manipulation.py:107-110): _get_random_object_pos(env_ids, 'drop')
    (:175-184: torch.rand((n, 3)), noise @ diag) then _get_random_quat (:186-191: torch_rand_float(-1, 1, (n, 2)),
    randomize_rotation). Returns CPU (pos (n, 3), quat (n, 4))."""
    from .torch_utils import randomize_rotation
    p = torch.tensor(pos, dtype=torch.float32).unsqueeze(0).repeat(n, 1)
    r = 2 * (torch.rand((n, 3), dtype=torch.float32, device="cpu") - 0.5)
    p = p + r @ torch.diag(torch.tensor(noise, dtype=torch.float32))
    rf = torch_rand_float(-1.0, 1.0, (n, 2))
    return p, randomize_rotation(rf[:, 0], rf[:, 1])


# --------------------------------------------------------------------------- AllegroKuka
def kuka_force_prob(n, prob_range):
    """random_force_prob (allegro_kuka_base.py:323-327 at __init__, :1262-1266 in reset_idx): one torch.rand(n).
    Returns (draw, prob) in float32 with the reference's arithmetic on the CPU."""
    r = torch.tensor(prob_range, dtype=torch.float32)
    u = torch.rand(n, device="cpu")
    return u, torch.exp((torch.log(r[0]) - torch.log(r[1])) * u + torch.log(r[1]))


class KukaDraws:
    """The draws of one AllegroKuka pre_physics_step (allegro_kuka_base.py:1355-1414), slot layout of ak_task.h.

    The per-step force selection ``torch.rand(N) < random_force_prob`` is made here, with the reference's CPU
    arithmetic and the host copy of random_force_prob; the kernel gets the decision as draw 0 (selected) or 1
    (not selected) in slot 71 (2 G + 53), which its ``u < prob`` test reproduces for every prob in (0, 1)."""

    def __init__(self, num_envs, subtask, prob_range, force_scale):
        self.n = num_envs
        self.subtask = subtask
        self.regrasping = subtask == "regrasping"
        self.G = 10 if subtask == "throw" else 9        # draws of one reset_target_pose (ak_task.h ak_goal_draws)
        self.prob_range = prob_range
        self.force_scale = force_scale
        _, self.prob = kuka_force_prob(num_envs, prob_range)          # __init__ draw (:323-327)

    def _target(self, D, ids, base):
        """reset_target_pose -> _reset_target (regrasping.py:76-98 / reorientation.py:104-128 / throw.py:85-103)."""
        k = len(ids)
        if self.subtask == "throw":
            D[ids, base:base + 1] = torch_rand_float(-1.0, 1.0, (k, 1))     # left / right of the table
            D[ids, base + 1:base + 2] = torch_rand_float(0, 0.4, (k, 1))
            D[ids, base + 2:base + 3] = torch_rand_float(-1.0, 0.7, (k, 1))
            D[ids, base + 3:base + 4] = torch_rand_float(0.0, 1.0, (k, 1))
            self._object(D, ids, base + 4)
            return
        D[ids, base:base + 3] = torch_rand_float(0.0, 1.0, (k, 3))
        if self.regrasping:
            self._object(D, ids, base + 3)                              # reset_object_pose (:1196-1220)
        else:
            D[ids, base + 3:base + 6] = torch_rand_float(0, 1.0, (k, 3))    # get_random_quat (:1178-1189)

    @staticmethod
    def _object(D, ids, base):
        k = len(ids)
        D[ids, base:base + 3] = torch_rand_float(-1.0, 1.0, (k, 3))
        D[ids, base + 3:base + 6] = torch_rand_float(0, 1.0, (k, 3))

    def step(self, reset, reset_goal, forces=True):
        """reset / reset_goal: host bool/int (N,) flags; forces=False for a bare reset_idx call (no
        pre_physics_step force draw). Returns (draws (N, HA_DRAW_STRIDE) float32, raw dict)."""
        N = self.n
        D = torch.zeros((N, HM.DRAW_STRIDE), dtype=torch.float32)
        goal_ids = torch.as_tensor(reset_goal).nonzero(as_tuple=False).squeeze(-1)
        env_ids = torch.as_tensor(reset).nonzero(as_tuple=False).squeeze(-1)
        self._target(D, goal_ids, 0)                                    # reset_target_pose(reset_goal_env_ids)
        G = self.G
        if len(env_ids) > 0:                                            # reset_idx(reset_env_ids), :1246-1353
            self._target(D, env_ids, G)
            self._object(D, env_ids, 2 * G)
            u, p = kuka_force_prob(len(env_ids), self.prob_range)
            D[env_ids, 2 * G + 6] = u
            self.prob[env_ids] = p
            D[env_ids, 2 * G + 7:2 * G + 30] = torch_rand_float(0.0, 1.0, (len(env_ids), 23))
            D[env_ids, 2 * G + 30:2 * G + 53] = torch_rand_float(-1.0, 1.0, (len(env_ids), 23))
        raw = {"force_u": None}
        if forces and self.force_scale > 0.0:                           # :1399-1410
            u = torch.rand(N, device="cpu")
            sel = (u < self.prob).nonzero()
            g = torch.randn((len(sel), 1, 3), device="cpu")
            D[:, 2 * G + 53] = 1.0
            D[sel[:, 0], 2 * G + 53] = 0.0
            D[sel[:, 0], 2 * G + 54:2 * G + 57] = g.reshape(len(sel), 3)
            raw["force_u"] = u
        return D, raw


# --------------------------------------------------------------------------- AllegroHand
class AllegroDraws:
    """The draws of one AllegroHand pre_physics_step (allegro_hand.py:586-599), slot layout of ah_task.h."""

    def __init__(self, num_envs, num_dofs=16, force_scale=0.0, force_prob_range=(0.001, 0.1)):
        self.n = num_envs
        self.nd = num_dofs
        self.force_scale = float(force_scale)
        self.lo, self.hi = torch.tensor(force_prob_range, dtype=torch.float32)
        self.prob = self._prob(torch.rand(num_envs, device="cpu"))     # random_force_prob at __init__ (:191-194)

    def _prob(self, u):
        return torch.exp((torch.log(self.lo) - torch.log(self.hi)) * u + torch.log(self.hi))

    def step(self, reset, reset_goal):
        N = self.n
        D = torch.zeros((N, HM.DRAW_STRIDE), dtype=torch.float32)
        env_ids = torch.as_tensor(reset).nonzero(as_tuple=False).squeeze(-1)
        goal_ids = torch.as_tensor(reset_goal).nonzero(as_tuple=False).squeeze(-1)
        if len(goal_ids) > 0:                                           # reset_target_pose (:506-521)
            D[goal_ids, 0:4] = torch_rand_float(-1.0, 1.0, (len(goal_ids), 4))
        if len(env_ids) > 0:                                            # reset_idx (:524-584)
            R = len(env_ids)
            D[env_ids, 4:4 + 2 * self.nd + 5] = torch_rand_float(-1.0, 1.0, (R, 2 * self.nd + 5))
            D[env_ids, 41:45] = torch_rand_float(-1.0, 1.0, (R, 4))   # reset_target_pose(env_ids)
            u = torch.rand(R, device="cpu")                             # random_force_prob (:557-560)
            D[env_ids, 45] = u
            self.prob[env_ids] = self._prob(u)
        if self.force_scale > 0.0:                                      # random forces (:617-623)
            u = torch.rand(N, device="cpu")
            D[:, 46] = u
            idx = (u < self.prob).nonzero(as_tuple=False)              # force_indices, (k, 1)
            g = torch.randn((len(idx), 1, 3), device="cpu")
            D[idx[:, 0], 47:50] = g[:, 0, :]
            D[idx[:, 0], 50] = 1.0                                      # the selection (ah_task.h AH_DRAW_FORCE_SEL)
        return D


# --------------------------------------------------------------------------- domain randomization
# HA_DRA_* of an actor property -> first dr_scale / dr_draws slot of its elements
DR_SLOT = {HM.DRA_LINK_MASS: HM.DR_LINK_MASS, HM.DRA_LINK_FRIC: HM.DR_LINK_FRIC, HM.DRA_DOF_KD: HM.DR_DOF_KD,
           HM.DRA_DOF_KP: HM.DR_DOF_KP, HM.DRA_DOF_LOWER: HM.DR_DOF_LOWER, HM.DRA_DOF_UPPER: HM.DR_DOF_UPPER,
           HM.DRA_OBJ_MASS: HM.DR_OBJ_MASS, HM.DRA_OBJ_FRIC: HM.DR_OBJ_FRIC, HM.DRA_OBJ_SCALE: HM.DR_OBJ_SCALE}
# the reference schemas' order (AllegroKuka.yaml:143-207, AllegroHand.yaml:88-150), when no plan is given
DR_PLAN = [("robot", "dof", [HM.DRA_DOF_KD, HM.DRA_DOF_KP, HM.DRA_DOF_LOWER, HM.DRA_DOF_UPPER]),
           ("robot", "body", [HM.DRA_LINK_MASS]), ("robot", "shape", [HM.DRA_LINK_FRIC]),
           ("object", "scale", [HM.DRA_OBJ_SCALE]), ("object", "body", [HM.DRA_OBJ_MASS]),
           ("object", "shape", [HM.DRA_OBJ_FRIC])]
U_BELOW_ONE = np.float32(1.0 - 2.0 ** -24)      # a double quantile just under 1 must not round up to 1


class DrApplied:
    """One apply_randomizations call's draws: `nonenv` / `all` / `envs` as dr.gate returns them, `draws` the
    (N, HA_DR_SIZE) float32 rows (the sampled envs' drawn slots filled, zero elsewhere), `gravity` the 3 gravity draws
    (None when this call drew none)."""

    def __init__(self, nonenv, all_, envs, draws, gravity):
        self.nonenv, self.all, self.envs, self.draws, self.gravity = nonenv, all_, envs, draws, gravity


class DrDraws:
    """The reference's DR draws of one VecTask.step on the host's global generators, in its order.

    ``apply`` is one apply_randomizations call (vec_task.py:646-876): numpy's legacy global stream, through
    ``np.random.uniform(0, 1, shape)`` / ``np.random.normal(0, 1, shape)``, which consume it exactly as the
    reference's ``uniform(lo, hi, shape)`` / ``normal(mu, var, shape)`` (dr_utils.py:98-130) do; the quantile / standard
    normal is what the kernel takes (csrc/ha_dr.h dr_value scales it with the scheduled range). Order: the sim_params
    gravity 3-vector when the non-env part runs (:756-786), then per actor in the schema's order, per sampled env in
    ascending id, per property in the schema's order (:788-864): a dof_properties attribute is one D-vector, a body /
    shape list property goes element by element and attribute by attribute within it, the object's scale is one draw;
    after the first randomization a robot list property draws only its ``later_elems`` elements and setup_only
    attributes draw nothing (handarm_hip/dr.py).

    ``noise`` is the torch side of one VecTask.step (vec_task.py:390-441) on the global CPU generator: the action
    lambda, the task's own pre-physics draws (KukaDraws.step / AllegroDraws.step), the observation lambda. A lambda
    draws ``corr`` (randn of the tensor's shape) when a non-env randomization has run since it last did, then
    ``white`` (randn, or rand for the uniform distribution); VecTask.reset() adds no noise and draws nothing.

    params / model: the sim's HaParams / HaModel; plan: dr.draw_plan of the schema (None: the reference yamls' order).
    """

    def __init__(self, params, model, num_envs, plan=None):
        self.n = int(num_envs)
        self.frequency = int(params.dr_frequency)
        a = params.dr_attr
        self.dist = [int(a[k].dist) for k in range(HM.DRA_N)]
        self.setup_only = [int(a[k].setup_only) for k in range(HM.DRA_N)]
        self.later_elems = [int(a[k].later_elems) for k in range(HM.DRA_N)]
        self.L, self.D, self.NO = int(model.n_links), int(model.n_dofs), int(params.n_objects)
        if self.NO != 1:
            raise NotImplementedError("reference_rng with task.randomize: one object actor (the Allegro scenes)")
        self.num_obs, self.num_actions = int(params.num_obs), int(params.num_actions)
        plan = DR_PLAN if plan is None else plan
        self.actors = []                                  # [(kind, [(group, [HA_DRA_*])])] in the schema's order
        for kind, group, idxs in plan:
            idxs = [k for k in idxs if self.dist[k]]
            if not idxs:
                continue
            if not self.actors or self.actors[-1][0] != kind:
                self.actors.append((kind, []))
            self.actors[-1][1].append((group, idxs))
        # dr_randomizations of the two lambdas: filled by the first non-env randomization; its 'corr' entry is dropped
        # by every later one (vec_task.py:727-728,753-754 replace the dict)
        self.valid = False
        self.pending = {HM.DRA_OBS: False, HM.DRA_ACT: False}

    def _draw(self, k, shape):
        """One generate_random_samples call of attribute k: float32 quantile(s) in [0, 1) or standard normal(s)."""
        if self.dist[k] == HM.DR_DIST["gaussian"]:
            return np.asarray(np.random.normal(0.0, 1.0, shape), np.float64).astype(np.float32)
        u = np.asarray(np.random.uniform(0.0, 1.0, shape), np.float64).astype(np.float32)
        return np.minimum(u, U_BELOW_ONE)

    def _active(self, k, all_):
        return self.dist[k] != 0 and (all_ or not self.setup_only[k])

    def _elems(self, k, all_):
        if not self._active(k, all_):
            return 0
        return self.L if (all_ or self.later_elems[k] < 0) else min(self.L, self.later_elems[k])

    def apply(self, g, reset, randomize_buf):
        """The draws of the apply_randomizations call the next step / reset launch will run. g: dr_global as that
        launch will read it; reset: the reset flags; randomize_buf: the per-env counts (dr.gate). -> DrApplied."""
        from . import dr as DR
        nonenv, all_, envs = DR.gate(g, self.frequency, reset, randomize_buf)
        gravity = None
        if nonenv and self.dist[HM.DRA_GRAVITY]:
            gravity = self._draw(HM.DRA_GRAVITY, 3)
        rows = np.zeros((len(envs), HM.DR_SIZE), np.float32)
        ids = np.nonzero(envs)[0]
        for kind, groups in self.actors:
            for e in ids:
                row = rows[e]
                for group, idxs in groups:
                    if group == "dof":
                        for k in idxs:
                            if self._active(k, all_):
                                row[DR_SLOT[k]:DR_SLOT[k] + self.D] = self._draw(k, self.D)
                    elif kind == "robot":
                        n = [self._elems(k, all_) for k in idxs]
                        for i in range(max(n)):
                            for k, nk in zip(idxs, n):
                                if i < nk:
                                    row[DR_SLOT[k] + i] = self._draw(k, 1)[0]
                    else:
                        for k in idxs:
                            if self._active(k, all_):
                                row[DR_SLOT[k]] = self._draw(k, 1)[0]
        return DrApplied(nonenv, all_, envs, rows, gravity)

    def _lambda(self, k, width):
        """noise_lambda of observations / actions: (corr or None when it is not redrawn, white), CPU float32."""
        if not self.valid or not self.dist[k]:
            return None, None
        corr = None
        if self.pending[k]:
            corr = torch.randn((self.n, width), dtype=torch.float32, device="cpu")
            self.pending[k] = False
        draw = torch.randn if self.dist[k] == HM.DR_DIST["gaussian"] else torch.rand
        return corr, draw((self.n, width), dtype=torch.float32, device="cpu")

    def noise(self, nonenv, task_draws=None, step=True):
        """The torch draws of one VecTask.step. nonenv: this step's apply() ran the non-env randomization (the
        observation lambda then redraws corr in this very step, the action lambda in the next); task_draws: a
        callable making the task's own pre-physics draws between the two lambdas; step=False: a bare reset_idx call
        (no lambda runs, the randomization is only noted). Returns {"act_corr", "act_white", "task", "obs_corr",
        "obs_white"}: tensors to upload, None for what was not drawn."""
        out = dict.fromkeys(("act_corr", "act_white", "task", "obs_corr", "obs_white"))
        if step:
            out["act_corr"], out["act_white"] = self._lambda(HM.DRA_ACT, self.num_actions)
        if task_draws is not None:
            out["task"] = task_draws()
        if nonenv:
            self.valid = True
            self.pending[HM.DRA_OBS] = self.pending[HM.DRA_ACT] = True
        if step:
            out["obs_corr"], out["obs_white"] = self._lambda(HM.DRA_OBS, self.num_obs)
        return out


def dr_draws_for(sim, task):
    """DrDraws of a HandArmSim with its replay buffers bound (the task classes, reference_rng + task.randomize)."""
    from . import dr as DR
    dd = DrDraws(sim.params, sim.model, sim.num_envs, DR.draw_plan(sim.cfg.get("randomization_params"), task))
    sim.bind_dr_replay()
    return dd


def dr_replay_step(sim, dd, reset, task_draws, step=True):
    """One step's (step=False: one bare reset_idx call's) DR draws for the launch that follows: the gate's inputs in
    one device->host read (randomize_buf and dr_global; `reset` is the host copy of the reset flags the caller
    already has), DrDraws.apply / noise around the task's own draws, and the uploads. Returns task_draws()'s result."""
    n = sim.num_envs
    buf = torch.cat([sim.t["randomize_buf"], sim.t["dr_global"].view(torch.int32)]).cpu().numpy()
    res = dd.apply(buf[n:].view(np.float32), np.asarray(reset), buf[:n])
    nz = dd.noise(res.nonenv, task_draws, step)
    sim.upload_dr_replay(res, nz)
    return nz["task"]


_ = math
