"""Gym-style simulation object over the HIP library: the lower surface the reference task code uses.

``HandArmSim`` owns one ``ha_handle`` and every device tensor (torch, on ``device``). Method names and
semantics follow the Isaac Gym tensor API the hand_arm task calls:

  acquire_actor_root_state_tensor / acquire_rigid_body_state_tensor / acquire_dof_state_tensor /
  acquire_net_contact_force_tensor   -> the live state tensors (zero-copy: they ARE the sim state)
  refresh_*                          -> no-ops (the kernels write the tensors in place)
  acquire_jacobian_tensor / acquire_mass_matrix_tensor -> derived tensors, allocated on first use;
  refresh_jacobian_tensors / refresh_mass_matrix_tensors -> one kernel launch from the current dof_state
  acquire_contact_tensor / refresh_contact_tensor -> the narrow phase's contact list of the current state (derived
                                        too; one query launch that changes no state; gym.get_rigid_contacts)
  simulate(n)                        -> n gym.simulate() calls in ONE kernel launch
  set_actor_root_state_tensor_indexed / set_dof_state_tensor_indexed /
  set_dof_position_target_tensor(_indexed)  -> copy-in for the listed global actor indices (int32)

Difference to Isaac Gym worth knowing: because the acquired tensors are the simulation state,
writes into them take effect even without a set_*_indexed call (the reference always calls it).
"""
import ctypes as C
import os

import torch

from . import _lib
from . import model as HM

TORCH_DTYPE = {"float32": torch.float32, "int64": torch.int64, "uint8": torch.uint8, "int32": torch.int32,
               "uint32": torch.int32}


class HandArmSim:
    def __init__(self, num_envs, device="cuda:0", task_cfg=None, scene=None, pool_names=None, stats_ring=64,
                 task=None, rebalance_every=None):
        if not str(device).startswith("cuda"):
            raise _lib.HandArmError("libhandarm_hip runs on a HIP device only (device must be 'cuda:N')")
        self.lib = _lib.load()
        self.device = torch.device(device)
        if task is None:
            task = (task_cfg or {}).get("task", HM.TASK_UR5SIH)
        self.task = task
        default_scene = {HM.TASK_ALLEGRO_HAND: HM.ALLEGRO_ASSET, HM.TASK_ALLEGRO_KUKA: HM.KUKA_ASSET}.get(task, HM.ASSET)
        self.scene = scene if scene is not None else HM.load_scene(default_scene)
        self.model = HM.build_model(self.scene, pool_names, posed=HM.posed_group(task, task_cfg))
        self.params, self.cfg = HM.build_params(task_cfg, task=task)
        self.num_envs = num_envs
        self.n_obj = self.params.n_objects
        self.num_dofs = self.model.n_dofs
        self.num_links = self.model.n_links
        self.num_actors = self.model.n_actors
        self.num_bodies = self.model.n_bodies
        self.stats_ring = stats_ring
        spec = HM.state_spec(num_envs, n_links=self.num_links, n_dofs=self.num_dofs, n_obj=self.n_obj,
                             num_initial_poses=self.params.num_initial_poses, num_actions=self.params.num_actions,
                             num_obs=self.params.num_obs, n_actors=self.num_actors, n_bodies=self.num_bodies,
                             n_pcm_slots=HM.pcm_slots(self.model, self.n_obj, self.params),
                             num_states=HM.num_states(self.params))
        spec["stats"] = ((stats_ring, HM.STAT_SIZE), spec["stats"][1])
        spec["term_sums"] = ((stats_ring, 4), spec["term_sums"][1])
        with torch.cuda.device(self.device):
            self.t = {k: torch.zeros(shape, dtype=TORCH_DTYPE[dt.__name__], device=self.device)
                      for k, (shape, dt) in spec.items()}
        self.t["root_state"].view(num_envs, self.num_actors, 13)[..., 6] = 1.0
        self.t["goal_state"][:, 6] = 1.0
        self.t["collision_enabled"].fill_(1)
        if task == HM.TASK_ALLEGRO_HAND:          # objectType: the scene's pool entry in every env
            self.t["object_indices"].fill_(int(self.params.ah_object_type))
        # domain-randomization rows start at the nominal values (mass ratio 1, friction, the model's DOF gains and
        # limits, scale 1) until an env's first sample, and the shard-wide state at frame 0 (handarm_hip/dr.py)
        from . import dr as DR
        self.t["dr_scale"].copy_(torch.from_numpy(DR.default_rows(self.model, self.params, num_envs)))
        self.t["dr_global"].copy_(torch.from_numpy(DR.init_global(self.params)))
        if task == HM.TASK_ALLEGRO_KUKA:
            self._init_kuka()
        h = C.c_void_p()
        if task == HM.TASK_ALLEGRO_HAND:            # object_rb_masses (allegro_hand.py:355-357): the object's mass
            self.params.ah_object_rb_mass = self.model.pool_mass[self.params.ah_object_type]
        _lib.check(self.lib.ha_create(C.byref(self.model), C.byref(self.params), num_envs, C.byref(h)), "ha_create")
        self.h = h
        # Jacobian / mass-matrix tensors (ha_refresh_kinematics), allocated by their acquire calls: derived from
        # dof_state, not simulation state, so snapshot() / restore() leave them out (refresh after a restore)
        self._jac = self._jac_key = self._jac_links = self._mm = None
        # contact tensor and counts (ha_refresh_contacts), allocated by acquire_contact_tensor: derived too
        self._contacts = self._contact_counts = None
        # contacts per substep the kernel family holds (clutter 84, Ur5Sih 21, AllegroKuka 21, AllegroHand 12)
        self.contact_capacity = int(self.lib.ha_contact_capacity(self.h))
        # persistent-manifold records per env (the contact_cache rows; zero = empty)
        assert int(self.lib.ha_contact_cache_slots(self.h)) == self.t["contact_cache"].shape[1]
        self.state = HM.HaState()
        null = HM.null_fields(task)
        for k in HM.STATE_FIELDS:
            setattr(self.state, k, None if k in null else self.t[k].data_ptr())
        _lib.check(self.lib.ha_bind_state(self.h, C.byref(self.state)), "ha_bind_state")
        _lib.check(self.lib.ha_set_stats_ring(self.h, stats_ring), "ha_set_stats_ring")
        # longest-first dispatch order of the fused step (ha_set_env_order), refreshed every `rebalance_every` steps
        # (0: identity order; one ha_update_env_order launch per refresh). An explicit argument wins; HA_REBALANCE (A/B
        # scripts) only replaces the default 1
        if rebalance_every is None:
            rebalance_every = int(os.environ.get("HA_REBALANCE", 1))
        self.rebalance_every = int(rebalance_every)
        self._snake = int(os.environ.get("HA_ORDER_SNAKE", 0))     # A/B: alternate-block reversal of the order
        # the refresh sorts by each env's workgroup span in the last step launch (round 4: C4 +13% against the
        # contacts offered). AllegroHand sorts by the contacts offered instead: its spans repeat poorly from step to
        # step (correlation 0.38 against C5's 0.60, profiles/r06_order_quality.txt) and the contact count, which
        # tracks an env's span at 0.8, measured its kernel 0.5-0.7% faster. HA_ORDER_COST overrides (A/B runs)
        order_cost = os.environ.get("HA_ORDER_COST", "contacts" if task == HM.TASK_ALLEGRO_HAND else "time")
        if order_cost not in ("time", "contacts"):
            raise ValueError(f"HA_ORDER_COST must be 'time' or 'contacts', not {order_cost!r}")
        self.order_cost = order_cost
        self._rb_count = 0
        if self.rebalance_every > 0:
            self._env_order = torch.arange(num_envs, dtype=torch.int32, device=self.device)
            self._cost_prev = torch.zeros(num_envs, dtype=torch.int32, device=self.device)
            if order_cost == "time":
                _lib.check(self.lib.ha_set_order_cost(self.h, 1), "ha_set_order_cost")
                self._cost_prev.zero_()             # the estimates restart with the cost they measure
            _lib.check(self.lib.ha_set_env_order(self.h, C.c_void_p(self._env_order.data_ptr()), num_envs),
                       "ha_set_env_order")

    def snapshot(self):
        """Device copy of the env-state SoA (every tensor the kernels read or write: gym state tensors, targets,
        controller and task state, counters, DR rows, draws). restore() puts the shard back exactly, so the next
        steps reproduce bit for bit (SURVEY.md §5 checkpoint row; the task classes' get_env_state / set_env_state
        keep the host-side curriculum values, as in the reference). One device-to-device copy per tensor."""
        return {k: v.clone() for k, v in self.t.items()}

    def restore(self, snap):
        """Copy a snapshot() back into the bound tensors (same shapes; the kernels keep their pointers)."""
        for k, v in snap.items():
            self.t[k].copy_(v)

    def rebalance(self):
        """Dispatch the envs that offered the most contacts since the last call first (device argsort, stable, no
        host sync). In a launch with more envs than resident workgroup slots, the slots that free up take the
        cheaper envs last, so the launch's tail shrinks (longest-processing-time order); a one-round launch spreads
        its heavy envs over the CUs. Results do not depend on the order (one workgroup per env)."""
        _lib.check(self.lib.ha_update_env_order(self.h, C.c_void_p(self._env_order.data_ptr()),
                                                C.c_void_p(self._cost_prev.data_ptr()), self._snake, self._stream()),
                   "ha_update_env_order")

    def _init_kuka(self):
        """AllegroKuka buffers at env creation: per-env object dims and keypoint offsets, goal_states
        (object start - 0.04 z, allegro_kuka_base.py:738-740), object/goal root states, the tolerance
        scalars, random_force_prob drawn at __init__ (:339-343) and the -1 'unset' markers (:356-360).
        reset_buf / reset_goal_buf start at 1 (vec_task.py allocate_buffers), so the first step resets all."""
        N, c, p = self.num_envs, self.cfg, self.params
        scales, offs = HM.kuka_env_tables(N, self.scene, c)
        self.t["object_scale"].copy_(torch.from_numpy(scales))
        ts = self.t["task_state"]
        ts[:, HM.AK_KP:HM.AK_KP + 12] = torch.from_numpy(offs.reshape(N, 12)).to(self.device)
        ts[:, HM.AK_CLOSEST_KP] = -1.0
        ts[:, HM.AK_CLOSEST_FT:HM.AK_CLOSEST_FT + 4] = -1.0
        ts[:, HM.AK_FURTHEST] = -1.0
        g = torch.Generator(device=self.device).manual_seed(int(p.seed))
        lo, hi = torch.log(torch.tensor(c["force_prob_range"], device=self.device))
        ts[:, HM.AK_FORCE_PROB] = torch.exp((lo - hi) * torch.rand(N, device=self.device, generator=g) + hi)
        init = torch.tensor(list(p.ak_object_init), device=self.device)
        self.t["goal_state"][:, 0:3] = init
        self.t["goal_state"][:, 2] -= 0.04
        root = self.t["root_state"].view(N, self.num_actors, 13)
        root[:, self.model.actor_object0, 0:3] = init
        root[:, self.model.actor_goal, 0:3] = self.t["goal_state"][:, 0:3]
        if p.ak_subtask == 2:
            # throw: the bucket actor at bucket_pose = allegro_pose + (-0.6, -1, 0.45) in gymapi.Vec3 (float32) until
            # the first reset places it (allegro_kuka_throw.py:68-72)
            root[:, self.model.actor_goal, 0:3] = torch.tensor(HM.AK_BUCKET_POSE, device=self.device)
        root[:, self.model.actor_table, 0:3] = torch.tensor(list(self.model.table_pos), device=self.device)
        self.t["task_scalars"].copy_(torch.from_numpy(HM.kuka_tolerance_scalars(c["success_tolerance"], c)))
        self.t["reset_buf"].fill_(1)
        self.t["reset_goal_buf"].fill_(1)
        self.t["dof_state"].view(N, self.num_dofs, 2)[..., 0] = torch.tensor(list(p.reset_pose)[:self.num_dofs],
                                                                              device=self.device)
        self.t["dof_position_targets"].copy_(self.t["dof_state"].view(N, self.num_dofs, 2)[..., 0])
        self.t["sim_targets"].copy_(self.t["dof_position_targets"])

    # -------------------------------------------------------------- helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.ha_destroy(self.h)
        except Exception:
            pass

    # -------------------------------------------------------------- Isaac Gym tensor API
    def acquire_actor_root_state_tensor(self):
        return self.t["root_state"]

    def acquire_rigid_body_state_tensor(self):
        return self.t["rigid_body_state"]

    def acquire_dof_state_tensor(self):
        return self.t["dof_state"]

    def acquire_net_contact_force_tensor(self):
        return self.t["net_contact_force"]

    def refresh_actor_root_state_tensor(self):
        _lib.check(self.lib.ha_refresh(self.h, self._stream()), "ha_refresh")

    refresh_rigid_body_state_tensor = refresh_actor_root_state_tensor
    refresh_dof_state_tensor = refresh_actor_root_state_tensor
    refresh_net_contact_force_tensor = refresh_actor_root_state_tensor

    def acquire_jacobian_tensor(self, links=None):
        """gym.acquire_jacobian_tensor: (N, L-1, 6, D), Isaac Gym's fixed-base shape (the base link is omitted: model
        link i is jac[:, i-1]); rows 0..2 the linear velocity of the link frame origin, 3..5 the angular velocity, env
        frame. ``links`` (model link indices in 1..L-1): (N, len(links), 6, D) of those links only. Allocated and
        filled for the current dof_state by the first call; later calls return the same tensor."""
        key = None if links is None else tuple(int(i) for i in links)
        if self._jac is not None:
            if key != self._jac_key:
                raise _lib.HandArmError("the Jacobian tensor was acquired with another link list")
            return self._jac
        if key is not None:
            if not 1 <= len(key) <= HM.MAX_LINKS or any(not 1 <= i < self.num_links for i in key):
                raise _lib.HandArmError(f"links must be 1..{HM.MAX_LINKS} link indices in 1..{self.num_links - 1}")
            self._jac_links = torch.tensor(key, dtype=torch.int32, device=self.device)
        k = self.num_links - 1 if key is None else len(key)
        self._jac_key = key
        self._jac = torch.zeros((self.num_envs, k, 6, self.num_dofs), dtype=torch.float32, device=self.device)
        self._refresh_kinematics()
        return self._jac

    def acquire_mass_matrix_tensor(self):
        """gym.acquire_mass_matrix_tensor: (N, D, D), the joint-space inertia the step uses (armature on the diagonal,
        the env's DR link-mass scales when dr_enable). Allocated and filled by the first call."""
        if self._mm is None:
            self._mm = torch.zeros((self.num_envs, self.num_dofs, self.num_dofs), dtype=torch.float32,
                                   device=self.device)
            self._refresh_kinematics()
        return self._mm

    def _refresh_kinematics(self):
        if self._jac is None and self._mm is None:
            raise _lib.HandArmError("refresh before acquire_jacobian_tensor / acquire_mass_matrix_tensor")
        k = HM.HaKinematics(self._jac.data_ptr() if self._jac is not None else None,
                            self._mm.data_ptr() if self._mm is not None else None,
                            self._jac_links.data_ptr() if self._jac_links is not None else None,
                            len(self._jac_key) if self._jac_key is not None else 0)
        _lib.check(self.lib.ha_refresh_kinematics(self.h, C.byref(k), self._stream()), "ha_refresh_kinematics")

    def refresh_jacobian_tensors(self):
        """One launch on the current stream; it writes the mass matrix too when that is acquired."""
        if self._jac is None:
            raise _lib.HandArmError("refresh_jacobian_tensors before acquire_jacobian_tensor")
        self._refresh_kinematics()

    def refresh_mass_matrix_tensors(self):
        """One launch on the current stream; it writes the Jacobian too when that is acquired."""
        if self._mm is None:
            raise _lib.HandArmError("refresh_mass_matrix_tensors before acquire_mass_matrix_tensor")
        self._refresh_kinematics()

    def acquire_contact_tensor(self):
        """The contacts of the current state as tensors: ``(contacts (N, contact_capacity, 20) float32, counts (N, 2)
        int32)``. Row layout in include/handarm_abi.h (ha_contacts_t): x, n (from body b to body a), sep, the body
        codes, the rigid_body_state rows of both bodies and the two surface points in their bodies' frames.
        counts[:, 0] rows of an env are valid (the rest keep what they held), counts[:, 1] is what the narrow phase
        offered. Allocated and filled for the current state by the first call; later calls return the same tensors."""
        if self._contacts is None:
            self._contacts = torch.zeros((self.num_envs, self.contact_capacity, HM.CONTACT_REC), dtype=torch.float32,
                                         device=self.device)
            self._contact_counts = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self.device)
            self.refresh_contact_tensor()
        return self._contacts, self._contact_counts

    def refresh_contact_tensor(self, env_ids=None):
        """One launch on the current stream: FK and the narrow phase on the bound state (persistent manifolds off),
        writing only the contact tensor and its counts. env_ids (int32 device tensor of distinct env indices): those
        envs only, the others' rows and counts stay."""
        if self._contacts is None:
            raise _lib.HandArmError("refresh_contact_tensor before acquire_contact_tensor")
        ids = None if env_ids is None else env_ids.to(device=self.device, dtype=torch.int32).contiguous()
        k = HM.HaContacts(self._contacts.data_ptr(), self._contact_counts.data_ptr(), self._contacts.shape[1],
                          ids.data_ptr() if ids is not None else None, int(ids.numel()) if ids is not None else 0)
        _lib.check(self.lib.ha_refresh_contacts(self.h, C.byref(k), self._stream()), "ha_refresh_contacts")

    def link_index(self, link):
        """Model link index of ``link``: an index, or the scene's link name (KeyError when the scene has none such)."""
        if isinstance(link, str):
            names = [l["name"] for l in self.scene["robot"]["links"]]
            if link not in names:
                raise KeyError(f"the scene has no link named {link!r}")
            return names.index(link)
        return int(link)

    def link_dofs(self, link):
        """The ancestor-or-self DOF indices of a model link, ascending."""
        i, out = int(link), []
        while 0 <= i < self.num_links:
            if self.model.link_dof[i] >= 0:
                out.append(int(self.model.link_dof[i]))
            i = self.model.link_parent[i] if i > 0 else -1
        return sorted(out)

    def cartesian_targets(self, goal, link, dofs=None, mode="pose", offset=(0.0, 0.0, 0.0), damping=0.05, max_step=0.0,
                          q_rest=None, null_gain=0.0, position_only=False, targets=None, err_out=None, env_ids=None):
        """One damped least-squares step of a Cartesian controller for ``link`` (index or scene link name), in one launch
        on the current stream and without a host sync (ha_cartesian_targets; no Isaac Gym counterpart):
        ``targets[env, d] = clamp(q + J^T (J J^T + damping^2 I)^-1 e, lower, upper)`` on ``dofs`` (DOF indices, default
        every ancestor DOF of the link; the others of them are held), every other element of ``targets`` untouched.
        goal: float32 device tensor, (n, 7) tool pose pos + quat xyzw in the env frame (mode "pose") or (n, 6) the task
        error itself (mode "delta"), n = num_envs or len(env_ids), row k for the k-th listed env. offset: the tool point
        in the link frame. max_step > 0 limits max |dq|. q_rest (D floats) with null_gain > 0 adds the posture term
        through the damped null-space projector, which leaks into task space: such a loop settles millimetres off the
        goal. position_only drops the orientation rows (fingertips). targets defaults to the bound sim_targets, the
        tensor the next simulate() drives to; err_out (N, 6) receives e. Returns targets."""
        if isinstance(mode, str):
            if mode not in ("pose", "delta"):
                raise _lib.HandArmError(f"mode must be 'pose' or 'delta', not {mode!r}")
            mode = HM.CART_POSE if mode == "pose" else HM.CART_DELTA
        mode = int(mode)                   # HM.CART_*: the library checks the value
        li = self.link_index(link)
        mask = 0
        for d in (self.link_dofs(li) if dofs is None else dofs):
            if not 0 <= int(d) < self.num_dofs:
                raise _lib.HandArmError(f"DOF index {d} outside 0..{self.num_dofs - 1}")
            mask |= 1 << int(d)
        ids = None if env_ids is None else env_ids.to(device=self.device, dtype=torch.int32).contiguous()
        n = self.num_envs if ids is None else int(ids.numel())
        if n < 1:
            raise _lib.HandArmError("env_ids is empty")
        width = 6 if mode == HM.CART_DELTA else 7

        def dev(x, shape, what):
            if x is None:
                return None
            x = torch.as_tensor(x, dtype=torch.float32, device=self.device)
            if tuple(x.shape) != shape or not x.is_contiguous():
                raise _lib.HandArmError(f"{what} must be a contiguous float32 tensor of shape {shape}")
            return x
        goal = dev(goal, (n, width), "goal")
        targets = dev(self.t["sim_targets"] if targets is None else targets, (self.num_envs, self.num_dofs), "targets")
        err_out = dev(err_out, (self.num_envs, 6), "err_out")
        q_rest = dev(q_rest, (self.num_dofs,), "q_rest")
        c = HM.HaCartesian(goal.data_ptr() if goal is not None else None, targets.data_ptr(),
                           err_out.data_ptr() if err_out is not None else None,
                           q_rest.data_ptr() if q_rest is not None else None,
                           ids.data_ptr() if ids is not None else None, n if ids is not None else 0, li, mode,
                           int(bool(position_only)), mask, (C.c_float * 3)(*[float(v) for v in offset]),
                           float(damping), float(max_step), float(null_gain))
        _lib.check(self.lib.ha_cartesian_targets(self.h, C.byref(c), self._stream()), "ha_cartesian_targets")
        # the launch reads these asynchronously: hold them until the next call replaces them
        self._cart_hold = (goal, q_rest, ids)
        return targets

    def cartesian_tasks(self, tasks, dofs=None):
        """``(HaCartTask array, n_tasks, dof_mask)`` of a whole-hand task list, checked: every refusal the library
        would make for the list is a HandArmError here, before any launch. tasks: dicts with ``link`` (index or scene
        link name) and optionally ``offset`` (3 floats, default 0), ``position_only`` (default False) and ``weight``
        (default 1)."""
        tasks = list(tasks)
        if not 1 <= len(tasks) <= HM.CART_MAX_TASKS:
            raise _lib.HandArmError(f"{len(tasks)} tasks: a launch takes 1..{HM.CART_MAX_TASKS}")
        mask = 0
        for d in (range(self.num_dofs) if dofs is None else dofs):
            if not 0 <= int(d) < self.num_dofs:
                raise _lib.HandArmError(f"DOF index {d} outside 0..{self.num_dofs - 1}")
            mask |= 1 << int(d)
        arr, rows = (HM.HaCartTask * HM.CART_MAX_TASKS)(), 0
        for t, task in enumerate(tasks):
            unknown = set(task) - {"link", "offset", "position_only", "weight"}
            if unknown or "link" not in task:
                raise _lib.HandArmError(f"task {t}: keys are link, offset, position_only, weight; got {sorted(task)}")
            try:
                li = self.link_index(task["link"])
            except KeyError as e:
                raise _lib.HandArmError(f"task {t}: {e.args[0]}") from None
            if not 1 <= li < self.num_links:
                raise _lib.HandArmError(f"task {t}: link index {li} outside 1..{self.num_links - 1}")
            w = float(task.get("weight", 1.0))
            if not (w > 0.0 and w != float("inf")):
                raise _lib.HandArmError(f"task {t}: weight {w} is not finite and > 0")
            if not any(mask >> d & 1 for d in self.link_dofs(li)):
                raise _lib.HandArmError(f"task {t}: none of the selected DOFs moves link {li}")
            ponly = bool(task.get("position_only", False))
            rows += 3 if ponly else 6
            arr[t] = HM.HaCartTask(li, int(ponly), (C.c_float * 3)(*[float(v) for v in task.get("offset", (0, 0, 0))]),
                                   w)
        if rows > HM.CART_MAX_ROWS:
            raise _lib.HandArmError(f"the tasks stack {rows} rows: a launch takes at most {HM.CART_MAX_ROWS}")
        return arr, len(tasks), mask

    def cartesian_multi_targets(self, goal, tasks, dofs=None, mode="pose", damping=0.05, max_step=0.0, q_rest=None,
                                null_gain=0.0, targets=None, err_out=None, env_ids=None):
        """One damped least-squares step for several links at once (a whole hand: the flange or palm pose and the
        fingertip positions), in one launch on the current stream and without a host sync (ha_cartesian_multi_targets;
        no Isaac Gym counterpart). tasks: a list of up to 6 dicts, ``link`` (index or scene link name), ``offset``,
        ``position_only``, ``weight``; a position-only task stacks 3 rows, every other 6, at most 24 in all. The rows are
        scaled by their task's weight and solved together, the R x R system in float64:
        ``targets[env, d] = clamp(q + Jw^T (Jw Jw^T + damping^2 I)^-1 ew, lower, upper)`` on the union of the tasks'
        ancestor DOFs within ``dofs`` (DOF indices, default all), every other element of ``targets`` untouched.
        goal: float32 device tensor (n, T, 7) tool poses (mode "pose"; a position-only task's quaternion is not read)
        or (n, T, 6) task errors (mode "delta"), n = num_envs or len(env_ids). max_step, q_rest / null_gain, targets and
        env_ids as cartesian_targets; err_out (N, T, 6) receives each task's unweighted error. Returns targets."""
        if isinstance(mode, str):
            if mode not in ("pose", "delta"):
                raise _lib.HandArmError(f"mode must be 'pose' or 'delta', not {mode!r}")
            mode = HM.CART_POSE if mode == "pose" else HM.CART_DELTA
        mode = int(mode)                   # HM.CART_*: the library checks the value
        arr, T, mask = self.cartesian_tasks(tasks, dofs)
        ids = None if env_ids is None else env_ids.to(device=self.device, dtype=torch.int32).contiguous()
        n = self.num_envs if ids is None else int(ids.numel())
        if n < 1:
            raise _lib.HandArmError("env_ids is empty")
        width = 6 if mode == HM.CART_DELTA else 7

        def dev(x, shape, what):
            if x is None:
                return None
            x = torch.as_tensor(x, dtype=torch.float32, device=self.device)
            if tuple(x.shape) != shape or not x.is_contiguous():
                raise _lib.HandArmError(f"{what} must be a contiguous float32 tensor of shape {shape}")
            return x
        goal = dev(goal, (n, T, width), "goal")
        targets = dev(self.t["sim_targets"] if targets is None else targets, (self.num_envs, self.num_dofs), "targets")
        err_out = dev(err_out, (self.num_envs, T, 6), "err_out")
        q_rest = dev(q_rest, (self.num_dofs,), "q_rest")
        c = HM.HaCartesianMulti(goal.data_ptr() if goal is not None else None, targets.data_ptr(),
                                err_out.data_ptr() if err_out is not None else None,
                                q_rest.data_ptr() if q_rest is not None else None,
                                ids.data_ptr() if ids is not None else None, n if ids is not None else 0, T, mode,
                                mask, float(damping), float(max_step), float(null_gain), arr)
        _lib.check(self.lib.ha_cartesian_multi_targets(self.h, C.byref(c), self._stream()),
                   "ha_cartesian_multi_targets")
        # the launch reads these asynchronously: hold them until the next call replaces them
        self._cart_multi_hold = (goal, q_rest, ids)
        return targets

    def simulate(self, n_calls=1, flags=0, env_ids=None):
        """gym.simulate n_calls times; env_ids (device tensor of distinct env indices): those envs only."""
        if env_ids is None:
            _lib.check(self.lib.ha_simulate(self.h, n_calls, flags, self._stream()), "ha_simulate")
            return
        ids = env_ids.to(device=self.device, dtype=torch.int32).contiguous()
        _lib.check(self.lib.ha_simulate_envs(self.h, n_calls, flags, C.c_void_p(ids.data_ptr()), ids.numel(),
                                             self._stream()), "ha_simulate_envs")

    def fetch_results(self, wait=True):
        if wait:
            torch.cuda.current_stream(self.device).synchronize()

    def _indexed(self, fn, data, idx, name):
        idx = idx.to(device=self.device, dtype=torch.int32).contiguous()
        data = data.contiguous()
        _lib.check(fn(self.h, C.c_void_p(data.data_ptr()), C.c_void_p(idx.data_ptr()), idx.numel(), self._stream()),
                   name)

    def set_actor_root_state_tensor_indexed(self, root_state, actor_indices):
        self._indexed(self.lib.ha_set_actor_root_state_indexed, root_state, actor_indices, "set_actor_root_state")

    def set_dof_state_tensor_indexed(self, dof_state, actor_indices):
        self._indexed(self.lib.ha_set_dof_state_indexed, dof_state, actor_indices, "set_dof_state")

    def set_dof_position_target_tensor_indexed(self, targets, actor_indices):
        self._indexed(self.lib.ha_set_dof_position_target_indexed, targets, actor_indices, "set_dof_target")

    def set_dof_position_target_tensor(self, targets):
        targets = targets.contiguous()
        _lib.check(self.lib.ha_set_dof_position_target(self.h, C.c_void_p(targets.data_ptr()), self._stream()),
                   "set_dof_position_target")

    def set_object_collisions(self, enabled):
        """enabled: (N, n_obj) bool/uint8 - replaces the per-env shape-filter loop (multi_object.py:693-703)."""
        self.t["collision_enabled"].copy_(enabled.to(torch.uint8))

    # -------------------------------------------------------------- fused task entry points
    def task_step(self, flags=0):
        if self.rebalance_every > 0:
            self._rb_count += 1
            if self._rb_count >= self.rebalance_every:
                self._rb_count = 0
                self.rebalance()
        _lib.check(self.lib.ha_task_step(self.h, flags, self._stream()), "ha_task_step")

    def task_step_io(self, flags, actions, clip_actions, obs_out, clip_obs, scalars=None):
        """task_step with VecTask.step's action clamp and the epilogue's outputs in the same launch (Allegro tasks):
        actions (raw, N x num_actions float32 on the device) clamped into the actions tensor, obs_out = clamp(obs),
        scalars (AllegroKuka, 4 floats) = the extras means."""
        if self.rebalance_every > 0:
            self._rb_count += 1
            if self._rb_count >= self.rebalance_every:
                self._rb_count = 0
                self.rebalance()
        a = actions
        if a.dtype != torch.float32 or a.device != self.device or not a.is_contiguous():
            a = a.to(self.device, torch.float32).contiguous()
        _lib.check(self.lib.ha_task_step_io(self.h, flags, C.c_void_p(a.data_ptr()), float(clip_actions),
                                            C.c_void_p(obs_out.data_ptr()), float(clip_obs),
                                            C.c_void_p(scalars.data_ptr()) if scalars is not None else None,
                                            self._stream()), "ha_task_step_io")
        # the launch reads the converted copy asynchronously: hold it until the next step replaces it (a caller on
        # another stream than the launch's would otherwise let the caching allocator reuse it too early)
        self._act_hold = a
        return a

    def bind_dr_replay(self):
        """Allocate and bind the replayed DR draws (ha_bind_dr_replay): launches with HM.FLAG_REPLAY_DR then take
        every DR sample from ``self.dr_replay`` (name -> tensor, HM.DR_REPLAY_FIELDS) instead of the counter hash.
        Launches without the flag do not read them. Idempotent."""
        if getattr(self, "dr_replay", None) is not None:
            return self.dr_replay
        N, p = self.num_envs, self.params
        shapes = {"dr_draws": (N, HM.DR_SIZE), "dr_gravity_draws": (3,), "dr_obs_corr": (N, p.num_obs),
                  "dr_obs_white": (N, p.num_obs), "dr_act_corr": (N, p.num_actions),
                  "dr_act_white": (N, p.num_actions)}
        with torch.cuda.device(self.device):
            bufs = {k: torch.zeros(shapes[k], dtype=torch.float32, device=self.device) for k in HM.DR_REPLAY_FIELDS}
        self._dr_replay_struct = HM.HaDrReplay(**{k: v.data_ptr() for k, v in bufs.items()})
        _lib.check(self.lib.ha_bind_dr_replay(self.h, C.byref(self._dr_replay_struct)), "ha_bind_dr_replay")
        self.dr_replay = bufs
        return bufs

    def upload_dr_replay(self, applied=None, noise=None):
        """Upload one step's host draws (handarm_hip/ref_rng.py DrDraws): `applied` (DrApplied: the sampled envs' draw
        rows and the gravity draws, when it made any) and `noise` (DrDraws.noise: the tensors it redrew)."""
        bufs = self.bind_dr_replay()
        if applied is not None:
            if applied.gravity is not None:
                bufs["dr_gravity_draws"].copy_(torch.from_numpy(applied.gravity))
            if applied.all:
                bufs["dr_draws"].copy_(torch.from_numpy(applied.draws))
            elif applied.envs.any():
                ids = torch.from_numpy(applied.envs.nonzero()[0])
                bufs["dr_draws"][ids.to(self.device)] = torch.from_numpy(applied.draws[applied.envs]).to(self.device)
        for k, v in (noise or {}).items():
            if k != "task" and v is not None:
                bufs["dr_" + k].copy_(v)

    def task_observe(self, flags=0):
        _lib.check(self.lib.ha_task_observe(self.h, flags, self._stream()), "ha_task_observe")

    def task_reset(self, flags=0):
        _lib.check(self.lib.ha_task_reset(self.h, flags, self._stream()), "ha_task_reset")

    def contact_stats(self, reset=False):
        """Contact-list diagnostics since the last reset (ha_state_t.contact_stats, added up by every launch):
        substeps, fraction of substeps whose narrow phases offered more contacts than the list holds (the
        shallowest are then dropped), mean and max contacts offered per substep, and percentiles of the per-env
        maximum. One device read."""
        cs = self.t["contact_stats"].cpu().numpy().astype("int64")
        if reset:
            self.t["contact_stats"].zero_()
        sub = int(cs[:, 0].sum())
        import numpy as np
        ref, nar = int(cs[:, 5].sum()), int(cs[:, 6].sum())
        return {"capacity": self.contact_capacity, "substeps": sub,
                "at_capacity_frac": float(cs[:, 1].sum() / max(sub, 1)),
                "offered_mean": float(cs[:, 3].sum() / max(sub, 1)), "offered_max": int(cs[:, 2].max()),
                "env_max_p50": float(np.percentile(cs[:, 2], 50)), "env_max_p99": float(np.percentile(cs[:, 2], 99)),
                "self_offered_mean": float(cs[:, 4].sum() / max(sub, 1)),
                "pcm_refreshed_per_substep": ref / max(sub, 1), "narrow_phases_per_substep": nar / max(sub, 1),
                "pcm_refreshed_frac": ref / max(ref + nar, 1)}

    def last_kernel_ms(self):
        return float(self.lib.ha_last_kernel_ms(self.h))

    def enable_kernel_timing(self, max_launches):
        _lib.check(self.lib.ha_enable_kernel_timing(self.h, max_launches), "ha_enable_kernel_timing")

    def kernel_times_ms(self, max_n=1 << 16):
        buf = (C.c_float * max_n)()
        n = C.c_int32()
        _lib.check(self.lib.ha_kernel_times(self.h, buf, max_n, C.byref(n)), "ha_kernel_times")
        return list(buf[:n.value])
