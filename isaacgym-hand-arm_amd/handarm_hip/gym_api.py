"""Reference-side binding of the lower surface: the Isaac Gym calls the hand_arm task code makes, with
Isaac Gym's own signatures (`gym.<fn>(sim, ...)`, `gymtorch.wrap_tensor/unwrap_tensor`), routed to
libhandarm_hip.so through ``HandArmSim``.

Call sites this serves (under /root/reference/isaacgymenvs):
  gym.simulate / fetch_results                    tasks/base/vec_task.py:412-416
  gym.acquire_*_tensor + gymtorch.wrap_tensor     tasks/hand_arm/base/observable_vec_task.py:123-155
  gym.refresh_*_tensor                            observable_vec_task.py:173-177
  gym.set_dof_position_target_tensor              tasks/hand_arm/base/actionable_vec_task.py:39-40
  gym.set_actor_root_state_tensor_indexed         tasks/hand_arm/task/multi_object_manipulation.py:89,118,167,228
  gym.set_dof_state_tensor_indexed                tasks/hand_arm/base/ur5sih.py:630
  gym.set_dof_position_target_tensor_indexed      ur5sih.py:626
  gym.apply_rigid_body_force_tensors              tasks/allegro_kuka/allegro_kuka_base.py:1412-1414 (LOCAL_SPACE forces),
                                                  :1417-1424 (privilegedActions: ENV_SPACE object torques)
  gym.acquire_dof_force_tensor / refresh          tasks/allegro_hand.py:151-152,409
  gym.acquire_jacobian_tensor / acquire_mass_matrix_tensor + refresh_jacobian_tensors / refresh_mass_matrix_tensors
                                                  Isaac Gym's tensor API for Cartesian / operational-space arm
                                                  controllers (no hand_arm call site; ha_refresh_kinematics)
  gym.get_rigid_contacts / get_env_rigid_contacts the contact list of the current state (no hand_arm call site: tactile
                                                  observations, grasp diagnostics; ha_refresh_contacts)
Isaac Gym returns bool from the set_* calls; so does this (a failing ABI call raises HandArmError
instead of being silently ignored).
"""
import types

import numpy as np
import torch

from . import model as HM
from .sim import HandArmSim


class _Unwrapped:
    """gymtorch.unwrap_tensor result: keeps the tensor (the ABI needs its device pointer and dtype)."""
    __slots__ = ("tensor",)

    def __init__(self, t):
        self.tensor = t


gymtorch = types.SimpleNamespace(
    unwrap_tensor=lambda t: _Unwrapped(t),
    wrap_tensor=lambda t: t,                 # acquire_* already returns the live torch tensor
)
# gymapi.CoordinateSpace values used by apply_rigid_body_force_tensors
gymapi = types.SimpleNamespace(ENV_SPACE=0, LOCAL_SPACE=1, GLOBAL_SPACE=2)


def _quat_rotate(q, v):
    """Rotate v (..., 3) by unit quaternions q (..., 4) xyzw."""
    qv, w = q[..., :3], q[..., 3:4]
    t = 2.0 * torch.cross(qv, v, dim=-1)
    return v + w * t + torch.cross(qv, t, dim=-1)


def _t(x):
    return x.tensor if isinstance(x, _Unwrapped) else x


# Isaac Gym's RigidContact fields that the contact query computes. lambda, friction, offset0 / offset1 and initialOverlap
# are left out rather than zero-filled: the query solves nothing
RIGID_CONTACT_DTYPE = np.dtype([("env0", np.int32), ("env1", np.int32), ("body0", np.int32), ("body1", np.int32),
                                ("localPos0", np.float32, (3,)), ("localPos1", np.float32, (3,)),
                                ("minDist", np.float32), ("normal", np.float32, (3,))])


def rigid_contacts_from_rows(rows, counts, env0=0):
    """Contact tensor rows (n, cap, 20) and counts (n, 2) or (n,) as numpy arrays -> one RIGID_CONTACT_DTYPE record per
    kept contact (rows < counts[e, 0] of env e, env by env in list order). env0 / env1: env0 + e; body0 / body1: the
    rigid_body_state rows of the two bodies within their env (-1: a static or the ground); localPos0 / localPos1: the
    surface points in the bodies' frames (env frame for a static); minDist: the separation (negative: penetration);
    normal: unit, from body1 to body0, env frame."""
    rows = np.asarray(rows, np.float32)
    kept = np.asarray(counts).reshape(rows.shape[0], -1)[:, 0].astype(np.int64)
    if rows.ndim != 3 or rows.shape[2] != HM.CONTACT_REC or (kept < 0).any() or (kept > rows.shape[1]).any():
        raise ValueError("rows must be (n, cap, 20) and 0 <= counts[:, 0] <= cap")
    env, slot = np.nonzero(np.arange(rows.shape[1])[None, :] < kept[:, None])
    r = rows[env, slot]
    out = np.zeros(len(r), RIGID_CONTACT_DTYPE)
    out["env0"] = out["env1"] = env + env0
    out["body0"], out["body1"] = r[:, 9], r[:, 10]
    out["localPos0"], out["localPos1"] = r[:, 11:14], r[:, 14:17]
    out["minDist"] = r[:, 6]
    out["normal"] = r[:, 3:6]
    return out


class Gym:
    """The subset of isaacgym.gymapi.Gym the hand-arm task calls. ``create_sim`` returns the sim handle."""

    def create_sim(self, num_envs, device="cuda:0", **kw):
        return HandArmSim(num_envs, device, **kw)

    def prepare_sim(self, sim):
        return True

    def simulate(self, sim):
        sim.simulate(1)

    def fetch_results(self, sim, wait):
        sim.fetch_results(wait)

    def acquire_actor_root_state_tensor(self, sim):
        return sim.acquire_actor_root_state_tensor()

    def acquire_rigid_body_state_tensor(self, sim):
        return sim.acquire_rigid_body_state_tensor()

    def acquire_dof_state_tensor(self, sim):
        return sim.acquire_dof_state_tensor()

    def acquire_net_contact_force_tensor(self, sim):
        return sim.acquire_net_contact_force_tensor()

    def acquire_dof_force_tensor(self, sim):
        return sim.t["dof_force"]

    def refresh_actor_root_state_tensor(self, sim):
        sim.refresh_actor_root_state_tensor()

    refresh_rigid_body_state_tensor = refresh_dof_state_tensor = refresh_net_contact_force_tensor = \
        refresh_dof_force_tensor = refresh_actor_root_state_tensor

    def acquire_jacobian_tensor(self, sim, name=None):
        """(N, L-1, 6, D) of the robot, the only articulation (``name`` is accepted for signature compatibility)."""
        return sim.acquire_jacobian_tensor()

    def acquire_mass_matrix_tensor(self, sim, name=None):
        return sim.acquire_mass_matrix_tensor()

    def refresh_jacobian_tensors(self, sim):
        sim.refresh_jacobian_tensors()

    def refresh_mass_matrix_tensors(self, sim):
        sim.refresh_mass_matrix_tensors()

    def acquire_contact_tensor(self, sim):
        """(contacts (N, capacity, 20), counts (N, 2)): the tensor form of get_rigid_contacts (no Isaac Gym counterpart;
        row layout in include/handarm_abi.h, ha_contacts_t)."""
        return sim.acquire_contact_tensor()

    def refresh_contact_tensor(self, sim):
        sim.refresh_contact_tensor()

    def set_cartesian_pose_target(self, sim, controller, goal):
        """Isaac Gym has no counterpart: one step of a handarm_hip.controllers.CartesianController of this sim (one
        launch that writes the joint position targets the next gym.simulate drives to), here so that code written
        against this namespace need not leave it. goal: (N, 7) pos + quat xyzw, or (N, 6) in "delta" mode. A
        controllers.WholeHandController is driven the same way (only ``.sim`` and ``.step`` are used): goal is then
        (N, T, 7) or (N, T, 6), row t for its task t."""
        if controller.sim is not sim:
            raise ValueError("the controller belongs to another sim")
        controller.step(_t(goal))
        return True

    def get_rigid_contacts(self, sim):
        """gym.get_rigid_contacts(sim): the contacts of the current state of all envs as a numpy structured array with
        Isaac Gym's RigidContact field names (RIGID_CONTACT_DTYPE; body indices are per env, the normal points from
        body1 to body0). One query launch, then a device synchronisation and a copy to the host."""
        rows, counts = sim.acquire_contact_tensor()
        sim.refresh_contact_tensor()
        return rigid_contacts_from_rows(rows.cpu().numpy(), counts.cpu().numpy())

    def get_env_rigid_contacts(self, sim, env_index):
        """gym.get_env_rigid_contacts for one env. Isaac Gym's call takes an env handle; this binding has no env
        handles, so it takes the sim and the env's index. Only that env is queried."""
        e = int(env_index)
        if not 0 <= e < sim.num_envs:
            raise IndexError(f"env_index {e} outside 0..{sim.num_envs - 1}")
        rows, counts = sim.acquire_contact_tensor()
        sim.refresh_contact_tensor(torch.tensor([e], dtype=torch.int32, device=sim.device))
        return rigid_contacts_from_rows(rows[e:e + 1].cpu().numpy(), counts[e:e + 1].cpu().numpy(), env0=e)

    @staticmethod
    def _object_rows(sim, tensor, space):
        """The free objects' rows of an (N*B or N, B, 3) rigid-body tensor, in the env frame."""
        o0, no = sim.model.body_object0, sim.n_obj
        v = _t(tensor).view(sim.num_envs, sim.num_bodies, 3)[:, o0:o0 + no, :]
        if space == gymapi.LOCAL_SPACE:
            a0 = sim.model.actor_object0
            q = sim.t["root_state"].view(sim.num_envs, sim.num_actors, 13)[:, a0:a0 + no, 3:7]
            v = _quat_rotate(q, v)
        return v

    def apply_rigid_body_force_tensors(self, sim, force_tensor=None, torque_tensor=None, space=gymapi.ENV_SPACE):
        """Forces at the COM of the free objects and torques on them (each N*B or N, B, 3; either may be None) for
        the next simulate call. LOCAL_SPACE forces and torques are rotated by the object's current orientation.
        Forces and torques on robot links are not supported by the simulator (the reference applies neither)."""
        if torque_tensor is not None:
            if "object_torque" in HM.null_fields(sim.task):
                raise NotImplementedError(f"task {sim.task} binds no object_torque: rigid-body torques are not "
                                          "supported for it")
            sim.t["object_torque"].view(sim.num_envs, sim.n_obj, 3).copy_(self._object_rows(sim, torque_tensor, space))
        if force_tensor is not None:
            sim.t["object_force"].view(sim.num_envs, sim.n_obj, 3).copy_(self._object_rows(sim, force_tensor, space))
        return True

    def set_dof_position_target_tensor(self, sim, targets):
        sim.set_dof_position_target_tensor(_t(targets))
        return True

    def set_actor_root_state_tensor_indexed(self, sim, root_state, actor_indices, n):
        sim.set_actor_root_state_tensor_indexed(_t(root_state), _t(actor_indices)[:n])
        return True

    def set_dof_state_tensor_indexed(self, sim, dof_state, actor_indices, n):
        sim.set_dof_state_tensor_indexed(_t(dof_state), _t(actor_indices)[:n])
        return True

    def set_dof_position_target_tensor_indexed(self, sim, targets, actor_indices, n):
        sim.set_dof_position_target_tensor_indexed(_t(targets), _t(actor_indices)[:n])
        return True


def acquire_gym():
    """gymapi.acquire_gym() analogue."""
    return Gym()
