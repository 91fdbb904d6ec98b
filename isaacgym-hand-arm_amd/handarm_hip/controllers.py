"""Controllers over the lower surface (HandArmSim) that are one kernel launch per control step.

``CartesianController`` commands one link of the robot in Cartesian space: end-effector poses for the UR5 flange or the
iiwa's last link, fingertip positions for a hand (``position_only=True``). Each ``step`` is one launch of
ha_cartesian_kernel (csrc/ha_cartesian.h): FK, the tool-point Jacobian, one damped least-squares step and the joint
position targets, with no host synchronisation. Isaac Gym has no counterpart; its users compose the same step in torch
on ``acquire_jacobian_tensor``.

``WholeHandController`` commands several links in one step, which is what a hand-arm user commands: the flange or palm
pose together with the fingertip positions. The fingertips share the arm's DOFs, so one CartesianController per
fingertip would overwrite the arm targets of the one before; here the tasks' rows are stacked, weighted and solved as
one system (in float64) by one launch of ha_cartesian_multi_kernel (csrc/ha_cartesian_multi.h).

The fused task step kernels (HandArmSim.task_step) keep their own joint-space action modes: a Cartesian action mode
inside them is not part of this controller. Use it with ``simulate()``:

    ctrl = CartesianController(sim, "flange", max_step=0.2)
    for _ in range(steps):
        ctrl.step(goal)            # (N, 7) pos + quat xyzw, env frame -> sim.t["sim_targets"]
        sim.simulate(1)

    hand = WholeHandController(sim, [dict(link="flange")] + [dict(link=f, position_only=True, weight=3.0)
                                                             for f in fingertip_names], max_step=0.2)
    hand.step(goals)               # (N, 6, 7): row t for task t
"""
import torch

from . import _lib


class CartesianController:
    """Holds what every step of one controlled link shares: the resolved link index, its DOF list, the rest posture on
    the device and the ``err`` tensor (N, 6) that receives each step's task error.

    gains: mode ("pose" / "delta"), offset, damping, max_step, null_gain, position_only, q_rest (D floats; needed when
    null_gain > 0), targets (default: the sim's bound sim_targets)."""

    def __init__(self, sim, link, dofs=None, mode="pose", offset=(0.0, 0.0, 0.0), damping=0.05, max_step=0.0,
                 q_rest=None, null_gain=0.0, position_only=False, targets=None):
        self.sim = sim
        self.link = sim.link_index(link)
        self.dofs = sim.link_dofs(self.link) if dofs is None else [int(d) for d in dofs]
        if not set(self.dofs) & set(sim.link_dofs(self.link)):
            raise _lib.HandArmError(f"none of the DOFs {self.dofs} moves link {self.link}")
        self.mask = sum(1 << d for d in set(self.dofs))
        self.q_rest = None if q_rest is None else \
            torch.as_tensor(q_rest, dtype=torch.float32, device=sim.device).contiguous()
        self.err = torch.zeros((sim.num_envs, 6), dtype=torch.float32, device=sim.device)
        self.targets = sim.t["sim_targets"] if targets is None else targets
        self.gains = dict(mode=mode, offset=tuple(float(v) for v in offset), damping=float(damping),
                          max_step=float(max_step), null_gain=float(null_gain), position_only=bool(position_only))

    def step(self, goal, env_ids=None):
        """One launch: the targets of ``goal`` (row k for the k-th listed env) written into ``self.targets``, which is
        returned; ``self.err`` holds the task error the step saw."""
        return self.sim.cartesian_targets(goal, self.link, dofs=self.dofs, q_rest=self.q_rest, targets=self.targets,
                                          err_out=self.err, env_ids=env_ids, **self.gains)


class WholeHandController:
    """Several links commanded together: what every step shares is resolved once (the task array, the DOF mask, the
    rest posture on the device) and ``err`` (N, T, 6) receives each task's unweighted error.

    tasks: a list of up to 6 dicts with ``link`` (index or scene link name), ``offset``, ``position_only`` and
    ``weight``; at most 24 rows in all (6 per task, 3 when position only). A row budget over that and a task none of
    whose DOFs is selected raise HandArmError here, before any launch.
    gains: mode ("pose" / "delta"), damping, max_step, null_gain, q_rest (D floats; needed when null_gain > 0), dofs
    (default: all), targets (default: the sim's bound sim_targets)."""

    def __init__(self, sim, tasks, dofs=None, mode="pose", damping=0.05, max_step=0.0, q_rest=None, null_gain=0.0,
                 targets=None):
        self.sim = sim
        self.tasks = [dict(t) for t in tasks]
        self.dofs = None if dofs is None else [int(d) for d in dofs]
        sim.cartesian_tasks(self.tasks, self.dofs)         # the refusals, now
        self.links = [sim.link_index(t["link"]) for t in self.tasks]
        self.q_rest = None if q_rest is None else \
            torch.as_tensor(q_rest, dtype=torch.float32, device=sim.device).contiguous()
        self.err = torch.zeros((sim.num_envs, len(self.tasks), 6), dtype=torch.float32, device=sim.device)
        self.targets = sim.t["sim_targets"] if targets is None else targets
        self.gains = dict(mode=mode, damping=float(damping), max_step=float(max_step), null_gain=float(null_gain))

    def step(self, goal, env_ids=None):
        """One launch: the targets of ``goal`` ((n, T, 7) or, in "delta" mode, (n, T, 6); row k for the k-th listed
        env) written into ``self.targets``, which is returned; ``self.err`` holds the task errors the step saw."""
        return self.sim.cartesian_multi_targets(goal, self.tasks, dofs=self.dofs, q_rest=self.q_rest,
                                                targets=self.targets, err_out=self.err, env_ids=env_ids, **self.gains)
