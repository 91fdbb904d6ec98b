#!/usr/bin/env python3
"""Whole-hand Cartesian controller probe: one stacked damped least-squares step per env, fused and composed, on random
joint states (GPU box).

  fused     HandArmSim.cartesian_multi_targets in delta mode (the task errors given): one ha_cartesian_multi_kernel
            launch
  fused_pose  the same launch in pose mode (it also forms the task errors from goal poses)
  jacobian  the ha_refresh_kinematics launch for the tasks' links alone (what the torch route starts with)
  torch     the torch composition on that Jacobian tensor, the only equivalent route without the kernel, for the same
            given task errors: refresh, slice, cat, weights, bmm, + lambda^2 I, a float64 torch.linalg.solve, bmm, the
            step limit, clamp, store

Task sets: AllegroKuka iiwa7_link_7 pose + 4 fingertip positions (5 tasks, 18 rows), Ur5Sih flange pose + 5 fingertip
positions (6 tasks, 21 rows); fingertip weight 3. HIP-event time per call: median and min over rounds of back-to-back
calls, after a warm-up; every case runs twice.
Usage: python tools/cartesian_multi_probe.py [--cases 2:4096 2:8192 0:4096 0:8192] [--rounds 20] [--launches 20]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "isaacgym-hand-arm_amd")]

import torch  # noqa: E402

from handarm_hip import model as HM  # noqa: E402
from handarm_hip.sim import HandArmSim  # noqa: E402
from tools.cartesian_probe import time_launches  # noqa: E402

TASKS = {HM.TASK_UR5SIH: ("flange", ["index_fingertip", "little_fingertip", "middle_fingertip", "ring_fingertip",
                                     "thumb_fingertip"]),
         HM.TASK_ALLEGRO_KUKA: ("iiwa7_link_7", ["index_link_3", "middle_link_3", "ring_link_3", "thumb_link_3"])}
TIP_WEIGHT = 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=[f"{t}:{n}" for t in (HM.TASK_ALLEGRO_KUKA, HM.TASK_UR5SIH)
                                                   for n in (4096, 8192)], help="task:envs")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    dev = "cuda:0"
    for case in args.cases:
        task, N = (int(x) for x in case.split(":"))
        sim = HandArmSim(N, dev, task=task)
        D = sim.num_dofs
        arm, tips = TASKS[task]
        tasks = [dict(link=arm)] + [dict(link=f, position_only=True, weight=TIP_WEIGHT) for f in tips]
        links = [sim.link_index(t["link"]) for t in tasks]
        T, R = len(tasks), 6 + 3 * len(tips)
        g = torch.Generator(device=dev).manual_seed(0)
        q = torch.tensor(list(sim.params.reset_pose)[:D], device=dev)
        dof = sim.t["dof_state"].view(N, D, 2)
        dof[..., 0] = q + 0.6 * torch.rand((N, D), device=dev, generator=g) - 0.3
        dof[..., 1] = 0.0
        e6 = torch.cat([0.02 * torch.nn.functional.normalize(torch.randn((N, T, 3), device=dev, generator=g), dim=2),
                        0.2 * torch.nn.functional.normalize(torch.randn((N, T, 3), device=dev, generator=g), dim=2)],
                       2).contiguous()
        pose = torch.cat([torch.rand((N, T, 3), device=dev, generator=g),
                          torch.nn.functional.normalize(torch.randn((N, T, 4), device=dev, generator=g), dim=2)],
                         2).contiguous()
        lo = torch.tensor(list(sim.model.dof_lower)[:D], device=dev)
        up = torch.tensor(list(sim.model.dof_upper)[:D], device=dev)
        jac = sim.acquire_jacobian_tensor(links=links)
        tgt = dof[..., 0].clone()
        w = torch.tensor([1.0] * 6 + [TIP_WEIGHT] * (R - 6), device=dev, dtype=torch.float64)
        eye = 0.05 ** 2 * torch.eye(R, device=dev, dtype=torch.float64)

        def fused():
            sim.cartesian_multi_targets(e6, tasks, mode="delta", damping=0.05, max_step=0.2, targets=tgt)

        def fused_pose():
            sim.cartesian_multi_targets(pose, tasks, damping=0.05, max_step=0.2, targets=tgt)

        def composed():
            sim.refresh_jacobian_tensors()
            J = torch.cat([jac[:, 0], jac[:, 1:, 0:3].reshape(N, -1, D)], 1).double() * w[None, :, None]
            e = torch.cat([e6[:, 0], e6[:, 1:, 0:3].reshape(N, -1)], 1).double() * w
            A = J @ J.transpose(1, 2) + eye
            dq = (J.transpose(1, 2) @ torch.linalg.solve(A, e.unsqueeze(-1))).squeeze(-1)
            mx = dq.abs().amax(dim=1, keepdim=True)
            dq = torch.where(mx > 0.2, dq * (0.2 / mx), dq)
            tgt[:] = torch.minimum(torch.maximum((dof[:, :, 0].double() + dq).float(), lo), up)

        fused()
        a = tgt.clone()
        composed()
        torch.cuda.synchronize()
        print(f"task {task} N {N} {T} tasks {R} rows: fused and torch targets differ by at most "
              f"{float((a - tgt).abs().max()):.2e} rad", flush=True)
        for run in (1, 2):
            for name, fn in (("fused", fused), ("fused_pose", fused_pose),
                             ("jacobian", sim.refresh_jacobian_tensors), ("torch", composed)):
                ms = time_launches(fn, args.rounds, args.launches)
                med, low = statistics.median(ms), min(ms)
                print(f"task {task} N {N} run {run} {name}: {med * 1e3:.1f} us median ({low * 1e3:.1f} min) per call",
                      flush=True)
        del sim


if __name__ == "__main__":
    main()
