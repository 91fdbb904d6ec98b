#!/usr/bin/env python3
"""Jacobian / mass-matrix kernel probe: ha_refresh_kinematics alone on random joint states (GPU box).

Reports, per env count and output set (Jacobian of all links, mass matrix, both), the HIP-event time per launch (median
and min over rounds of back-to-back launches, after a warm-up) and the store rate = bytes written / that time, to set
beside the 6.8 TB/s of tools/probes/hbm_write_probe.hip. The kernel's reads (dof_state, 8 D bytes per env, and the
L2-resident model) are not counted.
Usage: python tools/kin_probe.py [--task 2] [--envs 4096 65536] [--rounds 20] [--launches 20]
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


def time_launches(fn, rounds, launches):
    """ms per launch for each round: HIP events around `launches` back-to-back launches."""
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / launches)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", type=int, default=HM.TASK_ALLEGRO_KUKA)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    for N in args.envs:
        for what in ("jacobian", "mass_matrix", "both"):
            sim = HandArmSim(N, "cuda:0", task=args.task)
            D, L = sim.num_dofs, sim.num_links
            g = torch.Generator(device="cuda:0").manual_seed(0)
            q = torch.tensor(list(sim.params.reset_pose)[:D], device="cuda:0")
            dof = sim.t["dof_state"].view(N, D, 2)
            dof[..., 0] = q + 0.6 * torch.rand((N, D), device="cuda:0", generator=g) - 0.3
            dof[..., 1] = 2.0 * torch.rand((N, D), device="cuda:0", generator=g) - 1.0
            nbytes = 0
            if what != "mass_matrix":
                nbytes += sim.acquire_jacobian_tensor().numel() * 4
            if what != "jacobian":
                nbytes += sim.acquire_mass_matrix_tensor().numel() * 4
            refresh = sim.refresh_mass_matrix_tensors if what == "mass_matrix" else sim.refresh_jacobian_tensors
            ms = time_launches(refresh, args.rounds, args.launches)
            med, lo = statistics.median(ms), min(ms)
            print(f"task {args.task} N {N} {what}: {nbytes / N:.0f} B/env, {nbytes / 1e6:.1f} MB per launch, "
                  f"{med * 1e3:.1f} us median ({lo * 1e3:.1f} min) per launch, "
                  f"{nbytes / (med * 1e-3) / 1e12:.2f} TB/s stored ({nbytes / (lo * 1e-3) / 1e12:.2f} at the min)",
                  flush=True)
            del sim


if __name__ == "__main__":
    main()
