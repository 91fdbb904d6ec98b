#!/usr/bin/env python3
"""Contact-query probe: one refresh_contact_tensor() launch against one simulate(1) launch at the bench's sizes (needs a GPU).

Builds the bench's task (AllegroKuka 4096 envs, Ur5Sih 8192 envs with DR, as bench.py make_env does), steps it
`--steps` times with seeded U[-1, 1] actions, snapshots the state and then alternates, in one process, a round of
`--launches` back-to-back query launches between two device events with five single simulate(1) launches, each between
its own two events and each from the restored snapshot (the restore copies run before the first event). Prints both
medians over the rounds, the bytes the query stores per launch (80 B per kept contact + 8 B per env) and the store
rate.
Usage: python tools/contacts_probe.py [--task allegro_kuka ur5sih] [--steps 20] [--rounds 15] [--launches 50]
"""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "isaacgym-hand-arm_amd")]

import torch  # noqa: E402


def make_env(task, device, seed=42):
    from handarm_hip.tasks import AllegroKuka, Ur5SihMultiObjectManipulation
    if task == "allegro_kuka":
        return AllegroKuka({"env": {"numEnvs": 4096, "subtask": "regrasping"}, "seed": seed}, device, device)
    import bench
    cfg = {"env": {"numEnvs": 8192}, "seed": seed, "objects": {"dataset": {"ycb": bench.pool16_names(False)}},
           "task": {"randomize": True}}
    return Ur5SihMultiObjectManipulation(cfg, device, device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", nargs="+", default=["allegro_kuka", "ur5sih"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    device = "cuda:0"
    for task in args.task:
        random.seed(42)
        torch.manual_seed(42)
        env = make_env(task, device)
        env.reset()
        gen = torch.Generator(device=device).manual_seed(42)
        for _ in range(args.steps):
            env.step(torch.rand((env.sim.num_envs, env.num_acts), device=device, generator=gen) * 2 - 1)
        sim = env.sim
        torch.cuda.synchronize()
        snap = sim.snapshot()
        rows, counts = sim.acquire_contact_tensor()
        torch.cuda.synchronize()
        kept = int(counts[:, 0].sum())
        nbytes = 80 * kept + 8 * sim.num_envs
        for _ in range(args.launches):
            sim.refresh_contact_tensor()
        sim.simulate(1)
        torch.cuda.synchronize()
        q_ms, s_ms = [], []
        for _ in range(args.rounds):
            sim.restore(snap)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                sim.refresh_contact_tensor()
            e1.record()
            e1.synchronize()
            q_ms.append(e0.elapsed_time(e1) / args.launches)
            one = []
            for _ in range(5):
                sim.restore(snap)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sim.simulate(1)
                e1.record()
                e1.synchronize()
                one.append(e0.elapsed_time(e1))
            s_ms.append(statistics.median(one))
        q, s = statistics.median(q_ms), statistics.median(s_ms)
        print(f"{task} N {sim.num_envs} after {args.steps} steps: kept {kept} contacts ({kept / sim.num_envs:.1f} per env, "
              f"max {int(counts[:, 0].max())}, offered max {int(counts[:, 1].max())}); query {q * 1e3:.1f} us median "
              f"({min(q_ms) * 1e3:.1f} min) per launch; simulate(1) {s * 1e3:.1f} us median ({min(s_ms) * 1e3:.1f} min) per "
              f"launch ({sim.params.substeps} substeps); query stores {nbytes / 1e6:.2f} MB per launch, "
              f"{nbytes / (q * 1e-3) / 1e9:.1f} GB/s", flush=True)
        del env, sim


if __name__ == "__main__":
    main()
