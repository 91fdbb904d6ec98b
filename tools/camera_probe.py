#!/usr/bin/env python3
"""Camera kernel probe (GPU box): ha_render_camera on a simulated state at several env counts and resolutions, and with
--link NAME also ha_render_camera_mounted from a camera on that robot link (the palm_down mount of the tests) and from
the fixed camera's own view (position mode on the base link), which separates the kernel's cost from the view's.

Reports per launch the HIP-event median (one event pair per launch) and mean, rays per second and the image bytes
written per second.
Usage: python tools/camera_probe.py [--envs 1024 8192] [--res 160x90 640x480] [--iters 20] [--link palm]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "isaacgym-hand-arm_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from handarm_hip import cameras as CAM  # noqa: E402
from handarm_hip.sim import HandArmSim  # noqa: E402

TOPVIEW = dict(pos=[0.28, 1.05, 0.9], quat=[0.213, 0.213, -0.674, 0.674])
MOUNT = dict(pos=[0.0, 0.03, 0.04], quat=[0.0, 0.0, 0.707107, 0.707107])     # looks out of the palm


def time_launches(cam, iters):
    """(median, mean) ms per launch: 3 warm-up launches, then one HIP event pair around each of `iters` launches."""
    for _ in range(3):
        cam.render()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        cam.render()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), sum(ms) / len(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--res", nargs="+", default=["160x90", "640x480"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--link", default=None, help="also time a camera mounted on this robot link (scene link name)")
    args = ap.parse_args()
    from oracle.oracle_lib import HostState
    from tests import scenes
    for N in args.envs:
        sim = HandArmSim(N, "cuda:0")
        st = HostState(N, model=sim.model, params=sim.params)
        scenes.fill_scene(st, N, seed=0)
        for k in ("root_state", "dof_state", "sim_targets", "object_indices", "goal_pos"):
            sim.t[k].copy_(torch.from_numpy(np.ascontiguousarray(st[k])).reshape(sim.t[k].shape).to(sim.t[k].dtype))
        sim.simulate(10)
        for res in args.res:
            W, H = (int(v) for v in res.split("x"))
            if N * W * H > 8192 * 160 * 90 * 4:
                continue
            kinds = [("fixed", dict(TOPVIEW))]
            if args.link is not None:
                kinds.append((f"mounted on {args.link}", dict(MOUNT, link=args.link)))
                # the mounted launch on the fixed camera's own view: position mode on the robot's base link (it does
                # not move and stands at the same place in every env), so the two kernels cast the same rays
                rows = sim.t["rigid_body_state"].view(N, sim.num_bodies, 13)[:, sim.model.body_robot0, 0:3]
                assert bool((rows == rows[0]).all()), "the base link is not at one place in every env"
                base = rows[0].tolist()
                kinds.append(("mounted, the fixed camera's view", dict(
                    pos=[a - b for a, b in zip(TOPVIEW["pos"], base)], quat=TOPVIEW["quat"], link=0, follow="position")))
            for label, kw in kinds:
                cam = CAM.CameraSensor(sim, kw.pop("pos"), kw.pop("quat"), 87, (W, H), **kw)
                med, mean = time_launches(cam, args.iters)
                rays = N * W * H
                out_bytes = rays * (4 + 4 + 16)
                print(f"envs {N:6d} {W}x{H} {label}: median {med:.3f} ms per launch (mean {mean:.3f}), "
                      f"{rays / med / 1e6:.2f} G rays/s, {out_bytes / med / 1e6:.0f} GB/s of images written", flush=True)
                del cam
        del sim
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
