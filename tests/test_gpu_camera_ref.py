"""The camera kernels against references that share nothing with them.

ha_camera_kernel: the images CameraSensor.render() produces from simulated states, against the float64 ray caster of
tests/camera_ref.py (hull vertices, convex-hull triangles, ray-triangle intersection) on the state read back from the
device: the cases, the assertions and the bounds of tests/test_camera_ref.py (stable pixels only: ids all equal,
|t - t_ref| cos(theta) / (1 + t_ref) <= 8 x 2^-23, hit points within 2e-6 + |d| x that bound).

ha_camera_target_kernel: with more target pixels than P its contract is exact (csrc/ha_camera.h): the P smallest hash
keys among the target pixels, ties by pixel, written in pixel order, w x 2. The expectation restates the key with
oracle/f32.py mix32 and selects with a plain sort by (key, pixel); target_object_pointcloud must equal it bit for bit.

Measured on an MI355X (kernel vs reference; each test prints its own, DESIGN.md 3.10 lists them): stable share
0.986-1.0, depth error at most 1.8e-7 (1.5 ulp), hit-point error at most 0.15 of its tolerance.
"""
import numpy as np
import pytest
import torch

from handarm_hip import cameras as CAM
from oracle import f32
from tests import camera_ref as REF

pytestmark = pytest.mark.gpu
U = np.uint32


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def cpu(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("name", list(REF.CASES))
def test_kernel_against_reference(name):
    need_gpu()
    from handarm_hip.sim import HandArmSim
    from oracle.oracle_lib import HostState
    case = REF.CASES[name]
    scene = REF.case_scene(case)
    c = REF.case_camera(case, scene)
    N, n_obj = case["N"], 8 if case["kind"] == "bin" else 3
    sim = HandArmSim(N, "cuda:0", task_cfg={"n_objects": n_obj}, scene=scene)
    st = HostState(N, model=sim.model, params=sim.params)
    REF.fill_case(case, st, scene)
    for k in ("root_state", "dof_state", "sim_targets", "object_indices", "goal_pos"):
        sim.t[k].copy_(torch.from_numpy(np.ascontiguousarray(st[k])).reshape(sim.t[k].shape).to(sim.t[k].dtype))
    sim.simulate(REF.SIM_CALLS)
    cam = CAM.CameraSensor(sim, c["pos"], c["quat"], c["fovx"], (c["width"], c["height"]), scene=scene)
    cam.render()
    state = dict(root=cpu(sim.t["root_state"]).reshape(N, sim.num_actors, 13),
                 body=cpu(sim.t["rigid_body_state"]).reshape(N, sim.num_bodies, 13),
                 object_indices=cpu(sim.t["object_indices"]), goal=cpu(sim.t["goal_pos"]))
    REF.check_images(f"kernel {name}", scene, c, state, n_obj, cpu(cam.images["depth"]), cpu(cam.images["segmentation"]),
                     cpu(cam.images["pointcloud"]), case["show"])


# ----------------------------------------------------------------------------- exact selection
def cam_key(seed, counter, env, pix):
    """csrc/ha_camera.h cam_key in numpy (uint32, wrapping)."""
    with np.errstate(over="ignore"):
        lo, hi = U(seed & 0xFFFFFFFF), U((seed >> 32) & 0xFFFFFFFF)
        a = f32.mix32(lo ^ f32.mix32(hi + U(counter)))
        b = f32.mix32(a + U(env))
        return f32.mix32(b + np.asarray(pix, U) * U(0x9E3779B9))


def expected_target(pc, seg, tgt, P, seed, counter, env):
    """(P, 4): the target's points (seg == 3 + tgt) in pixel order; more than P of them: those with the P smallest
    (key, pixel), still in pixel order; zero padding; w x 2."""
    pix = np.nonzero(seg == 3 + tgt)[0]
    if len(pix) > P:
        key = cam_key(seed, counter, env, pix)
        order = sorted(range(len(pix)), key=lambda i: (int(key[i]), int(pix[i])))
        pix = np.sort(pix[order[:P]])
    out = np.zeros((P, 4), np.float32)
    out[:len(pix)] = pc[pix]
    out[:, 3] *= np.float32(2)
    return out


# (W, H), P: 160 x 90 has strips of 57 pixels per thread, which do not divide 14400 (the last strips are short or
# empty); 13 x 7 has fewer pixels than threads; 51 x 29 a ragged last strip again
SELECT = [((160, 90), 64), ((160, 90), 1), ((13, 7), 8), ((51, 29), 16)]


@pytest.mark.parametrize("res,P", SELECT, ids=[f"{w}x{h}-P{p}" for (w, h), p in SELECT])
def test_target_selection_is_exact(res, P):
    """Segmentation and depth written directly (render(from_depth=True) recomputes the point cloud and runs the
    target kernel). Per env a different count K of target pixels: P - 1 and P (all kept, padded), P + 1, half the
    image, the whole image (K >> P), and P + 1 target pixels that sit at the very end of the image (the last strips)."""
    need_gpu()
    from handarm_hip.sim import HandArmSim
    W, H = res
    HW = W * H
    rng = np.random.default_rng(HW + P)
    counts = [max(P - 1, 0), P, P + 1, HW // 2, HW, -(P + 1), -min(HW, 3 * P + 5)]
    N = len(counts)
    sim = HandArmSim(N, "cuda:0")
    tgt = np.arange(N) % 3
    sim.t["target_object_index"].copy_(torch.from_numpy(tgt).to(sim.t["target_object_index"].dtype))
    seg = np.zeros((N, HW), np.int32)
    for e, K in enumerate(counts):
        other = [0, 1] + [3 + i for i in range(3) if i != tgt[e]]
        seg[e] = rng.choice(other, HW)
        where = np.arange(HW - (-K), HW) if K < 0 else rng.choice(HW, K, replace=False)   # K < 0: the last -K pixels
        seg[e, where] = 3 + tgt[e]
    depth = -rng.uniform(0.3, 1.5, (N, H, W)).astype(np.float32)
    cam = CAM.CameraSensor(sim, REF.TOPVIEW["pos"], REF.TOPVIEW["quat"], REF.TOPVIEW["fovx"], (W, H),
                           ["depth", "target_object_pointcloud"], max_num_points=P)
    cam.images["depth"].copy_(torch.from_numpy(depth))
    cam.images["segmentation"].copy_(torch.from_numpy(seg.reshape(N, H, W)))
    seed = int(sim.params.seed)
    seen = []
    for _ in range(2):                                      # two refreshes: the counter moves, so does the subset
        cam.render(from_depth=True)
        counter = int(cam.args.rng_counter)
        pc = cpu(cam.images["pointcloud"]).reshape(N, HW, 4)
        np.testing.assert_array_equal(cpu(cam.images["segmentation"]).reshape(N, HW), seg)
        assert 0.1 < pc[..., 3].mean() < 0.9                # both values of w are selected from
        got = cpu(cam.images["target_object_pointcloud"])
        for e in range(N):
            want = expected_target(pc[e], seg[e], tgt[e], P, seed, counter, e)
            assert np.array_equal(got[e].view(U), want.view(U)), \
                f"{W}x{H} P {P} env {e} ({abs(counts[e])} target pixels): rows differ at {np.nonzero((got[e] != want).any(1))[0][:8]}"
        seen.append(got)
    big = [e for e, K in enumerate(counts) if abs(K) > P + 16]
    assert big and all(not np.array_equal(seen[0][e], seen[1][e]) for e in big)
