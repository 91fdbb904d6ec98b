"""Mounted cameras on the CPU: the cases of tests/camera_mount_ref.py pinned on the float64 reference alone, the numpy
oracle's ray cast seen from per-env poses against that reference, CameraSensor's link resolution, and the ABI binding.

  * Cases: per case and env the reference's stable share is >= 0.98 and every ``show`` id covers >= 3 stable pixels,
    with the C oracle's states and the camera pose composed in float64 (the table of camera_mount_ref's docstring).
  * Oracle: the pose composition of csrc/ha_camera.h is restated in float32 numpy (camera_mount_ref.compose) and each
    env's pose is fed as a camera dict to oracle/camera_oracle.py render_depth_segmentation / pointcloud_from_depth,
    the latter with the rigid inverse view (rows: the view axes; last row: the position). camera_ref.check_images then
    runs one env at a time with that env's float32 pose as ``cam``: DEPTH_BOUND and STABLE_SHARE unchanged.

tests/test_gpu_camera_mount.py runs the same cases and assertions on the kernel's images.
"""
import functools
import math
import types

import numpy as np
import pytest

from handarm_hip import _lib
from handarm_hip import cameras as CAM
from handarm_hip import model as HM
from oracle import camera_oracle as CO
from tests import camera_mount_ref as MREF
from tests import camera_ref as REF
from tests.test_camera_ref import simulated_state

F = np.float32


@functools.lru_cache(maxsize=None)
def state_of(name):
    """(scene, model, n_obj, state) of a camera_ref case after the C oracle's SIM_CALLS simulate calls."""
    case = REF.CASES[name]
    scene = REF.case_scene(case)
    m, n_obj, state = simulated_state(case, scene)
    return scene, m, n_obj, state


def poses_of(case, m, state, dtype):
    row = MREF.body_row(case, m.body_robot0)
    return [np.concatenate(MREF.compose(state["body"][e][row], case["mount"], case["follow"], dtype))
            for e in range(len(state["body"]))]


@pytest.mark.parametrize("name", list(MREF.ALL_CASES))
def test_cases_on_the_reference(name):
    case = MREF.ALL_CASES[name]
    scene, m, n_obj, state = state_of(case["state"])
    shares = []
    for e, pose in enumerate(poses_of(case, m, state, np.float64)):
        cam = MREF.env_camera(case, scene, pose[0:3], pose[3:7])
        t, sid, _, stable = REF.render(scene, cam, state["root"][e], state["body"][e], state["object_indices"][e],
                                       state["goal"][e], n_obj)
        shares.append(stable.mean())
        assert shares[-1] >= REF.STABLE_SHARE, f"{name} env {e}: stable share {shares[-1]:.4f}"
        for s in case["show"]:
            cnt = int((stable & (sid == s)).sum())
            assert cnt >= REF.MIN_PIXELS, f"{name} env {e}: id {s} covers {cnt} stable pixels"
    print(f"{name}: reference's stable share per env {', '.join(f'{s:.3f}' for s in shares)}")


def mounted_oracle_images(m, scene, case, state, n_obj, poses):
    """The numpy oracle's images with env e seen from poses[e] (float32), the point cloud through the rigid inverse."""
    W, H = case["res"]
    tanx = F(math.tan(0.5 * math.radians(MREF.FOVX)))
    tany = F(tanx * F(H) / F(W))
    depth, seg, pc = [], [], []
    for e, pose in enumerate(poses):
        c = dict(MREF.env_camera(case, scene, pose[0:3], pose[3:7]), static_seg=CAM.static_segmentation_ids(scene))
        d, s = CO.render_depth_segmentation(m, c, state["root"][e], state["body"][e], state["object_indices"][e],
                                            state["goal"][e], m.actor_object0, m.body_robot0, n_obj)
        vinv = np.zeros((4, 4), F)
        vinv[0:3, 0:3] = CO.camera_axes(pose[3:7]).T            # rows: the view axes in the env frame
        vinv[3, 0:3] = pose[0:3]
        vinv[3, 3] = 1
        depth.append(d)
        seg.append(s)
        pc.append(CO.pointcloud_from_depth(d[None], F(2) * tanx, F(2) * tany, vinv)[0])
    return np.stack(depth), np.stack(seg), np.stack(pc)


@pytest.mark.parametrize("name", list(MREF.ALL_CASES))
def test_oracle_against_reference(name):
    case = MREF.ALL_CASES[name]
    scene, m, n_obj, state = state_of(case["state"])
    poses = poses_of(case, m, state, np.float32)
    assert all(p.dtype == F for p in poses)
    for p32, p64 in zip(poses, poses_of(case, m, state, np.float64)):       # the two compositions agree (up to sign)
        sign = np.sign(p32[3:7] @ p64[3:7])
        assert np.abs(p32[0:3] - p64[0:3]).max() <= 1e-6 and np.abs(sign * p32[3:7] - p64[3:7]).max() <= 1e-6
    depth, seg, pc = mounted_oracle_images(m, scene, case, state, n_obj, poses)
    MREF.check_mounted_images(f"oracle {name}", scene, case, state, [p.astype(np.float64) for p in poses], depth, seg, pc)


def _sim_stub(scene):
    """What mount_body reads of a HandArmSim, without a device."""
    from handarm_hip.sim import HandArmSim
    m = HM.build_model(scene)
    stub = types.SimpleNamespace(scene=scene, model=m, num_links=m.n_links, num_bodies=m.n_bodies)
    stub.link_index = lambda link: HandArmSim.link_index(stub, link)
    return stub


def test_link_resolution():
    scene = HM.load_scene()
    sim = _sim_stub(scene)
    for mount in MREF.MOUNTS.values():
        row = CAM.mount_body(sim, link=mount["name"])
        assert row == CAM.mount_body(sim, link=mount["link"]) == sim.model.body_robot0 + mount["link"]
        assert CAM.mount_body(sim, body=row) == row
    assert CAM.mount_body(sim) is None
    with pytest.raises(KeyError):
        CAM.mount_body(sim, link="no_such_link")
    for bad in (dict(link=sim.num_links), dict(link=-1), dict(body=sim.num_bodies), dict(body=-1), dict(link=12, body=13)):
        with pytest.raises(ValueError):
            CAM.mount_body(sim, **bad)


def test_abi_declaration():
    import ctypes as C
    assert "ha_render_camera_mounted" in _lib.header_symbols()
    args, res = _lib.SIGNATURES["ha_render_camera_mounted"]
    assert res is C.c_int and args[2] is C.POINTER(HM.HaCameraMount) and len(args) == 5
    # int32 body, int32 mode, float pos[3], float quat[4], then the 8-byte pointer
    assert C.sizeof(HM.HaCameraMount) == 48 and HM.HaCameraMount.pose_out.offset == 40
    assert (HM.CAM_FOLLOW_TRANSFORM, HM.CAM_FOLLOW_POSITION) == (0, 1)
    lib = _lib.load()
    assert hasattr(lib, "ha_render_camera_mounted")
    assert lib.ha_render_camera_mounted(None, None, None, 0, None) == -1        # HA_E_ARG, no GPU touched
