"""ha_render_camera_mounted (csrc/ha_camera.h cam_render<true>): a camera mounted on a robot link, every env rendered
from its own pose in one launch, against references that share nothing with the kernel.

  * Pose: ``cam.pose`` (the pose the launch used) against the float64 composition of tests/camera_mount_ref.py from the
    read-back rigid_body_state. Positions within 1e-6 m, quaternion components within 1e-6 up to sign, unit norm within
    1e-6. The bound is derived: the product is four 4-term float32 chains on unit quaternions, about 4 ulps of 1
    (4.8e-7); the normalisation and a rotated offset of at most 0.1 m beside a position of order 1 m add less than
    that again; 1e-6 is about twice the sum.
  * Images: per env, camera_ref.check_images with ``cam`` = that env's row of ``cam.pose`` read back as float64, on the
    kernel's depth, segmentation and point cloud. Feeding the reference the pose the kernel reports puts the kernel in
    the situation DEPTH_BOUND was derived for (a given float32 pose); the pose test carries the composition error.
    Bounds unchanged: stable pixels' ids all equal, |t - t_ref| cos / (1 + t_ref) <= 8 x 2^-23, hit points within
    their tolerance (which holds the rigid inverse view to the ray convention).

Teeth (each applied to a scratch build of the kernel, test_pose_and_images_against_reference run on it on an MI355X):
  * a transposed rotation (the view axes built from the conjugate of q): the id assertion of the image test fails in
    all 9 cases (83-1852 stable pixels differ);
  * the mount offset left unrotated: the pose test fails in the 8 transform-mode cases (positions off by 2-20 cm; the
    position-mode case does not rotate the offset and passes);
  * the view inverse taken from the fixed path (the launch's vinv field): the hit-point assertion of the image test
    fails in all 9 cases.

Measured on an MI355X (each test prints its own; DESIGN.md 3.10 lists them beside the fixed camera's): pose error at
most 5.6e-8 m and 1.1e-7 per quaternion component, | |q| - 1 | at most 9.4e-8; stable share 0.986-1.0, depth error at
most 1.7e-7 (1.39 ulp), hit-point error at most 0.11 of its tolerance.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from handarm_hip import cameras as CAM
from handarm_hip import model as HM
from tests import camera_mount_ref as MREF
from tests import camera_ref as REF

pytestmark = pytest.mark.gpu
U = np.uint32
POSE_BOUND = 1e-6
STATE_KEYS = ("root_state", "dof_state", "sim_targets", "object_indices", "goal_pos")


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def cpu(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def make_sim(case):
    """The camera_ref state of the case on the device: (sim, scene), after SIM_CALLS simulate calls."""
    from handarm_hip.sim import HandArmSim
    from oracle.oracle_lib import HostState
    rc = MREF.state_case(case)
    scene = REF.case_scene(rc)
    N = rc["N"]
    sim = HandArmSim(N, "cuda:0", task_cfg={"n_objects": MREF.n_objects(case)}, scene=scene)
    st = HostState(N, model=sim.model, params=sim.params)
    REF.fill_case(rc, st, scene)
    for k in STATE_KEYS:
        sim.t[k].copy_(torch.from_numpy(np.ascontiguousarray(st[k])).reshape(sim.t[k].shape).to(sim.t[k].dtype))
    sim.simulate(REF.SIM_CALLS)
    return sim, scene


def make_camera(case, sim, scene, outputs=CAM.IMAGE_TYPES[:3], by_name=True, **kw):
    mt = case["mount"]
    return CAM.CameraSensor(sim, mt["pos"], mt["quat"], MREF.FOVX, case["res"], outputs, scene=scene,
                            link=mt["name"] if by_name else mt["link"], follow=case["follow"], **kw)


def read_state(sim):
    N = sim.num_envs
    return dict(root=cpu(sim.t["root_state"]).reshape(N, sim.num_actors, 13),
                body=cpu(sim.t["rigid_body_state"]).reshape(N, sim.num_bodies, 13),
                object_indices=cpu(sim.t["object_indices"]), goal=cpu(sim.t["goal_pos"]))


def check_pose(tag, case, sim, cam, state):
    """cam.pose against the float64 composition from the read-back body rows. Returns the float64 poses (N, 7)."""
    pose = cpu(cam.pose).astype(np.float64)
    row = MREF.body_row(case, sim.model.body_robot0)
    assert cam.body == row
    worst_p = worst_q = worst_n = 0.0
    for e in range(sim.num_envs):
        p, q = MREF.compose(state["body"][e][row], case["mount"], case["follow"], np.float64)
        sign = 1.0 if pose[e, 3:7] @ q >= 0 else -1.0
        worst_p = max(worst_p, np.abs(pose[e, 0:3] - p).max())
        worst_q = max(worst_q, np.abs(sign * pose[e, 3:7] - q).max())
        worst_n = max(worst_n, abs(np.linalg.norm(pose[e, 3:7]) - 1.0))
    print(f"{tag}: pose vs float64 composition: position {worst_p:.3e} m, quaternion {worst_q:.3e}, "
          f"| |q| - 1 | {worst_n:.3e} (bound {POSE_BOUND:.0e})")
    assert worst_p <= POSE_BOUND and worst_q <= POSE_BOUND and worst_n <= POSE_BOUND, (worst_p, worst_q, worst_n)
    return pose


def check_render(tag, case, sim, scene, cam):
    """Tests 1 and 2 on the images cam holds: pose, then check_images per env from the reported pose."""
    state = read_state(sim)
    pose = check_pose(tag, case, sim, cam, state)
    worst = MREF.check_mounted_images(tag, scene, case, state, pose, cpu(cam.images["depth"]),
                                      cpu(cam.images["segmentation"]), cpu(cam.images["pointcloud"]))
    print(f"{tag}: worst stable share {worst[0]:.4f}, depth error {worst[1]:.3e} ({worst[1] / 2.0 ** -23:.2f} ulp), "
          f"hit-point error / tolerance {worst[2]:.3f}")
    return pose


@pytest.mark.parametrize("name", list(MREF.ALL_CASES))
def test_pose_and_images_against_reference(name):
    """Every row of the table, and the position-mode case: the pose (test 1) and the images (test 2)."""
    need_gpu()
    case = MREF.ALL_CASES[name]
    sim, scene = make_sim(case)
    cam = make_camera(case, sim, scene)
    cam.render()
    check_render(f"kernel {name}", case, sim, scene, cam)
    V = cpu(cam.view_matrices())                            # per env the matrix view_matrix() builds from that pose
    pose = cpu(cam.pose)
    for e in range(sim.num_envs):
        np.testing.assert_allclose(V[e], CAM.view_matrix(pose[e, 0:3], pose[e, 3:7]), rtol=0, atol=2e-6)


def test_camera_follows_the_link():
    need_gpu()
    case = MREF.CASES["default_palm_tilt45"]
    sim, scene = make_sim(case)
    cam = make_camera(case, sim, scene, by_name=False)
    cam.render()
    first = check_render("follow, before", case, sim, scene, cam)
    sim.t["sim_targets"][:, 0:6] += 0.15                    # the arm's joints: the palm moves 8-9 cm in 10 calls
    sim.simulate(10)
    cam.render()
    second = check_render("follow, after", case, sim, scene, cam)
    moved = np.linalg.norm(second[:, 0:3] - first[:, 0:3], axis=1)
    print(f"follow: the camera moved {moved.min() * 1e3:.1f}-{moved.max() * 1e3:.1f} mm")
    assert (moved > 1e-3).all(), moved


def test_from_depth_reproduces_the_pointcloud():
    need_gpu()
    case = MREF.CASES["default_palm_down_51x29"]
    sim, scene = make_sim(case)
    cam = make_camera(case, sim, scene)
    cam.render()
    pc = cpu(cam.images["pointcloud"]).copy()
    depth, seg, pose = cpu(cam.images["depth"]).copy(), cpu(cam.images["segmentation"]).copy(), cpu(cam.pose).copy()
    assert np.isfinite(pc[..., 0:3]).all() and 0.0 < pc[..., 3].mean() < 1.0
    cam.images["pointcloud"].fill_(float("nan"))
    cam.pose.fill_(float("nan"))
    cam.render(from_depth=True)
    assert np.array_equal(cpu(cam.images["pointcloud"]).view(U), pc.view(U))
    assert np.array_equal(cpu(cam.pose).view(U), pose.view(U))
    assert np.array_equal(cpu(cam.images["depth"]).view(U), depth.view(U))
    assert np.array_equal(cpu(cam.images["segmentation"]), seg)


@pytest.mark.parametrize("name", ["default_palm_down_51x29", "default_palm_down_20x11"])
def test_write_discipline(name):
    """Every element of the images and of pose is written (prefilled with NaN / a sentinel); no bound state tensor
    changes; a fixed camera's images are the same before and after a mounted render."""
    need_gpu()
    case = MREF.CASES[name]
    sim, scene = make_sim(case)
    fixed = CAM.CameraSensor(sim, REF.TOPVIEW["pos"], REF.TOPVIEW["quat"], MREF.FOVX, case["res"], scene=scene)
    fixed.render()
    before_fixed = {k: cpu(v).copy() for k, v in fixed.images.items()}
    before_state = {k: cpu(v).copy() for k, v in sim.t.items()}
    cam = make_camera(case, sim, scene)
    cam.images["depth"].fill_(float("nan"))
    cam.images["pointcloud"].fill_(float("nan"))
    cam.images["segmentation"].fill_(-12345)
    cam.pose.fill_(float("nan"))
    cam.render()
    assert not np.isnan(cpu(cam.images["depth"])).any()
    assert not np.isnan(cpu(cam.images["pointcloud"])).any()
    assert not (cpu(cam.images["segmentation"]) == -12345).any()
    assert np.isfinite(cpu(cam.pose)).all()
    for k, v in sim.t.items():
        assert np.array_equal(cpu(v).view(np.uint8), before_state[k].view(np.uint8)), f"state tensor {k} changed"
    for v in fixed.images.values():
        v.zero_()
    fixed.render()
    for k, v in fixed.images.items():
        assert np.array_equal(cpu(v).view(np.uint8), before_fixed[k].view(np.uint8)), f"fixed camera's {k} changed"


def test_target_object_pointcloud():
    need_gpu()
    from tests.test_gpu_camera_ref import expected_target
    case = MREF.CASES["default_palm_down"]
    P = 8
    sim, scene = make_sim(case)
    N = sim.num_envs
    W, H = case["res"]
    tgt = np.arange(N) % 2                                  # objects 0 and 1 (ids 3 and 4): in view in every env
    sim.t["target_object_index"].copy_(torch.from_numpy(tgt).to(sim.t["target_object_index"].dtype))
    cam = make_camera(case, sim, scene, outputs=["depth", "target_object_pointcloud"], max_num_points=P)
    cam.render()
    pc = cpu(cam.images["pointcloud"]).reshape(N, W * H, 4)
    seg = cpu(cam.images["segmentation"]).reshape(N, W * H)
    got = cpu(cam.images["target_object_pointcloud"])
    counts = [(seg[e] == 3 + tgt[e]).sum() for e in range(N)]
    assert max(counts) > P and min(counts) > 0, counts      # the exact selection runs, and every env sees its target
    for e in range(N):
        want = expected_target(pc[e], seg[e], tgt[e], P, int(sim.params.seed), int(cam.args.rng_counter), e)
        assert np.array_equal(got[e].view(U), want.view(U)), f"env {e} ({counts[e]} target pixels)"


def test_argument_errors_launch_nothing():
    need_gpu()
    case = MREF.CASES["default_palm_down_20x11"]
    sim, scene = make_sim(case)
    cam = make_camera(case, sim, scene)
    for v in (cam.images["depth"], cam.images["pointcloud"], cam.pose):
        v.fill_(float("nan"))
    cam.images["segmentation"].fill_(-12345)

    def call(**kw):
        mt = HM.HaCameraMount.from_buffer_copy(cam.mount)
        for k, v in kw.items():
            if k == "quat":
                mt.quat[:] = v
            else:
                setattr(mt, k, v)
        return sim.lib.ha_render_camera_mounted(sim.h, C.byref(cam.args), C.byref(mt), 0, sim._stream())

    E_ARG = -1
    assert call(body=sim.num_bodies) == E_ARG
    assert call(body=-1) == E_ARG
    assert call(mode=2) == E_ARG
    assert call(quat=[0.0, 0.0, 0.0, 0.0]) == E_ARG
    assert sim.lib.ha_render_camera_mounted(sim.h, C.byref(cam.args), None, 0, sim._stream()) == E_ARG
    assert np.isnan(cpu(cam.images["depth"])).all() and np.isnan(cpu(cam.images["pointcloud"])).all()
    assert (cpu(cam.images["segmentation"]) == -12345).all() and np.isnan(cpu(cam.pose)).all()
    assert call() == 0                                      # the unperturbed copy is accepted
    assert np.isfinite(cpu(cam.pose)).all()
    with pytest.raises(ValueError):
        make_camera(dict(case, follow="orbit"), sim, scene)
    with pytest.raises(ValueError):
        make_camera(dict(case, mount=dict(case["mount"], quat=(0, 0, 0, 0))), sim, scene)


def test_mounted_camera_through_vectask():
    need_gpu()
    from handarm_hip.tasks import Ur5SihMultiObjectManipulation
    N = 2
    mt = MREF.MOUNTS["palm_down"]
    obs = ["ur5_flange_pose", "wrist_depth", "wrist_segmentation"]
    cfg = {"env": {"numEnvs": N, "observations": obs}, "seed": 1,
           "cameras": {"wrist": dict(link="palm", pos=list(mt["pos"]), quat=list(mt["quat"]), resolution=[20, 11])}}
    env = Ur5SihMultiObjectManipulation(cfg, "cuda:0", "cuda:0")
    assert env.observation_keys == ["obs", "wrist_depth", "wrist_segmentation"]
    out, _, _, _ = env.step(torch.zeros((N, 11), device="cuda:0"))
    assert out["wrist_depth"].shape == (N, 11, 20) and out["wrist_segmentation"].dtype == torch.int32
    depth, seg = cpu(out["wrist_depth"]).copy(), cpu(out["wrist_segmentation"]).copy()
    assert env.cameras["wrist"].body == env.sim.model.body_robot0 + mt["link"]
    direct = CAM.CameraSensor(env.sim, mt["pos"], mt["quat"], 87, (20, 11), ["depth", "segmentation"], scene=env.scene,
                              link=mt["link"])
    direct.render()
    assert np.array_equal(cpu(direct.images["depth"]).view(U), depth.view(U))
    assert np.array_equal(cpu(direct.images["segmentation"]), seg)
    assert np.array_equal(cpu(direct.pose).view(U), cpu(env.cameras["wrist"].pose).view(U))
    assert np.isfinite(depth).any() and len(np.unique(seg)) > 1
    envs_differ = not np.array_equal(depth[0].view(U), depth[1].view(U))
    assert envs_differ or np.array_equal(cpu(direct.pose)[0], cpu(direct.pose)[1])
