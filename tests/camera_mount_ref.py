"""Mounted cameras (ha_render_camera_mounted, csrc/ha_camera.h cam_render<true>): the mounts, the cases and the pose
composition both the CPU and the GPU test use. The ray cast's reference is tests/camera_ref.py, untouched: it takes
the camera as a plain dict per env, so a per-env pose is checked by calling ``check_images`` one env at a time.

Link indices are those of assets/ur5sih_scene.json; a mount is the camera frame (+X forward, +Z up) in the link
frame. The states are those of ``camera_ref.CASES`` (``fill_case``, then ``SIM_CALLS`` simulate calls); in them the
envs' palm positions differ by 10-15 cm, so one mount gives a different view in every env. fovx is 87 throughout.

The reference's own stable share per env and the ids each case shows (float64 reference alone, the C oracle's states,
pose composed in float64; tests/test_camera_mount.py asserts them):

  default_topview / palm_down / 64x36     0.995, 0.997, 0.999   0, 3, 4
  default_topview / palm_tilt45 / 64x36   0.998, 0.997, 0.998   0, 1
  default_topview / wrist2_side / 64x36   0.993, 0.996, 0.995   0, 1, 3, 4
  default_topview / thumbtip / 64x36      0.997, 0.995, 0.998   0, 1
  bin_topview / palm_down / 64x36         0.989, 0.990          0, 1, 2, 3, 4
  compound_objects / palm_down / 51x29    0.995, 0.997, 1.0     0, 1
  default_topview / palm_down / 51x29     0.996, 0.997, 0.997   0, 3, 4
  default_topview / palm_down / 20x11     0.991, 0.986, 0.991   0, 3

13x7 and 16x9 are not used with these mounts: the reference alone drops to 0.956-0.972 there, because the near finger
hulls leave too many silhouette pixels.
"""
import numpy as np

from tests import camera_ref as REF

FOVX = 87.0
FOLLOW_TRANSFORM, FOLLOW_POSITION = "transform", "position"

MOUNTS = {
    # looks out of the palm
    "palm_down": dict(link=12, name="palm", pos=(0.0, 0.03, 0.04), quat=(0.0, 0.0, 0.707107, 0.707107)),
    # sees the fingers and the table
    "palm_tilt45": dict(link=12, name="palm", pos=(0.0, 0.04, 0.0), quat=(0.270598, -0.270598, 0.653281, 0.653281)),
    # looks past the hand
    "wrist2_side": dict(link=7, name="wrist_2_link", pos=(0.1, 0.0, 0.0), quat=(0.653281, 0.270598, 0.653281, 0.270598)),
    # a link with no hull of its own
    "thumbtip": dict(link=28, name="thumb_fingertip", pos=(0.0, 0.0, 0.02), quat=(-0.5, -0.5, -0.5, 0.5)),
}


def _case(state, mount, res, show, follow=FOLLOW_TRANSFORM, quat=None):
    m = dict(MOUNTS[mount])
    if quat is not None:
        m["quat"] = tuple(quat)
    return dict(state=state, mount=m, res=res, show=show, follow=follow)


CASES = {
    "default_palm_down": _case("default_topview", "palm_down", (64, 36), [0, 3, 4]),
    "default_palm_tilt45": _case("default_topview", "palm_tilt45", (64, 36), [0, 1]),
    "default_wrist2_side": _case("default_topview", "wrist2_side", (64, 36), [0, 1, 3, 4]),
    "default_thumbtip": _case("default_topview", "thumbtip", (64, 36), [0, 1]),
    "bin_palm_down": _case("bin_topview", "palm_down", (64, 36), [0, 1, 2, 3, 4]),
    "compound_palm_down_51x29": _case("compound_objects", "palm_down", (51, 29), [0, 1]),
    "default_palm_down_51x29": _case("default_topview", "palm_down", (51, 29), [0, 3, 4]),
    "default_palm_down_20x11": _case("default_topview", "palm_down", (20, 11), [0, 3]),       # fewer than 256 pixels
}
# position mode: palm_down's offset added in env axes, the topview camera's orientation. The ids it shows were read off
# the float64 reference (stable share 0.995, 0.995, 0.996; the camera sits behind the hand and looks over it at the
# table, so every env shows the ground / table 0 and the robot 1; tests/test_camera_mount.py asserts both)
POSITION_CASE = _case("default_topview", "palm_down", (64, 36), [0, 1], FOLLOW_POSITION, REF.TOPVIEW["quat"])
ALL_CASES = dict(CASES, position_palm_topview=POSITION_CASE)


def state_case(case):
    """The camera_ref case whose state the mounted case uses."""
    return REF.CASES[case["state"]]


def n_objects(case):
    return 8 if state_case(case)["kind"] == "bin" else 3


def body_row(case, body_robot0):
    return body_robot0 + case["mount"]["link"]


def qmul(a, b):
    """Hamilton product of xyzw quaternions, in the dtype of the inputs."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def compose(row, mount, follow, dtype=np.float64):
    """Camera pose (pos (3,), unit quat (4,)) from a body's rigid_body_state row and the mount, in ``dtype``:
      follow transform: q = normalize(q_body x q_mount), p = p_body + rot(q_body, pos_mount)
      follow position:  q = normalize(q_mount),          p = p_body + pos_mount
    float64: the reference composition (the body quaternion is normalised first, a rotation matrix rotates the offset).
    float32: the restatement of what the kernel computes (v + w t + u x t, t = 2 u x v; no normalisation of q_body)."""
    T = dtype
    pb, qb = np.asarray(row[0:3], T), np.asarray(row[3:7], T)
    pm, qm = np.asarray(mount["pos"], T), np.asarray(mount["quat"], T)
    if T == np.float64:
        qb = qb / np.linalg.norm(qb)
        off = REF.rotation(qb) @ pm
    else:
        u = qb[0:3]
        t = np.cross(u, pm).astype(T) * T(2)
        off = ((pm + t * qb[3]) + np.cross(u, t).astype(T)).astype(T)
    if follow == FOLLOW_POSITION:
        q, off = qm, pm
    else:
        q = qmul(qb, qm).astype(T)
    n = np.sqrt((q * q).sum(dtype=T), dtype=T)
    return (pb + off).astype(T), (q / n).astype(T)


def env_camera(case, scene, pos, quat):
    """The camera dict camera_ref takes, for one env's pose."""
    W, H = case["res"]
    return dict(pos=[float(v) for v in pos], quat=[float(v) for v in quat], fovx=FOVX, width=W, height=H,
                goal_radius=scene.get("goal_radius", 0.02))


def env_state(state, e):
    """The one-env slice of a check_images state dict."""
    return {k: v[e:e + 1] for k, v in state.items()}


def check_mounted_images(tag, scene, case, state, poses, depth, seg, pointcloud):
    """camera_ref.check_images one env at a time, env e seen from poses[e] (7,). Bounds unchanged. Returns the worst
    (stable share, depth error, hit-point ratio) over the envs."""
    worst = [1.0, 0.0, 0.0]
    for e in range(len(poses)):
        cam = env_camera(case, scene, poses[e][0:3], poses[e][3:7])
        s, d, p = REF.check_images(f"{tag} env {e}", scene, cam, env_state(state, e), n_objects(case), depth[e:e + 1],
                                   seg[e:e + 1], None if pointcloud is None else pointcloud[e:e + 1], case["show"])
        worst = [min(worst[0], s), max(worst[1], d), max(worst[2], p)]
    return tuple(worst)
