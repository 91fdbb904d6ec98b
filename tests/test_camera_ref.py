"""The camera ray cast's numpy oracle (oracle/camera_oracle.py, the float32 restatement of csrc/ha_camera.h) against
the independent float64 reference built from the hull vertices (tests/camera_ref.py), on the CPU; the asset checks of
the hull records the ray cast's bounding spheres and plane slabs come from; and the host's hull-table count
(include/ha_cam_hulls.h) through the oracle library.

tests/test_gpu_camera_ref.py runs the same cases and the same assertions on the kernel's images.

Per case, on the pixels whose five reference rays (centre, +-0.05 pixel in col and row) agree on the id:
  * the stable share is >= 0.98 of every image and every id the case is built to show covers >= 3 stable pixels;
  * the ids are equal, all of them;
  * |t - t_ref| cos(theta) / (1 + t_ref) <= 8 x 2^-23 (9.5e-7): the float32 path from pose to t is two quaternion
    rotations, two dot products and a divide; the error grows by 1 / cos(theta) at grazing incidence and with 1 + t;
  * the point cloud's xyz lies within 2e-6 + |d| x (that depth bound as an error of t) of o + t_ref d, which ties the
    ray convention to the golden-pinned inverse mapping of the reference.

Measured (oracle vs reference; each case prints its own, DESIGN.md 3.10 lists them): stable share 0.986-1.0, depth
error at most 1.8e-7 (1.5 ulp), hit-point error at most 0.13 of its tolerance. Before the goal sphere's intersection
was rewritten through the closest approach (its discriminant cancelled) the goal's pixels reached 8.6e-7 (7.2 ulp).

Teeth (each applied to a scratch copy of the oracle): hull_radius x 0.8, the last plane of each hull skipped and two
object ids swapped each fail the id or depth assertion of 10-11 of the 11 cases; dropping ``t0 > 0`` fails
inside_table.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from handarm_hip import cameras as CAM
from handarm_hip import model as HM
from oracle import camera_oracle as CO
from oracle.oracle_lib import HostState, Oracle, load
from tests import camera_ref as REF

F = np.float32
SCENES = [HM.ASSET, HM.BIN_ASSET, HM.ALLEGRO_ASSET, HM.KUKA_ASSET]


def simulated_state(case, scene):
    """The case's state after SIM_CALLS gym.simulate calls of the C oracle: (model, state dict of per-env rows)."""
    n_obj = 8 if case["kind"] == "bin" else 3
    m = HM.build_model(scene)
    p, _ = HM.build_params({"n_objects": n_obj})
    N = case["N"]
    st = HostState(N, model=m, params=p)
    REF.fill_case(case, st, scene)
    Oracle(m, p, N).simulate(st, REF.SIM_CALLS)
    state = dict(root=st["root_state"].reshape(N, m.n_actors, 13).copy(),
                 body=st["rigid_body_state"].reshape(N, m.n_bodies, 13).copy(),
                 object_indices=st["object_indices"].copy(), goal=st["goal_pos"].copy())
    return m, n_obj, state


def oracle_images(m, scene, cam, state, n_obj):
    """depth (N, H, W), segmentation (N, H, W), pointcloud (N, H, W, 4) of the numpy oracle, as CameraSensor feeds the
    kernel (float32 view inverse, fu = 2 tan(fovx / 2))."""
    c = dict(cam, static_seg=CAM.static_segmentation_ids(scene))
    N = len(state["root"])
    out = [CO.render_depth_segmentation(m, c, state["root"][e], state["body"][e], state["object_indices"][e],
                                        state["goal"][e], m.actor_object0, m.body_robot0, n_obj) for e in range(N)]
    depth = np.stack([d for d, _ in out])
    seg = np.stack([s for _, s in out])
    vinv = torch.linalg.inv(torch.from_numpy(CAM.view_matrix(cam["pos"], cam["quat"]))).numpy()
    tanx = F(math.tan(0.5 * math.radians(cam["fovx"])))
    tany = F(tanx * F(cam["height"]) / F(cam["width"]))
    return depth, seg, CO.pointcloud_from_depth(depth, F(2) * tanx, F(2) * tany, vinv)


@pytest.mark.parametrize("name", list(REF.CASES))
def test_oracle_against_reference(name):
    case = REF.CASES[name]
    scene = REF.case_scene(case)
    cam = REF.case_camera(case, scene)
    m, n_obj, state = simulated_state(case, scene)
    depth, seg, pc = oracle_images(m, scene, cam, state, n_obj)
    REF.check_images(f"oracle {name}", scene, cam, state, n_obj, depth, seg, pc, case["show"])


def test_cases_reach_the_kernel_branches():
    """What the cases are built for, checked on the reference itself: a pixel column with d.y == 0 exactly (den == 0
    against an axis-aligned box) looking straight down, a horizon row with d.z == 0 and rows without a hit looking
    horizontally, the table unseen from inside, compound objects in every env, both image-size edge cases."""
    scene = HM.load_scene()
    c = REF.case_camera(REF.CASES["straight_down"], scene)
    row, col = np.divmod(np.arange(c["width"] * c["height"]), c["width"])
    d32 = CO.rays(c["width"], c["height"], c["fovx"], c["quat"])
    assert c["width"] % 2 == 0 and np.all(d32[col == c["width"] // 2, 1] == 0)
    for name in ("horizontal_plus_x", "horizontal_minus_x"):
        c = REF.case_camera(REF.CASES[name], scene)
        d32 = CO.rays(c["width"], c["height"], c["fovx"], c["quat"]).reshape(c["height"], c["width"], 3)
        assert np.all(d32[c["height"] // 2, :, 2] == 0)
        m, n_obj, state = simulated_state(REF.CASES[name], scene)
        t, sid, _, stable = REF.render(scene, c, state["root"][0], state["body"][0], state["object_indices"][0],
                                       state["goal"][0], n_obj)
        assert np.isinf(t[:c["height"] // 2]).mean() > 0.3                  # sky above the horizon
        ahead = np.sign(REF.rotation(c["quat"])[0, 0])
        behind = [(state["root"][0][3 + i, 0] - c["pos"][0]) * ahead < 0 for i in range(3)]
        assert any(behind)                                                  # a hull behind the camera
        assert all(not (sid == 3 + i).any() for i in range(3) if behind[i])
    case = REF.CASES["inside_table"]
    c = REF.case_camera(case, scene)
    tb = scene["table"]
    assert np.all(np.abs(np.array(c["pos"]) - tb["pos"]) < np.array(tb["half_extents"]) - 0.01)
    nh = [len(o.get("hulls") or [0]) for o in scene["objects"]]
    assert all(nh[i] >= 8 for row_ in REF.CASES["compound_objects"]["object_indices"] for i in row_)
    assert sorted(i for row_ in REF.CASES["compound_objects"]["object_indices"] for i in row_) == \
        [i for i, k in enumerate(nh) if k > 1]
    w, h = REF.CASES["image_13x7"]["res"]
    assert w * h < 256 and w % 2 and h % 2
    w, h = REF.CASES["image_51x29"]["res"]
    assert (w * h) % 256 != 0


# ----------------------------------------------------------------------------- assets
@pytest.mark.parametrize("path", SCENES, ids=[os.path.basename(p) for p in SCENES])
def test_hull_records_agree_with_their_vertices(path):
    """Every hull record: unit plane normals, every plane touching the hull (its farthest vertex on it), and the
    (center, radius) sphere containing every vertex, each within 1e-9 (measured 2.2e-16, 1.1e-16 and 0)."""
    worst = np.zeros(3)
    n = 0
    for label, h in REF.hull_records(HM.load_scene(path)):
        unit, support, out = REF.record_errors(h)
        assert unit <= 1e-9, (label, unit)
        assert support <= 1e-9, (label, support)
        assert out <= 1e-9, (label, out)
        worst = np.maximum(worst, [unit, support, out])
        n += 1
    assert n > 0
    print(f"{os.path.basename(path)}: {n} hull records, | |n| - 1 | <= {worst[0]:.1e}, plane support <= {worst[1]:.1e}, "
          f"vertex outside sphere by <= {worst[2]:.1e}")


@pytest.mark.parametrize("kind", ["default", "bin"])
def test_model_spheres_contain_the_float32_vertices(kind):
    """The built model's float32 hull_center / hull_radius (what the ray cast prunes with) contain the model's float32
    vertices to within one ulp of the radius."""
    m = HM.build_model(HM.load_scene(HM.BIN_ASSET if kind == "bin" else HM.ASSET))
    verts = np.ctypeslib.as_array(m.verts).astype(np.float64)
    for k in range(m.n_hulls):
        v = verts[m.hull_vert_start[k]:m.hull_vert_start[k] + m.hull_nverts[k], :3]
        c = np.array(m.hull_center[k][:], np.float64)
        r = F(m.hull_radius[k])
        far = np.linalg.norm(v - c, axis=1).max()
        assert far <= float(r) + float(np.spacing(r)), (k, far, float(r))


# ----------------------------------------------------------------------------- the hull-table count
def _count(lib, n_link_hulls, n_static, nhull, n_obj):
    a = (C.c_int32 * max(len(nhull), 1))(*nhull)
    return lib.hao_cam_hull_count(n_link_hulls, n_static, len(nhull), a, n_obj)


def test_hull_table_count():
    """ha_cam_hull_count (include/ha_cam_hulls.h), the text ha_create compiles for ha_render_camera's guard: link hulls
    + the n_obj largest pool_nhull + statics."""
    lib = load()
    lib.hao_cam_hull_count.restype = C.c_int
    lib.hao_cam_hull_count.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]
    cap = lib.hao_cam_max_hulls()
    assert cap == HM.MAX_HULLS + 1
    m = HM.build_model(HM.load_scene(), HM.POOL_WIDE)
    nh = list(m.pool_nhull[:m.n_pool])
    assert _count(lib, 0, 0, nh, 3) == 25 and _count(lib, 0, 0, nh, 8) == 65       # the wide pool's pieces
    assert _count(lib, m.n_link_hulls, m.n_static, nh, 3) == 22 + 25 + 1 <= cap
    mb = HM.build_model(HM.load_scene(HM.BIN_ASSET))
    assert _count(lib, mb.n_link_hulls, mb.n_static, list(mb.pool_nhull[:mb.n_pool]), 8) == 22 + 65 + 9 <= cap
    # the n_obj largest, whatever their order; a pool smaller than n_obj counts each entry once
    assert _count(lib, 2, 3, [1, 7, 2, 7, 5], 3) == 2 + 19 + 3
    assert _count(lib, 2, 3, [4, 6], 5) == 2 + 10 + 3
    assert _count(lib, 0, 0, [], 3) == 0
    # made-up counts beyond the table report so
    assert _count(lib, 22, 9, [33, 33, 33], 3) == 130 > cap
    assert _count(lib, 22, 9, [33, 33, 32], 3) == cap
    assert _count(lib, 22, 16, [HM.MAX_HULLS] * HM.MAX_POOL, 8) == 22 + 16 + 8 * HM.MAX_HULLS > cap
    assert _count(lib, 300, 0, [1], 1) == 301 > cap
    # counts outside the ABI's range are refused, not summed
    assert _count(lib, -1, 0, [1], 1) == -1 and _count(lib, 0, 0, [1, -2], 1) == -1
    assert lib.hao_cam_hull_count(0, 0, HM.MAX_POOL + 1, (C.c_int32 * 64)(), 1) == -1
    assert _count(lib, 2 ** 31 - 1, 2 ** 31 - 1, [2 ** 31 - 1], 1) == -1
