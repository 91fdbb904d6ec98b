"""An independent float64 reference of the camera ray cast (csrc/ha_camera.h ha_camera_kernel), for the tests only.

It shares no code and no derived data with the kernel or with its numpy restatement (oracle/camera_oracle.py), for
the reason tests/test_independent_dynamics.py gives: a defect both sides share cannot fail a kernel-vs-oracle test.

  * Geometry: each scene hull record's ``verts`` only. The surface of a hull is the triangles of the convex hull of
    its vertices (scipy ConvexHull); ``planes``, ``center``, ``radius`` and the built ha_model_t are not read.
  * Test: Moeller-Trumbore ray-triangle intersection in float64, not a plane slab. Only front faces count (the ray
    enters the hull there), so a hull that contains the camera is not seen: that is the kernel's ``t0 > 0`` rule, and
    it is the defined behaviour. The goal sphere is treated the same way. Only the closest hit counts; no hit gives
    t = +inf (depth -inf) and id 0.
  * Poses in float64: link hulls from rigid_body_state through link_hulls[].index, object pieces from root_state and
    object_indices in pool order, statics from the scene, the ground plane z = 0, the goal sphere at goal_pos.
  * Segmentation ids from the reference's rule (multi_object.py:581-642, ur5sih.py:123-125): table and ground 0,
    robot 1, bin pieces 2, object i -> 3 + i, goal -> 3 + num_objects.
  * Rays in float64 from the documented convention: the camera looks along its local +X with +Z up (so +Y is left);
    pixel (col, row) has the view direction ((col - W/2)/W 2 tan(fovx/2), -(row - H/2)/H 2 tan(fovy/2), -1) with
    tan(fovy/2) = tan(fovx/2) H/W, view x = right, y = up, z = back.

Per pixel it returns t (= -depth, in units of that view direction), the id and the cosine between the ray and the hit
face. It also casts the four rays shifted by +-0.05 pixel in col and in row; a pixel is *stable* when all five rays
give the same id. Only stable pixels are compared: the others are silhouette pixels, where a float32 ulp may
legitimately flip the result.

The module also holds the checks every comparison makes (``check_images``), the cases both the CPU and the GPU test
run (``CASES``) and the asset checks of the hull records (planes and spheres against the vertices).
"""
import functools
import hashlib
import math

import numpy as np
from scipy.spatial import ConvexHull

# |t - t_ref| cos(theta) / (1 + t_ref) on stable pixels: 8 float32 ulps of 1. The float32 path from pose to t is two
# quaternion rotations, two dot products and a divide; the error grows by 1 / cos(theta) at grazing incidence and
# with the magnitudes 1 + t.
DEPTH_BOUND = 8.0 * 2.0 ** -23
STABLE_SHARE = 0.98
MIN_PIXELS = 3
SHIFT = 0.05                       # pixels
MAX_DEPTH = 10.0                   # camera.py:302: deeper hits are clamped in the point cloud


def rotation(q):
    """Rotation matrix of quaternion q (xyzw), normalised, float64."""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def view_directions(cam, col, row):
    """World directions of the rays through (col, row) (arrays, fractional pixels allowed): (..., 3)."""
    W, H = cam["width"], cam["height"]
    tx = math.tan(0.5 * math.radians(cam["fovx"]))
    ty = tx * H / W
    Rc = rotation(cam["quat"])
    fwd, left, up = Rc[:, 0], Rc[:, 1], Rc[:, 2]
    xv = (np.asarray(col, np.float64) - W / 2) / W * 2 * tx
    yv = -(np.asarray(row, np.float64) - H / 2) / H * 2 * ty
    # view axes: x right = -left, y up, z back = -fwd; direction (xv, yv, -1)
    return xv[..., None] * (-left) + yv[..., None] * up + fwd


@functools.lru_cache(maxsize=None)
def _triangles_cached(key, shape):
    v = np.frombuffer(key, np.float64).reshape(shape)
    tri = v[ConvexHull(v).simplices]                       # (T, 3, 3); qhull triangulates coplanar facets (Qt)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    flip = ((tri[:, 0] - v.mean(0)) * n).sum(1) < 0        # outward: away from the vertex centroid (inside a convex hull)
    tri[flip] = tri[flip][:, [0, 2, 1]]
    return tri


def hull_triangles(verts):
    """(T, 3, 3) outward-oriented surface triangles of the convex hull of verts (body frame)."""
    v = np.ascontiguousarray(verts, np.float64)
    return _triangles_cached(v.tobytes(), v.shape)


def scene_surfaces(scene, root, body, object_indices, pool_names=None):
    """[(world triangles (T, 3, 3), id)] of one env: robot link hulls, object pieces, statics.
    root (A, 13), body (B, 13): the env's rows of root_state / rigid_body_state."""
    lay = scene.get("layout") or {}
    body_robot0 = lay.get("body_robot0", 1)               # bodies: goal, robot links, ... (multi_object.py:562-663)
    actor_object0 = lay.get("actor_object0", 3)           # actors: goal, robot, table, objects
    out = []

    def posed(verts, pos, quat, sid):
        tri = hull_triangles(verts)
        out.append((tri @ rotation(quat).T + np.asarray(pos, np.float64), sid))

    for h in scene["link_hulls"]:
        assert h.get("owner", "link") == "link"
        r = body[body_robot0 + h["index"]]
        posed(h["verts"], r[0:3], r[3:7], 1)
    objects = scene["objects"]
    if pool_names is not None:
        byname = {o["name"]: o for o in objects}
        objects = [byname[n] for n in pool_names]
    for i, pid in enumerate(object_indices):
        o = objects[int(pid)]
        r = root[actor_object0 + i]
        for h in (o.get("hulls") or [o["hull"]]):
            posed(h["verts"], r[0:3], r[3:7], 3 + i)
    statics = ([dict(scene["table"], name="table")] if scene.get("table") else []) + list(scene.get("statics", []))
    for s in statics:
        posed(s["hull"]["verts"], s["pos"], s["quat"], 2 if s["name"].startswith("bin") else 0)
    return out


def cast(o, D, surfaces, goal, goal_radius, goal_id):
    """Closest front-face hit of rays o + t D (D (R, 3)): t (inf: none), id, cos between ray and face normal."""
    o = np.asarray(o, np.float64)
    R = len(D)
    dn = D / np.linalg.norm(D, axis=1, keepdims=True)
    best = np.full(R, np.inf)
    seg = np.zeros(R, np.int64)
    cos = np.zeros(R)
    down = D[:, 2] < 0                                      # ground plane z = 0, seen from above
    if o[2] > 0:
        best[down] = -o[2] / D[down, 2]
        cos[down] = -dn[down, 2]
    oc = o - np.asarray(goal, np.float64)                   # goal sphere, front hit only
    dd = (D * D).sum(1)
    b = D @ oc
    disc = b * b - dd * (oc @ oc - goal_radius ** 2)
    ok = disc >= 0
    t = np.where(ok, (-b - np.sqrt(np.where(ok, disc, 0))) / dd, np.inf)
    hit = ok & (t > 0) & (t < best)
    nrm = (oc + t[hit, None] * D[hit]) / goal_radius
    best[hit], seg[hit], cos[hit] = t[hit], goal_id, np.abs((nrm * dn[hit]).sum(1))
    for tri, sid in surfaces:
        pts = tri.reshape(-1, 3)
        c = 0.5 * (pts.min(0) + pts.max(0))                 # a bounding sphere of the world vertices prunes the rays
        r2 = ((pts - c) ** 2).sum(1).max() * (1 + 1e-9) + 1e-18
        w = c - o
        idx = np.nonzero(w @ w - (dn @ w) ** 2 <= r2)[0]
        if len(idx) == 0:
            continue
        d = D[idx]
        v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        n = np.cross(e1, e2)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        p = np.cross(d[:, None, :], e2[None])               # (r, T, 3)
        det = (p * e1).sum(-1)                              # = -d . (e1 x e2): > 0 on front faces
        t0 = o - v0                                         # (T, 3): the origin is shared by all rays
        q = np.cross(t0, e1)
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (p * t0).sum(-1) / det
            v = (d @ q.T) / det
            tt = (e2 * q).sum(-1)[None] / det
        eps = 1e-10                                         # closes the hairline between two triangles of a face
        inside = (det > 0) & (u >= -eps) & (v >= -eps) & (u + v <= 1 + eps) & (tt > 0)
        tt = np.where(inside, tt, np.inf)
        k = tt.argmin(1)
        th = tt[np.arange(len(idx)), k]
        take = th < best[idx]
        sel = idx[take]
        best[sel], seg[sel] = th[take], sid
        cos[sel] = np.abs((n[k[take]] * dn[sel]).sum(1))
    seg[~np.isfinite(best)] = 0
    return best, seg, cos


_RENDER_CACHE = {}


def render(scene, cam, root, body, object_indices, goal, n_obj, pool_names=None):
    """One env: t (H, W) (inf where nothing is hit), id (H, W), cos (H, W), stable (H, W) bool.
    cam: pos, quat, fovx (degrees), width, height, goal_radius."""
    key = hashlib.sha1(b"".join([np.ascontiguousarray(a).tobytes() for a in (root, body, object_indices, goal)])
                       + repr((sorted((k, str(v)) for k, v in cam.items()), n_obj, pool_names,
                               scene.get("generator"), len(scene.get("statics", [])))).encode()).hexdigest()
    if key in _RENDER_CACHE:                                # the GPU state is the C oracle's bit for bit
        return _RENDER_CACHE[key]
    W, H = cam["width"], cam["height"]
    row, col = np.divmod(np.arange(W * H), W)
    shifts = [(0, 0), (SHIFT, 0), (-SHIFT, 0), (0, SHIFT), (0, -SHIFT)]
    D = np.concatenate([view_directions(cam, col + dc, row + dr) for dc, dr in shifts])
    surf = scene_surfaces(scene, np.asarray(root, np.float64), np.asarray(body, np.float64), object_indices, pool_names)
    t, seg, cos = cast(cam["pos"], D, surf, goal, cam["goal_radius"], 3 + n_obj)
    seg5 = seg.reshape(5, H, W)
    stable = (seg5 == seg5[0]).all(0)
    out = (t[:W * H].reshape(H, W), seg5[0].copy(), cos[:W * H].reshape(H, W), stable)
    _RENDER_CACHE[key] = out
    return out


def check_images(tag, scene, cam, state, n_obj, depth, seg, pointcloud, show, pool_names=None):
    """Every assertion of a comparison against the reference. state: root (N, A, 13), body (N, B, 13),
    object_indices (N, NO), goal (N, 3); depth (N, H, W), seg (N, H, W), pointcloud (N, H, W, 4) or None: the images
    under test. show: the ids the case is built to show. Returns (worst stable share, max scaled depth error,
    max hit-point error / its tolerance)."""
    N = depth.shape[0]
    o = np.asarray(cam["pos"], np.float64)
    H, W = cam["height"], cam["width"]
    row, col = np.divmod(np.arange(W * H), W)
    D = view_directions(cam, col, row).reshape(H, W, 3)
    dlen = np.linalg.norm(D, axis=-1)
    worst_share, worst_depth, worst_point = 1.0, 0.0, 0.0
    for e in range(N):
        t, sid, cos, stable = render(scene, cam, state["root"][e], state["body"][e], state["object_indices"][e],
                                     state["goal"][e], n_obj, pool_names)
        share = stable.mean()
        worst_share = min(worst_share, share)
        assert share >= STABLE_SHARE, f"{tag} env {e}: stable share {share:.4f}"
        for s in show:
            cnt = int((stable & (sid == s)).sum())
            assert cnt >= MIN_PIXELS, f"{tag} env {e}: id {s} covers {cnt} stable pixels; the case must show it"
        bad = stable & (seg[e] != sid)
        assert not bad.any(), (f"{tag} env {e}: {int(bad.sum())} stable pixels differ in id, first (row, col) "
                               f"{np.argwhere(bad)[0]}: got {seg[e][bad][0]}, reference {sid[bad][0]}")
        hit = stable & np.isfinite(t)
        miss = stable & ~np.isfinite(t)
        assert np.all(np.isneginf(depth[e][miss])), f"{tag} env {e}: a stable no-hit pixel has a depth"
        assert np.isfinite(depth[e][hit]).all(), f"{tag} env {e}: a stable hit pixel has no depth"
        err = np.abs(-depth[e][hit].astype(np.float64) - t[hit]) * cos[hit] / (1 + t[hit])
        if err.size:
            worst_depth = max(worst_depth, float(err.max()))
        if pointcloud is not None:
            near = hit & (t < MAX_DEPTH * (1 - 1e-6))        # deeper hits are clamped to max_depth by the reference
            want = o + t[near][:, None] * D[near]
            got = pointcloud[e][near][:, 0:3].astype(np.float64)
            tol = 2e-6 + dlen[near] * DEPTH_BOUND * (1 + t[near]) / cos[near]
            ratio = np.linalg.norm(got - want, axis=1) / tol
            if ratio.size:
                worst_point = max(worst_point, float(ratio.max()))
    print(f"{tag}: stable share >= {worst_share:.4f}, max |t - t_ref| cos / (1 + t_ref) = {worst_depth:.3e} "
          f"({worst_depth / 2.0 ** -23:.2f} ulp; bound {DEPTH_BOUND:.3e}), max hit-point error / tolerance = "
          f"{worst_point:.3f}")
    assert worst_depth <= DEPTH_BOUND, f"{tag}: depth error {worst_depth:.3e} > {DEPTH_BOUND:.3e}"
    assert worst_point <= 1.0, f"{tag}: hit point off by {worst_point:.3f} x its tolerance"
    return worst_share, worst_depth, worst_point


# ----------------------------------------------------------------------------- the cases (CPU and GPU tests)
TOPVIEW = dict(pos=[0.28, 1.05, 0.9], quat=[0.213, 0.213, -0.674, 0.674], fovx=87.0)
S45 = math.sqrt(0.5)
HEAVY = [13, 16, 17, 18, 19, 20, 21, 22, 23]              # the pool's compound objects: 9 and 8 convex pieces


SIDE_BY_SIDE = [(None, 0.48), (None, 0.60), (None, 0.72)]   # y only, 12 cm apart: seen along x, none hides another


def _cases():
    obj3, obj8 = [3, 4, 5], list(range(3, 11))
    return {
        # name: scene kind, envs, fill seed, camera, (W, H), the ids it is built to show, extras
        "default_topview": dict(kind="default", N=3, seed=3, cam=TOPVIEW, res=(64, 36), show=[0, 1] + obj3),
        "bin_topview": dict(kind="bin", N=2, seed=3, cam=TOPVIEW, res=(64, 36), show=[0, 1, 2] + obj8),
        # every env holds three compound objects (pool entries 13 and 16-23), placed by hand
        "compound_objects": dict(kind="default", N=3, seed=5, cam=TOPVIEW, res=(64, 36), show=[0, 1] + obj3,
                                 object_indices=[HEAVY[0:3], HEAVY[3:6], HEAVY[6:9]]),
        # looking straight down (+X -> -Z): the pixel column col = W/2 has d.y == 0 exactly, so den == 0 against the
        # axis-aligned table box's +-y planes
        "straight_down": dict(kind="default", N=2, seed=6, cam=dict(pos=[0.28, 0.7, 1.0], quat=[0, S45, 0, S45], fovx=87.0),
                              res=(48, 27), show=[0, 1] + obj3, place=[(0.1, 0.8), (0.3, 0.8), (0.5, 0.8)]),
        # at object height, looking along +x and along -x from between the objects: hulls behind the camera, and the
        # horizon row (d.z == 0 exactly at row H/2) and the rows above it with no hit
        "horizontal_plus_x": dict(kind="default", N=2, seed=7, cam=dict(pos=[0.17, 0.6, 0.58], quat=[0, 0, 0, 1], fovx=87.0),
                                  res=(64, 36), show=[0, 4, 5], place=SIDE_BY_SIDE),
        "horizontal_minus_x": dict(kind="default", N=2, seed=7, cam=dict(pos=[0.34, 0.6, 0.58], quat=[0, 0, 1, 0], fovx=87.0),
                                   res=(64, 36), show=[0, 3, 4], place=SIDE_BY_SIDE),
        # inside the table box, looking up through its top: the table is not seen (t0 > 0), what stands on it is
        "inside_table": dict(kind="default", N=2, seed=8, cam=dict(pos=[0.25, 0.6, 0.3], quat=[0, -S45, 0, S45], fovx=87.0),
                             res=(64, 36), show=[1] + obj3, place=[(0.2, 0.47), (0.3, 0.6), (0.22, 0.73)]),
        # 2 tan(85 deg) / 64 = 0.36 per pixel, 20 degrees at the image centre: the camera 10-20 cm from the pool's larger
        # objects (mustard bottle, sugar box, pudding box), two of them off to the sides where a pixel is 2-3 degrees
        "fovx_170": dict(kind="default", N=2, seed=9, cam=dict(TOPVIEW, fovx=170.0, pos=[0.26, 0.753, 0.616]), res=(64, 36),
                         show=[0, 1] + obj3, place=[(0.10, 0.70), (0.42, 0.70), (0.26, 0.66)],
                         object_indices=[[2, 3, 5], [3, 5, 2]]),
        "goal_in_view": dict(kind="default", N=2, seed=10, cam=TOPVIEW, res=(64, 36), show=[0, 1, 6] + obj3,
                             goal=[0.28, 0.9, 0.84]),
        # fewer than 256 pixels, odd sizes; 0.98 of 91 pixels leaves one silhouette pixel, so the objects stay small
        "image_13x7": dict(kind="default", N=2, seed=11, cam=dict(TOPVIEW, pos=[0.28, 0.85, 0.75]), res=(13, 7), show=[0, 1]),
        # a pixel count that is no multiple of the 256-pixel tile, odd sizes
        "image_51x29": dict(kind="default", N=2, seed=12, cam=TOPVIEW, res=(51, 29), show=[0, 1] + obj3),
    }


CASES = _cases()
SIM_CALLS = 30                                              # 0.5 s: the objects dropped onto the table / into the bin


def case_scene(case):
    from handarm_hip import model as HM
    return HM.load_scene(HM.BIN_ASSET if case["kind"] == "bin" else HM.ASSET)


def case_camera(case, scene):
    W, H = case["res"]
    return dict(case["cam"], width=W, height=H, goal_radius=scene.get("goal_radius", 0.02))


def fill_case(case, st, scene):
    """The case's start state in the HostState st (before the 0.5 s of simulation)."""
    from tests import scenes
    N = case["N"]
    if case["kind"] == "bin":
        scenes.fill_bin_scene(st, N, scene, seed=case["seed"])
    else:
        scenes.fill_scene(st, N, seed=case["seed"])
    if "object_indices" in case:
        st["object_indices"][:] = np.asarray(case["object_indices"])
    rs = st["root_state"].reshape(N, -1, 13)
    for i, (x, y) in enumerate(case.get("place", [])):      # objects placed by hand: (x, y), None keeps the seeded one
        if x is not None:
            rs[:, 3 + i, 0] = x
        rs[:, 3 + i, 1] = y
    st["goal_pos"][:] = case.get("goal", [0.28, 0.58, 0.8])
    return st


# ----------------------------------------------------------------------------- asset checks
def hull_records(scene):
    """(label, record) of every hull record of a scene: link hulls, object hulls and pieces, statics' boxes."""
    for k, h in enumerate(scene.get("link_hulls", [])):
        yield f"link_hull {k}", h
    for o in scene.get("objects", []):
        if "hull" in o:
            yield f"object {o['name']}", o["hull"]
        for j, h in enumerate(o.get("hulls") or []):
            yield f"object {o['name']} piece {j}", h
    for s in ([scene["table"]] if scene.get("table") else []) + list(scene.get("statics", [])):
        yield f"static {s.get('name', 'table')}", s["hull"]
    for name, g in (scene.get("posed_statics") or {}).items():
        for j, s in enumerate(g["pieces"]):
            yield f"posed static {name} {j}", s["hull"]


def record_errors(h):
    """(max | |n| - 1 |, max |max_v (n.v + d)|, max over vertices of |v - center| - radius) of a hull record."""
    v = np.asarray(h["verts"], np.float64)
    p = np.asarray(h["planes"], np.float64)
    support = (v @ p[:, :3].T + p[:, 3]).max(0)             # the farthest vertex lies on each plane
    out = np.linalg.norm(v - np.asarray(h["center"], np.float64), axis=1).max() - float(h["radius"])
    return float(np.abs(np.linalg.norm(p[:, :3], axis=1) - 1).max()), float(np.abs(support).max()), float(out)
