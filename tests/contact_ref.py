"""Independent float64 checker of contact rows: numpy only, from the scene's hull records and the host
state's poses. It shares no code with the narrow phase (csrc/ha_collide.h, oracle/physics_oracle.c): it never finds a
contact itself, it tests the rows it is given (Oracle.contacts on the CPU, the contact tensor on the GPU) against
properties any correct narrow phase has.

Rows: x[3], n[3] (from body b to body a), sep, a, b (first nine floats of a contact tensor row). Only rows between
objects and objects or statics are checked; rows with a robot link (code >= 100) are skipped (they are pinned by bit
identity between kernel and oracle, not by this checker). The scenes here have no object near the ground plane, so a
static code (-1) means the scene's static boxes.

Notation: d(n) = min_{v in A} n.v - max_{v in B} n.v, the gap of the two bodies along n; f_H(p) = max_k (n_k.p + d_k) over
the world planes of hull H (<= 0 inside), the minimum over the pieces for a compound object.

  (a) |n| = 1
  (b) no point is deeper than the bodies' overlap along its own normal: sep >= d(n) - tol
  (c) the surface points x + n sep / 2 (on a) and x - n sep / 2 (on b) are not inside their own hulls: f >= -tol; and
      (box scenes) not further outside than the contact margin
  (d) per pair, s* the brute-force SAT separation: s* < margin - 1e-4 gives at least one row, s* > margin + 1e-4 none
  (e) axis quality: the best d(n) of a pair's rows >= min(s*, (s* - edge_abs_tol) / edge_rel_tol) - 1e-6, what the
      narrow phase's preference for face axes allows
"""
import numpy as np

from handarm_hip import model as HM
from tests.test_edge_contacts import separation


def _rot(q):
    x, y, z, w = (float(t) for t in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


class Piece:
    """One convex hull record in its body frame: vertices, planes (n, d) with n.x + d <= 0 inside, edge directions."""

    def __init__(self, hull, edges=True):
        self.v = np.asarray(hull["verts"], np.float64)
        pl = np.asarray(hull["planes"], np.float64)
        self.n, self.d = pl[:, :3], pl[:, 3]
        self.e = None
        if edges:
            ed, _ = HM.hull_topology(hull["verts"], hull["planes"])
            self.e = np.array([self.v[b] - self.v[a] for a, b, _, _ in ed])

    def world(self, pose):
        """(vertices, plane normals, plane offsets, edge directions) at pose (p[3], q[4] xyzw)."""
        R, t = _rot(pose[3:7]), np.asarray(pose[0:3], np.float64)
        v = self.v @ R.T + t
        n = self.n @ R.T
        return v, n, self.d - n @ t, None if self.e is None else self.e @ R.T


class Body:
    """A rigid body at a pose: its convex pieces in the env frame."""

    def __init__(self, pieces, pose):
        self.w = [p.world(pose) for p in pieces]
        self.verts = np.concatenate([w[0] for w in self.w])

    def f(self, p):
        return min(float((w[1] @ p + w[2]).max()) for w in self.w)

    def sat_input(self):
        assert len(self.w) == 1, "the brute-force SAT is for one-piece bodies"
        v, n, _, e = self.w[0]
        return v, n, e


def gap(A, B, n):
    return float((A.verts @ n).min() - (B.verts @ n).max())


class SceneRef:
    """The scene's object pool and static boxes as Pieces. edges: build the edge lists the SAT of (d) / (e) needs."""

    def __init__(self, scene, edges=True):
        self.pool = [[Piece(h, edges) for h in (o.get("hulls") or [o["hull"]])] for o in scene["objects"]]
        statics = ([scene["table"]] if scene.get("table") else []) + list(scene.get("statics", []))
        self.statics = [Body([Piece(s["hull"], edges)], list(s["pos"]) + list(s["quat"])) for s in statics]

    def objects(self, st, model, env):
        n = st.num_envs
        rs = np.asarray(st["root_state"], np.float64).reshape(n, model.n_actors, 13)
        ids = np.asarray(st["object_indices"]).reshape(n, -1)
        return [Body(self.pool[int(ids[env, o])], rs[env, model.actor_object0 + o, 0:7]) for o in range(ids.shape[1])]


class Report:
    """Extremes over everything checked (so a test prints each figure before it asserts)."""

    def __init__(self):
        self.rows = 0
        self.norm = 0.0                     # (a) worst | |n| - 1 |
        self.depth = np.inf                 # (b) worst sep - d(n)
        self.inside = np.inf                # (c) worst f of a surface point on its own hull (lower)
        self.outside = -np.inf              # (c) largest f (upper)
        self.pairs = self.misses = self.spurious = 0    # (d)
        self.axis_pairs = self.axis_fail = 0            # (e)
        self.axis_worst = np.inf

    def __str__(self):
        return (f"{self.rows} rows: | |n| - 1 | {self.norm:.2e}, sep - d(n) {self.depth:.2e}, f lower {self.inside:.2e} "
                f"upper {self.outside:.5f}; {self.pairs} pairs, {self.misses} misses, {self.spurious} spurious; "
                f"axis quality {self.axis_fail} of {self.axis_pairs} fail, worst {self.axis_worst:.2e}")


def check_env(ref, model, params, st, env, rows, rep, pairs=True):
    """Add env's object rows (and, with `pairs`, its object-object and object-static pairs) to the report."""
    rows = np.asarray(rows, np.float64).reshape(-1, rows.shape[-1])[:, :9]
    objs = ref.objects(st, model, env)
    margin = float(params.contact_margin)
    best = {}

    def static_of(p):       # the static whose surface the point lies nearest to
        return min(range(len(ref.statics)), key=lambda k: abs(ref.statics[k].f(p)))

    for r in rows:
        a, b = int(r[7]), int(r[8])
        if a >= 100 or b >= 100:
            continue
        x, n, sep = r[0:3], r[3:6], float(r[6])
        pa, pb = x + n * (0.5 * sep), x - n * (0.5 * sep)
        ka = ("s", static_of(pa)) if a < 0 else ("o", a)
        kb = ("s", static_of(pb)) if b < 0 else ("o", b)
        A = ref.statics[ka[1]] if a < 0 else objs[a]
        B = ref.statics[kb[1]] if b < 0 else objs[b]
        rep.rows += 1
        rep.norm = max(rep.norm, abs(float(np.linalg.norm(n)) - 1.0))
        d = gap(A, B, n)
        rep.depth = min(rep.depth, sep - d)
        fa, fb = A.f(pa), B.f(pb)
        rep.inside = min(rep.inside, fa, fb)
        rep.outside = max(rep.outside, fa, fb)
        # the pair in a fixed orientation (first key, second key), the gap taken from the second to the first
        key, dn = ((ka, kb), d) if ka <= kb else ((kb, ka), gap(B, A, -n))
        best[key] = max(best.get(key, -np.inf), dn)
    if not pairs:
        return
    bodies = [(("o", o), objs[o]) for o in range(len(objs))] + [(("s", k), s) for k, s in enumerate(ref.statics)]
    for i, (ki, Bi) in enumerate(bodies):
        for kj, Bj in bodies[i + 1:]:
            if ki[0] == "s":
                continue                    # static-static
            s = separation(Bi.sat_input(), Bj.sat_input())
            key = (ki, kj) if ki <= kj else (kj, ki)
            rep.pairs += 1
            if s < margin - 1e-4 and key not in best:
                rep.misses += 1
            if s > margin + 1e-4 and key in best:
                rep.spurious += 1
            if key in best:
                rep.axis_pairs += 1
                q = best[key] - min(s, (s - float(params.edge_abs_tol)) / float(params.edge_rel_tol))
                rep.axis_worst = min(rep.axis_worst, q)
                rep.axis_fail += q < -1e-6


def assert_report(rep, margin=None, pairs=True):
    """The bounds of DESIGN.md §4. margin: the contact margin for (c)'s upper bound (box scenes), None: not asserted."""
    assert rep.rows > 0
    assert rep.norm <= 1e-6, f"(a) | |n| - 1 | {rep.norm:.2e}"
    assert rep.depth >= -1e-6, f"(b) a point {-rep.depth:.2e} m deeper than the bodies overlap along its normal"
    assert rep.inside >= -1e-6, f"(c) a surface point {-rep.inside:.2e} m inside its own hull"
    if margin is not None:
        assert rep.outside <= margin + 1e-6, f"(c) a surface point {rep.outside:.5f} m outside its own hull"
    if pairs:
        assert rep.misses == 0 and rep.spurious == 0, f"(d) {rep.misses} pairs missed, {rep.spurious} spurious"
        assert rep.axis_fail <= 0.005 * rep.axis_pairs, f"(e) {rep.axis_fail} of {rep.axis_pairs} pairs"
        assert rep.axis_worst >= -2e-4, f"(e) worst {rep.axis_worst:.2e}"


# ----------------------------------------------------------------------------- the fixed scenes
BOX_SEEDS = (1, 2, 3)
YCB_CASES = ((13, 0.0), (5, 0.3))


def box_pile_state(st, n, seed):
    """Three boxes thrown together above the table (seeds 1, 2) or at its far edge (seed 3)."""
    from tests import scenes
    scenes.fill_box_scene(st, n, "overhang")
    rng = np.random.default_rng(seed)
    cx = scenes.TABLE_X1 - 0.02 if seed == 3 else 0.35
    c = np.array([cx, 0.8, scenes.TABLE_TOP + 0.03])
    rs = st["root_state"].reshape(n, 6, 13)
    for o in range(3):
        rs[:, 3 + o, 0:3] = c + rng.uniform([-0.04, -0.04, -0.012], [0.04, 0.04, 0.05], (n, 3))
        rs[:, 3 + o, 3:7] = scenes.rand_quat(rng, (n,))
    return st


def ycb_pile_state(st, n, seed, near_hand):
    from tests import scenes
    scenes.fill_scene(st, n, seed, near_hand)
    rng = np.random.default_rng(seed)
    rs = st["root_state"].reshape(n, 6, 13)
    for o in range(3):
        rs[:, 3 + o, 0:3] = np.array([0.3, 0.6, 0.56]) + rng.uniform([-0.05, -0.05, -0.02], [0.05, 0.05, 0.06], (n, 3))
    return st
