"""Independent float64 checker of contact rows: numpy only, from the scene's hull records and the host
state's poses. It shares no code with the narrow phase (csrc/ha_collide.h, oracle/physics_oracle.c): it never finds a
contact itself, it tests the rows it is given (Oracle.contacts on the CPU, the contact tensor on the GPU) against
properties any correct narrow phase has.

Rows: x[3], n[3] (from body b to body a), sep, a, b (first nine floats of a contact tensor row). A robot link (code 100
+ link) is a body of several pieces like a compound object: the scene's link_hulls of that link, posed by the
independent float64 FK of tests/kinematics.py (Chain.fk at the state's q, from the robot's base pose). Link-object,
link-static and link-link rows get (a), (b) and the lower bound of (c) at the same 1e-6 as the object rows (LINK_TOL):
the link poses come from float64 FK while the rows were built on float32 FK, and the measured extremes (-4.7e-7 at
worst) leave no need for a wider margin. A row that names
a link without a hull, a link-link row in a scene without self-collision, and a link pair the self-collision filter
removes (the same link, parent and child, the scene's exclude list) are counted and fail the check. A link's pieces
overlap (the Ur5Sih palm's five hulls, the Allegro fingertips' two), and a point on one piece's surface may lie inside
its neighbour, so for link rows (c) asks that some piece holds the row by itself (Body.own_piece_f): the point not
inside that piece and the row no deeper than that piece's overlap with the other body along n. With one piece this is
(c) as above; the points found inside a neighbouring piece are counted and printed. AllegroKuka's
cuboid is scaled per env by the state's object_scale. The scenes here have no object near the ground plane, so a
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
from tests.kinematics import Chain
from tests.test_edge_contacts import separation

LINK_TOL = 1e-6


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

    def scaled(self, sc):
        """The piece scaled per axis (no edge list): vertices v s, planes n / s renormalised."""
        o = Piece.__new__(Piece)
        sc = np.asarray(sc, np.float64)
        o.v, o.e = self.v * sc, None
        n = self.n / sc
        ln = np.linalg.norm(n, axis=1)
        o.n, o.d = n / ln[:, None], self.d / ln
        return o

    def world(self, pose, R=None):
        """(vertices, plane normals, plane offsets, edge directions) at pose (p[3], q[4] xyzw), or at (p[3], R)."""
        R, t = _rot(pose[3:7]) if R is None else R, np.asarray(pose[0:3], np.float64)
        v = self.v @ R.T + t
        n = self.n @ R.T
        return v, n, self.d - n @ t, None if self.e is None else self.e @ R.T


class Body:
    """A rigid body at a pose: its convex pieces in the env frame."""

    def __init__(self, pieces, pose, R=None):
        self.w = [p.world(pose, R) for p in pieces]
        self.verts = np.concatenate([w[0] for w in self.w])

    def f(self, p):
        return min(float((w[1] @ p + w[2]).max()) for w in self.w)

    def own_piece_f(self, p, other, n, sep, sign):
        """(c) for a body whose pieces may overlap (a link's hulls do): a row is made by one piece, and a point on that
        piece's surface may lie inside a neighbouring piece, so min over the pieces is no property of a correct narrow
        phase. Some piece k must hold the row by itself: the point not inside it, f_k(p), and the row no deeper than
        that piece and the other body overlap along n, sep - d_k(n). Returns the best piece's min of the two (one
        piece: f(p) when (b) holds). sign +1: this body is side a."""
        best = -np.inf
        for v, pn, pd, _ in self.w:
            d = (v @ n).min() - (other.verts @ n).max() if sign > 0 else (other.verts @ n).min() - (v @ n).max()
            best = max(best, min(float((pn @ p + pd).max()), sep - float(d)))
        return best

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
        self.chain = Chain(scene)
        self.link_pieces = {}
        for h in scene.get("link_hulls", []):
            self.link_pieces.setdefault(int(h["index"]), []).append(Piece(h, edges=False))
        sc = scene.get("self_collision")
        self.self_collision = sc is not None
        self.excluded = {tuple(sorted(int(i) for i in pr)) for pr in (sc or {}).get("exclude", [])}

    def objects(self, st, model, env):
        n = st.num_envs
        rs = np.asarray(st["root_state"], np.float64).reshape(n, model.n_actors, 13)
        ids = np.asarray(st["object_indices"]).reshape(n, -1)
        pool = [self.pool[int(ids[env, o])] for o in range(ids.shape[1])]
        if "object_scale" not in st.null:
            sc = np.asarray(st["object_scale"], np.float64).reshape(n, -1, 3)
            pool = [[p.scaled(sc[env, o]) for p in pieces] for o, pieces in enumerate(pool)]
        return [Body(pool[o], rs[env, model.actor_object0 + o, 0:7]) for o in range(ids.shape[1])]

    def links(self, st, env):
        """{link: Body} of the links that have hulls, at the state's joint positions."""
        q = np.asarray(st["dof_state"], np.float64).reshape(st.num_envs, self.chain.D, 2)[env, :, 0]
        R, p, _, _ = self.chain.fk(q)
        return {k: Body(pc, p[k], R[k]) for k, pc in self.link_pieces.items()}

    def link_pair_filtered(self, la, lb):
        """Whether the self-collision filter removes the pair (so no row may name it)."""
        pa, pb = self.chain.links[la]["parent"], self.chain.links[lb]["parent"]
        return (not self.self_collision or la == lb or pa == lb or pb == la
                or (min(la, lb), max(la, lb)) in self.excluded)


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
        # rows with a robot link: counts, their own (a), (b), (c) extremes, and what must not appear at all
        self.link_rows = self.link_link = self.no_hull = self.filtered = self.link_in_neighbour = 0
        self.link_norm, self.link_depth, self.link_inside = 0.0, np.inf, np.inf

    def __str__(self):
        out = (f"{self.rows} rows: | |n| - 1 | {self.norm:.2e}, sep - d(n) {self.depth:.2e}, f lower {self.inside:.2e} "
               f"upper {self.outside:.5f}; {self.pairs} pairs, {self.misses} misses, {self.spurious} spurious; "
               f"axis quality {self.axis_fail} of {self.axis_pairs} fail, worst {self.axis_worst:.2e}")
        if self.link_rows or self.no_hull or self.filtered:
            out += (f"; {self.link_rows} link rows ({self.link_link} link-link): | |n| - 1 | {self.link_norm:.2e}, sep - "
                    f"d(n) {self.link_depth:.2e}, f lower {self.link_inside:.2e} ({self.link_in_neighbour} points inside a "
                    f"neighbouring piece of their link); {self.no_hull} without a hull, {self.filtered} of filtered pairs")
        return out


def check_env(ref, model, params, st, env, rows, rep, pairs=True):
    """Add env's rows (and, with `pairs`, its object-object and object-static pairs) to the report."""
    rows = np.asarray(rows, np.float64).reshape(-1, rows.shape[-1])[:, :9]
    objs = ref.objects(st, model, env)
    margin = float(params.contact_margin)
    best = {}

    def static_of(p):       # the static whose surface the point lies nearest to
        return min(range(len(ref.statics)), key=lambda k: abs(ref.statics[k].f(p)))

    links = ref.links(st, env) if len(rows) and (rows[:, 7:9] >= 100).any() else {}
    for r in rows:
        a, b = int(r[7]), int(r[8])
        x, n, sep = r[0:3], r[3:6], float(r[6])
        pa, pb = x + n * (0.5 * sep), x - n * (0.5 * sep)
        if a >= 100 or b >= 100:
            if any(c >= 100 and c - 100 not in links for c in (a, b)):
                rep.no_hull += 1
                continue
            if a >= 100 and b >= 100 and ref.link_pair_filtered(a - 100, b - 100):
                rep.filtered += 1
                continue
            A = links[a - 100] if a >= 100 else (ref.statics[static_of(pa)] if a < 0 else objs[a])
            B = links[b - 100] if b >= 100 else (ref.statics[static_of(pb)] if b < 0 else objs[b])
            rep.link_rows += 1
            rep.link_link += a >= 100 and b >= 100
            rep.link_norm = max(rep.link_norm, abs(float(np.linalg.norm(n)) - 1.0))
            rep.link_depth = min(rep.link_depth, sep - gap(A, B, n))
            fa, fb = A.own_piece_f(pa, B, n, sep, 1.0), B.own_piece_f(pb, A, n, sep, -1.0)
            rep.link_inside = min(rep.link_inside, fa, fb)
            rep.link_in_neighbour += (A.f(pa) < -LINK_TOL <= fa) + (B.f(pb) < -LINK_TOL <= fb)
            continue
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


def assert_report(rep, margin=None, pairs=True, object_rows=True):
    """The bounds of DESIGN.md §4. margin: the contact margin for (c)'s upper bound (box scenes), None: not asserted.
    object_rows False: a scene of link rows only (check_link_scene asserts its own floors)."""
    if object_rows:
        assert rep.rows > 0
    assert rep.no_hull == 0, f"{rep.no_hull} rows name a link without a hull"
    assert rep.filtered == 0, f"{rep.filtered} rows between links the self-collision filter removes"
    if rep.link_rows:
        assert rep.link_norm <= 1e-6, f"(a) link rows: | |n| - 1 | {rep.link_norm:.2e}"
        assert rep.link_depth >= -LINK_TOL, f"(b) a link row {-rep.link_depth:.2e} m deeper than the bodies overlap"
        assert rep.link_inside >= -LINK_TOL, f"(c) a link row's surface point {-rep.link_inside:.2e} m inside its hull"
    if not rep.rows:
        return
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


# ----------------------------------------------------------------------------- scenes with robot-link rows
# Host states only (no GPU): tests/test_contact_checker.py runs the checker on the oracle's rows of these states,
# tests/test_gpu_contact_tensor.py pushes the same states to a sim. Each returns (scene, model, params, state).
def ur5sih_hand_pile(n=64):
    """The pile-in-hand state of tests/test_gpu_overflow.py (seed 13): the three objects dropped together into the
    closed hand just above the table."""
    from oracle.oracle_lib import HostState, Oracle
    from tests import scenes
    scene = HM.load_scene()
    m = HM.build_model(scene)
    p, _ = HM.build_params()
    st = HostState(n)
    scenes.fill_scene(st, n, seed=13, near_hand=0.0)
    probe = st.copy()
    Oracle(m, p, n).simulate(probe, 1)
    body = probe["rigid_body_state"].reshape(n, 34, 13)
    rng = np.random.default_rng(13)
    hull_links = sorted({int(m.hull_link[k]) for k in range(m.n_link_hulls)})
    rs = st["root_state"].reshape(n, 6, 13)
    for o in range(3):
        lk = np.array(hull_links)[rng.integers(len(hull_links) // 2, len(hull_links), n)]
        rs[:, 3 + o, 0:3] = body[np.arange(n), m.body_robot0 + lk, 0:3] + rng.uniform(-0.015, 0.015, (n, 3))
        rs[:, 3 + o, 7:13] = 0.0
    return scene, m, p, st


def allegro_closing_hand(n=128):
    """AllegroHand: the cube on the palm, every finger target at its upper limit."""
    from oracle.oracle_lib import HostState
    from tests import scenes
    scene = HM.load_scene(HM.ALLEGRO_ASSET)
    m = HM.build_model(scene)
    p, _ = HM.build_params(task=HM.TASK_ALLEGRO_HAND)
    lo = np.array(m.dof_lower[:16], np.float32)
    up = np.array(m.dof_upper[:16], np.float32)
    st = HostState(n, model=m, params=p)
    scenes.fill_allegro_scene(st, n, lo, up, seed=0)
    st["sim_targets"][:] = up
    return scene, m, p, st


def kuka_closed_hand(n=128):
    """AllegroKuka: the half-closed hand around the cuboid in its palm (tests/scenes.py kuka_closed_hand_scene), per-env cuboid dimensions: link-object, link-link (self-collision) and link-table rows."""
    import types
    from oracle.oracle_lib import HostState
    from tests.scenes import kuka_closed_hand_scene
    scene = HM.load_scene(HM.KUKA_ASSET)
    m = HM.build_model(scene)
    p, c = HM.build_params(task=HM.TASK_ALLEGRO_KUKA)
    lo = np.array(m.dof_lower[:23], np.float32)
    up = np.array(m.dof_upper[:23], np.float32)
    st = HostState(n, model=m, params=p)
    st["object_scale"][:] = HM.kuka_env_tables(n, scene, c)[0]
    kuka_closed_hand_scene(types.SimpleNamespace(num_envs=n, params=p, model=m), st, lo, up)
    st["contact_stats"][:] = 0
    return scene, m, p, st


LINK_SCENES = {"ur5sih_hand_pile": (ur5sih_hand_pile, 64), "allegro_closing_hand": (allegro_closing_hand, 128),
               "kuka_closed_hand": (kuka_closed_hand, 64)}
# floors of what a scene must offer the checker: link rows, and link-link rows in the two hand scenes
LINK_ROWS_FLOOR, LINK_LINK_FLOOR = 200, {"ur5sih_hand_pile": 0, "allegro_closing_hand": 50, "kuka_closed_hand": 50}


def check_link_scene(name, scene, model, params, st, rows_of, tag=""):
    """Run the checker over every env's rows (rows_of(env) -> (k, >= 9) array) of the LINK_SCENES state `name`; returns
    the report after asserting the floors and the bounds. tag: what the printed line adds to the name."""
    ref = SceneRef(scene, edges=False)
    rep = Report()
    for e in range(st.num_envs):
        check_env(ref, model, params, st, e, rows_of(e), rep, pairs=False)
    print(f"{name}{tag}: {rep}")
    assert rep.link_rows >= LINK_ROWS_FLOOR, f"{name}: only {rep.link_rows} link rows"
    assert rep.link_link >= LINK_LINK_FLOOR[name], f"{name}: only {rep.link_link} link-link rows"
    assert_report(rep, margin=None, pairs=False, object_rows=rep.rows > 0)
    return rep
