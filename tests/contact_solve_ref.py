"""One substep of free rigid bodies with contacts in float64 numpy: the reference the contact *solve* is
held to. It shares no code with csrc/ha_solve.h or oracle/physics_oracle.c and reads masses, inertias and COMs from the
scene JSON, never from ha_model_t. The model is the one DESIGN.md §3.3 documents:

* a root-state row carries the body origin's pose and the COM's linear velocity; the COM is c = p + R com;
* free velocity v + h g + h f / m and w / (1 + h c_ang) + h I_w^-1 tau with I_w = R I R^T, no gyroscopic term;
* per contact row (x, n from body b to body a, sep, a, b) the normal constraint n.(v_a(x) - v_b(x)) >= vt with
  v_k(x) = v_k + w_k x (x - c_k), statics immovable; vt = -sep / h for sep > 0, otherwise
  -beta min(sep + slop, 0) / h, capped at max_depen_vel; impulses lambda >= 0;
* symplectic Euler: c += h v, q += h/2 (w, 0) (x) q, then normalised.

Without friction this is the strictly convex QP  min 1/2 (v - v_free)^T M (v - v_free)  s.t.  J v >= vt,  whose velocity
solution is unique even where the impulses are not. solve_qp() solves it as a least-distance problem with the
Lawson-Hanson active-set method and returns its own KKT residual (primal feasibility, lambda >= 0, complementarity,
stationarity), so a test can assert the reference before it uses it. The articulation enters the same QP through
`extra` (a mass block, its free velocity and the Jacobian columns of its coordinates; tests/test_contact_solve.py).
"""
import numpy as np

EPS32 = 2.0 ** -23


def rot(q):
    x, y, z, w = (float(t) for t in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def world_inertia(inertia, quat):
    """R I R^T of a body-frame inertia (3 x 3 about the COM) at orientation quat (xyzw)."""
    R = rot(np.asarray(quat, np.float64) / np.linalg.norm(quat))
    return R @ np.asarray(inertia, np.float64).reshape(3, 3) @ R.T


def pool_bodies(scene):
    """(mass, com[3], inertia[3, 3]) of every object of the scene's pool, from the JSON."""
    return [(float(o["mass"]), np.asarray(o["com"], np.float64), np.asarray(o["inertia"], np.float64).reshape(3, 3))
            for o in scene["objects"]]


def scaled_cuboid(scene, scale):
    """AllegroKuka's cuboid at per-axis `scale`: the analytic box, m' = rho a b c and I' = m'/12 (b^2 + c^2) ... from the
    scaled edge lengths, rho from the base cube's mass and volume. Returns (mass, com, inertia)."""
    o = scene["objects"][0]
    v = np.asarray(o["hull"]["verts"], np.float64)
    base = v.max(0) - v.min(0)
    rho = float(o["mass"]) / float(np.prod(base))
    a, b, c = base * np.asarray(scale, np.float64)
    m = rho * a * b * c
    return m, np.zeros(3), np.diag([m / 12 * (b * b + c * c), m / 12 * (a * a + c * c), m / 12 * (a * a + b * b)])


def nnls(E, f, tol=1e-15):
    """Lawson-Hanson: min |E y - f| over y >= 0 (active set, least squares on the passive columns)."""
    m = E.shape[1]
    P = np.zeros(m, bool)
    y = np.zeros(m)
    w = E.T @ f
    scale = max(np.abs(E).max(), 1.0) * max(np.abs(f).max(), 1.0)
    for _ in range(6 * m + 10):
        if P.all() or w[~P].max() <= tol * scale:
            break
        j = int(np.argmax(np.where(P, -np.inf, w)))
        P[j] = True
        while True:
            s = np.zeros(m)
            s[P] = np.linalg.lstsq(E[:, P], f, rcond=None)[0]
            if s[P].min() > 0:
                break
            bad = P & (s <= 0)
            alpha = float((y[bad] / (y[bad] - s[bad])).min())
            y = y + alpha * (s - y)
            P &= y > 1e-300
            y[~P] = 0.0
        y = s
        w = E.T @ (f - E @ y)
    return y


def solve_qp(M, v_free, J, vt):
    """min 1/2 (v - v_free)^T M (v - v_free) s.t. J v >= vt. Returns (v, lambda, KKT residual); the residual is inf
    where the constraints are infeasible."""
    v_free = np.asarray(v_free, np.float64)
    if len(J) == 0:
        return v_free.copy(), np.zeros(0), 0.0
    L = np.linalg.cholesky(M)
    G = np.linalg.solve(L, J.T).T               # J L^-T: constraints G u >= hh in u = L^T (v - v_free)
    hh = vt - J @ v_free
    E = np.vstack([G.T, hh[None, :]])
    f = np.zeros(E.shape[0])
    f[-1] = 1.0
    y = nnls(E, f)
    r = E @ y - f
    if -r[-1] < 1e-12:
        return v_free.copy(), np.zeros(len(J)), np.inf
    lam = y / -r[-1]
    v = v_free + np.linalg.solve(M, J.T @ lam)
    g = J @ v - vt
    kkt = max(float(np.maximum(-g, 0).max()), float(np.maximum(-lam, 0).max()), float(np.abs(lam * g).max()),
              float(np.abs(M @ (v - v_free) - J.T @ lam).max()))
    return v, lam, kkt


def normal_target(sep, h, prm):
    """The normal row's target velocity (speculative, Baumgarte beyond the slop, depenetration cap)."""
    sep = np.asarray(sep, np.float64)
    vt = np.where(sep > 0, -sep / h, -prm["baumgarte"] * np.minimum(sep + prm["contact_slop"], 0.0) / h)
    return np.minimum(vt, prm["max_depen_vel"])


def params_dict(p):
    """The physics parameters of an ha_params_t as python floats (the inputs of the step, not model data)."""
    return dict(h=float(p.dt) / int(p.substeps), gravity=np.array([float(g) for g in p.gravity]),
                friction=float(p.friction), baumgarte=float(p.baumgarte), contact_slop=float(p.contact_slop),
                max_depen_vel=float(p.max_depen_vel), object_ang_damping=float(p.object_ang_damping))


def free_velocity(bodies, root, force, torque, prm):
    """(NO, 6) free twists and the (NO) list of world inertias. bodies: (mass, com, inertia) per object; root: (NO, 13)."""
    h = prm["h"]
    out, Iw = np.zeros((len(bodies), 6)), []
    for o, (m, _, I) in enumerate(bodies):
        Iw.append(world_inertia(I, root[o, 3:7]))
        out[o, 0:3] = root[o, 7:10] + h * prm["gravity"] + h * np.asarray(force[o], np.float64) / m
        out[o, 3:6] = root[o, 10:13] / (1 + h * prm["object_ang_damping"]) + h * np.linalg.solve(Iw[o], torque[o])
    return out, Iw


def object_jacobian(bodies, root, rows):
    """(nc, 6 NO) normal-row Jacobian blocks of the objects: side a +(n, (x - c) x n), side b the negative."""
    NO = len(bodies)
    J = np.zeros((len(rows), 6 * NO))
    for i, r in enumerate(rows):
        x, n = r[0:3], r[3:6]
        for code, sg in ((int(r[7]), 1.0), (int(r[8]), -1.0)):
            if 0 <= code < 100:
                c = root[code, 0:3] + rot(root[code, 3:7] / np.linalg.norm(root[code, 3:7])) @ bodies[code][1]
                J[i, 6 * code:6 * code + 3] += sg * n
                J[i, 6 * code + 3:6 * code + 6] += sg * np.cross(x - c, n)
    return J


def step(bodies, root, force, torque, rows, prm, extra=None):
    """One frictionless substep of an env. root (NO, 13) float64, rows (nc, 9). extra: None or (M_r, v_free_r, J_r) of
    an articulation's coordinates, J_r (nc, D) the rows' blocks in them. Returns dict(v (NO, 6), lam, kkt, v_extra,
    root (NO, 13) the integrated state)."""
    root = np.asarray(root, np.float64)
    rows = np.asarray(rows, np.float64).reshape(-1, 9)
    NO, h = len(bodies), prm["h"]
    vf, Iw = free_velocity(bodies, root, force, torque, prm)
    D = 0 if extra is None else len(extra[1])
    M = np.zeros((D + 6 * NO, D + 6 * NO))
    for o in range(NO):
        k = D + 6 * o
        M[k:k + 3, k:k + 3] = bodies[o][0] * np.eye(3)
        M[k + 3:k + 6, k + 3:k + 6] = Iw[o]
    J = np.zeros((len(rows), D + 6 * NO))
    J[:, D:] = object_jacobian(bodies, root, rows)
    v0 = vf.reshape(-1)
    if extra is not None:
        M[:D, :D] = extra[0]
        J[:, :D] = extra[2]
        v0 = np.concatenate([extra[1], v0])
    v, lam, kkt = solve_qp(M, v0, J, normal_target(rows[:, 6], h, prm))
    vo = v[D:].reshape(NO, 6)
    new = root.copy()
    for o in range(NO):
        R = rot(root[o, 3:7] / np.linalg.norm(root[o, 3:7]))
        c = root[o, 0:3] + R @ bodies[o][1] + h * vo[o, 0:3]
        x, y, z, w = root[o, 3:7]
        wx, wy, wz = vo[o, 3:6]
        dq = np.array([wx * w + wy * z - wz * y, wy * w + wz * x - wx * z, wz * w + wx * y - wy * x,
                       -wx * x - wy * y - wz * z])           # (w, 0) (x) q
        q = root[o, 3:7] + 0.5 * h * dq
        q = q / np.linalg.norm(q)
        new[o, 3:7], new[o, 7:13] = q, vo[o]
        new[o, 0:3] = c - rot(q) @ bodies[o][1]
    return dict(v=vo, lam=lam, kkt=kkt, v_extra=v[:D], root=new)


def gauss_seidel_truncation(bodies, root, force, torque, rows, prm, v_ref, sweeps):
    """How far `sweeps` sweeps of exact (float64) projected Gauss-Seidel on the dual, rows in list order from lambda = 0,
    are from the QP's velocities v_ref: (linear, angular) largest component. A property of the QP (the conditioning
    of J M^-1 J^T on its active set), not of any solver's code: a scene meant to test a converged solve must keep it
    far below the test's tolerance, or the test measures the truncation."""
    root = np.asarray(root, np.float64)
    rows = np.asarray(rows, np.float64).reshape(-1, 9)
    NO = len(bodies)
    vf, Iw = free_velocity(bodies, root, force, torque, prm)
    J = object_jacobian(bodies, root, rows)
    Y = J.copy()
    for o in range(NO):
        Y[:, 6 * o:6 * o + 3] /= bodies[o][0]
        Y[:, 6 * o + 3:6 * o + 6] = np.linalg.solve(Iw[o], J[:, 6 * o + 3:6 * o + 6].T).T
    A, b = J @ Y.T, J @ vf.reshape(-1) - normal_target(rows[:, 6], prm["h"], prm)
    lam, d = np.zeros(len(J)), np.diag(J @ Y.T).copy()
    for _ in range(sweeps):
        for i in range(len(J)):
            lam[i] = max(0.0, lam[i] - (A[i] @ lam + b[i]) / d[i])
    dv = np.abs((vf.reshape(-1) + Y.T @ lam).reshape(NO, 6) - v_ref)
    return float(dv[:, 0:3].max()), float(dv[:, 3:6].max())


def spread(bodies, root, force, torque, rows, prm, draws=8, seed=0):
    """What float32 storage of the inputs alone does to the answer: re-solve with x, n, sep and the poses perturbed by
    relative 2^-23 noise; (linear, angular) spread of the velocities over the draws, the largest max - min of a
    component."""
    rng = np.random.default_rng(seed)
    root = np.asarray(root, np.float64)
    rows = np.asarray(rows, np.float64).reshape(-1, 9)
    vs = []
    for _ in range(draws):
        r2, s2 = rows.copy(), root.copy()
        r2[:, 0:7] *= 1 + EPS32 * rng.uniform(-1, 1, r2[:, 0:7].shape)
        s2[:, 0:7] *= 1 + EPS32 * rng.uniform(-1, 1, s2[:, 0:7].shape)
        vs.append(step(bodies, s2, force, torque, r2, prm)["v"])
    ptp = np.ptp(np.array(vs), axis=0)
    return float(ptp[:, 0:3].max()), float(ptp[:, 3:6].max())
