"""Float64 damped least-squares Cartesian controller from tests/kinematics.py's Chain and tests/jacobian_ref.py (test
infrastructure; shares no code with csrc/): the nine steps of csrc/ha_cartesian.h with rotation-matrix FK and
np.linalg.solve.

``cartesian_step(chain, q, goal, link, ...)`` is one step for one env and returns (targets, e): targets is a copy of
``q`` in which only the selected ancestor DOFs of the link moved."""
import numpy as np

from tests.jacobian_ref import origin_jacobian
from tests.kinematics import quat_mul

POSE, DELTA = 0, 1


def matrix_quat(R):
    """xyzw quaternion of a rotation matrix (the branch with the largest denominator)."""
    t = np.trace(R)
    if t > 0:
        s = 2.0 * np.sqrt(1.0 + t)
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0, 0.0, 0.0, (R[k, j] - R[j, k]) / s]
        q[i], q[j], q[k] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    return np.array(q)


def rotation_vector(qe):
    """Rotation vector of a unit xyzw quaternion, shortest arc."""
    qe = np.asarray(qe, np.float64)
    if qe[3] < 0:
        qe = -qe
    v = qe[0:3]
    vn = np.linalg.norm(v)
    return 2.0 * v if vn < 1e-6 else v / vn * 2.0 * np.arctan2(vn, qe[3])


def tool_pose(chain, q, link, offset=(0.0, 0.0, 0.0), fk=None):
    """(p_t, R_link) of the tool point on ``link``."""
    R, p, _, _ = fk if fk is not None else chain.fk(np.asarray(q, np.float64))
    return p[link] + R[link] @ np.asarray(offset, np.float64), R[link]


def task_error(chain, q, goal, link, mode=POSE, offset=(0.0, 0.0, 0.0), position_only=False, fk=None):
    goal = np.asarray(goal, np.float64)
    if mode == POSE:
        pt, Rl = tool_pose(chain, q, link, offset, fk)
        ql = matrix_quat(Rl)
        qg = goal[3:7] / np.linalg.norm(goal[3:7])
        e = np.concatenate([goal[0:3] - pt, rotation_vector(quat_mul(qg, ql * np.array([-1.0, -1.0, -1.0, 1.0])))])
    else:
        e = goal[0:6].copy()
    if position_only:
        e[3:6] = 0.0
    return e


def tool_jacobian(chain, q, link, dofs=None, offset=(0.0, 0.0, 0.0), position_only=False, fk=None):
    """6 x D Jacobian of the tool point: the origin Jacobian moved to p_t, on the selected ancestor DOFs."""
    fk = fk if fk is not None else chain.fk(np.asarray(q, np.float64))
    R, p, ax, an = fk
    J = origin_jacobian(chain, q, link, fk)
    r = R[link] @ np.asarray(offset, np.float64)
    sel = selected_dofs(chain, link, dofs)
    for d in range(chain.D):
        if d in sel:
            J[0:3, d] += np.cross(ax[d], r)
        else:
            J[:, d] = 0.0
    if position_only:
        J[3:6] = 0.0
    return J


def selected_dofs(chain, link, dofs=None):
    anc = set(chain.ancestors(link))
    return sorted(anc if dofs is None else anc & {int(d) for d in dofs})


def limits(chain):
    return tuple(np.array([d[k] for d in chain.dofs], np.float64) for k in ("lower", "upper"))


def case_joints(chain, centre, n, rng):
    """(n, D) float32: centre + U(-0.3, 0.3), kept 0.05 rad inside the limits."""
    lo, up = limits(chain)
    q = np.asarray(centre, np.float64)[:chain.D] + rng.uniform(-0.3, 0.3, (n, chain.D))
    return np.clip(q, lo + 0.05, up - 0.05).astype(np.float32)


def case_goals(chain, q, link, offset, rng, dist=0.05, rot=0.2):
    """(n, 7) float32 goals: each env's tool pose moved by ``dist`` in a random direction and turned by ``rot`` rad about
    a random axis."""
    out = np.zeros((len(q), 7))
    for e in range(len(q)):
        pt, Rl = tool_pose(chain, q[e].astype(np.float64), link, offset)
        u, w = rng.standard_normal(3), rng.standard_normal(3)
        w = w / np.linalg.norm(w)
        out[e, 0:3] = pt + dist * u / np.linalg.norm(u)
        out[e, 3:7] = quat_mul(np.concatenate([w * np.sin(rot / 2), [np.cos(rot / 2)]]), matrix_quat(Rl))
    return out.astype(np.float32)


OFFSET = (0.02, -0.01, 0.05)


def robot_case(chain, task, reset_pose, n, seed):
    """The inputs the CPU and the GPU tests share, per robot: the controlled link, its gains, (n, D) float32 joints and
    (n, 7) float32 goals. Arms: reset_pose + U(-0.3, 0.3), goals 5 cm and 0.2 rad away, lambda 0.05 (neither arm starts
    at its all-zero pose: both are singular there and the loop stalls centimetres off). AllegroHand: the mid-range
    pose in every env (its reset_pose row is not a hand pose), thumb-tip goals 1 cm away, position only, lambda 0.01
    (0.05 still leaves 1 mm after 40 iterations)."""
    names = [l["name"] for l in chain.links]
    rng = np.random.default_rng(seed)
    lo, up = limits(chain)
    if "thumb_link_3" in names and "iiwa7_link_7" not in names:
        c = dict(link=names.index("thumb_link_3"), damping=0.01, position_only=True, dist=0.01)
        c["q"] = np.tile(((lo + up) / 2).astype(np.float32), (n, 1))
    else:
        c = dict(link=names.index("flange" if "flange" in names else "iiwa7_link_7"), damping=0.05,
                 position_only=False, dist=0.05)
        c["q"] = case_joints(chain, reset_pose, n, rng)
    c["dofs"] = sorted(chain.ancestors(c["link"]))
    c["goal"] = case_goals(chain, c["q"], c["link"], OFFSET, rng, dist=c["dist"])
    c["gains"] = dict(offset=OFFSET, damping=c["damping"], max_step=0.2, position_only=c["position_only"])
    return c


def closed_loop(chain, q, goal, link, iters, **kw):
    """``iters`` steps that feed the targets back as the joint positions (no physics); every iterate, (iters, D)."""
    lo, up = limits(chain)
    q = np.asarray(q, np.float64)
    out = []
    for _ in range(iters):
        q, _ = cartesian_step(chain, q, goal, link, lower=lo, upper=up, **kw)
        out.append(q)
    return np.stack(out)


def cartesian_step(chain, q, goal, link, dofs=None, mode=POSE, offset=(0.0, 0.0, 0.0), damping=0.05, max_step=0.0,
                   q_rest=None, null_gain=0.0, position_only=False, lower=None, upper=None):
    q = np.asarray(q, np.float64)
    fk = chain.fk(q)
    e = task_error(chain, q, goal, link, mode, offset, position_only, fk)
    J = tool_jacobian(chain, q, link, dofs, offset, position_only, fk)
    A = J @ J.T + damping ** 2 * np.eye(6)
    dq = J.T @ np.linalg.solve(A, e)
    sel = selected_dofs(chain, link, dofs)
    if null_gain > 0:
        z = np.zeros(chain.D)
        z[sel] = null_gain * (np.asarray(q_rest, np.float64)[sel] - q[sel])
        dq = dq + (z - J.T @ np.linalg.solve(A, J @ z))
    mx = np.abs(dq).max()
    if max_step > 0 and mx > max_step:
        dq = dq * (max_step / mx)
    out = q.copy()
    lo = np.full(chain.D, -np.inf) if lower is None else np.asarray(lower, np.float64)
    up = np.full(chain.D, np.inf) if upper is None else np.asarray(upper, np.float64)
    out[sel] = np.clip(q[sel] + dq[sel], lo[sel], up[sel])
    return out, e
