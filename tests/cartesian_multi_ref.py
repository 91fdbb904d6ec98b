"""Float64 whole-hand Cartesian controller from tests/cartesian_ref.py's task_error / tool_jacobian and np.linalg.solve
(test infrastructure; shares no code with csrc/): several links' rows stacked, weighted and solved as one damped
least-squares step, the semantics of ha_cartesian_multi_t (include/handarm_abi.h).

``multi_step(chain, q, goals, tasks, ...)`` is one step for one env and returns (targets, e): targets is a copy of ``q``
in which only U, the union of the tasks' selected ancestor DOFs, moved; e is (T, 6), each task's UNWEIGHTED error.
tasks are dicts ``link`` (index), ``offset``, ``position_only``, ``weight``.

``emulated_dq`` is the same step with J and e rounded to float32 and the rest either in float64 (what the kernel does)
or in float32 (the design the kernel does not use): the precision emulations of tests/test_cartesian_multi_ref.py.

``robot_multi_case`` gives the task sets, joints and goals the CPU and the GPU tests share."""
import numpy as np

from tests import cartesian_ref as CR

POSE, DELTA = CR.POSE, CR.DELTA


def _task(t):
    return (int(t["link"]), tuple(t.get("offset", (0.0, 0.0, 0.0))), bool(t.get("position_only", False)),
            float(t.get("weight", 1.0)))


def stacked(chain, q, goals, tasks, dofs=None, mode=POSE):
    """(J (R, D), e (R,), w (R,), e6 (T, 6), U): the unweighted stacked rows, the row weights and the DOF union."""
    q = np.asarray(q, np.float64)
    fk = chain.fk(q)
    Js, es, ws, e6, U = [], [], [], [], set()
    for t, task in enumerate(tasks):
        link, off, ponly, w = _task(task)
        e = CR.task_error(chain, q, goals[t], link, mode, off, ponly, fk)
        J = CR.tool_jacobian(chain, q, link, dofs, off, ponly, fk)
        nr = 3 if ponly else 6
        Js.append(J[:nr])
        es.append(e[:nr])
        ws.append(np.full(nr, w))
        e6.append(e)
        U |= set(CR.selected_dofs(chain, link, dofs))
    return np.concatenate(Js), np.concatenate(es), np.concatenate(ws), np.stack(e6), sorted(U)


def _finish(chain, q, dq, U, max_step, lower, upper):
    mx = np.abs(dq).max()
    if max_step > 0 and mx > max_step:
        dq = dq * (max_step / mx)
    out = q.copy()
    lo = np.full(chain.D, -np.inf) if lower is None else np.asarray(lower, np.float64)
    up = np.full(chain.D, np.inf) if upper is None else np.asarray(upper, np.float64)
    out[U] = np.clip(q[U] + dq[U], lo[U], up[U])
    return out


def _posture_z(chain, q, U, q_rest, null_gain):
    z = np.zeros(chain.D)
    z[U] = null_gain * (np.asarray(q_rest, np.float64)[U] - q[U])
    return z


def multi_step(chain, q, goals, tasks, dofs=None, mode=POSE, damping=0.05, max_step=0.0, q_rest=None, null_gain=0.0,
               lower=None, upper=None):
    q = np.asarray(q, np.float64)
    J, e, w, e6, U = stacked(chain, q, np.asarray(goals, np.float64), tasks, dofs, mode)
    Jw, ew = J * w[:, None], e * w
    A = Jw @ Jw.T + damping ** 2 * np.eye(len(ew))
    dq = Jw.T @ np.linalg.solve(A, ew)
    if null_gain > 0:
        z = _posture_z(chain, q, U, q_rest, null_gain)
        dq = dq + (z - Jw.T @ np.linalg.solve(A, Jw @ z))
    return _finish(chain, q, dq, U, max_step, lower, upper), e6


def _chol_solve32(A, b):
    """x = A^-1 b with every operation rounded to float32: numpy's float32 Cholesky, then both substitutions."""
    G = np.linalg.cholesky(A.astype(np.float32))
    assert G.dtype == np.float32
    n = len(b)
    y = np.zeros(n, np.float32)
    for i in range(n):
        acc = np.float32(b[i])
        for k in range(i):
            acc = np.float32(acc - np.float32(G[i, k] * y[k]))
        y[i] = np.float32(acc / G[i, i])
    x = np.zeros(n, np.float32)
    for i in range(n - 1, -1, -1):
        acc = y[i]
        for k in range(i + 1, n):
            acc = np.float32(acc - np.float32(G[k, i] * x[k]))
        x[i] = np.float32(acc / G[i, i])
    return x


def emulated_dq(chain, q, goals, tasks, rest="float64", dofs=None, mode=POSE, damping=0.05, q_rest=None,
                null_gain=0.0):
    """The unlimited, unclamped dq with J and e rounded to float32 and the rest of the step (A, its Cholesky factor, the
    solves, J^T y) in ``rest`` precision. float64: the weights are applied in float64, so the float32 products promote
    exactly, as the kernel does. float32: Jw, ew, A, the factor and the products are all float32, as the 6 x 6
    single-link kernel works."""
    q = np.asarray(q, np.float64)
    J, e, w, _, U = stacked(chain, q, np.asarray(goals, np.float64), tasks, dofs, mode)
    J32, e32 = J.astype(np.float32), e.astype(np.float32)
    if rest == "float64":
        Jw, ew = J32.astype(np.float64) * w[:, None], e32.astype(np.float64) * w
        L = np.linalg.cholesky(Jw @ Jw.T + damping ** 2 * np.eye(len(ew)))

        def solve(b):
            return np.linalg.solve(L.T, np.linalg.solve(L, b))
        dq = Jw.T @ solve(ew)
        if null_gain > 0:
            z = _posture_z(chain, q, U, q_rest, null_gain).astype(np.float32).astype(np.float64)
            dq = dq + (z - Jw.T @ solve(Jw @ z))
        return dq
    w32 = w.astype(np.float32)
    Jw, ew = J32 * w32[:, None], e32 * w32
    A = Jw @ Jw.T + np.float32(damping) ** 2 * np.eye(len(ew), dtype=np.float32)
    dq = Jw.T @ _chol_solve32(A, ew)
    if null_gain > 0:
        z = _posture_z(chain, q, U, q_rest, null_gain).astype(np.float32)
        dq = dq + (z - Jw.T @ _chol_solve32(A, Jw @ z))
    assert dq.dtype == np.float32
    return dq.astype(np.float64)


def exact_dq(chain, q, goals, tasks, dofs=None, mode=POSE, damping=0.05, q_rest=None, null_gain=0.0):
    """The float64 dq the emulations are compared with (no step limit, no clamp)."""
    q = np.asarray(q, np.float64)
    J, e, w, _, U = stacked(chain, q, np.asarray(goals, np.float64), tasks, dofs, mode)
    Jw, ew = J * w[:, None], e * w
    A = Jw @ Jw.T + damping ** 2 * np.eye(len(ew))
    dq = Jw.T @ np.linalg.solve(A, ew)
    if null_gain > 0:
        z = _posture_z(chain, q, U, q_rest, null_gain)
        dq = dq + (z - Jw.T @ np.linalg.solve(A, Jw @ z))
    return dq


TASK_LINKS = {
    "ur5sih": ("flange", ["index_fingertip", "little_fingertip", "middle_fingertip", "ring_fingertip",
                          "thumb_fingertip"]),
    "allegro_kuka": ("iiwa7_link_7", ["index_link_3", "middle_link_3", "ring_link_3", "thumb_link_3"]),
    "allegro_hand": (None, ["index_link_3", "middle_link_3", "ring_link_3", "thumb_link_3"]),
}


def robot_kind(chain):
    names = [l["name"] for l in chain.links]
    return "ur5sih" if "flange" in names else "allegro_kuka" if "iiwa7_link_7" in names else "allegro_hand"


def tool_goals(chain, q, tasks):
    """(T, 7) float64: every task's tool pose (pos + quat xyzw) at the joints q."""
    fk = chain.fk(np.asarray(q, np.float64))
    out = np.zeros((len(tasks), 7))
    for t, task in enumerate(tasks):
        link, off, _, _ = _task(task)
        pt, Rl = CR.tool_pose(chain, q, link, off, fk)
        out[t, 0:3], out[t, 3:7] = pt, CR.matrix_quat(Rl)
    return out


def robot_multi_case(chain, task, n, seed):
    """The inputs the CPU and the GPU tests share, per robot (``task``: the HM.TASK_* id, for its reset pose):
    Ur5Sih        flange pose + the five *_fingertip positions      21 rows (more than its 17 DOFs)
    AllegroKuka   iiwa7_link_7 pose + the four *_link_3 positions   18 rows
    AllegroHand   the four *_link_3 positions                       12 rows
    Tool offset cartesian_ref.OFFSET, weights 1. Joints as cartesian_ref.robot_case draws them (arms: reset_pose +
    U(-0.3, 0.3)); the AllegroHand at mid-range + U(-0.2, 0.2); all kept 0.05 rad inside the limits. ``consistent`` goals
    are the tools' poses at q + U(-0.15, 0.15), clipped the same way, so one joint vector reaches them all;
    ``inconsistent`` goals are those with each position moved by U(-0.01, 0.01) m. Stored as float32, (n, T, 7)."""
    from handarm_hip import model as HM
    rng = np.random.default_rng(seed)
    names = [l["name"] for l in chain.links]
    arm, tips = TASK_LINKS[robot_kind(chain)]
    lo, up = CR.limits(chain)
    tasks = [] if arm is None else [dict(link=names.index(arm), offset=CR.OFFSET, position_only=False, weight=1.0)]
    tasks += [dict(link=names.index(f), offset=CR.OFFSET, position_only=True, weight=1.0) for f in tips]
    if arm is None:
        q = np.clip((lo + up) / 2 + rng.uniform(-0.2, 0.2, (n, chain.D)), lo + 0.05, up - 0.05).astype(np.float32)
    else:
        p, _ = HM.build_params(task=task)
        q = CR.case_joints(chain, np.array(list(p.reset_pose)[:chain.D]), n, rng)
    qg = np.clip(q.astype(np.float64) + rng.uniform(-0.15, 0.15, q.shape), lo + 0.05, up - 0.05)
    consistent = np.stack([tool_goals(chain, qg[e], tasks) for e in range(n)])
    inconsistent = consistent.copy()
    inconsistent[:, :, 0:3] += rng.uniform(-0.01, 0.01, (n, len(tasks), 3))
    return dict(tasks=tasks, arm=arm is not None, q=q, q_goal=qg, consistent=consistent.astype(np.float32),
                inconsistent=inconsistent.astype(np.float32), damping=0.01 if arm is None else 0.05,
                rows=sum(3 if t["position_only"] else 6 for t in tasks))


def weighted(tasks, arm_weight=1.0, tip_weight=3.0):
    """The task list with the position-only (fingertip) tasks at ``tip_weight`` and the others at ``arm_weight``."""
    return [dict(t, weight=tip_weight if t["position_only"] else arm_weight) for t in tasks]


def closed_loop(chain, q, goals, tasks, iters, **kw):
    """``iters`` steps that feed the targets back as the joint positions (no physics); every iterate, (iters, D)."""
    lo, up = CR.limits(chain)
    q = np.asarray(q, np.float64)
    out = []
    for _ in range(iters):
        q, _ = multi_step(chain, q, goals, tasks, lower=lo, upper=up, **kw)
        out.append(q)
    return np.stack(out)


def position_residual(chain, q, goals, tasks):
    """Largest position error component over the tasks at the joints q."""
    _, _, _, e6, _ = stacked(chain, q, np.asarray(goals, np.float64), tasks)
    return np.abs(e6[:, 0:3]).max()


def one_step_variants(chain, task, n, seed):
    """(case, variants) of the one-step tests for a robot and N: ``case`` is robot_multi_case's, every variant a dict of
    multi_step's arguments (tasks, goals (n, T, 7 or 6) float32, mode, damping, max_step and, for the posture variant,
    q_rest and null_gain).
    consistent             consistent goals, the case's damping (arms 0.05, hand 0.01), max_step 0.2
    weighted_inconsistent  inconsistent goals, damping 0.05, arm task weight 1, fingertip weights 3, no step limit
    delta                  delta mode: e drawn U(-0.03, 0.03) m and U(-0.12, 0.12) rad
    step_binding           the consistent variant with max_step 0.02
    posture                AllegroKuka only: the consistent variant with q_rest = reset pose, null_gain 0.5
    subset                 T = 2: the arm pose and the thumb tip (AllegroHand: the index and the thumb tip)
    same_link_twice        the subset tasks and a third on the thumb's last link with offset 0: two tool points on one
                           link"""
    from handarm_hip import model as HM
    c = robot_multi_case(chain, task, n, seed)
    rng = np.random.default_rng(seed + 1)
    tasks, T = c["tasks"], len(c["tasks"])
    base = dict(tasks=tasks, goals=c["consistent"], mode=POSE, damping=c["damping"], max_step=0.2)
    v = {"consistent": base,
         "weighted_inconsistent": dict(base, tasks=weighted(tasks), goals=c["inconsistent"], damping=0.05,
                                       max_step=0.0),
         "delta": dict(base, mode=DELTA,
                       goals=(rng.uniform(-0.03, 0.03, (n, T, 6)) * ([1] * 3 + [4] * 3)).astype(np.float32)),
         "step_binding": dict(base, max_step=0.02)}
    if robot_kind(chain) == "allegro_kuka":
        p, _ = HM.build_params(task=task)
        v["posture"] = dict(base, q_rest=np.array(list(p.reset_pose)[:chain.D], np.float32), null_gain=0.5)
    sub = [0, T - 1]                                   # the thumb tip is the last task of every robot
    v["subset"] = dict(base, tasks=[tasks[t] for t in sub], goals=np.ascontiguousarray(c["consistent"][:, sub]))
    twin = dict(tasks[T - 1], offset=(0.0, 0.0, 0.0))
    g3 = np.stack([np.concatenate([c["consistent"][e][sub], tool_goals(chain, c["q_goal"][e], [twin])])
                   for e in range(n)]).astype(np.float32)
    v["same_link_twice"] = dict(base, tasks=[tasks[t] for t in sub] + [twin], goals=g3)
    return c, v


def variant_kwargs(var):
    """multi_step's keyword arguments of a variant (everything but the goals)."""
    return {k: x for k, x in var.items() if k != "goals"}
