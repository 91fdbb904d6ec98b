"""Float64 link Jacobians from tests/kinematics.py's Chain (test infrastructure; shares no code with csrc/).

``origin_jacobian(chain, q, i)`` is the 6 x D Jacobian of link i's FRAME ORIGIN (the point of
rigid_body_state[..., 0:3], not the COM): column d = (a_d x (p_i - o_d), a_d) for d in Chain.ancestors(i), with the
world axes a_d and anchors o_d of Chain.fk(); every other column stays exactly 0."""
import numpy as np


def origin_jacobian(chain, q, i, fk=None):
    R, p, ax, an = fk if fk is not None else chain.fk(np.asarray(q, np.float64))
    J = np.zeros((6, chain.D))
    for d in chain.ancestors(i):
        J[0:3, d] = np.cross(ax[d], p[i] - an[d])
        J[3:6, d] = ax[d]
    return J


def cancellation_mask(chain, q, links=None):
    """(K, 6, D) bool: linear-row entries of an ancestor DOF's column whose cross-product component subtracts two
    NON-ZERO products. Where the link origin lies on the joint axis (r parallel to a_d) the true value is 0 and the
    float64 difference comes out exactly 0.0 or ~1e-17 by rounding luck; such a zero says nothing about structure. The
    reference's other zeros (columns never written, a x 0, zero axis components) involve no cancellation."""
    q = np.asarray(q, np.float64)
    R, p, ax, an = chain.fk(q)
    links = list(range(1, chain.L) if links is None else links)
    out = np.zeros((len(links), 6, chain.D), bool)
    for k, i in enumerate(links):
        for d in chain.ancestors(i):
            r = p[i] - an[d]
            for c in range(3):
                c1, c2 = (c + 1) % 3, (c + 2) % 3
                out[k, c, d] = ax[d][c1] * r[c2] != 0.0 and ax[d][c2] * r[c1] != 0.0
    return out


def jacobian_tensor(chain, q, links=None):
    """(K, 6, D): the origin Jacobians of ``links`` (default 1..L-1, Isaac Gym's fixed-base order)."""
    q = np.asarray(q, np.float64)
    fk = chain.fk(q)
    links = range(1, chain.L) if links is None else links
    return np.stack([origin_jacobian(chain, q, i, fk) for i in links])
