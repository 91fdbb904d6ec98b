"""Jacobian / mass-matrix tensors, the parts that need no GPU: the float64 yardstick tests/jacobian_ref.py is held
against Chain.fk by central differences and against Chain.jacobians' Jw, and ha_refresh_kinematics' argument checks
and struct mirror are checked on the host."""
import ctypes as C

import numpy as np
import pytest

from handarm_hip import _lib
from handarm_hip import model as HM
from tests.jacobian_ref import cancellation_mask, jacobian_tensor
from tests.kinematics import Chain
from tests.test_independent_dynamics import ROBOTS


@pytest.fixture(scope="module")
def lib():
    from handarm_hip import build
    build.build()
    return _lib.load()


def _pose(chain, task, seed):
    p, _ = HM.build_params(task=task)
    rng = np.random.default_rng(seed)
    return np.array(list(p.reset_pose)[:chain.D], np.float64) + rng.uniform(-0.3, 0.3, chain.D)


@pytest.mark.parametrize("task,asset", ROBOTS)
def test_reference_linear_rows_are_the_derivative_of_fk(task, asset):
    """d p_i / d q_d by central differences (step 1e-6) equals rows 0..2 within 1e-7, for every link and DOF."""
    ch = Chain(HM.load_scene(asset))
    q = _pose(ch, task, 1)
    J = jacobian_tensor(ch, q)
    h = 1e-6
    for d in range(ch.D):
        e = np.zeros(ch.D)
        e[d] = h
        pp, pm = np.array(ch.fk(q + e)[1]), np.array(ch.fk(q - e)[1])
        np.testing.assert_allclose(J[:, 0:3, d], ((pp - pm) / (2 * h))[1:], rtol=0, atol=1e-7, err_msg=f"dof {d}")


@pytest.mark.parametrize("task,asset", ROBOTS)
def test_reference_angular_rows_are_chain_jw(task, asset):
    ch = Chain(HM.load_scene(asset))
    q = _pose(ch, task, 2)
    J = jacobian_tensor(ch, q)
    bodies, _ = ch.jacobians(q)
    for i in range(1, ch.L):
        np.testing.assert_array_equal(J[i - 1, 3:6], bodies[i][3])
    sub = jacobian_tensor(ch, q, links=[ch.L - 1, 2])
    np.testing.assert_array_equal(sub, J[[ch.L - 2, 1]])


@pytest.mark.parametrize("task,asset", ROBOTS)
def test_cancellation_mask_leaves_the_structural_zeros(task, asset):
    """The mask only ever covers linear rows of ancestor columns, so every never-written column stays an exact zero the
    device must match; and the zeros it does cover are a handful (link origins on a joint axis)."""
    ch = Chain(HM.load_scene(asset))
    q = _pose(ch, task, 3)
    J, mask = jacobian_tensor(ch, q), cancellation_mask(ch, q)
    assert mask.shape == J.shape and not mask[:, 3:6].any()
    for i in range(1, ch.L):
        other = [d for d in range(ch.D) if d not in ch.ancestors(i)]
        assert not mask[i - 1][:, other].any() and (J[i - 1][:, other] == 0.0).all()
    assert ((J == 0.0) & mask).sum() <= 3 * ch.L


def test_refresh_kinematics_rejects_bad_arguments(lib):
    """Null handle, null struct and a struct with both outputs null: HA_E_ARG before anything touches a device."""
    k = HM.HaKinematics()
    assert lib.ha_refresh_kinematics(None, C.byref(k), None) == -1
    fake = C.create_string_buffer(1 << 16)          # a zeroed stand-in for a handle: never bound, never launched
    assert lib.ha_refresh_kinematics(C.cast(fake, C.c_void_p), None, None) == -1
    assert lib.ha_refresh_kinematics(C.cast(fake, C.c_void_p), C.byref(k), None) == -1


def test_kinematics_struct_mirror():
    assert C.sizeof(HM.HaKinematics) == 32
    assert [f[0] for f in HM.HaKinematics._fields_] == ["jacobian", "mass_matrix", "links", "n_links"]
    assert HM.HaKinematics.n_links.offset == 24
