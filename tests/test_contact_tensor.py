"""The contact tensor's host side without a GPU: the ABI entry and its struct mirror, the gym_api calls, and the
conversion of tensor rows into Isaac Gym's RigidContact records (tests/test_gpu_contact_tensor.py runs the kernels)."""
import ctypes as C

import numpy as np
import pytest

from handarm_hip import _lib
from handarm_hip import gym_api
from handarm_hip import model as HM


def test_abi_entry_and_struct_mirror():
    assert "ha_refresh_contacts" in _lib.SIGNATURES
    assert "ha_refresh_contacts" in _lib.header_symbols()
    # LP64: ptr, ptr, i32 + pad, ptr, i32 + pad
    assert C.sizeof(HM.HaContacts) == 40
    assert [HM.HaContacts.contacts.offset, HM.HaContacts.counts.offset, HM.HaContacts.max_contacts.offset,
            HM.HaContacts.env_ids.offset, HM.HaContacts.n_envs.offset] == [0, 8, 16, 24, 32]
    assert HM.CONTACT_REC == 20
    with open(_lib.HEADER) as f:
        assert "#define HA_CONTACT_REC 20" in f.read()


def test_refresh_contacts_rejects_bad_arguments_without_a_gpu():
    from handarm_hip import build
    build.build()
    lib = _lib.load()
    k = HM.HaContacts()
    assert lib.ha_refresh_contacts(None, C.byref(k), None) == -1        # HA_E_ARG, no GPU touched
    assert lib.ha_refresh_contacts(None, None, None) == -1


def test_gym_has_the_contact_calls():
    for name in ("acquire_contact_tensor", "refresh_contact_tensor", "get_rigid_contacts", "get_env_rigid_contacts"):
        assert callable(getattr(gym_api.Gym, name))


def _rows(n, cap, rng):
    rows = rng.standard_normal((n, cap, 20)).astype(np.float32)
    rows[..., 7:11] = rng.integers(-1, 40, (n, cap, 4))
    return rows


def test_rigid_contacts_from_rows():
    rng = np.random.default_rng(0)
    n, cap = 4, 6
    rows = _rows(n, cap, rng)
    rows[1, 2:] = np.nan                        # rows >= kept are never read
    counts = np.array([[3, 9], [2, 2], [0, 0], [6, 11]], np.int32)
    rc = gym_api.rigid_contacts_from_rows(rows, counts)
    assert rc.dtype == gym_api.RIGID_CONTACT_DTYPE
    assert rc.dtype.names == ("env0", "env1", "body0", "body1", "localPos0", "localPos1", "minDist", "normal")
    assert [rc.dtype[k] for k in ("env0", "body1", "minDist")] == [np.int32, np.int32, np.float32]
    assert rc.dtype["localPos0"].shape == (3,) and rc.dtype["normal"].base == np.float32
    assert len(rc) == 11
    env = np.repeat(np.arange(n), counts[:, 0])
    slot = np.concatenate([np.arange(k) for k in counts[:, 0]])
    np.testing.assert_array_equal(rc["env0"], env)
    np.testing.assert_array_equal(rc["env1"], env)
    src = rows[env, slot]
    assert np.isfinite(src).all()
    np.testing.assert_array_equal(rc["body0"], src[:, 9].astype(np.int32))
    np.testing.assert_array_equal(rc["body1"], src[:, 10].astype(np.int32))
    np.testing.assert_array_equal(rc["localPos0"], src[:, 11:14])
    np.testing.assert_array_equal(rc["localPos1"], src[:, 14:17])
    np.testing.assert_array_equal(rc["minDist"], src[:, 6])
    np.testing.assert_array_equal(rc["normal"], src[:, 3:6])
    # one env's slice (get_env_rigid_contacts): the env index comes from the caller
    one = gym_api.rigid_contacts_from_rows(rows[3:4], counts[3:4], env0=3)
    assert len(one) == 6 and (one["env0"] == 3).all() and (one["env1"] == 3).all()
    np.testing.assert_array_equal(one["minDist"], rows[3, :, 6])
    # no contacts at all, and counts beyond the tensor
    assert len(gym_api.rigid_contacts_from_rows(rows, np.zeros((n, 2), np.int32))) == 0
    with pytest.raises(ValueError):
        gym_api.rigid_contacts_from_rows(rows, np.full((n, 2), cap + 1, np.int32))
