"""gym.apply_rigid_body_force_tensors with a torque tensor (allegro_kuka_base.py:1417-1424, privilegedActions): the
object bodies' rows reach ha_state_t.object_torque exactly as a direct write does, in ENV_SPACE and LOCAL_SPACE, alone
or after the LOCAL_SPACE force call of the same step (:1412-1414)."""
import numpy as np
import pytest
import torch

from handarm_hip import model as HM
from handarm_hip.gym_api import _quat_rotate, acquire_gym, gymapi, gymtorch
from tests import scenes

pytestmark = pytest.mark.gpu
N = 8
OUT = ("dof_state", "root_state", "rigid_body_state")


def _kuka_sim(seed=3):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from handarm_hip.sim import HandArmSim
    from oracle.oracle_lib import HostState
    sim = HandArmSim(N, "cuda:0", task_cfg={"task": HM.TASK_ALLEGRO_KUKA, "privileged_actions": True},
                     task=HM.TASK_ALLEGRO_KUKA)
    st = HostState(N, model=sim.model, params=sim.params)
    lo = np.array(sim.model.dof_lower[:23], np.float32)
    up = np.array(sim.model.dof_upper[:23], np.float32)
    scenes.fill_kuka_scene(st, N, lo, up, list(sim.params.reset_pose), sim.t["object_scale"].cpu().numpy(),
                           list(sim.model.table_pos), seed=seed)
    for k in HM.STATE_FIELDS:
        if k not in ("stats", "term_sums", "task_state", "task_scalars"):
            sim.t[k].copy_(torch.as_tensor(st[k]).reshape(sim.t[k].shape).to(sim.t[k].dtype))
    return sim, lo, up


def _inputs(sim, lo, up, steps, seed=4):
    """Per step: DOF targets (N, D), rigid-body forces and torques (N * B, 3), non-zero on the object body only."""
    rng = np.random.default_rng(seed)
    B, ob = sim.num_bodies, sim.model.body_object0
    out = []
    for _ in range(steps):
        tgt = rng.uniform(lo, up, (N, 23)).astype(np.float32)
        f = np.zeros((N, B, 3), np.float32)
        tq = np.zeros((N, B, 3), np.float32)
        f[:, ob] = 0.3 * rng.standard_normal((N, 3))
        tq[:, ob] = rng.uniform(-0.005, 0.005, (N, 3))
        out.append(tuple(torch.as_tensor(x.reshape(-1, x.shape[-1]) if x.ndim == 3 else x).to(sim.device)
                         for x in (tgt, f, tq)))
    return out


def _object_quat(sim):
    a = sim.model.actor_object0
    return sim.t["root_state"].view(N, sim.num_actors, 13)[:, a:a + 1, 3:7]


def _state(sim):
    torch.cuda.synchronize()
    return {k: sim.t[k].cpu().numpy().copy() for k in OUT}


def test_torque_call_equals_direct_write_bit_for_bit():
    gym = acquire_gym()
    (A, lo, up), (Bs, _, _), (Z, _, _) = _kuka_sim(), _kuka_sim(), _kuka_sim()
    ob = A.model.body_object0
    differs = False
    for tgt, f, tq in _inputs(A, lo, up, 3):
        # sim A: the reference's per-step sequence through gym_api
        assert gym.set_dof_position_target_tensor(A, gymtorch.unwrap_tensor(tgt))
        assert gym.apply_rigid_body_force_tensors(A, gymtorch.unwrap_tensor(f), None, gymapi.LOCAL_SPACE)
        assert gym.apply_rigid_body_force_tensors(A, None, gymtorch.unwrap_tensor(tq), gymapi.ENV_SPACE)
        gym.simulate(A)
        # sim B: the state tensors written directly
        fo = f.view(N, A.num_bodies, 3)[:, ob:ob + 1]
        to = tq.view(N, A.num_bodies, 3)[:, ob:ob + 1]
        Bs.set_dof_position_target_tensor(tgt)
        Bs.t["object_force"].copy_(_quat_rotate(_object_quat(Bs), fo))
        Bs.t["object_torque"].copy_(to)
        Bs.simulate(1)
        # sim Z: the same step without the torque
        Z.set_dof_position_target_tensor(tgt)
        Z.t["object_force"].copy_(_quat_rotate(_object_quat(Z), fo))
        Z.simulate(1)
        a, b, z = _state(A), _state(Bs), _state(Z)
        for k in OUT:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), f"{k} differs from the direct write"
        assert not A.t["object_torque"].any() and not A.t["object_force"].any()     # consumed by the simulate
        wa = a["root_state"].reshape(N, -1, 13)[:, A.model.actor_object0, 10:13]
        wz = z["root_state"].reshape(N, -1, 13)[:, A.model.actor_object0, 10:13]
        differs = differs or (np.abs(wa - wz).max(axis=1) > 1e-3).all()
    assert differs, "the object's angular velocity is the same with and without the torque"


def test_local_space_torque_equals_prerotated_env_space_torque():
    gym = acquire_gym()
    (A, lo, up), (Bs, _, _) = _kuka_sim(), _kuka_sim()
    ob = A.model.body_object0
    (tgt, f, tq), = _inputs(A, lo, up, 1, seed=5)
    # force and torque in ONE call, LOCAL_SPACE
    gym.apply_rigid_body_force_tensors(A, gymtorch.unwrap_tensor(f), gymtorch.unwrap_tensor(tq), gymapi.LOCAL_SPACE)
    pre = torch.zeros_like(tq).view(N, A.num_bodies, 3)
    pre[:, ob:ob + 1] = _quat_rotate(_object_quat(Bs), tq.view(N, A.num_bodies, 3)[:, ob:ob + 1])
    gym.apply_rigid_body_force_tensors(Bs, f, None, gymapi.LOCAL_SPACE)
    gym.apply_rigid_body_force_tensors(Bs, None, pre, gymapi.ENV_SPACE)
    assert torch.equal(A.t["object_torque"], Bs.t["object_torque"]) and A.t["object_torque"].any()
    assert torch.equal(A.t["object_force"], Bs.t["object_force"]) and A.t["object_force"].any()
    for s in (A, Bs):
        s.set_dof_position_target_tensor(tgt)
        s.simulate(1)
    a, b = _state(A), _state(Bs)
    for k in OUT:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_ur5sih_binds_object_torque_too():
    """Every task binds ha_state_t.object_torque (HM.null_fields leaves it out for none), so the torque call is applied
    for Ur5Sih as well: its objects' rows land in the tensor and the next simulate consumes them."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from handarm_hip.sim import HandArmSim
    assert all("object_torque" not in HM.null_fields(t)
               for t in (HM.TASK_UR5SIH, HM.TASK_ALLEGRO_HAND, HM.TASK_ALLEGRO_KUKA))
    from oracle.oracle_lib import HostState
    n = 4
    sim = HandArmSim(n, "cuda:0")
    st = HostState(n)
    scenes.fill_scene(st, n, seed=0)
    for k in ("root_state", "dof_state", "sim_targets", "object_indices"):
        sim.t[k].copy_(torch.as_tensor(st[k]).reshape(sim.t[k].shape).to(sim.t[k].dtype))
    o0, no = sim.model.body_object0, sim.n_obj
    tq = torch.zeros((n * sim.num_bodies, 3), device=sim.device)
    tq.view(n, sim.num_bodies, 3)[:, o0:o0 + no] = torch.as_tensor(
        np.random.default_rng(6).uniform(-0.02, 0.02, (n, no, 3)).astype(np.float32)).to(sim.device)
    gym = acquire_gym()
    assert gym.apply_rigid_body_force_tensors(sim, None, gymtorch.unwrap_tensor(tq), gymapi.ENV_SPACE)
    assert torch.equal(sim.t["object_torque"], tq.view(n, sim.num_bodies, 3)[:, o0:o0 + no])
    assert not sim.t["object_force"].any()
    gym.simulate(sim)
    torch.cuda.synchronize()
    assert not sim.t["object_torque"].any()
