"""gym_api.apply_rigid_body_force_tensors, the part that needs no GPU: a task whose state binds no object_torque
(HM.null_fields) refuses a torque tensor by name instead of dropping it. No shipped task is such a task today, so the
null set is patched."""
import types

import pytest
import torch

from handarm_hip import gym_api
from handarm_hip import model as HM


def test_torque_for_a_task_without_object_torque_is_refused(monkeypatch):
    monkeypatch.setattr(gym_api.HM, "null_fields", lambda task: {"object_scale", "object_torque"})
    sim = types.SimpleNamespace(task=HM.TASK_ALLEGRO_HAND)
    with pytest.raises(NotImplementedError, match=f"task {HM.TASK_ALLEGRO_HAND} "):
        gym_api.Gym().apply_rigid_body_force_tensors(sim, None, torch.zeros(3), gym_api.gymapi.ENV_SPACE)
    assert gym_api.Gym().apply_rigid_body_force_tensors(sim, None, None, gym_api.gymapi.ENV_SPACE) is True
