"""bench.py --dump-outputs and the lean / --full split.

--dump-outputs DIR writes what the last timed VecTask.step() returned as DIR/<name>.npy (float32 / float64, at most
64 MB in all, a seeded row sample of anything larger; an env whose values are not finite is written as zeros and
flagged in env_finite.npy). A plain run times the headline config alone; sub-records, CPU
baselines and episode windows need --full. The CPU tests cover the writer; the GPU test runs one small plain bench."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _step_return(n=6):
    import torch
    obs = torch.arange(n * 4, dtype=torch.float32).reshape(n, 4)
    extras = {"time_outs": torch.tensor([True, False] * (n // 2)), "successes": torch.tensor(0.5),
              "rewards_episode": {"lifting_rew": torch.ones(n)}, "scalars": {"success_tolerance": 0.075},
              "success_rate_ewma/overall": 0.25, "note": "not an array"}
    return ({"obs": obs, "states": torch.zeros(n, 4)}, torch.ones(n), torch.arange(n, dtype=torch.int64) % 2, extras)


def test_dump_outputs_names_and_dtypes(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    ret = _step_return()
    assert bench.dump_outputs(ret, str(tmp_path / "d")) == 0
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    np.testing.assert_array_equal(got.pop("env_finite"), np.ones(6))
    assert sorted(got) == ["extras.rewards_episode.lifting_rew", "extras.scalars.success_tolerance",
                           "extras.success_rate_ewma_overall", "extras.successes", "extras.time_outs", "obs.obs",
                           "obs.states", "reset", "rew"]
    assert got["obs.obs"].dtype == np.float32 and got["rew"].dtype == np.float32
    np.testing.assert_array_equal(got["obs.obs"], ret[0]["obs"].numpy())
    assert got["reset"].dtype == np.float64 and got["extras.time_outs"].dtype == np.float64
    np.testing.assert_array_equal(got["reset"], [0, 1, 0, 1, 0, 1])
    np.testing.assert_array_equal(got["extras.time_outs"], [1, 0, 1, 0, 1, 0])
    assert got["extras.scalars.success_tolerance"].dtype == np.float64
    assert got["extras.scalars.success_tolerance"].item() == 0.075 and got["extras.successes"].item() == 0.5


def test_dump_outputs_zeroes_and_flags_an_env_with_non_finite_values(tmp_path):
    """A diverged env (NaN / inf in any per-env array) is written as zeros in every per-env array and flagged in
    env_finite; the other envs and the caller's tensors stay as they are."""
    sys.path.insert(0, ROOT)
    import bench
    ret = _step_return()
    ret[1][2] = float("nan")                                          # rew of env 2
    ret[3]["rewards_episode"]["lifting_rew"][4] = float("-inf")       # an episode sum of env 4
    ref_obs = ret[0]["obs"].numpy().copy()
    assert bench.dump_outputs(ret, str(tmp_path / "d")) == 2
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    np.testing.assert_array_equal(got["env_finite"], [1, 1, 0, 1, 0, 1])
    assert all(np.isfinite(a).all() for a in got.values())
    want = ref_obs.copy()
    want[[2, 4]] = 0
    np.testing.assert_array_equal(got["obs.obs"], want)
    np.testing.assert_array_equal(got["rew"], [1, 1, 0, 1, 0, 1])
    np.testing.assert_array_equal(got["reset"], [0, 1, 0, 1, 0, 1])
    np.testing.assert_array_equal(got["extras.time_outs"], [1, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(got["extras.rewards_episode.lifting_rew"], [1, 1, 0, 1, 0, 1])
    assert got["extras.successes"].item() == 0.5                      # not per env: untouched
    np.testing.assert_array_equal(ret[0]["obs"].numpy(), ref_obs)     # the task's own buffers are not written
    assert np.isnan(ret[1][2].item())


def test_dump_outputs_samples_the_same_rows_under_the_budget(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 3 * 160)        # three arrays: a share of 160 B each
    big = torch.arange(100 * 5, dtype=torch.float32).reshape(100, 5)    # 2000 B, 20 B per row -> 8 rows
    ret = ({"obs": big}, torch.ones(7), None, {})
    bench.dump_outputs(ret, str(tmp_path / "a"))
    bench.dump_outputs(ret, str(tmp_path / "b"))
    a, b = np.load(tmp_path / "a" / "obs.obs.npy"), np.load(tmp_path / "b" / "obs.obs.npy")
    assert a.shape == (8, 5) and a.nbytes + 7 * 4 + 7 * 8 <= 3 * 160
    np.testing.assert_array_equal(a, b)
    rows = (a[:, 0] / 5).astype(int)
    assert (np.diff(rows) > 0).all()                                 # distinct rows, in order
    np.testing.assert_array_equal(a, big.numpy()[rows])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "rew.npy"), np.ones(7, np.float32))   # under its share: whole


@pytest.mark.gpu
def test_plain_bench_is_the_headline_alone_and_dumps_its_last_step(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    d = tmp_path / "dump"
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--envs", "256", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 2 and out["config"]["envs_per_gpu"] == 256
    assert out["ms_per_step"] > 0 and out["unit"] == "env-steps/s" and out["higher_is_better"] is True
    assert abs(out["value"] - 256 * 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]
    assert out["cpu_baseline"] is None and "configs" not in out and "episode_window" not in out    # --full only
    obs, rew, reset = (np.load(d / f) for f in ("obs.obs.npy", "rew.npy", "reset.npy"))
    assert obs.shape == (256, 99) and obs.dtype == np.float32 and np.isfinite(obs).all() and np.abs(obs).max() <= 10.0
    assert np.abs(obs).max() > 0
    assert rew.shape == (256,) and rew.dtype == np.float32 and np.isfinite(rew).all()
    assert reset.shape == (256,) and set(np.unique(reset)) <= {0.0, 1.0}
    ok = np.load(d / "env_finite.npy")
    assert ok.shape == (256,) and out["dump_non_finite_envs"] == int((ok == 0).sum())
    for f in os.listdir(d):
        a = np.load(d / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 * 1000 * 1000
