"""bench.py's two modes and its output dump, without a GPU: main() runs against a stand-in for the HIP package (a context that counts
iterations and hands back fixed arrays), so what is checked is the benchmark's own control flow -- a plain run prints the headline line
only, --full adds the legs that take runs of their own or quote the committed profile set, and --dump-outputs writes the same arrays in
both modes, a fixed sample of each array above DUMP_CAP elements, within 64 MB."""
import json
import os
import sys
import types

import numpy as np
import pytest

import __graft_entry__
import bench

FULL_ONLY = ("value_runs", "other_workloads", "gae_roofline", "cpu_baseline", "profiles")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")


class FakeContext:
    def __init__(self, cfg):
        self.cfg, self.P, self.iterations = cfg, 9155, 0

    def init_orthogonal(self, seed):
        pass

    def env_reset(self):
        pass

    def sync(self):
        pass

    def train_iteration(self):
        self.iterations += 1

    def profile_enable(self, on):
        pass

    def profile_read(self):
        return dict(fwd_bwd_launches=5, gae_launches=1, rollout_launches=1, optimizer_launches=0, reduce_launches=0, fwd_bwd_ms=0.2, gae_ms=0.005,
                    rollout_ms=0.1, optimizer_ms=0.0, reduce_ms=0.0, allreduce_launches=0, allreduce_ms=0.0)

    def stats(self):
        return dict(pg_loss=0.1, v_loss=1.0, entropy_loss=0.5, approx_kl=0.0, loss=1.0, clipfrac_last=0.0, clipfrac_mean=0.0, total_norm=1.0,
                    explained_variance=0.1, learning_rate=1e-3, ep_len_mean=20.0, ep_rew_mean=20.0, ep_count=3, global_step=self.iterations,
                    optimizer_steps=40, updates=self.iterations)

    def close(self):
        pass

    def get_params(self):
        return np.arange(self.P, dtype=np.float32) * np.float32(self.iterations)

    def get_optimizer(self):
        return np.ones(self.P, np.float32), np.full(self.P, 2, np.float32), self.iterations

    def read(self, name):
        n = self.cfg["envs"] * self.cfg["num_steps"] * (self.cfg["obs_size"] if name == "OBS" else 1)
        return np.arange(n, dtype=np.int32 if name == "ACTIONS" else np.float32)

    def buffer_ptr(self, name):
        return 0, 0

    def dev(self, host):
        return host

    def empty(self, shape, dtype):
        return np.zeros(shape, dtype)


@pytest.fixture
def run_bench(monkeypatch):
    fake = types.SimpleNamespace(ENV_CARTPOLE=0, ENV_MOUNTAINCAR=1, ENV_SYNTHETIC=2, DIST_CATEGORICAL=0, DIST_MASKED=1, DTYPE_F32=0, DTYPE_BF16=1,
                                 KERNEL_UPDATE_VECTOR=2, KERNEL_COMM_SELFTEST=8, Context=FakeContext, make_config=None,
                                 gae_launch=lambda *a, **k: None)
    fake.dist = types.SimpleNamespace(shard_config=lambda make, rank, world, n, **kw: dict(kw, envs=n // world))
    monkeypatch.setattr(__graft_entry__, "load_package", lambda: fake)
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a: {"value": 1.0, "unit": "env-steps/s", "kind": "port"})
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    def run(capsys, *argv):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
        bench.main()
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        return json.loads(lines[0])
    return run


def test_plain_run_prints_the_headline_only_and_full_adds_the_other_legs(run_bench, capsys, tmp_path):
    plain = run_bench(capsys, "--gpus", "1", "--steps", "20", "--warmup", "2", "--dump-outputs", str(tmp_path / "plain"))
    full = run_bench(capsys, "--gpus", "1", "--steps", "20", "--warmup", "2", "--full", "--dump-outputs", str(tmp_path / "full"))
    for line, iterations in ((plain, 2 + 20), (full, 2 + 20 + 5 * 20)):   # --full's statistics are read after its five repeated regions
        assert all(k in line for k in HEADLINE) and line["steps"] == 20 and line["warmup"] == 2
        assert line["train_stats"]["global_step"] == iterations and "roofline" in line
    assert [k for k in FULL_ONLY if k in plain] == [] and "traffic" not in plain["roofline"]
    assert all(k in full for k in FULL_ONLY) and "traffic" in full["roofline"] and full["value_runs"]["runs"] == 6
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) and "params.npy" in names and "stats.npy" in names
    for n in names:   # dumped right after the headline's K steps: the repeats of --full come later
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    assert np.array_equal(np.load(tmp_path / "plain" / "params.npy"), np.arange(9155, dtype=np.float32) * 22)


def test_large_arrays_are_dumped_as_a_fixed_sample_within_64_mb(tmp_path):
    n = 3 * bench.DUMP_CAP + 7
    ctx = FakeContext(dict(envs=n, num_steps=1, obs_size=1))
    for d in ("a", "b"):
        bench.dump_outputs(ctx, str(tmp_path / d))
    total = 0
    for f in sorted(os.listdir(tmp_path / "a")):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.size <= bench.DUMP_CAP and np.array_equal(a, b), f
        total += os.path.getsize(tmp_path / "a" / f)
    rewards = np.load(tmp_path / "a" / "rewards.npy")     # arange: the values are the sampled positions, sorted and distinct
    assert rewards.size == bench.DUMP_CAP and np.all(np.diff(rewards) > 0) and rewards[-1] < n
    assert total <= 64 * 2 ** 20


def test_parse_args_defaults_to_a_plain_run():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "1", "--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
