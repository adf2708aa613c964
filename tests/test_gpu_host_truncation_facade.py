"""The C++ facade's `bootstrap_truncated` (PPO_HostEnv::setBootstrapTruncated / the key in [environment] of PPOConfig.toml) on the GPU:
host/tests/host_env_test's `truncation` mode, run in a fresh directory.  PPO_HostEnv<CartPole>, 16 envs x 32 steps, max_episode_steps 20, 3 updates:
with the key absent it ends with PPO_Discrete's parameters; with it on, every rollout's ppo_host_truncations are the time-limit ends the envs counted
themselves, PPO_BUF_REWARDS differs from the reward CartPole paid (1.0; -1.0 where the pole fell) exactly there, and 2 env groups end with the parameters of 1."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_env_test")


def test_host_truncation_facade(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_env_test"])
    r = subprocess.run([EXE, "truncation"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_env_test truncation ok" in r.stdout
    assert "Using config file bootstrap_truncated = true" in r.stdout
