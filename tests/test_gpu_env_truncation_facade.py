"""The C++ facade's `bootstrap_truncated` on the classes that own their envs (PPO_Discrete::setBootstrapTruncated / the key in [environment] of
PPOConfig.toml) on the GPU: host/tests/env_truncation_test, run in a fresh directory.  16 envs x 32 steps, max_episode_steps 20, 3 updates: with the key
PPO_Discrete ends with the statistics, parameters and AdamW moments of PPO_HostEnv<CartPole> with the same key, bit for bit, and reports events; without
it -- or with setBootstrapTruncated(false) -- it trains as before and prints nothing about the key."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "env_truncation_test")


def test_env_truncation_facade(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "env_truncation_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "env_truncation_test ok" in r.stdout
    assert "Using config file bootstrap_truncated = true" in r.stdout
