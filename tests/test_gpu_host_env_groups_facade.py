"""The C++ facade's env groups (PPO_HostEnv::setEnvGroups / `env_groups` in PPOConfig.toml) on the GPU: host/tests/host_env_groups_test trains
PPO_HostEnv<CartPole> with 1, 2 and 3 groups in a fresh directory; the three runs must agree in every statistic, table line, parameter and AdamW moment."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_env_groups_test")


def test_host_env_groups_facade(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_env_groups_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_env_groups_test ok" in r.stdout
    assert "rollout/" in r.stdout   # the console table printed
