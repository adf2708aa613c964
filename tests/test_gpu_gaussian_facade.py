"""The C++ facade's PPO_HostEnvBox<Env> (ppo-libtorch_amd/host/PPO/PPO_HostEnvBox.h) on the GPU: host/tests/host_gaussian_test in a fresh directory.  A Box
env of D = 3 trains two iterations from a TOML with action_dim = 3, norm_obs = true and norm_reward = true, saves, loads into a fresh object with bit-equal
parameters (log_std included), and throws the library's message on env_groups = 2."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_gaussian_test")


def test_box_env_facade(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_gaussian_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_gaussian_test ok" in r.stdout
    assert "refusal:" in r.stdout and "log_std after 2 updates" in r.stdout
