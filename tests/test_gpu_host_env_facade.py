"""The C++ facade's PPO_HostEnv<Env> (ppo-libtorch_amd/host/PPO/PPO_HostEnv.h) on the GPU: host/tests/host_env_test, one mode per run in a fresh directory.
PPO_HostEnv<CartPole> is the reference's own configuration (its CartPoles in m_envs, stepped on the thread pool) and must train exactly as PPO_Discrete."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_env_test")


@pytest.mark.parametrize("mode", ["parity", "width", "resume"])
def test_host_env_facade(mode, tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_env_test"])
    r = subprocess.run([EXE, mode], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert ("host_env_test %s ok" % mode) in r.stdout
    if mode == "parity":
        assert "rollout/" in r.stdout   # the console table printed
