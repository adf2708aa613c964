"""`[network] hidden_size = H` of the C++ facade (PPO_KERNEL_ENV_GENERIC) on the GPU: host/tests/host_env_generic_test in a fresh directory.  PPO_Discrete and
PPO_MultiDiscrete train two iterations at 2 x 128 (the key is printed, the context carries the flag and the width, the statistics are finite), save, and the
checkpoint loads into a fresh object with bit-equal parameters; with the key absent nothing is said, the context's kernel_flags lacks the bit and the
network is the reference's."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_env_generic_test")


def test_hidden_size_key(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_env_generic_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_env_generic_test ok" in r.stdout
    assert "PPO_Discrete: hidden_size = 128 trained 2 updates" in r.stdout and "PPO_MultiDiscrete: hidden_size = 128 trained 2 updates" in r.stdout
