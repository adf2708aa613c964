"""`matrix_cores = true` in [environment] of the C++ facade on a fused device-env class (PPO_KERNEL_ENV_MATRIX; include/ppo_hip.h) on the GPU:
host/tests/host_env_matrix_test in a fresh directory.  PPO_MultiDiscreteTaxi reads the key, its context carries the flag next to its family flag, one iteration
trains, and bootstrap_truncated beside the key throws the library's refusal naming the flag."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_env_matrix_test")


def test_matrix_cores_on_a_device_env_class(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_env_matrix_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_env_matrix_test ok" in r.stdout and "fused launches act" in r.stdout
    assert "refusal: " in r.stdout and "PPO_KERNEL_ENV_MATRIX" in r.stdout
