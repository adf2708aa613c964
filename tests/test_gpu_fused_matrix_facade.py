"""`matrix_cores = true` in [environment] of the C++ facade (PPO_KERNEL_FUSED_MATRIX) on the GPU: host/tests/host_matrix_cores_test in a fresh directory.
PPO_Discrete with the key throws the library's refusal naming the flag; PPO_HostEnvBox at obs_size 100 with fused_policy, wide_obs and the key trains one
iteration on the fused kernels and prints the key."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_matrix_cores_test")


def test_matrix_cores_key(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.dirname(EXE)])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_matrix_cores_test ok" in r.stdout
    assert "refusal: " in r.stdout and "PPO_KERNEL_FUSED_MATRIX" in r.stdout and "fused launches: act" in r.stdout
