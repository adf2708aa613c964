"""`hidden_size = 128` in [network] of the C++ facade on a caller-stepped Gaussian class, on the GPU: host/tests/host_fused_h128_test in a fresh directory.
PPO_HostEnvBox at obs_size 100 with fused_policy, wide_obs, matrix_cores and the key builds a 2 x 128 context without PPO_KERNEL_ENV_GENERIC and trains one
iteration on the fused kernels."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_fused_h128_test")


def test_hidden_size_key_on_a_host_env_class(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.dirname(EXE)])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_fused_h128_test ok" in r.stdout and "fused launches: act" in r.stdout
