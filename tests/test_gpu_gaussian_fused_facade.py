"""`fused_policy = true` in [environment] of the C++ facade (PPO_KERNEL_GAUSS_FUSED) on the GPU: host/tests/host_gaussian_fused_test in a fresh directory.
PPO_HostEnvBox trains two iterations on the fused Gaussian kernels (non-zero launch counters), saves, loads into a fresh object with bit-equal parameters;
PPO_HostEnv with the key throws the library's message."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_gaussian_fused_test")


def test_fused_policy_key(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_gaussian_fused_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_gaussian_fused_test ok" in r.stdout
    assert "refusal:" in r.stdout and "fused launches: act" in r.stdout
