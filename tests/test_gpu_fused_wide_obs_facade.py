"""`wide_obs = true` in [environment] of the C++ facade (PPO_KERNEL_FUSED_WIDE_OBS) on the GPU: host/tests/host_wide_obs_test in a fresh directory.
PPO_HostEnvBox at obs_size 100 with fused_policy and the key trains one iteration on the fused kernels and prints the key; without the key the library's
"obs_size <= 64" refusal is thrown."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_wide_obs_test")


def test_wide_obs_key(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_wide_obs_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_wide_obs_test ok" in r.stdout
    assert "refusal:" in r.stdout and "fused launches: act" in r.stdout
