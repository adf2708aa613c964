"""`fused_categorical = true` in [environment] of the C++ facade (PPO_KERNEL_CAT_FUSED) on the GPU: host/tests/host_cat_fused_test in a fresh directory.
PPO_HostEnv trains two iterations on the fused categorical kernels (the key is printed, the context carries the flag, the statistics are finite, the launch
counters are non-zero), saves, and the checkpoint loads into an object without the key with bit-equal parameters; with the key absent nothing is said and no
flag is set."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_cat_fused_test")


def test_fused_categorical_key(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_cat_fused_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_cat_fused_test ok" in r.stdout
    assert "fused launches: act" in r.stdout
