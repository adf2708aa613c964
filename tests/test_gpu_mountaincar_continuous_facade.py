"""PPO_ContinuousMountainCar of the C++ facade (a Gaussian policy on the device's MountainCarContinuous-v0, PPO_ENV_MOUNTAINCAR_CONTINUOUS) on the GPU:
host/tests/host_mcc_test in a fresh directory.  Two iterations train with bootstrap_truncated = true and a small time limit, ppo_env_truncations reports a
positive count, evaluate(8) returns ppo_evaluate's numbers on the same context and prints nothing, the checkpoint loads into a fresh object with bit-equal
parameters, and the host-side MountainCarContinuous class steps a raw action of 5 as ppo_env_transition_f32 does (clipped force, raw penalty)."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_mcc_test")


def test_ppo_continuous_mountaincar(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_mcc_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_mcc_test ok" in r.stdout
    assert "fused launches: act 0 " in r.stdout
    events = re.search(r"truncation events: (\d+)", r.stdout)
    assert events and int(events.group(1)) > 0
    assert "evaluate: return mean" in r.stdout
