"""PPO_MultiDiscreteTaxi of the C++ facade (a masked categorical policy on the device's Taxi-v3, PPO_ENV_TAXI) on the GPU: host/tests/host_taxi_test in a
fresh directory.  Constructed from a TOML with bootstrap_truncated = true, two iterations train, the rollout is none of the act launches and the fold finds
time-limit ends, the stored masks allow every stored action, evaluate(8) returns ppo_evaluate's numbers on the same context and prints nothing, the
checkpoint loads into a fresh object with bit-equal parameters, and the host-side Taxi class -- which computes on the CPU -- steps all 500 x 6 (state,
action) pairs to the numbers of ppo_env_transition."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_taxi_test")


def test_ppo_multidiscrete_taxi(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_taxi_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_taxi_test ok" in r.stdout
    assert "fused launches: act 0 " in r.stdout
    assert "truncation events of the last rollout: " in r.stdout
    assert "evaluate: return mean" in r.stdout
    assert "host Taxi against ppo_env_transition: 0 of 3000 rows differ; 1392 allowed pairs" in r.stdout
