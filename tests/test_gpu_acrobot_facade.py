"""PPO_DiscreteAcrobot of the C++ facade (a categorical policy on the device's Acrobot-v1, PPO_ENV_ACROBOT) on the GPU: host/tests/host_acrobot_test in a
fresh directory.  Two iterations train and the rollout is none of the act launches, evaluate(8) returns ppo_evaluate's numbers on the same context and prints
nothing, the checkpoint loads into a fresh object with bit-equal parameters, bootstrap_truncated = true throws the library's refusal, and the host-side
Acrobot class -- which computes on the CPU -- steps 64 states, the 16 corners of the state box under each action among them, to the bits of
ppo_env_transition."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_acrobot_test")


def test_ppo_discrete_acrobot(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_acrobot_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_acrobot_test ok" in r.stdout
    assert "fused launches: act 0 " in r.stdout
    assert "evaluate: return mean" in r.stdout
    assert "bootstrap_truncated: " in r.stdout and "does not hold the angles" in r.stdout
    assert "host Acrobot against ppo_env_transition: 0 of 64 rows differ" in r.stdout
