"""PPO_DiscreteFrozenLake of the C++ facade (a categorical policy on the device's slippery FrozenLake, PPO_ENV_FROZENLAKE / PPO_ENV_FROZENLAKE8X8) on the GPU:
host/tests/host_frozenlake_test in a fresh directory.  Two iterations train on the 4x4 map, the rollout is none of the act launches, evaluate(8) returns
ppo_evaluate's numbers on the same context and prints nothing, the checkpoint loads into a fresh object with bit-equal parameters, setBootstrapTruncated(true)
throws the library's refusal, obs_size = 64 picks the 8x8 env kind, and the host-side FrozenLake class -- which computes on the CPU, its own Philox included --
steps every (cell, action) pair x 12 step counts x two keys of both maps to the numbers of ppo_env_transition."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_frozenlake_test")


def test_ppo_discrete_frozenlake(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_frozenlake_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_frozenlake_test ok" in r.stdout
    assert "fused launches: act 0 " in r.stdout
    assert "evaluate: return mean" in r.stdout
    assert "bootstrap_truncated: " in r.stdout and "holds neither the step count nor the key" in r.stdout
    assert "host FrozenLake against ppo_env_transition: 0 of 7680 rows differ" in r.stdout
