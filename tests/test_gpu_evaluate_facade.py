"""evaluate() of the C++ facade on the GPU (ppo-libtorch_amd/host/PPO/PPOAlgorithm.h, PPO_HostEnv.h, Agent.h): host/tests/host_eval_test, one mode per run
in a fresh directory.  PPO_Discrete::evaluate gives ppo_evaluate's numbers and disturbs neither the console nor training; PPO_HostEnv<CartPole>::evaluate on
fresh CartPole(1000 + e) envs reproduces, per episode, the device evaluation started from the same reset stream."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_eval_test")


@pytest.mark.parametrize("mode", ["discrete", "hostenv"])
def test_facade_evaluate(mode, tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_eval_test"])
    r = subprocess.run([EXE, mode], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert ("host_eval_test %s ok" % mode) in r.stdout
