"""`keep_cut_states = true` in [environment] of the C++ facade (PPO_KERNEL_ENV_CUT_STATE; include/ppo_hip.h) on the GPU: host/tests/host_cut_state_test in a
fresh directory.  PPO_Continuous (Pendulum) and PPO_DiscreteAcrobot, whose envs refuse bootstrap_truncated without the key, train two iterations with both keys
set, ppo_env_truncations reports events, the checkpoint loads into a fresh object with bit-equal parameters; the same file without keep_cut_states throws the
library's existing refusal, and PPO_Discrete refuses the key with the library's message."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_cut_state_test")


def test_keep_cut_states_through_the_facade(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), "host_cut_state_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_cut_state_test ok" in r.stdout
    for name in ("PPO_Continuous", "PPO_DiscreteAcrobot"):
        assert "%s: " % name in r.stdout and "truncation events in the last rollout" in r.stdout
    assert "PPO_Continuous without keep_cut_states: " in r.stdout and "does not hold theta" in r.stdout
    assert "PPO_DiscreteAcrobot without keep_cut_states: " in r.stdout and "does not hold the angles" in r.stdout
    assert "PPO_Discrete with keep_cut_states: " in r.stdout and "PPO_KERNEL_ENV_CUT_STATE" in r.stdout
