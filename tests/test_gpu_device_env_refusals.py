"""The context-level refusals of the fused device envs, word for word (ppo-libtorch_amd/csrc/api.hip: envt_state, ppo_evaluate, ppo_env_step,
ppo_env_step_f32, ppo_rollout, ppo_env_set_state_h).  tests/golden/device_env_refusals.json holds the answer of every call of tests/refusal_grid.py's
device_env_cases as the library gave it when the file was recorded (tools/record_device_env_refusals.py): one context per env kind at N = 8, T = 4, no rollout."""
import json
import os

import pytest

from __graft_entry__ import load_package

import refusal_grid as G

pytestmark = pytest.mark.gpu


def test_every_recorded_answer_is_given_again(golden_dir):
    P = load_package()
    with open(os.path.join(golden_dir, "device_env_refusals.json")) as f:
        want = json.load(f)
    # the file is whole: every env kind's state shape, both truncation calls and the wrong-action-type step; a status-1 answer per checked state word
    for name, _, state in G.fused_envs(P).values():
        assert want["%s state_shape" % name] == "%s want %s" % ([8, state], [8, state]), name
        assert "%s truncation_bootstrap" % name in want and "%s truncations" % name in want, name
        assert ("%s env_step" % name in want) != ("%s env_step_f32" % name in want), name
    assert sum(" set_state " in k and v.startswith("PPOError: ppo_hip status 1: ppo_env_set_state_h: state[5]") for k, v in want.items()) == 4 + 4 + 4 + 6
    assert want["PPO_ENV_PENDULUM evaluate"].startswith("PPOError: ppo_hip status 5: ppo_evaluate is not built for PPO_ENV_PENDULUM")
    got = G.device_env_cases(P)
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    wrong = [(k, got[k], want[k]) for k in want if got[k] != want[k]]
    assert not wrong, "%d of %d differ; first: %r" % (len(wrong), len(want), wrong[0])
