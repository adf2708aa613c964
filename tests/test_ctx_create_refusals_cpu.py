"""ppo_ctx_create's refusals, word for word (ppo-libtorch_amd/csrc/api.hip).  tests/golden/ctx_create_refusals.json holds status and message of every config
of the grid (tests/refusal_grid.py: the accepted form of each env_kind 0..14, every single perturbation of it and every pair) that the library refused with
PPO_ERR_INVALID or PPO_ERR_UNSUPPORTED when the file was recorded (tools/record_ctx_create_refusals.py).  A refused config is answered before the device is
touched, so this needs no GPU: an accepted config ends at hipSetDevice with status 2 on a machine without one, and is a live context, closed at once, on a machine with one."""
import json
import os

import pytest

from __graft_entry__ import load_package

import refusal_grid as G


@pytest.fixture(scope="module")
def P():
    return load_package()


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "ctx_create_refusals.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def answers(P):
    return G.ctx_create_cases(P)


def test_fixture_covers_every_fused_env(P, recorded):
    """an empty or thinned file cannot pass: per fused kind at least six distinct messages of its own block, and the observation-size message of its width"""
    messages = {g["message"] for g in recorded}
    for name, obs, _ in G.fused_envs(P).values():
        own = {m for m in messages if m.startswith("env_kind = %s " % name)}
        assert len(own) >= 6, (name, sorted(own))
        assert any(m.startswith("The environment returned an observation of size %d," % obs) for m in messages), name
    assert len(by_case_ids(recorded)) == sum(len(g["cases"]) for g in recorded), "a case is recorded twice"
    assert all(g["status"] in (1, 5) for g in recorded)


def by_case_ids(recorded):
    return {case for g in recorded for case in g["cases"]}


def test_every_recorded_refusal_is_answered_the_same(recorded, answers):
    want = G.by_case(recorded)
    assert set(want) <= set(answers), sorted(set(want) - set(answers))[:5]
    wrong = [(case, answers[case], want[case]) for case in want if answers[case] != want[case]]
    assert not wrong, "%d of %d differ; first: %r" % (len(wrong), len(want), wrong[0])


def test_no_other_config_is_refused(recorded, answers):
    want = G.by_case(recorded)
    extra = [(case, a) for case, a in answers.items() if a[0] in (1, 5) and case not in want]
    assert not extra, "%d configs outside the file are refused; first: %r" % (len(extra), extra[0])
    assert all(a[0] in (0, 2) for case, a in answers.items() if case not in want), "an accepted config is a context, or ends at hipSetDevice (status 2)"
