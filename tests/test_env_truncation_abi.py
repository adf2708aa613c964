"""Time-limit truncations of the library's own environments (include/ppo_hip.h: ppo_env_truncation_bootstrap / ppo_env_truncations) without a GPU:
the header declares the two calls and states their contract, and the binding lists and wraps them."""
import inspect
import os
import re

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ppo_hip.h")
CALLS = ["ppo_env_truncation_bootstrap", "ppo_env_truncations"]


def header():
    return open(HDR).read()


def block(src):
    """the comment block in front of ppo_env_truncation_bootstrap, as one line of single-spaced text"""
    end = src.index("PPO_API ppo_status ppo_env_truncation_bootstrap")
    start = src.rindex("/* Time-limit truncations of the context's own environments", 0, end)
    return re.sub(r"[\s*]+", " ", src[start:end])


def test_header_declares_the_calls():
    src = header()
    assert re.search(r"#define PPO_ABI_VERSION 5\b", src)   # additions only
    assert re.search(r"PPO_API\s+ppo_status\s+ppo_env_truncation_bootstrap\s*\(\s*ppo_ctx\s*\*\s*\w+\s*,\s*int32_t\s+on\s*\)", src)
    assert re.search(r"PPO_API\s+ppo_status\s+ppo_env_truncations\s*\(\s*ppo_ctx\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*count\s*,\s*int32_t\s*\*\s*index_h\s*,"
                     r"\s*float\s*\*\s*value_h\s*,\s*int64_t\s+cap\s*\)", src)


def test_header_states_the_contract():
    text = block(header())
    assert "PPO_Discrete.cpp:443-452" in text                     # what the reference does
    assert "Off by default" in text and "launch for launch and bit for bit" in text
    assert "ONE more launch" in text
    # who sees which reward
    assert "FIN_REW, EP_REW, the episode ring and every episode statistic keep the raw reward" in text
    assert "ppo_evaluate is untouched" in text
    # the three error classes
    assert "PPO_ERR_UNSUPPORTED on a PPO_ENV_SYNTHETIC context" in text
    assert "PPO_ENV_HOST context (the message names ppo_host_observe_truncated)" in text
    assert "PPO_ERR_INVALID for `on` outside 0..1" in text
    assert "A failing call changes nothing" in text
    # the memory line of ppo_ctx_create
    src = re.sub(r"[\s*]+", " ", header())
    assert "the event list of ppo_env_truncation_bootstrap (num_steps num_envs entries plus a counter), allocated by the first enable and kept" in src


def test_binding_lists_and_wraps_the_calls():
    P = load_package()
    for name in CALLS:
        assert name in P.binding.ABI_SYMBOLS, name
    assert len(P.binding.ABI_SYMBOLS) == len(set(P.binding.ABI_SYMBOLS))
    assert inspect.signature(P.Context.env_truncation_bootstrap).parameters["on"].default is True
    assert callable(P.Context.env_truncations)
