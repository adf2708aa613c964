"""Early stop at a target KL: the C-ABI's three calls as the header declares them and the binding exposes them (no GPU).  The behaviour is
tests/test_gpu_target_kl.py's."""
import os
import re

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ppo_target_kl_set", "ppo_target_kl_get", "ppo_early_stop_read")


def header():
    with open(os.path.join(ROOT, "include", "ppo_hip.h")) as f:
        return f.read()


def test_header_declares_the_three_calls():
    h = header()
    assert re.search(r"PPO_API ppo_status ppo_target_kl_set\(ppo_ctx\* ctx, double target_kl\);", h)
    assert re.search(r"PPO_API ppo_status ppo_target_kl_get\(ppo_ctx\* ctx, double\* out\);", h)
    assert re.search(r"PPO_API ppo_status ppo_early_stop_read\(ppo_ctx\* ctx, int32_t\* epochs_run, int32_t\* stopped, double\* kl_at_stop, "
                     r"int64_t\* epochs_total\);", h)
    assert re.search(r"#define PPO_ABI_VERSION 5\b", h)


def test_header_block_states_the_contract():
    h = header()
    block = h[h.index("Early stop at a target KL"):h.index("ppo_early_stop_read(ppo_ctx*")]
    assert "off is off" in block
    assert "PPO_Discrete.cpp:567-644" in block and ":352" in block      # the reference's epoch loop and its estimator
    assert "PPO_ERR_INVALID" in block and "NaN compares" in block
    assert "NOT built" in block                                           # the forward / backward launches of unapplied steps still run


def test_binding_exposes_them():
    P = load_package()
    for name in CALLS:
        assert name in P.binding.ABI_SYMBOLS
    for name in ("target_kl_set", "target_kl_get", "early_stop"):
        assert callable(getattr(P.Context, name))
    assert P.binding.ABI_VERSION == 5
