"""Truncation flags in ppo_dev_observe on the fused 2 x 64 families, without a GPU: nothing was added to the surface (ABI version 5, 92 symbols), and the header
says who is served -- the ppo_dev_* block and the two kernel-flag entries name the fused families, and the sentence that refused them is gone."""
import inspect
import os
import re

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()


def flat(text):
    """the comment's words without its line structure"""
    return re.sub(r"\s+", " ", re.sub(r"\n\s*\*", " ", text))


def test_abi_version_and_symbols_are_unchanged():
    P = load_package()
    assert re.search(r"#define\s+PPO_ABI_VERSION\s+5\b", HEADER)
    assert P.binding.lib().ppo_abi_version() == 5 == P.binding.ABI_VERSION
    assert len(P.binding.ABI_SYMBOLS) == len(set(P.binding.ABI_SYMBOLS)) == 92
    assert len(re.findall(r"^PPO_API\s", HEADER, re.M)) == 92
    params = inspect.signature(P.Context.dev_observe).parameters
    assert "truncated" in params and "final_obs" in params


def test_dev_block_names_the_fused_families_as_served():
    block = flat(HEADER[HEADER.index("/* Caller-stepped environments on the device"):HEADER.index("PPO_API ppo_status ppo_dev_env_reset")])
    served = block[block.index("The fused families"):block.index("The plain generic engine")]
    for words in ("PPO_KERNEL_GAUSS_FUSED", "PPO_KERNEL_CAT_FUSED", "take the flags", "gauss_values_kernel", "gauss_dev_fold_kernel", "ppo_get_value's bit for bit",
                  "two with `truncated`", "ppo_gauss_fused_launches"):
        assert words in served, words
    refused = block[block.index("The plain generic engine"):]
    assert "PPO_ERR_UNSUPPORTED" in refused and "ppo_bootstrap_rewards" in refused


def test_kernel_flag_entries_name_the_fold():
    flags = HEADER[HEADER.index(" *   PPO_KERNEL_GAUSS_FUSED      dist_kind"):HEADER.index("enum { PPO_KERNEL_ROLLOUT_VECTOR")]
    gauss = flat(flags[:flags.index(" *   PPO_KERNEL_SEPARATE_LAUNCHES")])
    cat = flat(flags[flags.index(" *   PPO_KERNEL_CAT_FUSED"):])
    for entry in (gauss, cat):
        assert "runcation flags in ppo_dev_observe are served" in entry and "gauss_dev_fold_kernel" in entry, entry
    assert "ppo_evaluate stays refused" in cat
    assert "truncation flags in ppo_dev_observe stay refused" not in flat(HEADER)
    counters = flat(HEADER[HEADER.index("/* Host-side counts, since the context's creation"):HEADER.index("PPO_API ppo_status ppo_gauss_fused_launches")])
    assert "ppo_dev_observe that passes `truncated` adds 1 to `value`" in counters
