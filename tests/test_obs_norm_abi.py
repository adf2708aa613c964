"""Observation normalisation of caller-stepped environments (include/ppo_hip.h, "Observation normalisation": ppo_obs_norm_enable / ppo_obs_norm_get_h /
ppo_obs_norm_set_h / ppo_obs_norm_apply) without a GPU: the header declares the four calls in a block behind the ppo_dev_* block and the ABI version is
unchanged, the binding lists them and has the Context methods with the documented parameters, the built library exports them, and the device calls
still only enqueue.  tests/test_gpu_obs_norm.py runs them."""
import inspect
import os
import re
import subprocess

from __graft_entry__ import ROOT, load_package

HDR = os.path.join(ROOT, "include", "ppo_hip.h")
CALLS = ["ppo_obs_norm_enable", "ppo_obs_norm_get_h", "ppo_obs_norm_set_h", "ppo_obs_norm_apply"]


def test_header_declares_the_normaliser_calls():
    src = open(HDR).read()
    assert re.search(r"#define PPO_ABI_VERSION 5\b", src)   # additions only
    for name in CALLS:
        assert re.search(r"PPO_API\s+ppo_status\s+%s\s*\(" % name, src), name
    # the block sits behind the ppo_dev_* block and in front of the evaluation section
    start = src.index("Observation normalisation of caller-stepped environments")
    assert src.index("PPO_API ppo_status ppo_dev_observe(ppo_ctx") < start < src.index("PPO_API ppo_status ppo_evaluate(")
    for name in CALLS:
        assert src.index("PPO_API ppo_status %s(" % name) > start, name
    block = src[start:src.index("PPO_API ppo_status ppo_obs_norm_apply(")]
    # the semantics, the launch count, where the two feeds differ, and the refusals are stated
    for phrase in ("mean = 0, var = 1, count = 0", "delta = bm - mean", "sqrt(var + eps)", "ONE more per env step", "WITHOUT updating the statistics",
                   "ppo_host_rollout_end", "ppo_bootstrap_rewards", "ppo_host_rollout_begin_groups", "PPO_ERR_UNSUPPORTED", "PPO_ERR_STATE",
                   "PPO_ERR_INVALID", "fp16 ranges"):
        assert phrase in block, phrase
    # the allocation policy of ppo_ctx_create names the new allocation
    policy = src[src.index("PPO_Discrete::PPO_Discrete() (PPO_Discrete.cpp:4-100)"):src.index("PPO_API ppo_status ppo_ctx_create(")]
    assert "ppo_obs_norm_enable" in policy
    # ppo_config is untouched: kernel_flags is still its last field
    cfg = src[src.index("typedef struct ppo_config {"):src.index("} ppo_config;")]
    assert cfg.rstrip().splitlines()[-1].lstrip().startswith("int32_t kernel_flags;")


def test_binding_lists_the_normaliser_calls():
    P = load_package()
    for name in CALLS:
        assert name in P.binding.ABI_SYMBOLS, name
    assert P.binding.ABI_VERSION == 5
    want = {"obs_norm_enable": (["self", "mode", "clip", "eps"], {"mode": 1, "clip": 10.0, "eps": 1e-8}),
            "obs_norm_get": (["self"], {}),
            "obs_norm_set": (["self", "mean", "var", "count"], {}),
            "obs_norm_apply": (["self", "obs", "out", "stream"], {"out": None, "stream": None})}
    for meth, (names, defaults) in want.items():
        sig = inspect.signature(getattr(P.Context, meth))
        assert list(sig.parameters) == names, (meth, list(sig.parameters))
        for k, v in defaults.items():
            assert sig.parameters[k].default == v, (meth, k)


def test_library_exports_the_normaliser_calls():
    P = load_package()
    subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.join(ROOT, "ppo-libtorch_amd", "csrc")])
    out = subprocess.check_output(["nm", "-D", "--defined-only", P.binding.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in CALLS:
        assert name in exported, name
        assert hasattr(P.binding.lib(), name)


def test_the_kernel_file_is_built_into_the_library():
    mk = open(os.path.join(ROOT, "ppo-libtorch_amd", "csrc", "Makefile")).read()
    assert "kernels_obsnorm.hip" in mk
    src = open(os.path.join(ROOT, "ppo-libtorch_amd", "csrc", "kernels_obsnorm.hip")).read()
    assert "__global__" in src and "atomicAdd" not in src   # a fixed reduction tree, no floating-point atomics


def test_the_device_calls_still_never_wait():
    """ppo_dev_observe and ppo_dev_act gained a launch, not a wait: no stream / event / device synchronisation and no blocking copy in their bodies."""
    src = open(os.path.join(ROOT, "ppo-libtorch_amd", "csrc", "api.hip")).read()
    for name in ("ppo_dev_observe", "ppo_dev_act", "ppo_dev_env_reset"):
        start = src.index('extern "C" ppo_status %s(' % name)
        body = src[start:src.index("\n}\n", start)]
        assert len(body) > 400 and not re.search(r"Synchronize|hipMemcpy\(", body), name
    start = src.index('extern "C" ppo_status ppo_dev_observe(')
    assert "launch_obsnorm" in src[start:src.index("\n}\n", start)] or "on_batch" in src[start:src.index("\n}\n", start)]
