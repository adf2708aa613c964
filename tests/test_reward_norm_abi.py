"""Reward normalisation of caller-stepped environments (include/ppo_hip.h, "Reward normalisation": ppo_reward_norm_enable / ppo_reward_norm_get_h /
ppo_reward_norm_set_h) without a GPU: the header declares the three calls in a block behind ppo_obs_norm_apply and in front of the evaluation section,
the ABI version and ppo_config are unchanged, the binding lists them and has the Context methods with the documented parameters, the built library
exports them, and the kernel file is built without floating-point atomics.  tests/test_gpu_reward_norm.py runs them."""
import inspect
import os
import re
import subprocess

from __graft_entry__ import ROOT, load_package

HDR = os.path.join(ROOT, "include", "ppo_hip.h")
CSRC = os.path.join(ROOT, "ppo-libtorch_amd", "csrc")
CALLS = ["ppo_reward_norm_enable", "ppo_reward_norm_get_h", "ppo_reward_norm_set_h"]


def test_header_declares_the_reward_normaliser_calls():
    src = open(HDR).read()
    assert re.search(r"#define PPO_ABI_VERSION 5\b", src)   # additions only
    for name in CALLS:
        assert re.search(r"PPO_API\s+ppo_status\s+%s\s*\(" % name, src), name
    start = src.index("Reward normalisation of caller-stepped environments")
    assert src.index("PPO_API ppo_status ppo_obs_norm_apply(ppo_ctx") < start < src.index("PPO_API ppo_status ppo_evaluate(")
    for name in CALLS:
        assert start < src.index("PPO_API ppo_status %s(" % name) < src.index("PPO_API ppo_status ppo_evaluate("), name
    # the signatures of the issue
    flat = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "ppo_reward_norm_enable(ppo_ctx* ctx, int32_t mode, float clip, float eps);" in flat
    assert "ppo_reward_norm_get_h(ppo_ctx* ctx, double* mean, double* var, double* count, double* ret_h , int64_t N);" in flat
    assert "ppo_reward_norm_set_h(ppo_ctx* ctx, double mean, double var, double count);" in flat
    block = src[start:src.index("PPO_API ppo_status ppo_reward_norm_set_h(")]
    # the semantics, who sees which reward, the order against the fold, the launch count and the refusals are stated
    for phrase in ("ret = 0, mean = 0, var = 1, count = 0", "R[n] = ret[n] * g + (double)r[n]", "delta = bm - mean", "ret[n] = done[n] ? 0 : R[n]",
                   "sqrt(var + eps)", "No mean is subtracted", "var = 0", "RAW", "NORMALISED", "precedes the fold", "bit for bit", "ONE more per env step",
                   "ppo_host_env_reset", "ppo_dev_env_reset", "ppo_host_rollout_begin_groups", "PPO_ERR_UNSUPPORTED", "PPO_ERR_STATE", "PPO_ERR_INVALID"):
        assert phrase in block, phrase
    # the allocation policy of ppo_ctx_create names the new allocation
    policy = src[src.index("PPO_Discrete::PPO_Discrete() (PPO_Discrete.cpp:4-100)"):src.index("PPO_API ppo_status ppo_ctx_create(")]
    assert "ppo_reward_norm_enable" in policy and "ppo_reward_norm_set_h" in policy
    # ppo_config is untouched: kernel_flags is still its last field
    cfg = src[src.index("typedef struct ppo_config {"):src.index("} ppo_config;")]
    assert cfg.rstrip().splitlines()[-1].lstrip().startswith("int32_t kernel_flags;")


def test_binding_lists_the_reward_normaliser_calls():
    P = load_package()
    for name in CALLS:
        assert name in P.binding.ABI_SYMBOLS, name
    assert P.binding.ABI_VERSION == 5
    want = {"reward_norm_enable": (["self", "mode", "clip", "eps"], {"mode": 1, "clip": 10.0, "eps": 1e-8}),
            "reward_norm_get": (["self", "returns"], {"returns": False}),
            "reward_norm_set": (["self", "mean", "var", "count"], {})}
    for meth, (names, defaults) in want.items():
        sig = inspect.signature(getattr(P.Context, meth))
        assert list(sig.parameters) == names, (meth, list(sig.parameters))
        for k, v in defaults.items():
            assert sig.parameters[k].default == v, (meth, k)


def test_library_exports_the_reward_normaliser_calls():
    P = load_package()
    subprocess.check_call(["make", "-s", "-j", "4", "-C", CSRC])
    out = subprocess.check_output(["nm", "-D", "--defined-only", P.binding.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in CALLS:
        assert name in exported, name
        assert hasattr(P.binding.lib(), name)


def test_the_kernel_file_is_built_into_the_library():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "kernels_rewnorm.hip" in mk
    assert "-ffp-contract=off" in mk and "-fno-fast-math" in mk and not re.search(r"kernels_rewnorm\.o.*FLAGS", mk)   # the common flags, nothing of its own
    src = open(os.path.join(CSRC, "kernels_rewnorm.hip")).read()
    assert "__global__" in src and "atomicAdd" not in src   # a fixed reduction order, no floating-point atomics
    assert "rewnorm_update_apply_kernel" in src and "rewnorm_apply_kernel" in src
    assert re.search(r"hipLaunchKernelGGL\(rewnorm_update_apply_kernel, dim3\(1\)", src)   # one workgroup


def test_the_commit_stores_the_scratch_and_sums_the_raw_reward():
    """HostStepArgs::st_rew_store: null keeps today's store; the episode sums never read it"""
    hdr = open(os.path.join(CSRC, "ppo_internal.hpp")).read()
    assert re.search(r"const float\* st_rew_store;", hdr)
    src = open(os.path.join(CSRC, "kernels_rollout.hip")).read()
    body = src[src.index("void host_commit_row("):]
    body = body[:body.index("\n}\n")]
    assert "hs.rewards_prev[row] = hs.st_rew_store ? hs.st_rew_store[row] : r;" in body
    assert "hs.ep_rew[row] + r" in body and body.count("st_rew_store") == 2


def test_the_launch_sits_in_front_of_the_commit_and_the_device_calls_never_wait():
    src = open(os.path.join(CSRC, "api.hip")).read()
    start = src.index('extern "C" ppo_status ppo_dev_observe(')
    body = src[start:src.index("\n}\n", start)]
    assert body.index("rn_batch(c, h)") < body.index("launch_host_commit(h") < body.index("launch_dev_fold")
    assert not re.search(r"Synchronize|hipMemcpy\(", body)
    # the acts enqueue through the shared step bodies: there the launch sits in front of the commit, and of the 2 x 64 launch that commits and acts
    for name, decl in (("act_slice", "static"), ("act_slice_f32", "static"), ("ppo_host_rollout_end", 'extern "C"')):
        start = src.index('%s ppo_status %s(' % (decl, name))
        body = src[start:src.index("\n}\n", start)]
        assert body.index("rn_batch(c, h)") < body.index("launch_host_commit(h"), name
        if decl == "static":   # shared with the device feed: they only enqueue
            assert not re.search(r"Synchronize|hipMemcpy\(", body), name
    body = src[src.index("static ppo_status act_slice("):]
    assert body.index("rn_batch(c, h)") < body.index("launch_host_act(")
    for name, via in (("ppo_host_act", "act_slice("), ("ppo_host_act_f32", "act_slice_f32("), ("ppo_dev_act", "act_slice("), ("ppo_dev_act_f32", "act_slice_f32(")):
        start = src.index('extern "C" ppo_status %s(' % name)
        assert via in src[start:src.index("\n}\n", start)], name
