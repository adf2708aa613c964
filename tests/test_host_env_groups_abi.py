"""Env groups of caller-stepped environments (include/ppo_hip.h, "Env groups") at the C-ABI, without a GPU: the header declares the four group calls and
PPO_HOST_MAX_GROUPS, the built library exports them, the binding lists them, the ABI version is still 5, and a pipelined env loop written against the
header compiles as C and as C++."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ppo_hip.h")
GROUP_CALLS = ["ppo_host_rollout_begin_groups", "ppo_host_group_act", "ppo_host_group_actions", "ppo_host_group_observe"]


def test_header_declares_the_group_calls():
    src = open(HDR).read()
    assert re.search(r"#define PPO_ABI_VERSION 5\b", src)   # additions only: no struct changed
    assert re.search(r"#define PPO_HOST_MAX_GROUPS 8\b", src)
    for name in GROUP_CALLS:
        assert re.search(r"PPO_API\s+ppo_status\s+%s\s*\(" % name, src), name


def test_binding_lists_the_group_calls():
    P = load_package()
    for name in GROUP_CALLS:
        assert name in P.binding.ABI_SYMBOLS, name
    for meth in ("host_group_act", "host_group_actions", "host_group_observe"):
        assert callable(getattr(P.Context, meth)), meth
    import inspect
    assert "groups" in inspect.signature(P.Context.host_rollout_begin).parameters


def test_library_exports_the_group_calls():
    P = load_package()
    if not os.path.exists(P.binding.LIB_PATH):
        pytest.fail("libppo_hip.so is not built")
    L = ctypes.CDLL(P.binding.LIB_PATH)
    for name in GROUP_CALLS:
        assert hasattr(L, name), name
    assert L.ppo_abi_version() == 5 == P.binding.ABI_VERSION


USER_PIPELINE = r'''
#include <stdint.h>
#include <stdlib.h>
#include "ppo_hip.h"

/* step the envs [b0, b1) of a user's batch (in a real program: on worker threads) */
typedef void (*step_rows_fn)(int b0, int b1, const int64_t* act, float* obs, float* rew, int32_t* done);

/* two halves of the envs in alternation: while one half is stepped, the policy call of the other is in flight */
int train_pipelined(ppo_ctx* ctx, int N, int T, int O, step_rows_fn step_rows) {
    int32_t bounds[PPO_HOST_MAX_GROUPS + 1];
    const int32_t G = 2;
    bounds[0] = 0; bounds[1] = N / 2; bounds[2] = N;
    float* obs = (float*)malloc(sizeof(float) * O * N);
    float* rew = (float*)malloc(sizeof(float) * N);
    int32_t* done = (int32_t*)malloc(sizeof(int32_t) * N);
    int64_t* act = (int64_t*)malloc(sizeof(int64_t) * N);
    ppo_status s = ppo_host_rollout_begin_groups(ctx, G, bounds);
    if (s == PPO_OK) s = ppo_host_group_act(ctx, 0, NULL);
    for (int k = 0; k < T * G && s == PPO_OK; k++) {
        const int32_t g = k % G, b0 = bounds[g], b1 = bounds[g + 1];
        if (k + 1 < T * G) s = ppo_host_group_act(ctx, (k + 1) % G, NULL);     /* enqueued: returns at once */
        if (s == PPO_OK) s = ppo_host_group_actions(ctx, g, act + b0);         /* waits for group g only */
        step_rows(b0, b1, act, obs, rew, done);
        if (s == PPO_OK) s = ppo_host_group_observe(ctx, g, obs + (size_t)O * b0, rew + b0, done + b0, NULL, NULL);
    }
    if (s == PPO_OK) s = ppo_host_rollout_end(ctx);
    free(obs); free(rew); free(done); free(act);
    return s;
}
'''


@pytest.mark.parametrize("compiler", ["gcc", "g++"])
def test_a_pipelined_env_loop_compiles_against_the_header(tmp_path, compiler):
    if shutil.which(compiler) is None:
        pytest.skip(compiler + " not installed")
    src = tmp_path / ("pipeline.c" if compiler == "gcc" else "pipeline.cpp")
    src.write_text(USER_PIPELINE)
    r = subprocess.run([compiler, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


FACADE_USER = r'''
#include <tuple>
#include <vector>
#include "PPO/PPO_HostEnv.h"

struct MyEnv {
    explicit MyEnv(int64_t seed) : x(6, static_cast<float>(seed)) {}
    std::vector<float> reset() { episode_length = 0; episode_reward = 0.0f; return x; }
    std::tuple<std::vector<float>, float, bool, bool> step(const int64_t& a) { episode_length++; episode_reward += 1.0f; x[0] += a ? 0.1f : -0.1f; return { x, 1.0f, false, false }; }
    std::vector<bool> getActionMask() const { return { true, false, true }; }
    std::vector<float> x;
    int64_t episode_length = 0;
    float episode_reward = 0.0f;
};

void instantiate() {
    PPO_HostEnv<MyEnv> algo;
    algo.setEnvGroups(2);
    algo.train();
    PPO_HostEnv<MyEnv, true> masked;
    masked.setEnvGroups(masked.envGroups() + 1);
    masked.train();
}
'''


def test_facade_env_groups_instantiate_with_a_user_env(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    src = tmp_path / "user_env_groups.cpp"
    src.write_text(FACADE_USER)
    host = os.path.join(ROOT, "ppo-libtorch_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.dirname(HDR), "-I", host, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
