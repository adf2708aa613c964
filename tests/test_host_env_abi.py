"""Caller-stepped environments (PPO_ENV_HOST) at the C-ABI, without a GPU: the header declares the env kind, the staging-path flag and the five
ppo_host_* entry points, the binding lists them (tests/test_abi_symbols.py then checks the library exports them), and a user's env loop written
against the header compiles."""
import os
import re
import shutil
import subprocess

import pytest

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ppo_hip.h")
HOST_CALLS = ["ppo_host_env_reset", "ppo_host_rollout_begin", "ppo_host_act", "ppo_host_observe", "ppo_host_rollout_end"]


def test_header_declares_the_host_env_interface():
    src = open(HDR).read()
    assert re.search(r"PPO_ENV_HOST\s*=\s*3\b", src)
    assert re.search(r"#define PPO_ABI_VERSION 5\b", src)   # backward compatible additions: no struct changed
    for name in HOST_CALLS:
        assert re.search(r"PPO_API\s+ppo_status\s+%s\s*\(" % name, src), name


def test_binding_lists_the_host_env_interface():
    P = load_package()
    for name in HOST_CALLS:
        assert name in P.binding.ABI_SYMBOLS, name
    assert P.ENV_HOST == 3
    for meth in ("host_env_reset", "host_rollout_begin", "host_act", "host_observe", "host_rollout_end"):
        assert callable(getattr(P.Context, meth)), meth


USER_LOOP = r'''
#include <stdint.h>
#include <stdlib.h>
#include "ppo_hip.h"

/* a user's env: six observations the library has no kernel for */
typedef struct { float x[6]; int32_t len; float ret; } my_env;
static void my_reset(my_env* e, float* obs) { for (int k = 0; k < 6; k++) obs[k] = e->x[k] = 0.0f; e->len = 0; e->ret = 0.0f; }
static float my_step(my_env* e, int64_t a, float* obs, int32_t* done) {
    e->x[0] += a ? 0.1f : -0.1f; e->len += 1; e->ret += 1.0f;
    *done = e->len >= 50;
    for (int k = 0; k < 6; k++) obs[k] = e->x[k];
    return 1.0f;
}

int train(ppo_config cfg, my_env* envs, int iterations) {
    ppo_ctx* ctx = NULL;
    const int N = cfg.num_envs, T = cfg.num_steps;
    cfg.env_kind = PPO_ENV_HOST;
    if (ppo_ctx_create(&cfg, &ctx) != PPO_OK) return 1;
    float* obs = (float*)malloc(sizeof(float) * 6 * N);
    float* rew = (float*)malloc(sizeof(float) * N);
    int32_t *done = (int32_t*)malloc(sizeof(int32_t) * N), *fin_len = (int32_t*)malloc(sizeof(int32_t) * N);
    float* fin_rew = (float*)malloc(sizeof(float) * N);
    int64_t* act = (int64_t*)malloc(sizeof(int64_t) * N);
    for (int n = 0; n < N; n++) my_reset(&envs[n], obs + 6 * n);
    ppo_status s = ppo_host_env_reset(ctx, obs);
    for (int it = 0; it < iterations && s == PPO_OK; it++) {
        s = ppo_host_rollout_begin(ctx);
        for (int t = 0; t < T && s == PPO_OK; t++) {
            s = ppo_host_act(ctx, NULL, act);
            for (int n = 0; n < N; n++) {
                rew[n] = my_step(&envs[n], act[n], obs + 6 * n, &done[n]);
                fin_len[n] = done[n] ? envs[n].len : 0;
                fin_rew[n] = done[n] ? envs[n].ret : 0.0f;
                if (done[n]) my_reset(&envs[n], obs + 6 * n);
            }
            if (s == PPO_OK) s = ppo_host_observe(ctx, obs, rew, done, fin_len, fin_rew);
        }
        if (s == PPO_OK) s = ppo_host_rollout_end(ctx);
    }
    ppo_stats st;
    if (s == PPO_OK) s = ppo_read_stats(ctx, &st);
    ppo_ctx_destroy(ctx);
    free(obs); free(rew); free(done); free(fin_len); free(fin_rew); free(act);
    return s;
}
'''


@pytest.mark.parametrize("compiler", ["gcc", "g++"])
def test_a_user_env_loop_compiles_against_the_header(tmp_path, compiler):
    if shutil.which(compiler) is None:
        pytest.skip(compiler + " not installed")
    src = tmp_path / ("loop.c" if compiler == "gcc" else "loop.cpp")
    src.write_text(USER_LOOP)
    r = subprocess.run([compiler, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


FACADE_USER = r'''
#include <tuple>
#include <vector>
#include "PPO/PPO_HostEnv.h"

struct MyEnv {   // the reference's duck type: a user env with 6 observations
    explicit MyEnv(int64_t seed) : x(6, static_cast<float>(seed)) {}
    std::vector<float> reset() { episode_length = 0; episode_reward = 0.0f; return x; }
    std::tuple<std::vector<float>, float, bool, bool> step(const int64_t& a) { episode_length++; episode_reward += 1.0f; x[0] += a ? 0.1f : -0.1f; return { x, 1.0f, false, false }; }
    std::vector<float> x;
    int64_t episode_length = 0;
    float episode_reward = 0.0f;
};
struct MyMaskedEnv : MyEnv {
    using MyEnv::MyEnv;
    std::vector<bool> getActionMask() const { return { true, false, true }; }
};

void instantiate() {
    PPO_HostEnv<MyEnv> algo([](int64_t i) { return std::make_shared<MyEnv>(i); });
    algo.initEnvs();
    algo.stepEnvs(std::vector<int64_t>(algo.m_envs.size(), 1));
    algo.train();
    PPO_HostEnv<MyMaskedEnv, true> masked;
    masked.train();
}
'''


def test_facade_host_env_template_instantiates_with_a_user_env(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    src = tmp_path / "user_env.cpp"
    src.write_text(FACADE_USER)
    host = os.path.join(ROOT, "ppo-libtorch_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.dirname(HDR), "-I", host, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
