// `hidden_size = 128` in [network] beside `matrix_cores = true` and `fused_policy = true` (tests/test_gpu_fused_h128_facade.py), run in a fresh directory:
// PPO_HostEnvBox at obs_size 100, action_dim 3 reads the key, its context is 2 x 128 with the family flag, PPO_KERNEL_FUSED_WIDE_OBS and PPO_KERNEL_FUSED_MATRIX
// and WITHOUT PPO_KERNEL_ENV_GENERIC, and one training iteration runs on the fused kernels (the launch counters move).
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../PPO/PPO_HostEnvBox.h"

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 16, T = 32, D = 3, O = 100;

// reward = -|a - target|^2 with the target in the first columns of a 100-wide observation, the rest a fixed pattern; episodes of 6 .. 9 steps
struct WideReachEnv {
    explicit WideReachEnv(int64_t index) : idx(index) {}
    std::vector<float> obs() const {
        std::vector<float> o(O);
        for (int k = 0; k < O; k++) o[k] = k < D ? tgt[k] : std::sin(0.1f * static_cast<float>(k + idx + episode_length));
        return o;
    }
    void draw() { for (int d = 0; d < D; d++) { state = state * 1664525u + 1013904223u; tgt[d] = static_cast<float>(state >> 8) * (2.0f / 16777216.0f) - 1.0f; } }
    std::vector<float> reset() { draw(); episode_length = 0; episode_reward = 0.0f; return obs(); }
    std::tuple<std::vector<float>, float, bool, bool> step(const std::vector<float>& a) {
        float r = 0.0f;
        for (int d = 0; d < D && d < static_cast<int>(a.size()); d++) r -= (a[d] - tgt[d]) * (a[d] - tgt[d]);
        finite_ok = finite_ok && std::isfinite(r) && a.size() == static_cast<size_t>(D);
        draw();
        episode_length++;
        episode_reward += r;
        return { obs(), r, episode_length >= 6 + idx % 4, false };
    }
    int64_t idx;
    uint32_t state = 12345u + 977u * static_cast<uint32_t>(idx);
    float tgt[3] = { 0, 0, 0 };
    bool finite_ok = true;
    int64_t episode_length = 0;
    float episode_reward = 0.0f;
};

int main() {
    {
        std::ofstream f("PPOConfig.toml");
        f << "[environment]\nobs_size = " << O << "\naction_dim = " << D << "\nmax_episode_steps = 40\nfused_policy = true\nwide_obs = true\nmatrix_cores = true\n"
          << "[network]\nhidden_size = 128\n"
          << "[general]\nseed = 3\ntotal_timesteps = " << N * T << "\nuse_cuda = true\ncheckpoint_updates = 1\n"
             "[ppo]\nlearning_rate = 0.001\nnum_envs = " << N << "\nnum_steps = " << T << "\nanneal_lr = true\nuse_gae = true\ngamma = 0.98\n"
             "gae_lambda = 0.95\nnum_minibatches = 4\nupdate_epochs = 4\nnorm_adv = true\nclip_coef = 0.2\nclip_vloss = true\n"
             "ent_coef = 0.01\nvf_coef = 0.5\nmax_grad_norm = 0.5\n";
    }
    using Algo = PPO_HostEnvBox<WideReachEnv>;
    std::stringstream out;
    std::streambuf* old = std::cout.rdbuf(out.rdbuf());
    std::unique_ptr<Algo> algo;
    try { algo = std::make_unique<Algo>([](int64_t i) { return std::make_shared<WideReachEnv>(i); }); } catch (...) { std::cout.rdbuf(old); throw; }
    std::cout.rdbuf(old);
    REQUIRE(out.str().find("Using config file hidden_size = 128") != std::string::npos);
    ppo_config cfg{};
    cfg.struct_size = sizeof cfg;
    REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK);
    REQUIRE(cfg.hidden == 128 && cfg.n_hidden == 2);
    REQUIRE(cfg.kernel_flags == (PPO_KERNEL_GAUSS_FUSED | PPO_KERNEL_FUSED_WIDE_OBS | PPO_KERNEL_FUSED_MATRIX));
    int finite = 0;
    algo->m_on_update = [&](int64_t, const ppo_stats& s) { finite += std::isfinite(s.loss) && std::isfinite(s.entropy_loss) && std::isfinite(s.explained_variance) ? 1 : 0; };
    old = std::cout.rdbuf(out.rdbuf());
    try { algo->train(); } catch (...) { std::cout.rdbuf(old); throw; }
    std::cout.rdbuf(old);
    REQUIRE(finite == 1);
    for (const auto& e : algo->m_envs) REQUIRE(e->finite_ok);
    int64_t act = 0, value = 0, update = 0;
    REQUIRE(ppo_gauss_fused_launches(algo->m_ctx, &act, &value, &update) == PPO_OK);
    std::printf("fused launches: act %lld value %lld update %lld\n", (long long)act, (long long)value, (long long)update);
    REQUIRE(act >= T && value >= 2 && update == 4 * 4);
    std::printf("host_fused_h128_test ok\n");
    return 0;
}
