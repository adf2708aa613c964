// `fused_policy = true` in [environment] (PPO_KERNEL_GAUSS_FUSED through the facade) on a GPU, driven by tests/test_gpu_gaussian_fused_facade.py in a fresh
// directory: PPO_HostEnvBox trains two iterations on the fused Gaussian kernels (their launch counters say so), its checkpoint loads into a fresh object
// with bit-equal parameters, the key prints like the other extension keys, and PPO_HostEnv (a categorical policy) with the key throws the library's message.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../PPO/PPO_HostEnv.h"
#include "../PPO/PPO_HostEnvBox.h"

namespace fs = std::filesystem;

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 16, T = 32, UPDATES = 2, D = 3, O = 5;

// reward = -|a - target|^2 with the target in the observation, episodes of 6 .. 9 steps
struct ReachEnv {
    explicit ReachEnv(int64_t index) : idx(index) {}
    std::vector<float> obs() const { return { tgt[0], tgt[1], tgt[2], static_cast<float>(episode_length) / 8.0f, 1.0f }; }
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

// a discrete-action env for PPO_HostEnv: never stepped here, the context is refused before
struct CoinEnv {
    explicit CoinEnv(int64_t) {}
    std::vector<float> reset() { episode_length = 0; episode_reward = 0.0f; return std::vector<float>(O, 0.0f); }
    std::tuple<std::vector<float>, float, bool, bool> step(int64_t) { episode_length++; return { std::vector<float>(O, 0.0f), 0.0f, false, false }; }
    int64_t episode_length = 0;
    float episode_reward = 0.0f;
};

static void writeConfig(const std::string& action_key, const std::string& extra) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = " << O << "\n" << action_key << "\nmax_episode_steps = 40\n" << extra
      << "[general]\nseed = 3\ntotal_timesteps = " << N * T * UPDATES << "\nuse_cuda = true\ncheckpoint_updates = 1\n"
         "[ppo]\nlearning_rate = 0.001\nnum_envs = " << N << "\nnum_steps = " << T << "\nanneal_lr = true\nuse_gae = true\ngamma = 0.98\n"
         "gae_lambda = 0.95\nnum_minibatches = 4\nupdate_epochs = 4\nnorm_adv = true\nclip_coef = 0.2\nclip_vloss = true\n"
         "ent_coef = 0.01\nvf_coef = 0.5\nmax_grad_norm = 0.5\n";
}

template <class Fn> static std::string captured(Fn fn) {
    std::stringstream out;
    std::streambuf* old = std::cout.rdbuf(out.rdbuf());
    try { fn(); } catch (...) { std::cout.rdbuf(old); throw; }
    std::cout.rdbuf(old);
    return out.str();
}

int main() {
    auto factory = [](int64_t i) { return std::make_shared<ReachEnv>(i); };
    using Algo = PPO_HostEnvBox<ReachEnv>;
    // a categorical class with the key: the library's refusal, with its message
    writeConfig("action_size = 2", "fused_policy = true\n");
    std::string refusal;
    captured([&] { try { PPO_HostEnv<CoinEnv> algo([](int64_t i) { return std::make_shared<CoinEnv>(i); }); } catch (const std::runtime_error& e) { refusal = e.what(); } });
    std::printf("refusal: %s\n", refusal.c_str());
    REQUIRE(refusal.find("PPO_KERNEL_GAUSS_FUSED") != std::string::npos && refusal.find("PPO_DIST_GAUSSIAN") != std::string::npos);

    // the key absent: nothing printed about it, and the context is not flagged
    writeConfig("action_dim = 3", "");
    {
        std::unique_ptr<Algo> plain;
        const std::string said = captured([&] { plain = std::make_unique<Algo>(factory); });
        REQUIRE(said.find("fused_policy") == std::string::npos);
        ppo_config cfg{};
        cfg.struct_size = sizeof cfg;
        REQUIRE(ppo_get_config(plain->m_ctx, &cfg) == PPO_OK && (cfg.kernel_flags & PPO_KERNEL_GAUSS_FUSED) == 0);
    }

    writeConfig("action_dim = 3", "fused_policy = true\n");
    std::vector<float> trained;
    int64_t P = 0;
    {
        std::unique_ptr<Algo> algo;
        const std::string said = captured([&] { algo = std::make_unique<Algo>(factory); });
        REQUIRE(said.find("Using config file fused_policy = true") != std::string::npos && algo->actionDim() == D);
        P = ppo_param_count(algo->m_ctx);
        REQUIRE(P == 2 * (64 * O + 64 + 64 * 64 + 64) + (64 + 1) + (64 * D + D) + D);
        int finite = 0;
        algo->m_on_update = [&](int64_t, const ppo_stats& s) { finite += std::isfinite(s.loss) && std::isfinite(s.entropy_loss) && std::isfinite(s.explained_variance) ? 1 : 0; };
        const std::string table = captured([&] { algo->train(); });
        REQUIRE(finite == UPDATES && table.find("rollout/") != std::string::npos);
        for (const auto& e : algo->m_envs) REQUIRE(e->finite_ok);
        int64_t act = 0, value = 0, update = 0;
        REQUIRE(ppo_gauss_fused_launches(algo->m_ctx, &act, &value, &update) == PPO_OK);
        std::printf("fused launches: act %lld value %lld update %lld\n", (long long)act, (long long)value, (long long)update);
        REQUIRE(act >= UPDATES * T && value >= UPDATES * 2 && update == UPDATES * 4 * 4);
        trained.resize(static_cast<size_t>(P));
        REQUIRE(ppo_params_get_h(algo->m_ctx, trained.data(), P) == PPO_OK);
        bool moved = false;
        for (int d = 0; d < D; d++) moved = moved || trained[static_cast<size_t>(P - D + d)] != 0.0f;
        REQUIRE(moved);
    }
    const std::string ckpt = "./ModelCheckpoints/PPO_Agent_" + std::to_string(N * T * UPDATES) + "_steps.pt";
    REQUIRE(fs::exists(ckpt));
    {
        std::unique_ptr<Algo> again;
        const std::string said = captured([&] { again = std::make_unique<Algo>(factory); });
        REQUIRE(said.find("Loading model") != std::string::npos && said.find("ignoring it") == std::string::npos);
        std::vector<float> loaded(static_cast<size_t>(P));
        REQUIRE(ppo_param_count(again->m_ctx) == P && ppo_params_get_h(again->m_ctx, loaded.data(), P) == PPO_OK);
        REQUIRE(std::memcmp(loaded.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
    }
    std::printf("host_gaussian_fused_test ok\n");
    return 0;
}
