// `fused_categorical = true` in [environment] (PPO_KERNEL_CAT_FUSED through the facade) on a GPU, driven by tests/test_gpu_cat_fused_facade.py in a fresh
// directory: PPO_HostEnv trains two iterations on the fused categorical kernels (their launch counters say so), the key prints like the other extension
// keys, and its checkpoint loads into an object WITHOUT the key -- at obs_size 4 that one runs the reference-shape kernels -- with bit-equal parameters: the
// parameter order is Agent::parameters() order either way.  With the key absent nothing is said about it and no flag is set.
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

namespace fs = std::filesystem;

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 16, T = 32, UPDATES = 2, A = 3, O = 4;

// reward 1 where the action is the index of the largest of the first three observations, episodes of 6 .. 9 steps
struct PickEnv {
    explicit PickEnv(int64_t index) : idx(index) {}
    std::vector<float> obs() const { return { x[0], x[1], x[2], static_cast<float>(episode_length) / 8.0f }; }
    void draw() { for (int d = 0; d < 3; d++) { state = state * 1664525u + 1013904223u; x[d] = static_cast<float>(state >> 8) * (2.0f / 16777216.0f) - 1.0f; } }
    std::vector<float> reset() { draw(); episode_length = 0; episode_reward = 0.0f; return obs(); }
    std::tuple<std::vector<float>, float, bool, bool> step(const int64_t& a) {
        in_range = in_range && a >= 0 && a < A;
        int best = 0;
        for (int d = 1; d < 3; d++) if (x[d] > x[best]) best = d;
        const float r = a == best ? 1.0f : 0.0f;
        draw();
        episode_length++;
        episode_reward += r;
        return { obs(), r, episode_length >= 6 + idx % 4, false };
    }
    int64_t idx;
    uint32_t state = 4321u + 977u * static_cast<uint32_t>(idx);
    float x[3] = { 0, 0, 0 };
    bool in_range = true;
    int64_t episode_length = 0;
    float episode_reward = 0.0f;
};

static void writeConfig(const std::string& extra) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = " << O << "\naction_size = " << A << "\nmax_episode_steps = 40\n" << extra
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
    auto factory = [](int64_t i) { return std::make_shared<PickEnv>(i); };
    using Algo = PPO_HostEnv<PickEnv>;

    // the key absent: nothing printed about it, the context is not flagged and counts nothing
    writeConfig("");
    {
        std::unique_ptr<Algo> plain;
        const std::string said = captured([&] { plain = std::make_unique<Algo>(factory); });
        REQUIRE(said.find("fused_categorical") == std::string::npos);
        ppo_config cfg{};
        cfg.struct_size = sizeof cfg;
        REQUIRE(ppo_get_config(plain->m_ctx, &cfg) == PPO_OK && (cfg.kernel_flags & PPO_KERNEL_CAT_FUSED) == 0);
        int64_t act = -1, value = -1, update = -1;
        REQUIRE(ppo_gauss_fused_launches(plain->m_ctx, &act, &value, &update) == PPO_OK && act == 0 && value == 0 && update == 0);
    }

    writeConfig("fused_categorical = true\n");
    std::vector<float> trained;
    int64_t P = 0;
    {
        std::unique_ptr<Algo> algo;
        const std::string said = captured([&] { algo = std::make_unique<Algo>(factory); });
        REQUIRE(said.find("Using config file fused_categorical = true") != std::string::npos);
        ppo_config cfg{};
        cfg.struct_size = sizeof cfg;
        REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK && (cfg.kernel_flags & PPO_KERNEL_CAT_FUSED) != 0 && (cfg.kernel_flags & PPO_KERNEL_GAUSS_FUSED) == 0);
        P = ppo_param_count(algo->m_ctx);
        REQUIRE(P == 2 * (64 * O + 64 + 64 * 64 + 64) + (64 + 1) + (64 * A + A));
        int finite = 0;
        algo->m_on_update = [&](int64_t, const ppo_stats& s) { finite += std::isfinite(s.loss) && std::isfinite(s.entropy_loss) && std::isfinite(s.explained_variance) ? 1 : 0; };
        const std::string table = captured([&] { algo->train(); });
        REQUIRE(finite == UPDATES && table.find("rollout/") != std::string::npos);
        for (const auto& e : algo->m_envs) REQUIRE(e->in_range);
        int64_t act = 0, value = 0, update = 0;
        REQUIRE(ppo_gauss_fused_launches(algo->m_ctx, &act, &value, &update) == PPO_OK);   // the fused family's one set of counters, for either flag
        std::printf("fused launches: act %lld value %lld update %lld\n", (long long)act, (long long)value, (long long)update);
        REQUIRE(act >= UPDATES * T && value >= UPDATES * 2 && update == UPDATES * 4 * 4);
        trained.resize(static_cast<size_t>(P));
        REQUIRE(ppo_params_get_h(algo->m_ctx, trained.data(), P) == PPO_OK);
    }
    const std::string ckpt = "./ModelCheckpoints/PPO_Agent_" + std::to_string(N * T * UPDATES) + "_steps.pt";
    REQUIRE(fs::exists(ckpt));
    // the checkpoint into an object without the key
    writeConfig("");
    {
        std::unique_ptr<Algo> again;
        const std::string said = captured([&] { again = std::make_unique<Algo>(factory); });
        REQUIRE(said.find("Loading model") != std::string::npos && said.find("ignoring it") == std::string::npos && said.find("fused_categorical") == std::string::npos);
        ppo_config cfg{};
        cfg.struct_size = sizeof cfg;
        REQUIRE(ppo_get_config(again->m_ctx, &cfg) == PPO_OK && (cfg.kernel_flags & PPO_KERNEL_CAT_FUSED) == 0);
        std::vector<float> loaded(static_cast<size_t>(P));
        REQUIRE(ppo_param_count(again->m_ctx) == P && ppo_params_get_h(again->m_ctx, loaded.data(), P) == PPO_OK);
        REQUIRE(std::memcmp(loaded.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
    }
    std::printf("host_cat_fused_test ok\n");
    return 0;
}
