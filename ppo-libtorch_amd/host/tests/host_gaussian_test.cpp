// PPO_HostEnvBox (PPO/PPO_HostEnvBox.h: caller-stepped envs with real-valued actions, PPO_DIST_GAUSSIAN) on a GPU, driven by
// tests/test_gpu_gaussian_facade.py in a fresh directory: a Box env of D = 3 trains two iterations from a TOML with action_dim = 3, norm_obs and
// norm_reward; the checkpoint it wrote loads into a fresh object with bit-equal parameters, log_std included; env_groups = 2 throws the library's message.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../PPO/PPO_HostEnvBox.h"

namespace fs = std::filesystem;

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 16, T = 32, UPDATES = 2, D = 3, O = 5;

// reach the point the observation names: reward = -|a - target|^2, episodes of 6 .. 9 steps, observations in the hundreds (norm_obs has work to do)
struct ReachEnv {
    explicit ReachEnv(int64_t index) : idx(index) {}
    std::vector<float> obs() const { return { 100.0f * tgt[0], 100.0f * tgt[1], 100.0f * tgt[2], static_cast<float>(episode_length), 300.0f }; }
    void draw() { for (int d = 0; d < D; d++) { state = state * 1664525u + 1013904223u; tgt[d] = static_cast<float>(state >> 8) * (2.0f / 16777216.0f) - 1.0f; } }
    std::vector<float> reset() { draw(); episode_length = 0; episode_reward = 0.0f; return obs(); }
    std::tuple<std::vector<float>, float, bool, bool> step(const std::vector<float>& a) {
        widths_ok = widths_ok && a.size() == static_cast<size_t>(D);
        float r = 0.0f;
        for (int d = 0; d < D && d < static_cast<int>(a.size()); d++) r -= (a[d] - tgt[d]) * (a[d] - tgt[d]);
        finite_ok = finite_ok && std::isfinite(r);
        draw();
        episode_length++;
        episode_reward += 50.0f * r;
        return { obs(), 50.0f * r, episode_length >= 6 + idx % 4, false };
    }
    int64_t idx;
    uint32_t state = 12345u + 977u * static_cast<uint32_t>(idx);
    float tgt[3] = { 0, 0, 0 };
    bool widths_ok = true, finite_ok = true;
    int64_t episode_length = 0;
    float episode_reward = 0.0f;
};

static void writeConfig(const std::string& extra) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = " << O << "\naction_dim = " << D << "\nmax_episode_steps = 40\n" << extra
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
    // env groups are not built for Gaussian contexts: the library's message at construction
    writeConfig("env_groups = 2\n");
    std::string refusal;
    captured([&] { try { Algo algo(factory); } catch (const std::runtime_error& e) { refusal = e.what(); } });
    std::printf("refusal: %s\n", refusal.c_str());
    REQUIRE(refusal.find("ppo_host_rollout_begin_groups") != std::string::npos && refusal.find("GAUSSIAN") != std::string::npos);

    writeConfig("norm_obs = true\nnorm_reward = true\n");
    std::vector<float> trained;
    int64_t P = 0;
    {
        std::unique_ptr<Algo> algo;
        const std::string said = captured([&] { algo = std::make_unique<Algo>(factory); });
        REQUIRE(said.find("Using config file action_dim = 3") != std::string::npos && algo->actionDim() == D && algo->normObs() && algo->normReward());
        P = ppo_param_count(algo->m_ctx);
        REQUIRE(P == 2 * (64 * O + 64 + 64 * 64 + 64) + (64 + 1) + (64 * D + D) + D);
        std::vector<float> fresh(static_cast<size_t>(P));
        REQUIRE(ppo_params_get_h(algo->m_ctx, fresh.data(), P) == PPO_OK);
        for (int d = 0; d < D; d++) REQUIRE(fresh[static_cast<size_t>(P - D + d)] == 0.0f);   // log_std starts at 0
        int finite = 0;
        algo->m_on_update = [&](int64_t, const ppo_stats& s) { finite += std::isfinite(s.loss) && std::isfinite(s.entropy_loss) && std::isfinite(s.explained_variance) ? 1 : 0; };
        const std::string table = captured([&] { algo->train(); });
        REQUIRE(finite == UPDATES && table.find("rollout/") != std::string::npos);
        for (const auto& e : algo->m_envs) REQUIRE(e->widths_ok && e->finite_ok);
        trained.resize(static_cast<size_t>(P));
        REQUIRE(ppo_params_get_h(algo->m_ctx, trained.data(), P) == PPO_OK);
        bool moved = false;
        for (int d = 0; d < D; d++) moved = moved || trained[static_cast<size_t>(P - D + d)] != 0.0f;
        REQUIRE(moved);   // the optimizer steps log_std like any other tensor
        const std::vector<float> acts = algo->m_actions.cpu<float>();
        REQUIRE(acts.size() == static_cast<size_t>(T) * N * D);
        for (float a : acts) REQUIRE(std::isfinite(a));
    }
    const std::string ckpt = "./ModelCheckpoints/PPO_Agent_" + std::to_string(N * T * UPDATES) + "_steps.pt";
    REQUIRE(fs::exists(ckpt) && fs::exists(ObsNormFile::pathFor(ckpt)) && fs::exists(RewardNormFile::pathFor(ckpt)));
    {
        std::unique_ptr<Algo> again;
        const std::string said = captured([&] { again = std::make_unique<Algo>(factory); });
        REQUIRE(said.find("Loading model") != std::string::npos && said.find("ignoring it") == std::string::npos);
        REQUIRE(ppo_param_count(again->m_ctx) == P);
        std::vector<float> loaded(static_cast<size_t>(P));
        REQUIRE(ppo_params_get_h(again->m_ctx, loaded.data(), P) == PPO_OK);
        REQUIRE(std::memcmp(loaded.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
        std::printf("log_std after %d updates: %g %g %g\n", UPDATES, loaded[static_cast<size_t>(P - 3)], loaded[static_cast<size_t>(P - 2)], loaded[static_cast<size_t>(P - 1)]);
    }
    std::printf("host_gaussian_test ok\n");
    return 0;
}
