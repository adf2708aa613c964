// PPO_Continuous (PPO/PPO_Continuous.h: a Gaussian policy on the device's Pendulum-v1) on a GPU, driven by tests/test_gpu_pendulum_facade.py in a fresh
// directory: two iterations train on the fused rollout (the act counter stays 0: no per-step launch), the checkpoint loads into a fresh object with
// bit-equal parameters, log_std moved, and the host-side Pendulum class steps with the library's arithmetic.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../PPO/PPO_Continuous.h"

namespace fs = std::filesystem;

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 64, T = 32, UPDATES = 2;

static void writeConfig(const std::string& extra) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = 3\nmax_episode_steps = 20\n" << extra
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
    writeConfig("");
    std::vector<float> trained;
    int64_t P = 0;
    {
        std::unique_ptr<PPO_Continuous> algo;
        captured([&] { algo = std::make_unique<PPO_Continuous>(); });
        ppo_config cfg{};
        REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK);
        REQUIRE(cfg.env_kind == PPO_ENV_PENDULUM && cfg.dist_kind == PPO_DIST_GAUSSIAN && (cfg.kernel_flags & PPO_KERNEL_GAUSS_FUSED) && cfg.max_episode_steps == 20);
        REQUIRE(algo->actionDim() == 1 && algo->m_obs_size == 3);
        P = ppo_param_count(algo->m_ctx);
        REQUIRE(P == 2 * (64 * 3 + 64 + 64 * 64 + 64) + (64 + 1) + (64 + 1) + 1);
        int finite = 0;
        double ep_len = 0.0;
        algo->m_on_update = [&](int64_t, const ppo_stats& s) {
            finite += std::isfinite(s.loss) && std::isfinite(s.entropy_loss) && std::isfinite(s.explained_variance) ? 1 : 0;
            ep_len = s.ep_len_mean;
        };
        const std::string table = captured([&] { algo->train(); });
        REQUIRE(finite == UPDATES && table.find("rollout/") != std::string::npos && ep_len == 20.0);
        int64_t act = 0, value = 0, update = 0;
        REQUIRE(ppo_gauss_fused_launches(algo->m_ctx, &act, &value, &update) == PPO_OK);
        std::printf("fused launches: act %lld value %lld update %lld\n", (long long)act, (long long)value, (long long)update);
        REQUIRE(act == 0 && value >= UPDATES * 2 && update == UPDATES * 4 * 4);
        trained.resize(static_cast<size_t>(P));
        REQUIRE(ppo_params_get_h(algo->m_ctx, trained.data(), P) == PPO_OK);
        REQUIRE(trained[static_cast<size_t>(P - 1)] != 0.0f);   // log_std was stepped
        // what the class leaves to later work is refused with the library's words
        std::string refusal;
        try { algo->evaluate(4); } catch (const std::runtime_error& e) { refusal = e.what(); }
        std::printf("refusal: %s\n", refusal.c_str());
        REQUIRE(refusal.find("ppo_env_transition_f32") != std::string::npos);
    }
    const std::string ckpt = "./ModelCheckpoints/PPO_Agent_" + std::to_string(N * T * UPDATES) + "_steps.pt";
    REQUIRE(fs::exists(ckpt));
    {
        std::unique_ptr<PPO_Continuous> again;
        const std::string said = captured([&] { again = std::make_unique<PPO_Continuous>(); });
        REQUIRE(said.find("Loading model") != std::string::npos && said.find("ignoring it") == std::string::npos);
        std::vector<float> loaded(static_cast<size_t>(P));
        REQUIRE(ppo_param_count(again->m_ctx) == P && ppo_params_get_h(again->m_ctx, loaded.data(), P) == PPO_OK);
        REQUIRE(std::memcmp(loaded.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
    }
    {   // the host class: a raw action beyond the torque range steps like its clipped copy, and the observation is that of the new state
        Pendulum a(nullptr, 7, 0), b(nullptr, 7, 0);
        const std::vector<float> o0 = a.reset();
        REQUIRE(o0 == b.reset() && o0.size() == 3 && std::fabs(o0[0] * o0[0] + o0[1] * o0[1] - 1.0f) < 1e-6f && a.state.size() == 2);
        auto [oa, ra, ta, ua] = a.step({ 5.0f });
        auto [ob, rb, tb, ub] = b.step({ 2.0f });
        REQUIRE(oa == ob && ra == rb && !ta && !tb && !ua && !ub && ra < 0.0f && a.episode_length == 1 && a.episode_reward == ra);
        REQUIRE(std::fabs(oa[0] - std::cos(a.state[0])) < 1e-6f && std::fabs(oa[1] - std::sin(a.state[0])) < 1e-6f && oa[2] == a.state[1]);
    }
    std::printf("host_pendulum_test ok\n");
    return 0;
}
