// `keep_cut_states = true` in [environment] (PPO_KERNEL_ENV_CUT_STATE through the facade; include/ppo_hip.h) on a GPU, driven by
// tests/test_gpu_cut_state_facade.py in a fresh directory: PPO_Continuous (Pendulum) and PPO_DiscreteAcrobot -- two classes whose env refuses
// bootstrap_truncated without the key -- train two iterations with both keys, ppo_env_truncations reports events, the checkpoint loads into a fresh object
// with bit-equal parameters; the same file without keep_cut_states throws the library's refusal, and PPO_Discrete refuses the key with the library's message.
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
#include "../PPO/PPO_Discrete.h"
#include "../PPO/PPO_DiscreteAcrobot.h"

namespace fs = std::filesystem;

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 64, T = 32, UPDATES = 2, LIMIT = 5;

static void writeConfig(int obs_size, const std::string& extra) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = " << obs_size << "\nmax_episode_steps = " << LIMIT << "\n" << extra
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

template <class Algo> static int run(const char* name, int obs_size, int family_flag, const char* refusal) {
    fs::remove_all("./ModelCheckpoints");
    writeConfig(obs_size, "bootstrap_truncated = true\nkeep_cut_states = true\n");
    std::vector<float> trained;
    int64_t P = 0;
    {
        std::unique_ptr<Algo> algo;
        const std::string said = captured([&] { algo = std::make_unique<Algo>(); });
        REQUIRE(said.find("Using config file keep_cut_states = true") != std::string::npos);
        ppo_config cfg{};
        REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK);
        REQUIRE((cfg.kernel_flags & PPO_KERNEL_ENV_CUT_STATE) && (cfg.kernel_flags & family_flag) && cfg.max_episode_steps == LIMIT && algo->bootstrapTruncated());
        P = ppo_param_count(algo->m_ctx);
        int finite = 0;
        double ep_len = 0.0;
        algo->m_on_update = [&](int64_t, const ppo_stats& s) {
            finite += std::isfinite(s.loss) && std::isfinite(s.v_loss) && std::isfinite(s.explained_variance) ? 1 : 0;
            ep_len = s.ep_len_mean;
        };
        const std::string table = captured([&] { algo->train(); });
        REQUIRE(finite == UPDATES && table.find("rollout/") != std::string::npos && ep_len == static_cast<double>(LIMIT));
        int64_t events = 0;
        REQUIRE(ppo_env_truncations(algo->m_ctx, &events, nullptr, nullptr, 0) == PPO_OK);
        std::printf("%s: %lld truncation events in the last rollout\n", name, (long long)events);
        // neither env terminates within five steps of a reset: every sample whose episode reached the limit is an event
        REQUIRE(events > 0 && events <= static_cast<int64_t>(N) * T && events >= static_cast<int64_t>(N));
        std::vector<int32_t> idx(static_cast<size_t>(events));
        std::vector<float> val(static_cast<size_t>(events));
        REQUIRE(ppo_env_truncations(algo->m_ctx, &events, idx.data(), val.data(), events) == PPO_OK);
        for (size_t k = 0; k < idx.size(); k++) REQUIRE(std::isfinite(val[k]) && idx[k] >= 0 && idx[k] < N * T && (k == 0 || idx[k] > idx[k - 1]));
        trained.resize(static_cast<size_t>(P));
        REQUIRE(ppo_params_get_h(algo->m_ctx, trained.data(), P) == PPO_OK);
        algo->setBootstrapTruncated(false);
        REQUIRE(!algo->bootstrapTruncated());
    }
    const std::string ckpt = "./ModelCheckpoints/PPO_Agent_" + std::to_string(N * T * UPDATES) + "_steps.pt";
    REQUIRE(fs::exists(ckpt));
    {
        std::unique_ptr<Algo> again;
        const std::string said = captured([&] { again = std::make_unique<Algo>(); });
        REQUIRE(said.find("Loading model") != std::string::npos && said.find("ignoring it") == std::string::npos);
        std::vector<float> loaded(static_cast<size_t>(P));
        REQUIRE(ppo_param_count(again->m_ctx) == P && ppo_params_get_h(again->m_ctx, loaded.data(), P) == PPO_OK);
        REQUIRE(std::memcmp(loaded.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
    }
    fs::remove_all("./ModelCheckpoints");
    {   // the same file without the key: the library's refusal, as before
        writeConfig(obs_size, "bootstrap_truncated = true\n");
        std::string what;
        try {
            captured([&] { Algo refused; });
        } catch (const std::exception& e) {
            what = e.what();
        }
        std::printf("%s without keep_cut_states: %s\n", name, what.c_str());
        REQUIRE(what.find(refusal) != std::string::npos);
    }
    return 0;
}

int main() {
    if (run<PPO_Continuous>("PPO_Continuous", 3, PPO_KERNEL_GAUSS_FUSED, "does not hold theta")) return 1;
    if (run<PPO_DiscreteAcrobot>("PPO_DiscreteAcrobot", 6, PPO_KERNEL_CAT_FUSED, "does not hold the angles")) return 1;
    {   // a class whose env is no fused device env refuses the key with the library's message
        std::ofstream("PPOConfig.toml") << "[environment]\nobs_size = 4\naction_size = 2\nmax_episode_steps = 500\nkeep_cut_states = true\n"
                                           "[general]\nseed = 3\ntotal_timesteps = 1024\nuse_cuda = true\ncheckpoint_updates = 1000\n"
                                           "[ppo]\nnum_envs = 16\nnum_steps = 32\nnum_minibatches = 4\nupdate_epochs = 4\n";
        std::string what;
        try {
            captured([&] { PPO_Discrete refused; });
        } catch (const std::exception& e) {
            what = e.what();
        }
        std::printf("PPO_Discrete with keep_cut_states: %s\n", what.c_str());
        REQUIRE(what.find("PPO_KERNEL_ENV_CUT_STATE serves the device envs of the fused 2 x 64 families only") != std::string::npos);
    }
    std::printf("host_cut_state_test ok\n");
    return 0;
}
