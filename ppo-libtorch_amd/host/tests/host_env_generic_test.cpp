// `[network] hidden_size = H` of PPOConfig.toml (PPO_KERNEL_ENV_GENERIC through the facade; include/ppo_hip.h) on a GPU: driven by
// tests/test_gpu_env_generic_facade.py, run in a fresh directory.  PPO_Discrete and PPO_MultiDiscrete, 16 envs x 32 steps, 2 updates.
//   - key absent: nothing is printed about it, the context's kernel_flags lacks the bit, hidden is 64
//   - hidden_size = 128: the key prints like the other extension keys, the context carries the flag and a 2 x 128 network, two iterations train with finite
//     statistics, evaluate() and setBootstrapTruncated(true) throw the library's refusal, the checkpoint is written with the width and loads into a fresh
//     object with the same key with bit-equal parameters, AdamW moments and step count
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../PPO/PPO_Discrete.h"
#include "../PPO/PPO_MultiDiscrete.h"

namespace fs = std::filesystem;

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 16, T = 32, UPDATES = 2, H = 128;

static void writeConfig(int obs, int act, const std::string& network) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = " << obs << "\naction_size = " << act << "\nmax_episode_steps = 20\n" << network   // (episodes end inside the run on MountainCar too: the table has its rollout/ rows)
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

template <class Algo> static int run(const char* name, int obs, int act) {
    std::error_code ec;
    fs::remove_all("./ModelCheckpoints", ec);
    fs::remove_all("./OptimizerCheckpoints", ec);
    // the key absent: nothing printed about it, no flag, the reference's width
    writeConfig(obs, act, "");
    {
        std::unique_ptr<Algo> plain;
        const std::string said = captured([&] { plain = std::make_unique<Algo>(); });
        REQUIRE(said.find("hidden_size") == std::string::npos);
        ppo_config cfg{};
        cfg.struct_size = sizeof cfg;
        REQUIRE(ppo_get_config(plain->m_ctx, &cfg) == PPO_OK && (cfg.kernel_flags & PPO_KERNEL_ENV_GENERIC) == 0 && cfg.hidden == 64 && cfg.n_hidden == 2);
        REQUIRE(!plain->m_hidden_size_given && plain->m_hidden_size == 64);
    }
    const std::string network = "[network]\nhidden_size = " + std::to_string(H) + "\n";
    writeConfig(obs, act, network);
    std::vector<float> trained, trained_m, trained_v;
    int64_t P = 0, trained_step = -1;
    {
        std::unique_ptr<Algo> algo;
        const std::string said = captured([&] { algo = std::make_unique<Algo>(); });
        REQUIRE(said.find("Using config file hidden_size = " + std::to_string(H)) != std::string::npos);
        ppo_config cfg{};
        cfg.struct_size = sizeof cfg;
        REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK && (cfg.kernel_flags & PPO_KERNEL_ENV_GENERIC) != 0 && cfg.hidden == H && cfg.n_hidden == 2);
        P = ppo_param_count(algo->m_ctx);
        REQUIRE(P == 2 * (H * obs + H + H * H + H) + (H + 1) + (H * act + act));
        int finite = 0;
        int64_t steps = 0;
        algo->m_on_update = [&](int64_t, const ppo_stats& s) {
            finite += std::isfinite(s.loss) && std::isfinite(s.entropy_loss) && std::isfinite(s.explained_variance) ? 1 : 0;
            steps = s.optimizer_steps;
        };
        const std::string table = captured([&] { algo->train(); });
        REQUIRE(finite == UPDATES && steps == UPDATES * 4 * 4 && table.find("rollout/") != std::string::npos);
        trained.resize(static_cast<size_t>(P));
        REQUIRE(ppo_params_get_h(algo->m_ctx, trained.data(), P) == PPO_OK);
        for (float x : trained) REQUIRE(std::isfinite(x));
        trained_m.resize(static_cast<size_t>(P));
        trained_v.resize(static_cast<size_t>(P));
        REQUIRE(ppo_optimizer_get_h(algo->m_ctx, trained_m.data(), trained_v.data(), P, &trained_step) == PPO_OK && trained_step == UPDATES * 4 * 4);
        // what the class offers and the flagged context refuses is thrown with the library's words
        bool threw = false;
        try { algo->evaluate(4); } catch (const std::runtime_error& e) { threw = std::string(e.what()).find("PPO_KERNEL_ENV_GENERIC") != std::string::npos; }
        REQUIRE(threw);
        threw = false;
        try { algo->setBootstrapTruncated(true); } catch (const std::runtime_error& e) { threw = std::string(e.what()).find("PPO_KERNEL_ENV_GENERIC") != std::string::npos; }
        REQUIRE(threw && !algo->bootstrapTruncated());
    }
    const std::string ckpt = "./ModelCheckpoints/PPO_Agent_" + std::to_string(N * T * UPDATES) + "_steps.pt";
    REQUIRE(fs::exists(ckpt));
    // the checkpoint into a fresh object with the same key: bit-equal parameters
    {
        std::unique_ptr<Algo> again;
        const std::string said = captured([&] { again = std::make_unique<Algo>(); });
        REQUIRE(said.find("Loading model") != std::string::npos && said.find("ignoring it") == std::string::npos);
        std::vector<float> loaded(static_cast<size_t>(P));
        REQUIRE(ppo_param_count(again->m_ctx) == P && ppo_params_get_h(again->m_ctx, loaded.data(), P) == PPO_OK);
        REQUIRE(std::memcmp(loaded.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
        // ... and AdamW's moments and step count (OptimizerCheckpoints)
        std::vector<float> m(static_cast<size_t>(P)), v(static_cast<size_t>(P));
        int64_t step = -1;
        REQUIRE(ppo_optimizer_get_h(again->m_ctx, m.data(), v.data(), P, &step) == PPO_OK && step == trained_step);
        REQUIRE(std::memcmp(m.data(), trained_m.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
        REQUIRE(std::memcmp(v.data(), trained_v.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
    }
    // ... and an object without the key says that the file is not its agent's and starts fresh
    writeConfig(obs, act, "");
    {
        std::unique_ptr<Algo> other;
        const std::string said = captured([&] { other = std::make_unique<Algo>(); });
        REQUIRE(said.find("ignoring it") != std::string::npos);
    }
    std::printf("%s: hidden_size = %d trained %d updates, %lld parameters round-trip\n", name, H, UPDATES, (long long)P);
    return 0;
}

int main() {
    try {
        if (run<PPO_Discrete>("PPO_Discrete", 4, 2) != 0) return 1;
        if (run<PPO_MultiDiscrete>("PPO_MultiDiscrete", 2, 3) != 0) return 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    std::printf("host_env_generic_test ok\n");
    return 0;
}
