// `matrix_cores = true` in [environment] on a fused device-env class (PPO_KERNEL_ENV_MATRIX through the facade; include/ppo_hip.h) on a GPU, driven by
// tests/test_gpu_env_matrix_facade.py in a fresh directory: PPO_MultiDiscreteTaxi reads the key, its context carries PPO_KERNEL_ENV_MATRIX next to
// PPO_KERNEL_CAT_FUSED (and not PPO_KERNEL_FUSED_MATRIX, the flag of the caller-stepped classes), one iteration trains on the matrix kernels, and
// bootstrap_truncated beside the key throws the library's refusal naming the flag.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../PPO/PPO_MultiDiscreteTaxi.h"

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 64, T = 32;

static void writeConfig(const std::string& extra) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = 19\nmax_episode_steps = 20\nmatrix_cores = true\n" << extra
      << "[general]\nseed = 3\ntotal_timesteps = " << N * T << "\nuse_cuda = true\ncheckpoint_updates = 1000\n"
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
    {
        std::unique_ptr<PPO_MultiDiscreteTaxi> algo;
        const std::string said = captured([&] { algo = std::make_unique<PPO_MultiDiscreteTaxi>(); });
        REQUIRE(said.find("Using config file matrix_cores = true") != std::string::npos);
        ppo_config cfg{};
        REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK);
        REQUIRE(cfg.kernel_flags == (PPO_KERNEL_CAT_FUSED | PPO_KERNEL_ENV_MATRIX));
        int finite = 0;
        algo->m_on_update = [&](int64_t, const ppo_stats& s) {
            finite += std::isfinite(s.loss) && std::isfinite(s.v_loss) && std::isfinite(s.explained_variance) ? 1 : 0;
        };
        const std::string table = captured([&] { algo->train(); });
        REQUIRE(finite == 1 && table.find("rollout/") != std::string::npos);
        int64_t act = 0, crit = 0, upd = 0;
        REQUIRE(ppo_gauss_fused_launches(algo->m_ctx, &act, &crit, &upd) == PPO_OK);
        std::printf("PPO_MultiDiscreteTaxi with matrix_cores: fused launches act %lld critic %lld update %lld\n", (long long)act, (long long)crit, (long long)upd);
        REQUIRE(crit >= 2 && upd == 16);   // the rollout's two critic launches; 4 epochs x 4 minibatches
    }
    {   // the time-limit bootstrap is not built under the flag: the library's refusal
        writeConfig("bootstrap_truncated = true\n");
        std::string what;
        try {
            captured([&] { PPO_MultiDiscreteTaxi refused; });
        } catch (const std::exception& e) {
            what = e.what();
        }
        std::printf("refusal: %s\n", what.c_str());
        REQUIRE(what.find("PPO_KERNEL_ENV_MATRIX") != std::string::npos);
    }
    std::printf("host_env_matrix_test ok\n");
    return 0;
}
