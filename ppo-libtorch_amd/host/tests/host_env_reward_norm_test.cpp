// `norm_reward = true` in [environment] on a fused device-env class (PPO_KERNEL_ENV_REWARD_NORM through the facade; include/ppo_hip.h) on a GPU, driven by
// tests/test_gpu_env_reward_norm_facade.py in a fresh directory: PPO_Continuous (Pendulum) trains two iterations with the key, its context carries the flag,
// the ".rewnorm" file beside the checkpoint holds what ppo_reward_norm_get_h returns and loads into a fresh object; the same file without the key creates the
// context without the flag, is refused the three calls as before, writes no statistics file and trains to other parameters.
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

static const int N = 64, T = 32, UPDATES = 2, LIMIT = 8;

static void writeConfig(const std::string& extra) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = 3\nmax_episode_steps = " << LIMIT << "\n" << extra
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

// trains UPDATES iterations; -> the parameters, the last ep_rew_mean, and the context's flags / statistics through the out arguments
static int train(PPO_Continuous& algo, std::vector<float>& params, double& ep_rew) {
    int finite = 0;
    algo.m_on_update = [&](int64_t, const ppo_stats& s) {
        finite += std::isfinite(s.loss) && std::isfinite(s.v_loss) ? 1 : 0;
        ep_rew = s.ep_rew_mean;
    };
    captured([&] { algo.train(); });
    REQUIRE(finite == UPDATES);
    params.resize(static_cast<size_t>(ppo_param_count(algo.m_ctx)));
    REQUIRE(ppo_params_get_h(algo.m_ctx, params.data(), static_cast<int64_t>(params.size())) == PPO_OK);
    return 0;
}

int main() {
    const std::string ckpt = "./ModelCheckpoints/PPO_Agent_" + std::to_string(N * T * UPDATES) + "_steps.pt";
    std::vector<float> with_key, without_key;
    double mean = 0.0, var = 0.0, count = 0.0, ep_rew = 0.0;
    fs::remove_all("./ModelCheckpoints");
    writeConfig("norm_reward = true\n");
    {
        std::unique_ptr<PPO_Continuous> algo;
        const std::string said = captured([&] { algo = std::make_unique<PPO_Continuous>(); });
        REQUIRE(said.find("Using config file norm_reward = true") != std::string::npos);
        ppo_config cfg{};
        REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK);
        REQUIRE((cfg.kernel_flags & PPO_KERNEL_ENV_REWARD_NORM) && (cfg.kernel_flags & PPO_KERNEL_GAUSS_FUSED) && !(cfg.kernel_flags & PPO_KERNEL_ENV_CUT_STATE));
        if (train(*algo, with_key, ep_rew)) return 1;
        REQUIRE(ppo_reward_norm_get_h(algo->m_ctx, &mean, &var, &count, nullptr, 0) == PPO_OK);
        std::printf("with norm_reward: count %.0f mean %.6g var %.6g ep_rew_mean %.6g\n", count, mean, var, ep_rew);
        REQUIRE(count == static_cast<double>(UPDATES) * T * N && var > 0.0 && std::isfinite(mean) && std::isfinite(var));
        REQUIRE(ep_rew < -1.0 * LIMIT && ep_rew >= -16.2736 * LIMIT);   // raw units: an episode is LIMIT steps at -16.27 at the worst
    }
    {   // the file beside the checkpoint: count, mean, var as ppo_reward_norm_get_h returned them, bit for bit
        const RewardNormFile f = RewardNormFile::read(RewardNormFile::pathFor(ckpt));
        REQUIRE(fs::file_size(RewardNormFile::pathFor(ckpt)) == 24);
        REQUIRE(std::memcmp(&f.mean, &mean, 8) == 0 && std::memcmp(&f.var, &var, 8) == 0 && std::memcmp(&f.count, &count, 8) == 0);
    }
    {   // a fresh object resumes from the checkpoint: parameters and statistics
        std::unique_ptr<PPO_Continuous> again;
        const std::string said = captured([&] { again = std::make_unique<PPO_Continuous>(); });
        REQUIRE(said.find("Loading model") != std::string::npos && said.find("Loading reward statistics") != std::string::npos && said.find("ignoring it") == std::string::npos);
        std::vector<float> loaded(with_key.size());
        REQUIRE(ppo_params_get_h(again->m_ctx, loaded.data(), static_cast<int64_t>(loaded.size())) == PPO_OK);
        REQUIRE(std::memcmp(loaded.data(), with_key.data(), loaded.size() * sizeof(float)) == 0);
        double m2 = 0.0, v2 = 0.0, c2 = 0.0;
        std::vector<double> ret(N, 1.0);
        REQUIRE(ppo_reward_norm_get_h(again->m_ctx, &m2, &v2, &c2, ret.data(), N) == PPO_OK);
        REQUIRE(std::memcmp(&m2, &mean, 8) == 0 && std::memcmp(&v2, &var, 8) == 0 && c2 == count);
        for (double r : ret) REQUIRE(r == 0.0);   // the accumulators are not saved: a resume resets the envs
    }
    for (const char* dir : { "./ModelCheckpoints", "./OptimizerCheckpoints", "./Models" }) fs::remove_all(dir);
    writeConfig("");
    {   // the same file without the key: what it ran before
        std::unique_ptr<PPO_Continuous> algo;
        captured([&] { algo = std::make_unique<PPO_Continuous>(); });
        ppo_config cfg{};
        REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK);
        REQUIRE(cfg.kernel_flags == PPO_KERNEL_GAUSS_FUSED);
        double ep_rew_raw = 0.0;
        if (train(*algo, without_key, ep_rew_raw)) return 1;
        REQUIRE(ppo_reward_norm_get_h(algo->m_ctx, &mean, &var, &count, nullptr, 0) == PPO_ERR_UNSUPPORTED);
        REQUIRE(std::string(ppo_last_error(algo->m_ctx)).find("reward normalisation serves PPO_ENV_HOST contexts") != std::string::npos);
        REQUIRE(fs::exists(ckpt) && !fs::exists(RewardNormFile::pathFor(ckpt)));
        REQUIRE(without_key.size() == with_key.size() && std::memcmp(without_key.data(), with_key.data(), with_key.size() * sizeof(float)) != 0);
        std::printf("without norm_reward: ep_rew_mean %.6g\n", ep_rew_raw);
    }
    std::printf("host_env_reward_norm_test ok\n");
    return 0;
}
