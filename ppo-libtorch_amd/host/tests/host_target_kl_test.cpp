// `target_kl` in [ppo] of PPOConfig.toml (PPOAlgorithm::m_target_kl; include/ppo_hip.h ppo_target_kl_set) on a GPU: driven by
// tests/test_gpu_target_kl_facade.py, run in a fresh directory.  PPO_Discrete, 16 envs x 32 steps, 4 minibatches, update_epochs 4, 3 updates.
//   - key absent: the constructor prints nothing about it, the last table says n_updates = 12 and the last statistics optimizer_steps = 48
//   - target_kl = 1e-12 (every update stops behind its first epoch): n_updates = 3, optimizer_steps = 3 * 4, ppo_optimizer_get_h's step likewise, and the
//     context reports (1, 1, kl, 3) with kl the last table's approx_kl
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../PPO/PPO_Discrete.h"

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

struct Run { std::vector<ppo_stats> stats; long long n_updates = -1; int64_t step = -1; std::string said; };

static void writeConfig(const char* extra) {
    std::ofstream("PPOConfig.toml") << "[environment]\nobs_size = 4\naction_size = 2\nmax_episode_steps = 500\n"
                                       "[general]\nseed = 3\ntotal_timesteps = 1536\nuse_cuda = true\ncheckpoint_updates = 1000\n"
                                       "[ppo]\nlearning_rate = 0.003\nnum_envs = 16\nnum_steps = 32\nanneal_lr = false\nuse_gae = true\ngamma = 0.98\n"
                                       "gae_lambda = 0.95\nnum_minibatches = 4\nupdate_epochs = 4\nnorm_adv = true\nclip_coef = 0.2\nclip_vloss = true\n"
                                       "ent_coef = 0.0\nvf_coef = 0.5\nmax_grad_norm = 0.5\n" << extra;
}

// the integer in the LAST n_updates row of the printed tables
static long long lastNUpdates(const std::string& out) {
    const size_t at = out.rfind("n_updates");
    if (at == std::string::npos) return -1;
    const size_t bar = out.find("| ", at);
    return bar == std::string::npos ? -1 : std::atoll(out.c_str() + bar + 2);
}

static Run run(std::unique_ptr<PPO_Discrete>& algo) {
    Run r;
    std::stringstream out;
    std::streambuf* old = std::cout.rdbuf(out.rdbuf());
    std::cout << std::defaultfloat << std::setprecision(6);   // a train() before this one left the table's number format on std::cout
    try {
        algo = std::make_unique<PPO_Discrete>();
        r.said = out.str();
        algo->m_on_update = [&](int64_t, const ppo_stats& s) { r.stats.push_back(s); };
        algo->train();
    } catch (...) { std::cout.rdbuf(old); throw; }
    std::cout.rdbuf(old);
    r.n_updates = lastNUpdates(out.str());
    if (ppo_optimizer_get_h(algo->m_ctx, nullptr, nullptr, ppo_param_count(algo->m_ctx), &r.step) != PPO_OK) r.step = -1;
    return r;
}

int main() {
    try {
        std::unique_ptr<PPO_Discrete> algo;
        writeConfig("");
        const Run off = run(algo);
        REQUIRE(off.said.find("target_kl") == std::string::npos);
        REQUIRE(algo->m_target_kl == 0.0f);
        std::printf("key absent: n_updates %lld optimizer_steps %lld\n", off.n_updates, (long long)off.stats.back().optimizer_steps);
        REQUIRE(off.stats.size() == 3 && off.n_updates == 12 && off.stats.back().optimizer_steps == 48 && off.step == 48);
        for (const ppo_stats& s : off.stats) REQUIRE(s.approx_kl > 1e-12);   // the precondition of the run below, from the run with the feature off

        writeConfig("target_kl = 1e-12\n");
        const Run on = run(algo);
        REQUIRE(on.said.find("Using config file target_kl = 1e-12") != std::string::npos);
        std::printf("Using config file target_kl = 1e-12\n");
        double got = -1.0;
        REQUIRE(ppo_target_kl_get(algo->m_ctx, &got) == PPO_OK && got == static_cast<double>(1e-12f));
        std::printf("target_kl: n_updates %lld optimizer_steps %lld\n", on.n_updates, (long long)on.stats.back().optimizer_steps);
        REQUIRE(on.stats.size() == 3 && on.n_updates == 3 && on.stats.back().optimizer_steps == 3 * 4 && on.step == 3 * 4);
        for (size_t i = 0; i < 3; i++) REQUIRE(on.stats[i].optimizer_steps == 4 * (int64_t)(i + 1));
        int32_t epochs = -1, stopped = -1;
        double kl = -1.0;
        int64_t total = -1;
        REQUIRE(ppo_early_stop_read(algo->m_ctx, &epochs, &stopped, &kl, &total) == PPO_OK);
        REQUIRE(epochs == 1 && stopped == 1 && total == 3 && kl == on.stats.back().approx_kl);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    std::printf("host_target_kl_test ok\n");
    return 0;
}
