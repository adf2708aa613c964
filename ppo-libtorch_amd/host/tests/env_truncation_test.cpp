// `bootstrap_truncated` on the algorithm classes that own their envs (PPO_Discrete; include/ppo_hip.h ppo_env_truncation_bootstrap) on a GPU: driven by
// tests/test_gpu_env_truncation_facade.py, run in a fresh directory.  The config is host_env_test's `truncation` one: 16 envs x 32 steps,
// max_episode_steps 20, 3 updates.
//   - key absent: the constructor prints nothing about it, no event is reported, and the parameters are those of a run whose file says true and whose
//     caller said setBootstrapTruncated(false)
//   - key true: PPO_Discrete ends with the statistics, parameters and AdamW moments of PPO_HostEnv<CartPole> with the same key, bit for bit; the event
//     count is positive and the parameters differ from the key-absent run's
#include <cstdio>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../Environments/CartPole.h"
#include "../PPO/PPO_Discrete.h"
#include "../PPO/PPO_HostEnv.h"

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

struct Run { std::vector<std::string> stats; std::vector<float> p, m, v; int64_t step = 0; };

template <class Algo> static Run train(Algo& algo) {
    Run r;
    algo.m_on_update = [&](int64_t u, const ppo_stats& s) {
        char b[512];
        std::snprintf(b, sizeof b, "%lld %a %a %a %a %a %a %a %a %a %a %a %a %lld %lld %lld", (long long)u, s.pg_loss, s.v_loss, s.entropy_loss, s.approx_kl,
                      s.loss, s.clipfrac_last, s.clipfrac_mean, s.total_norm, s.explained_variance, s.learning_rate, s.ep_len_mean, s.ep_rew_mean,
                      (long long)s.ep_count, (long long)s.global_step, (long long)s.optimizer_steps);
        r.stats.push_back(b);
    };
    std::stringstream out;   // the console table is not under test here
    std::streambuf* old = std::cout.rdbuf(out.rdbuf());
    algo.train();
    std::cout.rdbuf(old);
    const int64_t P = ppo_param_count(algo.m_ctx);
    r.p.resize(P); r.m.resize(P); r.v.resize(P);
    if (ppo_params_get_h(algo.m_ctx, r.p.data(), P) != PPO_OK || ppo_optimizer_get_h(algo.m_ctx, r.m.data(), r.v.data(), P, &r.step) != PPO_OK) r.step = -1;
    return r;
}

// PPO_Discrete that counts every rollout's events as it closes
struct CountingDiscrete : PPO_Discrete {
    int64_t rollouts = 0, events = 0;
    void trainRollout() override {
        PPO_Discrete::trainRollout();
        int64_t K = -1;
        ppo::check(ppo_env_truncations(m_ctx, &K, nullptr, nullptr, 0), m_ctx, "truncations");
        events += K;
        rollouts++;
    }
};

static uint32_t crc(const std::vector<float>& v) {   // FNV-1a over the bytes: a short name for a parameter vector in the log
    uint32_t h = 2166136261u;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(float); i++) h = (h ^ b[i]) * 16777619u;
    return h;
}

static void writeConfig(const char* extra) {
    std::ofstream("PPOConfig.toml") << "[environment]\nobs_size = 4\naction_size = 2\nmax_episode_steps = 20\n" << extra
                                    << "[general]\nseed = 3\ntotal_timesteps = 1536\nuse_cuda = true\ncheckpoint_updates = 1000\n"
                                       "[ppo]\nlearning_rate = 0.001\nnum_envs = 16\nnum_steps = 32\nanneal_lr = true\nuse_gae = true\ngamma = 0.98\n"
                                       "gae_lambda = 0.95\nnum_minibatches = 4\nupdate_epochs = 4\nnorm_adv = true\nclip_coef = 0.2\nclip_vloss = true\n"
                                       "ent_coef = 0.0\nvf_coef = 0.5\nmax_grad_norm = 0.5\n";
}

// constructs with std::cout captured into `said`
template <class Algo> static std::unique_ptr<Algo> construct(std::string& said) {
    std::stringstream out;
    std::streambuf* old = std::cout.rdbuf(out.rdbuf());
    std::unique_ptr<Algo> algo;
    try { algo = std::make_unique<Algo>(); } catch (...) { std::cout.rdbuf(old); throw; }
    std::cout.rdbuf(old);
    said = out.str();
    return algo;
}

int main() {
    try {
        Run absent, off, on, host;
        std::string said;
        writeConfig("");
        {
            auto algo = construct<CountingDiscrete>(said);
            REQUIRE(said.find("bootstrap_truncated") == std::string::npos);
            REQUIRE(!algo->bootstrapTruncated());
            absent = train(*algo);
            REQUIRE(algo->rollouts == 3 && algo->events == 0);
        }
        writeConfig("bootstrap_truncated = true\n");
        {
            auto algo = construct<CountingDiscrete>(said);
            REQUIRE(said.find("Using config file bootstrap_truncated = true") != std::string::npos);
            std::printf("Using config file bootstrap_truncated = true\n");
            REQUIRE(algo->bootstrapTruncated());
            algo->setBootstrapTruncated(false);
            REQUIRE(!algo->bootstrapTruncated());
            off = train(*algo);
            REQUIRE(algo->rollouts == 3 && algo->events == 0);
        }
        std::printf("key absent %08x  setBootstrapTruncated(false) %08x\n", crc(absent.p), crc(off.p));
        REQUIRE(absent.step > 0 && absent.step == off.step && crc(absent.p) == crc(off.p) && absent.p == off.p && absent.stats == off.stats);
        {
            auto algo = construct<CountingDiscrete>(said);
            REQUIRE(algo->bootstrapTruncated());
            on = train(*algo);
            std::printf("bootstrap_truncated: %lld events in %lld rollouts\n", (long long)algo->events, (long long)algo->rollouts);
            REQUIRE(algo->rollouts == 3 && algo->events > 0);
        }
        {
            auto algo = construct<PPO_HostEnv<CartPole>>(said);
            REQUIRE(algo->bootstrapTruncated());
            host = train(*algo);
        }
        REQUIRE(on.stats.size() == 3 && host.stats.size() == 3);
        for (size_t i = 0; i < on.stats.size(); i++) std::printf("discrete %s\nhost     %s\n", on.stats[i].c_str(), host.stats[i].c_str());
        std::printf("PPO_Discrete %08x  PPO_HostEnv<CartPole> %08x\n", crc(on.p), crc(host.p));
        REQUIRE(on.step == absent.step && on.p != absent.p);
        REQUIRE(on.step == host.step && on.p == host.p && on.m == host.m && on.v == host.v && on.stats == host.stats);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    std::printf("env_truncation_test ok\n");
    return 0;
}
