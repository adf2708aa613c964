// PPO_HostEnv (PPO/PPO_HostEnv.h) on a GPU: driven by tests/test_gpu_host_env_facade.py, one mode per call, run in a fresh directory.
//   parity   PPO_HostEnv<CartPole> and PPO_Discrete on the same PPOConfig.toml: the same per-update statistics (hex floats), the same console table
//            (time / fps columns aside), the same final parameters and AdamW state, bit for bit
//   width    a user env whose reset returns 3 floats for obs_size 4: the reference's message (PPO_Discrete.cpp:370-375)
//   resume   a checkpoint PPO_HostEnv wrote is picked up by the next PPO_HostEnv in the same directory
//   truncation  `bootstrap_truncated` (16 envs x 32 steps, max_episode_steps 20, 3 updates): absent, PPO_HostEnv trains as PPO_Discrete does; on, every
//            rollout's ppo_host_truncations are the time-limit ends the envs counted themselves, PPO_BUF_REWARDS differs from what CartPole paid (1.0; -1.0
//            where the pole fell) exactly there, and env_groups = 2 ends with the same parameters as env_groups = 1
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../Environments/CartPole.h"
#include "../PPO/PPO_Discrete.h"
#include "../PPO/PPO_HostEnv.h"

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

struct Run { std::vector<std::string> stats; std::string table; std::vector<float> p, m, v; int64_t step = 0; };

template <class Algo> static Run train(Algo& algo) {
    Run r;
    algo.m_on_update = [&](int64_t u, const ppo_stats& s) {
        char b[512];
        std::snprintf(b, sizeof b, "%lld %a %a %a %a %a %a %a %a %a %a %a %a %lld %lld %lld", (long long)u, s.pg_loss, s.v_loss, s.entropy_loss, s.approx_kl,
                      s.loss, s.clipfrac_last, s.clipfrac_mean, s.total_norm, s.explained_variance, s.learning_rate, s.ep_len_mean, s.ep_rew_mean,
                      (long long)s.ep_count, (long long)s.global_step, (long long)s.optimizer_steps);
        r.stats.push_back(b);
    };
    std::stringstream out;
    std::streambuf* old = std::cout.rdbuf(out.rdbuf());
    algo.train();
    std::cout.rdbuf(old);
    std::string line;
    while (std::getline(out, line))   // the table without its clock columns
        if (line.find("time") == std::string::npos && line.find("fps") == std::string::npos && line.find("Saving") == std::string::npos) r.table += line + "\n";
    const int64_t P = ppo_param_count(algo.m_ctx);
    r.p.resize(P); r.m.resize(P); r.v.resize(P);
    if (ppo_params_get_h(algo.m_ctx, r.p.data(), P) != PPO_OK || ppo_optimizer_get_h(algo.m_ctx, r.m.data(), r.v.data(), P, &r.step) != PPO_OK) r.step = -1;
    return r;
}

struct ThreeWide {   // a user env of the wrong width
    explicit ThreeWide(int64_t) {}
    std::vector<float> reset() { return { 0.0f, 0.0f, 0.0f }; }
    std::tuple<std::vector<float>, float, bool, bool> step(const int64_t&) { return { reset(), 1.0f, false, false }; }
    int64_t episode_length = 0;
    float episode_reward = 0.0f;
};

// CartPole that notes, by its own step count, where a time limit (and not the pole) ended an episode
struct ProbeCartPole {
    static constexpr int64_t kLimit = 20;   // = max_episode_steps of writeTruncationConfig
    explicit ProbeCartPole(int64_t seed) : env(seed) {}
    std::vector<float> reset() { auto o = env.reset(); mirror(); return o; }
    std::tuple<std::vector<float>, float, bool, bool> step(const int64_t& a) {
        auto r = env.step(a);
        mirror();
        if (std::get<2>(r)) fell_steps.push_back(steps);
        else if (episode_length == kLimit) cut_steps.push_back(steps);
        steps++;
        return r;
    }
    void mirror() { episode_length = env.episode_length; episode_reward = env.episode_reward; }
    CartPole env;
    int64_t episode_length = 0;
    float episode_reward = 0.0f;
    int64_t steps = 0;
    std::vector<int64_t> cut_steps, fell_steps;   // fell: the pole ended the episode (CartPole's reward is -1 there, 1 everywhere else)
};

// PPO_HostEnv that checks every rollout as it closes against what the envs noted
struct TruncationProbe : PPO_HostEnv<ProbeCartPole> {
    int64_t rollouts = 0, events = 0;
    std::string failure;
    void trainRollout() override {
        PPO_HostEnv<ProbeCartPole>::trainRollout();
        const int64_t T = m_num_steps, N = m_num_envs, u = rollouts++;
        std::vector<int32_t> want;
        for (int64_t n = 0; n < N; n++)
            for (int64_t s : m_envs[static_cast<size_t>(n)]->cut_steps)
                if (s / T == u) want.push_back(static_cast<int32_t>((s % T) * N + n));
        std::sort(want.begin(), want.end());
        int64_t K = -1;
        ppo::check(ppo_host_truncations(m_ctx, &K, nullptr, nullptr, 0), m_ctx, "truncations");
        std::vector<int32_t> idx(static_cast<size_t>(std::max<int64_t>(K, 1)));
        std::vector<float> val(idx.size());
        ppo::check(ppo_host_truncations(m_ctx, &K, idx.data(), val.data(), static_cast<int64_t>(idx.size())), m_ctx, "truncations");
        idx.resize(static_cast<size_t>(K));
        if (!bootstrapTruncated()) want.clear();
        if (idx != want) failure += "rollout " + std::to_string(u) + ": " + std::to_string(K) + " events reported, " + std::to_string(want.size()) + " counted; ";
        events += K;
        ppo::check(ppo_sync(m_ctx), m_ctx, "sync");
        void* p = nullptr;
        size_t bytes = 0;
        ppo::check(ppo_buffer(m_ctx, PPO_BUF_REWARDS, &p, &bytes), m_ctx, "ppo_buffer");
        std::vector<float> rew(static_cast<size_t>(T * N));
        ppo::check(ppo_memcpy_d2h(m_ctx, rew.data(), p, bytes), m_ctx, "rewards");
        std::vector<float> raw(rew.size(), 1.0f);   // what the envs paid: 1, and -1 where the pole fell (CartPole.cpp:80-91)
        for (int64_t n = 0; n < N; n++)
            for (int64_t s : m_envs[static_cast<size_t>(n)]->fell_steps)
                if (s / T == u) raw[static_cast<size_t>((s % T) * N + n)] = -1.0f;
        for (int64_t i = 0; i < T * N; i++) {
            const bool folded = std::binary_search(want.begin(), want.end(), static_cast<int32_t>(i));
            if ((rew[static_cast<size_t>(i)] != raw[static_cast<size_t>(i)]) != folded) { failure += "rollout " + std::to_string(u) + ": reward " + std::to_string(i) + "; "; break; }
        }
    }
};

static uint32_t crc(const std::vector<float>& v) {   // FNV-1a over the bytes: a short name for a parameter vector in the log
    uint32_t h = 2166136261u;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(float); i++) h = (h ^ b[i]) * 16777619u;
    return h;
}

static void writeTruncationConfig(const char* extra) {
    std::ofstream("PPOConfig.toml") << "[environment]\nobs_size = 4\naction_size = 2\nmax_episode_steps = " << ProbeCartPole::kLimit << "\n" << extra
                                    << "[general]\nseed = 3\ntotal_timesteps = 1536\nuse_cuda = true\ncheckpoint_updates = 1000\n"
                                       "[ppo]\nlearning_rate = 0.001\nnum_envs = 16\nnum_steps = 32\nanneal_lr = true\nuse_gae = true\ngamma = 0.98\n"
                                       "gae_lambda = 0.95\nnum_minibatches = 4\nupdate_epochs = 4\nnorm_adv = true\nclip_coef = 0.2\nclip_vloss = true\n"
                                       "ent_coef = 0.0\nvf_coef = 0.5\nmax_grad_norm = 0.5\n";
}

static void writeConfig(int checkpoint_updates) {
    std::ofstream("PPOConfig.toml") << "[environment]\nobs_size = 4\naction_size = 2\nmax_episode_steps = 40\n"
                                       "[general]\nseed = 3\ntotal_timesteps = 1536\nuse_cuda = true\ncheckpoint_updates = " << checkpoint_updates << "\n"
                                       "[ppo]\nlearning_rate = 0.001\nnum_envs = 16\nnum_steps = 32\nanneal_lr = true\nuse_gae = true\ngamma = 0.98\n"
                                       "gae_lambda = 0.95\nnum_minibatches = 4\nupdate_epochs = 4\nnorm_adv = true\nclip_coef = 0.2\nclip_vloss = true\n"
                                       "ent_coef = 0.0\nvf_coef = 0.5\nmax_grad_norm = 0.5\n";
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    try {
        if (mode == "parity") {
            writeConfig(1000);
            Run d, h;
            { PPO_Discrete algo; d = train(algo); }
            { PPO_HostEnv<CartPole> algo; REQUIRE(algo.m_envs.size() == 16); h = train(algo); }
            REQUIRE(d.stats.size() == 3 && h.stats.size() == 3);
            for (size_t i = 0; i < d.stats.size(); i++) {
                std::printf("discrete %s\nhost     %s\n", d.stats[i].c_str(), h.stats[i].c_str());
                REQUIRE(d.stats[i] == h.stats[i]);
            }
            REQUIRE(d.table.find("ep_len_mean") != std::string::npos || d.table.find("rollout/") != std::string::npos);
            if (d.table != h.table) { std::fprintf(stderr, "tables differ:\n%s--- host\n%s", d.table.c_str(), h.table.c_str()); return 1; }
            std::printf("%s", h.table.c_str());
            REQUIRE(d.step == h.step && d.step > 0);
            REQUIRE(d.p == h.p && d.m == h.m && d.v == h.v);
        } else if (mode == "width") {
            writeConfig(1000);
            PPO_HostEnv<ThreeWide> algo;
            try {
                algo.initEnvs();
            } catch (const std::runtime_error& e) {
                const std::string want = "The environment returned an observation of size 3, but your config defined the expected observation size to be 4.\n"
                                         "Have you properly defined your PPOConfig.toml file for your environment?";
                std::printf("%s\n", e.what());
                REQUIRE(want == e.what());
                std::printf("host_env_test width ok\n");
                return 0;
            }
            REQUIRE(!"no exception");
        } else if (mode == "resume") {
            writeConfig(1);
            std::vector<float> p;
            {
                PPO_HostEnv<CartPole> algo;
                Run r = train(algo);
                p = r.p;
                REQUIRE(algo.m_global_step == 1536);
            }
            PPO_HostEnv<CartPole> resumed;   // the newest checkpoint: 3 updates x 16 x 32
            REQUIRE(resumed.m_global_step == 1536);
            std::vector<float> q(p.size());
            REQUIRE(ppo_params_get_h(resumed.m_ctx, q.data(), (int64_t)q.size()) == PPO_OK);
            REQUIRE(q == p);
        } else if (mode == "truncation") {
            Run d, off, on, grouped;
            writeTruncationConfig("");
            { PPO_Discrete algo; d = train(algo); }
            {
                TruncationProbe algo;
                REQUIRE(!algo.bootstrapTruncated());
                off = train(algo);
                std::printf("key absent: %lld rollouts, %lld events %s\n", (long long)algo.rollouts, (long long)algo.events, algo.failure.c_str());
                REQUIRE(algo.rollouts == 3 && algo.events == 0 && algo.failure.empty());
            }
            std::printf("discrete %08x  host, key absent %08x\n", crc(d.p), crc(off.p));
            REQUIRE(d.step > 0 && d.step == off.step && d.p == off.p);
            writeTruncationConfig("bootstrap_truncated = true\n");
            {
                TruncationProbe algo;
                REQUIRE(algo.bootstrapTruncated());
                on = train(algo);
                std::printf("bootstrap_truncated: %lld events in %lld rollouts %s\n", (long long)algo.events, (long long)algo.rollouts, algo.failure.c_str());
                REQUIRE(algo.rollouts == 3 && algo.events > 0 && algo.failure.empty());
            }
            REQUIRE(on.stats.size() == 3 && on.step == d.step && on.p != d.p);
            writeTruncationConfig("env_groups = 2\nbootstrap_truncated = true\n");
            {
                TruncationProbe algo;
                REQUIRE(algo.bootstrapTruncated() && algo.envGroups() == 2);
                grouped = train(algo);
                REQUIRE(algo.rollouts == 3 && algo.events > 0 && algo.failure.empty());
                algo.setBootstrapTruncated(false);
                REQUIRE(!algo.bootstrapTruncated());
            }
            std::printf("env_groups 1 %08x  env_groups 2 %08x\n", crc(on.p), crc(grouped.p));
            REQUIRE(on.p == grouped.p && on.m == grouped.m && on.v == grouped.v && on.stats == grouped.stats);
        } else {
            std::fprintf(stderr, "usage: host_env_test parity|width|resume|truncation\n");
            return 2;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    std::printf("host_env_test %s ok\n", mode.c_str());
    return 0;
}
