// PPO_HostEnv (PPO/PPO_HostEnv.h) on a GPU: driven by tests/test_gpu_host_env_facade.py, one mode per call, run in a fresh directory.
//   parity   PPO_HostEnv<CartPole> and PPO_Discrete on the same PPOConfig.toml: the same per-update statistics (hex floats), the same console table
//            (time / fps columns aside), the same final parameters and AdamW state, bit for bit
//   width    a user env whose reset returns 3 floats for obs_size 4: the reference's message (PPO_Discrete.cpp:370-375)
//   resume   a checkpoint PPO_HostEnv wrote is picked up by the next PPO_HostEnv in the same directory
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
        } else {
            std::fprintf(stderr, "usage: host_env_test parity|width|resume\n");
            return 2;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    std::printf("host_env_test %s ok\n", mode.c_str());
    return 0;
}
