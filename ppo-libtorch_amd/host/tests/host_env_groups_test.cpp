// PPO_HostEnv's env groups (PPO/PPO_HostEnv.h: setEnvGroups / `env_groups` in PPOConfig.toml) on a GPU: driven by
// tests/test_gpu_host_env_groups_facade.py, run in a fresh directory.  PPO_HostEnv<CartPole> trained with 1, 2 and 3 env groups -- 2 through the config
// file's key, 3 through setEnvGroups, 16 envs so that three groups are 5 + 5 + 6 -- ends with the same per-update statistics (hex floats), the same
// console table (time / fps columns aside), the same parameters and the same AdamW state, bit for bit.  Then the masked pipeline (masks gathered group
// by group): PPO_HostEnv<MaskEnv, true>, a user env whose action mask changes with every step and differs from env to env, with 1 and 3 groups.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../Environments/CartPole.h"
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

// a user env with three actions, one of them forbidden at any time: which one depends on the env and on the step
struct MaskEnv {
    explicit MaskEnv(int64_t index) : idx(index) {}
    std::vector<float> obs() const { return { x, v, static_cast<float>(episode_length) / 32.0f, static_cast<float>(idx % 5) / 5.0f }; }
    std::vector<float> reset() { x = 0.01f * static_cast<float>(idx % 7); v = 0.0f; episode_length = 0; episode_reward = 0.0f; return obs(); }
    std::tuple<std::vector<float>, float, bool, bool> step(const int64_t& a) {
        if (a == forbidden()) broke_mask = true;
        v += 0.05f * static_cast<float>(a - 1);
        x += v;
        episode_length++;
        const float r = 1.0f - (x < 0.0f ? -x : x);
        episode_reward += r;
        const bool done = x > 1.0f || x < -1.0f || episode_length >= 11 + idx % 6;
        return { obs(), r, done, false };
    }
    int64_t forbidden() const { return (episode_length + idx) % 3; }
    std::vector<bool> getActionMask() const { const int64_t f = forbidden(); return { f != 0, f != 1, f != 2 }; }
    int64_t idx;
    float x = 0.0f, v = 0.0f;
    int64_t episode_length = 0;
    float episode_reward = 0.0f;
    bool broke_mask = false;
};

static void writeConfig(int env_groups, int actions = 2) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = 4\naction_size = " << actions << "\nmax_episode_steps = 40\n";
    if (env_groups > 0) f << "env_groups = " << env_groups << "\n";
    f << "[general]\nseed = 3\ntotal_timesteps = 1536\nuse_cuda = true\ncheckpoint_updates = 1000\n"
         "[ppo]\nlearning_rate = 0.001\nnum_envs = 16\nnum_steps = 32\nanneal_lr = true\nuse_gae = true\ngamma = 0.98\n"
         "gae_lambda = 0.95\nnum_minibatches = 4\nupdate_epochs = 4\nnorm_adv = true\nclip_coef = 0.2\nclip_vloss = true\n"
         "ent_coef = 0.0\nvf_coef = 0.5\nmax_grad_norm = 0.5\n";
}

// what the constructor prints (getArgs and the device lines)
template <class Make> static std::string constructorOutput(Make make) {
    std::stringstream out;
    std::streambuf* old = std::cout.rdbuf(out.rdbuf());
    try { make(); } catch (...) { std::cout.rdbuf(old); throw; }
    std::cout.rdbuf(old);
    return out.str();
}

int main() {
    try {
        Run one, two, three;
        std::string said_one, said_two;
        writeConfig(0);
        said_one = constructorOutput([&] { PPO_HostEnv<CartPole> algo; if (algo.envGroups() != 1) throw std::runtime_error("default env groups"); });
        { PPO_HostEnv<CartPole> algo; one = train(algo); }
        writeConfig(2);
        said_two = constructorOutput([&] { PPO_HostEnv<CartPole> algo; if (algo.envGroups() != 2) throw std::runtime_error("env_groups key not read"); });
        { PPO_HostEnv<CartPole> algo; REQUIRE(algo.envGroups() == 2); two = train(algo); }
        writeConfig(0);
        {
            PPO_HostEnv<CartPole> algo;
            algo.setEnvGroups(3);
            REQUIRE(algo.envGroups() == 3);
            three = train(algo);
            bool refused = false;
            try { algo.setEnvGroups(PPO_HOST_MAX_GROUPS + 1); } catch (const std::runtime_error&) { refused = true; }
            REQUIRE(refused && algo.envGroups() == 3);
        }
        REQUIRE(said_one.find("env_groups") == std::string::npos);   // an absent key prints nothing
        REQUIRE(said_two.find("Using config file env_groups = 2") != std::string::npos);
        REQUIRE(one.stats.size() == 3 && two.stats.size() == 3 && three.stats.size() == 3);
        for (size_t i = 0; i < one.stats.size(); i++) {
            std::printf("groups 1 %s\ngroups 2 %s\ngroups 3 %s\n", one.stats[i].c_str(), two.stats[i].c_str(), three.stats[i].c_str());
            REQUIRE(one.stats[i] == two.stats[i] && one.stats[i] == three.stats[i]);
        }
        REQUIRE(one.table.find("rollout/") != std::string::npos);
        if (one.table != two.table || one.table != three.table) {
            std::fprintf(stderr, "tables differ:\n%s--- 2 groups\n%s--- 3 groups\n%s", one.table.c_str(), two.table.c_str(), three.table.c_str());
            return 1;
        }
        std::printf("%s", one.table.c_str());
        REQUIRE(one.step > 0 && one.step == two.step && one.step == three.step);
        REQUIRE(one.p == two.p && one.m == two.m && one.v == two.v);
        REQUIRE(one.p == three.p && one.m == three.m && one.v == three.v);

        writeConfig(0, 3);
        Run m1, m3;
        auto factory = [](int64_t i) { return std::make_shared<MaskEnv>(i); };
        for (int groups : { 1, 3 }) {
            PPO_HostEnv<MaskEnv, true> algo(factory);
            algo.setEnvGroups(groups);
            (groups == 1 ? m1 : m3) = train(algo);
            for (const auto& e : algo.m_envs) REQUIRE(!e->broke_mask);   // every action taken was allowed by the mask gathered for its step
        }
        REQUIRE(m1.stats.size() == 3 && m3.stats.size() == 3);
        for (size_t i = 0; i < m1.stats.size(); i++) {
            std::printf("masked groups 1 %s\nmasked groups 3 %s\n", m1.stats[i].c_str(), m3.stats[i].c_str());
            REQUIRE(m1.stats[i] == m3.stats[i]);
        }
        REQUIRE(m1.table == m3.table);
        REQUIRE(m1.step > 0 && m1.step == m3.step && m1.p == m3.p && m1.m == m3.m && m1.v == m3.v);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    std::printf("host_env_groups_test ok\n");
    return 0;
}
