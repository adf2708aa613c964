// PPO_HostEnv's reward normalisation (PPO/PPO_HostEnv.h: setNormReward / `norm_reward` in PPOConfig.toml) and the statistics file beside a checkpoint
// (PPO/PPOAlgorithm.h: RewardNormFile), driven by tests/test_reward_norm_facade.py in a fresh directory.
//   sidecar   no GPU: RewardNormFile written and read back bit for bit, the file's size and layout, a truncated, a foreign and an absent file refused
//   train     on a GPU: the key is parsed (and prints nothing when absent), norm_reward with env_groups = 2 throws the library's message at construction,
//             two updates of a toy env that pays in thousands train to finite statistics, the rewards the update saw are within the clip while the
//             episode statistics stay in the env's units, the file beside the final model holds what ppo_reward_norm_get_h returns, with
//             count = 2 T N, and a new PPO_HostEnv in the same directory loads it
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../PPO/PPO_HostEnv.h"

namespace fs = std::filesystem;

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 16, T = 32, UPDATES = 2;

// a point pushed left or right; the reward is a score in thousands: 1000 * (1 - |x|)
struct ScoreEnv {
    explicit ScoreEnv(int64_t index) : idx(index) {}
    std::vector<float> obs() const { return { x, v, 0.1f * static_cast<float>(episode_length), 0.25f * static_cast<float>(idx % 5) }; }
    std::vector<float> reset() { x = 0.01f * static_cast<float>(idx % 7); v = 0.0f; episode_length = 0; episode_reward = 0.0f; return obs(); }
    std::tuple<std::vector<float>, float, bool, bool> step(const int64_t& a) {
        v += 0.05f * static_cast<float>(2 * a - 1);
        x += v;
        episode_length++;
        const float r = 1000.0f * (1.0f - (x < 0.0f ? -x : x));
        episode_reward += r;
        const bool done = x > 1.0f || x < -1.0f || episode_length >= 11 + idx % 6;
        return { obs(), r, done, false };
    }
    int64_t idx;
    float x = 0.0f, v = 0.0f;
    int64_t episode_length = 0;
    float episode_reward = 0.0f;
};

static void writeConfig(const std::string& extra) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = 4\naction_size = 2\nmax_episode_steps = 40\n" << extra
      << "[general]\nseed = 3\ntotal_timesteps = " << N * T * UPDATES << "\nuse_cuda = true\ncheckpoint_updates = 1\n"
         "[ppo]\nlearning_rate = 0.001\nnum_envs = " << N << "\nnum_steps = " << T << "\nanneal_lr = true\nuse_gae = true\ngamma = 0.98\n"
         "gae_lambda = 0.95\nnum_minibatches = 4\nupdate_epochs = 4\nnorm_adv = true\nclip_coef = 0.2\nclip_vloss = true\n"
         "ent_coef = 0.0\nvf_coef = 0.5\nmax_grad_norm = 0.5\n";
}

template <class Fn> static std::string captured(Fn fn) {
    std::stringstream out;
    std::streambuf* old = std::cout.rdbuf(out.rdbuf());
    try { fn(); } catch (...) { std::cout.rdbuf(old); throw; }
    std::cout.rdbuf(old);
    return out.str();
}

static bool sameBits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static int sidecar(const std::string& dir) {
    RewardNormFile f;
    f.count = 1234567.0;
    f.mean = -2.5e7 / 3.0;
    f.var = 1e300;
    const std::string path = RewardNormFile::pathFor(dir + "/PPO_Agent_64_steps.pt");
    REQUIRE(path == dir + "/PPO_Agent_64_steps.pt.rewnorm");
    f.write(path);
    REQUIRE(fs::file_size(path) == 24 && !fs::exists(path + ".tmp"));
    const RewardNormFile g = RewardNormFile::read(path);
    REQUIRE(sameBits(g.count, f.count) && sameBits(g.mean, f.mean) && sameBits(g.var, f.var));
    // the layout: count, mean, var as raw f64
    double raw[3] = { 0.0, 0.0, 0.0 };
    std::ifstream(path, std::ios::binary).read(reinterpret_cast<char*>(raw), 24);
    REQUIRE(raw[0] == 1234567.0 && sameBits(raw[1], f.mean) && raw[2] == 1e300);
    // var = 0 is a state the normaliser reaches (a first batch of identical rewards) and must survive the file
    f.var = 0.0;
    f.write(path);
    REQUIRE(RewardNormFile::read(path).var == 0.0);
    int refused = 0;
    fs::resize_file(path, 16);
    try { RewardNormFile::read(path); } catch (const std::runtime_error&) { refused++; }
    std::ofstream(path, std::ios::binary | std::ios::trunc) << "PK\x03\x04 some other program's file, long enough to hold a header";
    try { RewardNormFile::read(path); } catch (const std::runtime_error&) { refused++; }
    try { RewardNormFile::read(dir + "/absent.rewnorm"); } catch (const std::runtime_error&) { refused++; }
    REQUIRE(refused == 3);
    std::printf("REWARD_NORM_SIDECAR_OK\n");
    return 0;
}

static int train() {
    auto factory = [](int64_t i) { return std::make_shared<ScoreEnv>(i); };
    using Algo = PPO_HostEnv<ScoreEnv>;
    // the key absent: nothing printed, off
    writeConfig("");
    const std::string said_off = captured([&] { Algo algo(factory); if (algo.normReward()) throw std::runtime_error("norm_reward on by default"); });
    REQUIRE(said_off.find("norm_reward") == std::string::npos);
    // norm_reward with env groups: refused at construction with the library's message
    writeConfig("env_groups = 2\nnorm_reward = true\n");
    std::string refusal;
    captured([&] { try { Algo algo(factory); } catch (const std::runtime_error& e) { refusal = e.what(); } });
    std::printf("refusal: %s\n", refusal.c_str());
    REQUIRE(refusal.find("group") != std::string::npos && refusal.find("ppo_host_rollout_begin_groups") != std::string::npos &&
            refusal.find("reward normalisation") != std::string::npos);
    // the key alone
    writeConfig("norm_reward = true\n");
    double mean = 0.0, var = 0.0, count = 0.0;
    {
        std::string said_on;
        std::unique_ptr<Algo> algo;
        said_on = captured([&] { algo = std::make_unique<Algo>(factory); });
        REQUIRE(said_on.find("Using config file norm_reward = true") != std::string::npos && algo->normReward() && !algo->normObs());
        bool refused = false;
        try { algo->setEnvGroups(2); } catch (const std::runtime_error&) { refused = true; }
        REQUIRE(refused && algo->envGroups() == 1);
        std::vector<std::string> losses;
        double ep_rew = 0.0;
        algo->m_on_update = [&](int64_t, const ppo_stats& s) {
            losses.push_back(std::isfinite(s.loss) && std::isfinite(s.explained_variance) ? "ok" : "not finite");
            ep_rew = s.ep_rew_mean;
        };
        const std::string table = captured([&] { algo->train(); });
        REQUIRE(losses.size() == static_cast<size_t>(UPDATES) && losses[0] == "ok" && losses[1] == "ok");
        REQUIRE(table.find("rollout/") != std::string::npos);
        std::vector<double> ret(N);
        REQUIRE(ppo_reward_norm_get_h(algo->m_ctx, &mean, &var, &count, ret.data(), N) == PPO_OK);
        std::printf("count %.0f mean %g var %g ep_rew_mean %g\n", count, mean, var, ep_rew);
        REQUIRE(count == static_cast<double>(UPDATES * T * N));
        REQUIRE(std::isfinite(mean) && std::isfinite(var) && var > 1e4);   // returns of a score in thousands
        for (double r : ret) REQUIRE(std::isfinite(r));
        // the rewards the update saw are normalised and clipped; the episode statistics are in the env's own units
        const std::vector<float> rew = algo->m_rewards.cpu<float>();
        float top = 0.0f;
        for (float r : rew) top = std::max(top, std::fabs(r));
        REQUIRE(top <= 10.0f && top > 0.01f);
        REQUIRE(ep_rew > 1000.0);
    }
    const std::string total = std::to_string(N * T * UPDATES);
    const std::string model = "./Models/PPO_Agent_" + total + "_steps.pt", ckpt = "./ModelCheckpoints/PPO_Agent_" + total + "_steps.pt";
    for (const std::string& agent : { model, ckpt }) {
        const std::string side = RewardNormFile::pathFor(agent);
        REQUIRE(fs::exists(agent) && fs::exists(side) && fs::file_size(side) == 24 && !fs::exists(ObsNormFile::pathFor(agent)));
        const RewardNormFile f = RewardNormFile::read(side);
        REQUIRE(sameBits(f.count, count) && sameBits(f.mean, mean) && sameBits(f.var, var));
    }
    REQUIRE(fs::exists(RewardNormFile::pathFor("./ModelCheckpoints/PPO_Agent_" + std::to_string(N * T) + "_steps.pt")));
    // a new run in the same directory resumes from the newest agent file (never from a statistics file) and takes the statistics over
    {
        std::unique_ptr<Algo> algo;
        const std::string said = captured([&] { algo = std::make_unique<Algo>(factory); });
        REQUIRE(said.find("Loading model ./ModelCheckpoints/PPO_Agent_") != std::string::npos);
        REQUIRE(said.find(".rewnorm...") != std::string::npos && said.find("Loading reward statistics") != std::string::npos);
        REQUIRE(said.find("ignoring it") == std::string::npos);
        double m2 = 0.0, v2 = 0.0, c2 = 0.0;
        REQUIRE(ppo_reward_norm_get_h(algo->m_ctx, &m2, &v2, &c2, nullptr, 0) == PPO_OK);
        REQUIRE(sameBits(c2, count) && sameBits(m2, mean) && sameBits(v2, var));
        REQUIRE(algo->m_global_step == static_cast<uint64_t>(N * T * UPDATES));
    }
    std::printf("REWARD_NORM_FACADE_OK\n");
    return 0;
}

int main(int argc, char** argv) {
    try {
        if (argc == 3 && std::string(argv[1]) == "sidecar") return sidecar(argv[2]);
        if (argc == 2 && std::string(argv[1]) == "train") return train();
        std::fprintf(stderr, "usage: host_reward_norm_test sidecar <dir> | train\n");
        return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
