// PPO_HostEnv's observation normalisation (PPO/PPO_HostEnv.h: setNormObs / `norm_obs` in PPOConfig.toml) and the statistics file beside a checkpoint
// (PPO/PPOAlgorithm.h: ObsNormFile), driven by tests/test_obs_norm_facade.py in a fresh directory.
//   sidecar   no GPU: ObsNormFile written and read back bit for bit, the file's size, a truncated and a foreign file refused
//   train     on a GPU: the key is parsed (and prints nothing when absent), norm_obs with env_groups = 2 throws the library's message at construction,
//             two updates of a toy env whose observation columns differ in scale by seven orders of magnitude train to finite statistics, the file beside
//             the final model holds what ppo_obs_norm_get_h returns, with count = (1 + 2 T) N, and a new PPO_HostEnv in the same directory loads it
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

// position in millimetres around 500, velocity in kilometres per step, a step counter in hundreds, a constant in the ten thousands
struct ScaledEnv {
    explicit ScaledEnv(int64_t index) : idx(index) {}
    std::vector<float> obs() const { return { 1000.0f * x + 500.0f, 0.001f * v, 100.0f * static_cast<float>(episode_length), 10000.0f + static_cast<float>(idx % 5) }; }
    std::vector<float> reset() { x = 0.01f * static_cast<float>(idx % 7); v = 0.0f; episode_length = 0; episode_reward = 0.0f; return obs(); }
    std::tuple<std::vector<float>, float, bool, bool> step(const int64_t& a) {
        v += 0.05f * static_cast<float>(2 * a - 1);
        x += v;
        episode_length++;
        const float r = 1.0f - (x < 0.0f ? -x : x);
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

static bool sameBits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

static int sidecar(const std::string& dir) {
    ObsNormFile f;
    f.count = 1234567.0;
    f.mean = { 0.1, -2.5e7, 3.0, 1e-300, 5.0 };
    f.var = { 1.0, 0.0, 2.0 / 3.0, 1e300, 4.0 };
    const std::string path = ObsNormFile::pathFor(dir + "/PPO_Agent_64_steps.pt");
    REQUIRE(path == dir + "/PPO_Agent_64_steps.pt.obsnorm");
    f.write(path);
    REQUIRE(fs::file_size(path) == 8 * (2 + 2 * 5) && !fs::exists(path + ".tmp"));
    const ObsNormFile g = ObsNormFile::read(path);
    REQUIRE(g.count == f.count && sameBits(g.mean, f.mean) && sameBits(g.var, f.var));
    // the layout: O, count, mean, var as raw f64
    std::vector<double> raw(12);
    std::ifstream(path, std::ios::binary).read(reinterpret_cast<char*>(raw.data()), 96);
    REQUIRE(raw[0] == 5.0 && raw[1] == 1234567.0 && raw[2] == 0.1 && raw[7] == 1.0 && raw[11] == 4.0);
    int refused = 0;
    fs::resize_file(path, 88);
    try { ObsNormFile::read(path); } catch (const std::runtime_error&) { refused++; }
    std::ofstream(path, std::ios::binary | std::ios::trunc) << "PK\x03\x04 some other program's file, long enough to hold a header";
    try { ObsNormFile::read(path); } catch (const std::runtime_error&) { refused++; }
    try { ObsNormFile::read(dir + "/absent.obsnorm"); } catch (const std::runtime_error&) { refused++; }
    REQUIRE(refused == 3);
    std::printf("OBS_NORM_SIDECAR_OK\n");
    return 0;
}

static int train() {
    auto factory = [](int64_t i) { return std::make_shared<ScaledEnv>(i); };
    using Algo = PPO_HostEnv<ScaledEnv>;
    // the key absent: nothing printed, off
    writeConfig("");
    const std::string said_off = captured([&] { Algo algo(factory); if (algo.normObs()) throw std::runtime_error("norm_obs on by default"); });
    REQUIRE(said_off.find("norm_obs") == std::string::npos);
    // norm_obs with env groups: refused at construction with the library's message
    writeConfig("env_groups = 2\nnorm_obs = true\n");
    std::string refusal;
    captured([&] { try { Algo algo(factory); } catch (const std::runtime_error& e) { refusal = e.what(); } });
    std::printf("refusal: %s\n", refusal.c_str());
    REQUIRE(refusal.find("group") != std::string::npos && refusal.find("ppo_host_rollout_begin_groups") != std::string::npos);
    // the key alone
    writeConfig("norm_obs = true\n");
    std::vector<double> mean(4), var(4);
    double count = 0.0;
    {
        std::string said_on;
        std::unique_ptr<Algo> algo;
        said_on = captured([&] { algo = std::make_unique<Algo>(factory); });
        REQUIRE(said_on.find("Using config file norm_obs = true") != std::string::npos && algo->normObs());
        bool refused = false;
        try { algo->setEnvGroups(2); } catch (const std::runtime_error&) { refused = true; }
        REQUIRE(refused && algo->envGroups() == 1);
        std::vector<std::string> losses;
        algo->m_on_update = [&](int64_t, const ppo_stats& s) { losses.push_back(std::isfinite(s.loss) && std::isfinite(s.explained_variance) ? "ok" : "not finite"); };
        const std::string table = captured([&] { algo->train(); });
        REQUIRE(losses.size() == static_cast<size_t>(UPDATES) && losses[0] == "ok" && losses[1] == "ok");
        REQUIRE(table.find("rollout/") != std::string::npos);
        REQUIRE(ppo_obs_norm_get_h(algo->m_ctx, mean.data(), var.data(), 4, &count) == PPO_OK);
        std::printf("count %.0f mean %g %g %g %g var %g %g %g %g\n", count, mean[0], mean[1], mean[2], mean[3], var[0], var[1], var[2], var[3]);
        REQUIRE(count == static_cast<double>((1 + UPDATES * T) * N));
        REQUIRE(std::fabs(mean[3] - 10002.0) < 3.0 && std::fabs(mean[0] - 500.0) < 1100.0 && var[2] > 1e4);   // (x stays within +-1.05)
        // every stored observation is normalised and clipped
        const std::vector<float> obs = algo->m_obs.cpu<float>();
        float top = 0.0f;
        for (float o : obs) top = std::max(top, std::fabs(o));
        REQUIRE(top <= 10.0f && top > 0.5f);
    }
    const std::string total = std::to_string(N * T * UPDATES);
    const std::string model = "./Models/PPO_Agent_" + total + "_steps.pt", ckpt = "./ModelCheckpoints/PPO_Agent_" + total + "_steps.pt";
    for (const std::string& agent : { model, ckpt }) {
        const std::string side = ObsNormFile::pathFor(agent);
        REQUIRE(fs::exists(agent) && fs::exists(side) && fs::file_size(side) == 8 * (2 + 2 * 4));
        const ObsNormFile f = ObsNormFile::read(side);
        REQUIRE(f.count == count && sameBits(f.mean, mean) && sameBits(f.var, var));
    }
    REQUIRE(fs::exists(ObsNormFile::pathFor("./ModelCheckpoints/PPO_Agent_" + std::to_string(N * T) + "_steps.pt")));
    // a new run in the same directory resumes from the newest agent file (never from a statistics file) and takes the statistics over
    {
        std::unique_ptr<Algo> algo;
        const std::string said = captured([&] { algo = std::make_unique<Algo>(factory); });
        REQUIRE(said.find("Loading model " + ckpt) != std::string::npos || said.find("Loading model ./ModelCheckpoints/PPO_Agent_") != std::string::npos);
        REQUIRE(said.find(".obsnorm...") != std::string::npos && said.find("Loading observation statistics") != std::string::npos);
        REQUIRE(said.find("ignoring it") == std::string::npos);
        std::vector<double> m2(4), v2(4);
        double c2 = 0.0;
        REQUIRE(ppo_obs_norm_get_h(algo->m_ctx, m2.data(), v2.data(), 4, &c2) == PPO_OK);
        REQUIRE(c2 == count && sameBits(m2, mean) && sameBits(v2, var));
        REQUIRE(algo->m_global_step == static_cast<uint64_t>(N * T * UPDATES));
    }
    std::printf("OBS_NORM_FACADE_OK\n");
    return 0;
}

int main(int argc, char** argv) {
    try {
        if (argc == 3 && std::string(argv[1]) == "sidecar") return sidecar(argv[2]);
        if (argc == 2 && std::string(argv[1]) == "train") return train();
        std::fprintf(stderr, "usage: host_obs_norm_test sidecar <dir> | train\n");
        return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
