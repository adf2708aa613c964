// PPO_DiscreteFrozenLake (PPO/PPO_DiscreteFrozenLake.h: a categorical policy on the device's slippery FrozenLake) on a GPU, driven by
// tests/test_gpu_frozenlake_facade.py in a fresh directory: two iterations train on the 4x4 map, the rollout is none of the act launches, evaluate(8) returns
// ppo_evaluate's numbers on the same context and prints nothing, the checkpoint loads into a fresh object with bit-equal parameters, setBootstrapTruncated(true)
// throws the library's refusal, obs_size = 64 picks the 8x8 env kind, and the host-side FrozenLake class steps every (cell, action) pair x 12 step counts x
// two keys of both maps to the numbers of ppo_env_transition.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../PPO/PPO_DiscreteFrozenLake.h"

namespace fs = std::filesystem;

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 64, T = 32, UPDATES = 2;

static void writeConfig(int obs, const std::string& extra) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = " << obs << "\nmax_episode_steps = 20\n" << extra
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

// the host class against ppo_env_transition on one map: every (cell, action) pair, terminal cells too, x j in 0..11 (every word of three Philox calls) x two keys
static int compareMap(int side, int env_kind, const std::shared_ptr<ppo::Device>& dev, int& rows, int& differing) {
    const int S = side * side;
    const float keys[2][2] = { { 0.0f, 0.0f }, { 11259375.0f, 16777215.0f } };
    std::vector<float> st;
    std::vector<int64_t> act;
    for (int key = 0; key < 2; key++)
        for (int j = 0; j < 12; j++)
            for (int cell = 0; cell < S; cell++)
                for (int a = 0; a < 4; a++) {
                    st.insert(st.end(), { static_cast<float>(cell), static_cast<float>(j), keys[key][0], keys[key][1] });
                    act.push_back(a);
                }
    const int n = static_cast<int>(act.size());
    REQUIRE(n == 2 * 12 * S * 4);
    ppo::Tensor s = ppo::Tensor::from_host<float>(dev, st, { n, 4 }), a = ppo::Tensor::from_host<int64_t>(dev, act, { n });
    ppo::Tensor ns(dev, { n, 4 }, ppo::DType::f32), r(dev, { n }, ppo::DType::f32), t(dev, { n }, ppo::DType::i32);
    REQUIRE(ppo_env_transition(env_kind, s.data<float>(), a.data<int64_t>(), n, ns.data<float>(), r.data<float>(), t.data<int32_t>(), dev->stream()) == PPO_OK);
    const std::vector<float> dns = ns.cpu<float>(), dr = r.cpu<float>();
    const std::vector<int32_t> dt = t.cpu<int32_t>();
    int moved[3] = { 0, 0, 0 };
    for (int k = 0; k < n; k++) {
        FrozenLake env(side, 7, k);
        env.state.assign(st.begin() + 4 * k, st.begin() + 4 * k + 4);
        auto [obs, rew, term, trunc] = env.step(act[static_cast<size_t>(k)]);
        const int cell = static_cast<int>(env.state[0]);
        REQUIRE(static_cast<int>(obs.size()) == S && cell >= 0 && cell < S && obs[static_cast<size_t>(cell)] == 1.0f);
        float ones = 0.0f;
        for (float v : obs) ones += v;
        REQUIRE(ones == 1.0f && env.state[1] == st[4 * static_cast<size_t>(k) + 1] + 1.0f && (rew == 0.0f || (rew == 1.0f && cell == S - 1 && term)));
        const bool eq = std::memcmp(env.state.data(), dns.data() + 4 * k, 4 * sizeof(float)) == 0 && rew == dr[static_cast<size_t>(k)] &&
                        term == (dt[static_cast<size_t>(k)] != 0) && !trunc;
        if (!eq) differing++;
        // the slip of this row, for the count below: cell 0 under action 1 (down) goes left (stays), down or right
        if (static_cast<int>(st[4 * static_cast<size_t>(k)]) == 0 && act[static_cast<size_t>(k)] == 1) moved[cell == 0 ? 0 : (cell == side ? 1 : 2)]++;
    }
    REQUIRE(moved[0] + moved[1] + moved[2] == 24 && moved[0] > 0 && moved[1] > 0 && moved[2] > 0);   // all three outcomes occur among 24 draws
    rows += n;
    return 0;
}

int main() {
    writeConfig(16, "");
    std::vector<float> trained;
    int64_t P = 0;
    {
        std::unique_ptr<PPO_DiscreteFrozenLake> algo;
        captured([&] { algo = std::make_unique<PPO_DiscreteFrozenLake>(); });
        ppo_config cfg{};
        REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK);
        REQUIRE(cfg.env_kind == PPO_ENV_FROZENLAKE && cfg.dist_kind == PPO_DIST_CATEGORICAL && (cfg.kernel_flags & PPO_KERNEL_CAT_FUSED) && cfg.max_episode_steps == 20 &&
                cfg.n_heads == 1 && cfg.head_dims[0] == 4 && cfg.obs_size == 16);
        REQUIRE(algo->m_obs_size == 16 && !algo->bootstrapTruncated() && algo->envKind() == PPO_ENV_FROZENLAKE);
        P = ppo_param_count(algo->m_ctx);
        REQUIRE(P == 2 * (64 * 16 + 64 + 64 * 64 + 64) + (64 + 1) + 4 * (64 + 1));
        int finite = 0;
        double ep_len = 0.0;
        algo->m_on_update = [&](int64_t, const ppo_stats& s) {
            finite += std::isfinite(s.loss) && std::isfinite(s.entropy_loss) && std::isfinite(s.explained_variance) ? 1 : 0;
            ep_len = s.ep_len_mean;
        };
        const std::string table = captured([&] { algo->train(); });
        REQUIRE(finite == UPDATES && table.find("rollout/") != std::string::npos && ep_len >= 1.0 && ep_len <= 20.0);
        int64_t act = 0, value = 0, update = 0;
        REQUIRE(ppo_gauss_fused_launches(algo->m_ctx, &act, &value, &update) == PPO_OK);
        std::printf("fused launches: act %lld value %lld update %lld\n", (long long)act, (long long)value, (long long)update);
        REQUIRE(act == 0 && value >= UPDATES * 2 && update == UPDATES * 4 * 4);
        trained.resize(static_cast<size_t>(P));
        REQUIRE(ppo_params_get_h(algo->m_ctx, trained.data(), P) == PPO_OK);
        // evaluate(): ppo_evaluate's numbers on the same context, nothing printed, nothing moved
        EvalResult ev;
        const std::string said = captured([&] { ev = algo->evaluate(8); });
        REQUIRE(said.empty() && ev.returns.size() == 8 && ev.lengths.size() == 8 && ev.stats.episodes == 8);
        ppo::Tensor ret(algo->m_device, { 8 }, ppo::DType::f32), len(algo->m_device, { 8 }, ppo::DType::i32);
        ppo_eval_stats direct{};
        REQUIRE(ppo_evaluate(algo->m_ctx, 8, algo->m_seed, 1, ret.data<float>(), len.data<int32_t>(), &direct) == PPO_OK);
        const std::vector<float> dret = ret.cpu<float>();
        const std::vector<int32_t> dlen = len.cpu<int32_t>();
        REQUIRE(std::memcmp(dret.data(), ev.returns.data(), 8 * sizeof(float)) == 0 && dlen == ev.lengths);
        REQUIRE(std::memcmp(&direct, &ev.stats, sizeof(direct)) == 0);
        REQUIRE(direct.length_max <= 20 && direct.truncated >= 0 && direct.env_steps > 0);
        for (float v : dret) REQUIRE(v == 0.0f || v == 1.0f);   // a return is 0 or 1
        std::printf("evaluate: return mean %.6f, length mean %.3f, truncated %lld\n", direct.return_mean, direct.length_mean, (long long)direct.truncated);
        int64_t act2 = 0, value2 = 0, update2 = 0;
        REQUIRE(ppo_gauss_fused_launches(algo->m_ctx, &act2, &value2, &update2) == PPO_OK && act2 == act && value2 == value && update2 == update);
        std::vector<float> after(static_cast<size_t>(P));
        REQUIRE(ppo_params_get_h(algo->m_ctx, after.data(), P) == PPO_OK && std::memcmp(after.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
        // the time-limit fold is not built for this env: the library's refusal comes through, with its message, and the switch stays off
        std::string what;
        try {
            algo->setBootstrapTruncated(true);
        } catch (const std::exception& e) {
            what = e.what();
        }
        std::printf("bootstrap_truncated: %s\n", what.c_str());
        REQUIRE(what.find("holds neither the step count nor the key") != std::string::npos && !algo->bootstrapTruncated());
    }
    const std::string ckpt = "./ModelCheckpoints/PPO_Agent_" + std::to_string(N * T * UPDATES) + "_steps.pt";
    REQUIRE(fs::exists(ckpt));
    {
        std::unique_ptr<PPO_DiscreteFrozenLake> again;
        const std::string said = captured([&] { again = std::make_unique<PPO_DiscreteFrozenLake>(); });
        REQUIRE(said.find("Loading model") != std::string::npos && said.find("ignoring it") == std::string::npos);
        std::vector<float> loaded(static_cast<size_t>(P));
        REQUIRE(ppo_param_count(again->m_ctx) == P && ppo_params_get_h(again->m_ctx, loaded.data(), P) == PPO_OK);
        REQUIRE(std::memcmp(loaded.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
    }
    {   // obs_size = 64 picks the 8x8 map (in a directory of its own: the 4x4 checkpoint does not fit this network)
        fs::create_directory("lake8");
        const fs::path home = fs::current_path();
        fs::current_path(home / "lake8");
        writeConfig(64, "");
        std::unique_ptr<PPO_DiscreteFrozenLake> big;
        captured([&] { big = std::make_unique<PPO_DiscreteFrozenLake>(); });
        ppo_config cfg{};
        REQUIRE(ppo_get_config(big->m_ctx, &cfg) == PPO_OK);
        REQUIRE(cfg.env_kind == PPO_ENV_FROZENLAKE8X8 && cfg.obs_size == 64 && cfg.head_dims[0] == 4 && big->envKind() == PPO_ENV_FROZENLAKE8X8);
        big.reset();
        fs::current_path(home);
    }
    {
        auto dev = std::make_shared<ppo::Device>(0);
        int rows = 0, differing = 0;
        if (compareMap(4, PPO_ENV_FROZENLAKE, dev, rows, differing) != 0) return 1;
        if (compareMap(8, PPO_ENV_FROZENLAKE8X8, dev, rows, differing) != 0) return 1;
        std::printf("host FrozenLake against ppo_env_transition: %d of %d rows differ\n", differing, rows);
        REQUIRE(differing == 0 && rows == 2 * 12 * 4 * (16 + 64));
        FrozenLake e1(4, 7, 0), e2(4, 7, 0);
        const std::vector<float> o0 = e1.reset();
        REQUIRE(o0 == e2.reset() && o0.size() == 16 && o0[0] == 1.0f && e1.episode_length == 0 && e1.episode_reward == 0.0f);
        REQUIRE(e1.state[0] == 0.0f && e1.state[1] == 0.0f && e1.state == e2.state);
        e1.step(2);
        REQUIRE(e1.episode_length == 1 && e1.state[1] == 1.0f);
        (void)e1.reset();
        REQUIRE(e1.state[2] != e2.state[2] || e1.state[3] != e2.state[3]);   // the next reset draws another key
    }
    std::printf("host_frozenlake_test ok\n");
    return 0;
}
