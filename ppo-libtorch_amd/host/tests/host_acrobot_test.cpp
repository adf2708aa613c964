// PPO_DiscreteAcrobot (PPO/PPO_DiscreteAcrobot.h: a categorical policy on the device's Acrobot-v1) on a GPU, driven by tests/test_gpu_acrobot_facade.py in a
// fresh directory: two iterations train, the rollout is none of the act launches, evaluate(8) returns ppo_evaluate's numbers on the same context and prints
// nothing, the checkpoint loads into a fresh object with bit-equal parameters, bootstrap_truncated = true throws the library's refusal, and the host-side
// Acrobot class steps 64 states -- the corners of the state box among them -- to the bits of ppo_env_transition.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../PPO/PPO_DiscreteAcrobot.h"

namespace fs = std::filesystem;

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 64, T = 32, UPDATES = 2;

static void writeConfig(const std::string& extra) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = 6\nmax_episode_steps = 20\n" << extra
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

int main() {
    writeConfig("");
    std::vector<float> trained;
    int64_t P = 0;
    {
        std::unique_ptr<PPO_DiscreteAcrobot> algo;
        captured([&] { algo = std::make_unique<PPO_DiscreteAcrobot>(); });
        ppo_config cfg{};
        REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK);
        REQUIRE(cfg.env_kind == PPO_ENV_ACROBOT && cfg.dist_kind == PPO_DIST_CATEGORICAL && (cfg.kernel_flags & PPO_KERNEL_CAT_FUSED) && cfg.max_episode_steps == 20 &&
                cfg.n_heads == 1 && cfg.head_dims[0] == 3 && cfg.obs_size == 6);
        REQUIRE(algo->m_obs_size == 6 && !algo->bootstrapTruncated());
        P = ppo_param_count(algo->m_ctx);
        REQUIRE(P == 2 * (64 * 6 + 64 + 64 * 64 + 64) + (64 + 1) + 3 * (64 + 1));
        int finite = 0;
        double ep_len = 0.0;
        algo->m_on_update = [&](int64_t, const ppo_stats& s) {
            finite += std::isfinite(s.loss) && std::isfinite(s.entropy_loss) && std::isfinite(s.explained_variance) ? 1 : 0;
            ep_len = s.ep_len_mean;
        };
        const std::string table = captured([&] { algo->train(); });
        REQUIRE(finite == UPDATES && table.find("rollout/") != std::string::npos && ep_len == 20.0);   // an untrained Acrobot never swings up in 20 steps
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
        std::printf("evaluate: return mean %.6f, length mean %.3f, truncated %lld\n", direct.return_mean, direct.length_mean, (long long)direct.truncated);
        int64_t act2 = 0, value2 = 0, update2 = 0;
        REQUIRE(ppo_gauss_fused_launches(algo->m_ctx, &act2, &value2, &update2) == PPO_OK && act2 == act && value2 == value && update2 == update);
        std::vector<float> after(static_cast<size_t>(P));
        REQUIRE(ppo_params_get_h(algo->m_ctx, after.data(), P) == PPO_OK && std::memcmp(after.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
    }
    const std::string ckpt = "./ModelCheckpoints/PPO_Agent_" + std::to_string(N * T * UPDATES) + "_steps.pt";
    REQUIRE(fs::exists(ckpt));
    {
        std::unique_ptr<PPO_DiscreteAcrobot> again;
        const std::string said = captured([&] { again = std::make_unique<PPO_DiscreteAcrobot>(); });
        REQUIRE(said.find("Loading model") != std::string::npos && said.find("ignoring it") == std::string::npos);
        std::vector<float> loaded(static_cast<size_t>(P));
        REQUIRE(ppo_param_count(again->m_ctx) == P && ppo_params_get_h(again->m_ctx, loaded.data(), P) == PPO_OK);
        REQUIRE(std::memcmp(loaded.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
    }
    {   // the time-limit fold is not built for this env: the library's refusal comes through, with its message
        writeConfig("bootstrap_truncated = true\n");
        std::string what;
        try {
            captured([&] { PPO_DiscreteAcrobot refused; });
        } catch (const std::exception& e) {
            what = e.what();
        }
        std::printf("bootstrap_truncated: %s\n", what.c_str());
        REQUIRE(what.find("does not hold the angles") != std::string::npos);
        writeConfig("");
    }
    {   // the host class against ppo_env_transition: 64 states, the 16 corners of the box x 3 actions first, then 16 rows inside it
        const float lim[4] = { 3.14159265358979323846f, 3.14159265358979323846f, 12.566370614359172f, 28.274333882308138f };
        std::vector<float> st;
        std::vector<int64_t> act;
        for (int c = 0; c < 16; c++)
            for (int a = 0; a < 3; a++) {
                for (int i = 0; i < 4; i++) st.push_back(((c >> i) & 1) ? lim[i] : -lim[i]);
                act.push_back(a);
            }
        for (int k = 0; k < 16; k++) {
            for (int i = 0; i < 4; i++) st.push_back(lim[i] * std::sin(1.7f * static_cast<float>(4 * k + i + 1)));
            act.push_back(k % 3);
        }
        const int n = 64;
        REQUIRE(static_cast<int>(act.size()) == n && static_cast<int>(st.size()) == 4 * n);
        auto dev = std::make_shared<ppo::Device>(0);
        ppo::Tensor s = ppo::Tensor::from_host<float>(dev, st, { n, 4 }), a = ppo::Tensor::from_host<int64_t>(dev, act, { n });
        ppo::Tensor ns(dev, { n, 4 }, ppo::DType::f32), r(dev, { n }, ppo::DType::f32), t(dev, { n }, ppo::DType::i32);
        REQUIRE(ppo_env_transition(PPO_ENV_ACROBOT, s.data<float>(), a.data<int64_t>(), n, ns.data<float>(), r.data<float>(), t.data<int32_t>(), dev->stream()) == PPO_OK);
        const std::vector<float> dns = ns.cpu<float>(), dr = r.cpu<float>();
        const std::vector<int32_t> dt = t.cpu<int32_t>();
        int differing = 0;
        for (int k = 0; k < n; k++) {
            Acrobot env(7, k);
            env.state.assign(st.begin() + 4 * k, st.begin() + 4 * k + 4);
            auto [obs, rew, term, trunc] = env.step(act[static_cast<size_t>(k)]);
            const bool eq = std::memcmp(env.state.data(), dns.data() + 4 * k, 4 * sizeof(float)) == 0 && rew == dr[static_cast<size_t>(k)] &&
                            term == (dt[static_cast<size_t>(k)] != 0) && !trunc && obs.size() == 6 && obs[4] == env.state[2] && obs[5] == env.state[3];
            if (!eq) {
                differing++;
                std::fprintf(stderr, "row %d: host (%a %a %a %a) device (%a %a %a %a)\n", k, env.state[0], env.state[1], env.state[2], env.state[3], dns[4 * k], dns[4 * k + 1],
                             dns[4 * k + 2], dns[4 * k + 3]);
            }
            for (int i = 0; i < 4; i++) REQUIRE(std::isfinite(env.state[static_cast<size_t>(i)]) && std::fabs(env.state[static_cast<size_t>(i)]) <= lim[i]);
        }
        std::printf("host Acrobot against ppo_env_transition: %d of %d rows differ\n", differing, n);
        REQUIRE(differing == 0);
        Acrobot e1(7, 0), e2(7, 0);
        const std::vector<float> o0 = e1.reset();
        REQUIRE(o0 == e2.reset() && o0.size() == 6 && e1.episode_length == 0 && e1.episode_reward == 0.0f);
        for (float v : e1.state) REQUIRE(v >= -0.1f && v < 0.1f);
        e1.step(2);
        REQUIRE(e1.episode_length == 1 && e1.episode_reward == -1.0f);
    }
    std::printf("host_acrobot_test ok\n");
    return 0;
}
