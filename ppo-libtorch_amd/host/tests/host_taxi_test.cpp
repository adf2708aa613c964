// PPO_MultiDiscreteTaxi (PPO/PPO_MultiDiscreteTaxi.h: a masked categorical policy on the device's Taxi-v3) on a GPU, driven by tests/test_gpu_taxi_facade.py
// in a fresh directory: constructed from a TOML with bootstrap_truncated = true, two iterations train (the fold finds time-limit ends: max_episode_steps = 20),
// the rollout is none of the act launches, the stored masks allow every stored action, evaluate(8) returns ppo_evaluate's numbers on the same context and
// prints nothing, the checkpoint loads into a fresh object with bit-equal parameters, and the host-side Taxi class steps all 500 x 6 (state, action) pairs
// to the numbers of ppo_env_transition.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../PPO/PPO_MultiDiscreteTaxi.h"

namespace fs = std::filesystem;

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 64, T = 32, UPDATES = 2;

static void writeConfig(const std::string& extra) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = 19\nmax_episode_steps = 20\n" << extra
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
    writeConfig("bootstrap_truncated = true\n");
    std::vector<float> trained;
    int64_t P = 0;
    {
        std::unique_ptr<PPO_MultiDiscreteTaxi> algo;
        captured([&] { algo = std::make_unique<PPO_MultiDiscreteTaxi>(); });
        ppo_config cfg{};
        REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK);
        REQUIRE(cfg.env_kind == PPO_ENV_TAXI && cfg.dist_kind == PPO_DIST_MASKED && (cfg.kernel_flags & PPO_KERNEL_CAT_FUSED) && cfg.max_episode_steps == 20 &&
                cfg.n_heads == 1 && cfg.head_dims[0] == 6 && cfg.obs_size == 19);
        REQUIRE(algo->m_obs_size == 19 && algo->bootstrapTruncated());
        P = ppo_param_count(algo->m_ctx);
        REQUIRE(P == 2 * (64 * 19 + 64 + 64 * 64 + 64) + (64 + 1) + 6 * (64 + 1));
        int finite = 0;
        algo->m_on_update = [&](int64_t, const ppo_stats& s) {
            finite += std::isfinite(s.loss) && std::isfinite(s.entropy_loss) && std::isfinite(s.explained_variance) ? 1 : 0;
        };
        const std::string table = captured([&] { algo->train(); });
        REQUIRE(finite == UPDATES && table.find("rollout/") != std::string::npos);
        int64_t act = 0, value = 0, update = 0;
        REQUIRE(ppo_gauss_fused_launches(algo->m_ctx, &act, &value, &update) == PPO_OK);
        std::printf("fused launches: act %lld value %lld update %lld\n", (long long)act, (long long)value, (long long)update);
        REQUIRE(act == 0 && value >= UPDATES * 2 && update == UPDATES * 4 * 4);
        // the fold found the time-limit ends of the last rollout (an untrained taxi does not deliver in 20 steps)
        int64_t events = 0;
        REQUIRE(ppo_env_truncations(algo->m_ctx, &events, nullptr, nullptr, 0) == PPO_OK);
        std::printf("truncation events of the last rollout: %lld\n", (long long)events);
        REQUIRE(events > 0 && events <= N * T / 20 + N);
        // the stored masks are the env's: 0 / 1, never empty, and every stored action is allowed
        std::vector<uint8_t> masks(static_cast<size_t>(N) * T * 6);
        std::vector<int32_t> actions(static_cast<size_t>(N) * T);
        void* p = nullptr;
        size_t bytes = 0;
        REQUIRE(ppo_buffer(algo->m_ctx, PPO_BUF_MASKS, &p, &bytes) == PPO_OK && bytes == masks.size());
        REQUIRE(ppo_memcpy_d2h(algo->m_ctx, masks.data(), p, bytes) == PPO_OK);
        REQUIRE(ppo_buffer(algo->m_ctx, PPO_BUF_ACTIONS, &p, &bytes) == PPO_OK && bytes == actions.size() * sizeof(int32_t));
        REQUIRE(ppo_memcpy_d2h(algo->m_ctx, actions.data(), p, bytes) == PPO_OK);
        int zeros = 0;
        for (size_t i = 0; i < actions.size(); i++) {
            REQUIRE(actions[i] >= 0 && actions[i] < 6 && masks[6 * i + static_cast<size_t>(actions[i])] == 1);
            REQUIRE(masks[6 * i] + masks[6 * i + 1] >= 1);
            for (int k = 0; k < 6; k++) { REQUIRE(masks[6 * i + k] <= 1); zeros += masks[6 * i + k] == 0; }
        }
        REQUIRE(zeros > 0);
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
        for (float r : dret) REQUIRE(r == std::floor(r) && r >= -20.0f);   // masked: no -10 ever, so an episode of k steps returns at least -k
        std::printf("evaluate: return mean %.6f, length mean %.3f, truncated %lld\n", direct.return_mean, direct.length_mean, (long long)direct.truncated);
        int64_t act2 = 0, value2 = 0, update2 = 0;
        REQUIRE(ppo_gauss_fused_launches(algo->m_ctx, &act2, &value2, &update2) == PPO_OK && act2 == act && value2 == value && update2 == update);
        std::vector<float> after(static_cast<size_t>(P));
        REQUIRE(ppo_params_get_h(algo->m_ctx, after.data(), P) == PPO_OK && std::memcmp(after.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
        // the switch can be turned off again
        algo->setBootstrapTruncated(false);
        REQUIRE(!algo->bootstrapTruncated());
    }
    const std::string ckpt = "./ModelCheckpoints/PPO_Agent_" + std::to_string(N * T * UPDATES) + "_steps.pt";
    REQUIRE(fs::exists(ckpt));
    {
        writeConfig("");
        std::unique_ptr<PPO_MultiDiscreteTaxi> again;
        const std::string said = captured([&] { again = std::make_unique<PPO_MultiDiscreteTaxi>(); });
        REQUIRE(said.find("Loading model") != std::string::npos && said.find("ignoring it") == std::string::npos);
        REQUIRE(!again->bootstrapTruncated());
        std::vector<float> loaded(static_cast<size_t>(P));
        REQUIRE(ppo_param_count(again->m_ctx) == P && ppo_params_get_h(again->m_ctx, loaded.data(), P) == PPO_OK);
        REQUIRE(std::memcmp(loaded.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
    }
    {   // the host class against ppo_env_transition: all 500 states x 6 actions
        std::vector<float> st;
        std::vector<int64_t> act;
        for (int r = 0; r < 5; r++)
            for (int c = 0; c < 5; c++)
                for (int p = 0; p < 5; p++)
                    for (int d = 0; d < 4; d++)
                        for (int a = 0; a < 6; a++) {
                            st.insert(st.end(), { static_cast<float>(r), static_cast<float>(c), static_cast<float>(p), static_cast<float>(d) });
                            act.push_back(a);
                        }
        const int n = 3000;
        REQUIRE(static_cast<int>(act.size()) == n && static_cast<int>(st.size()) == 4 * n);
        auto dev = std::make_shared<ppo::Device>(0);
        ppo::Tensor s = ppo::Tensor::from_host<float>(dev, st, { n, 4 }), a = ppo::Tensor::from_host<int64_t>(dev, act, { n });
        ppo::Tensor ns(dev, { n, 4 }, ppo::DType::f32), r(dev, { n }, ppo::DType::f32), t(dev, { n }, ppo::DType::i32);
        REQUIRE(ppo_env_transition(PPO_ENV_TAXI, s.data<float>(), a.data<int64_t>(), n, ns.data<float>(), r.data<float>(), t.data<int32_t>(), dev->stream()) == PPO_OK);
        const std::vector<float> dns = ns.cpu<float>(), dr = r.cpu<float>();
        const std::vector<int32_t> dt = t.cpu<int32_t>();
        int differing = 0, allowed = 0;
        for (int k = 0; k < n; k++) {
            Taxi env(7, k);
            env.state.assign(st.begin() + 4 * k, st.begin() + 4 * k + 4);
            const std::array<uint8_t, 6> m = env.actionMask();
            auto [obs, rew, term, trunc] = env.step(act[static_cast<size_t>(k)]);
            const bool changed = std::memcmp(env.state.data(), st.data() + 4 * k, 4 * sizeof(float)) != 0;
            REQUIRE(changed == (m[static_cast<size_t>(act[static_cast<size_t>(k)])] == 1));   // an action is allowed exactly when it changes the state
            allowed += changed;
            float back[4];
            Taxi::stateOf(obs.data(), back);
            REQUIRE(obs.size() == 19 && std::memcmp(back, env.state.data(), sizeof(back)) == 0);
            const bool eq = std::memcmp(env.state.data(), dns.data() + 4 * k, 4 * sizeof(float)) == 0 && rew == dr[static_cast<size_t>(k)] &&
                            term == (dt[static_cast<size_t>(k)] != 0) && !trunc;
            if (!eq) differing++;
        }
        std::printf("host Taxi against ppo_env_transition: %d of %d rows differ; %d allowed pairs\n", differing, n, allowed);
        REQUIRE(differing == 0 && allowed == 1392);
        Taxi e1(7, 0), e2(7, 0);
        const std::vector<float> o0 = e1.reset();
        REQUIRE(o0 == e2.reset() && o0.size() == 19 && e1.episode_length == 0 && e1.episode_reward == 0.0f);
        REQUIRE(e1.state[2] < 4.0f && e1.state[2] != e1.state[3]);
        e1.step(0);
        REQUIRE(e1.episode_length == 1 && e1.episode_reward == -1.0f);
    }
    std::printf("host_taxi_test ok\n");
    return 0;
}
