// PPO_ContinuousMountainCar (PPO/PPO_ContinuousMountainCar.h: a Gaussian policy on the device's MountainCarContinuous-v0) on a GPU, driven by
// tests/test_gpu_mountaincar_continuous_facade.py in a fresh directory: two iterations train with bootstrap_truncated = true and a small time limit, the fold
// reports events, evaluate(8) returns ppo_evaluate's numbers on the same context and prints nothing, the checkpoint loads into a fresh object with bit-equal
// parameters, and the host-side MountainCarContinuous class steps with the library's arithmetic.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../PPO/PPO_ContinuousMountainCar.h"

namespace fs = std::filesystem;

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static const int N = 64, T = 32, UPDATES = 2;

static void writeConfig(const std::string& extra) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = 2\nmax_episode_steps = 20\n" << extra
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
        std::unique_ptr<PPO_ContinuousMountainCar> algo;
        captured([&] { algo = std::make_unique<PPO_ContinuousMountainCar>(); });
        ppo_config cfg{};
        REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK);
        REQUIRE(cfg.env_kind == PPO_ENV_MOUNTAINCAR_CONTINUOUS && cfg.dist_kind == PPO_DIST_GAUSSIAN && (cfg.kernel_flags & PPO_KERNEL_GAUSS_FUSED) &&
                cfg.max_episode_steps == 20);
        REQUIRE(algo->actionDim() == 1 && algo->m_obs_size == 2 && algo->bootstrapTruncated());
        P = ppo_param_count(algo->m_ctx);
        REQUIRE(P == 2 * (64 * 2 + 64 + 64 * 64 + 64) + (64 + 1) + (64 + 1) + 1);
        int finite = 0;
        double ep_len = 0.0;
        algo->m_on_update = [&](int64_t, const ppo_stats& s) {
            finite += std::isfinite(s.loss) && std::isfinite(s.entropy_loss) && std::isfinite(s.explained_variance) ? 1 : 0;
            ep_len = s.ep_len_mean;
        };
        const std::string table = captured([&] { algo->train(); });
        REQUIRE(finite == UPDATES && table.find("rollout/") != std::string::npos && ep_len == 20.0);   // an untrained car never reaches the goal in 20 steps
        int64_t act = 0, value = 0, update = 0;
        REQUIRE(ppo_gauss_fused_launches(algo->m_ctx, &act, &value, &update) == PPO_OK);
        std::printf("fused launches: act %lld value %lld update %lld\n", (long long)act, (long long)value, (long long)update);
        REQUIRE(act == 0 && value >= UPDATES * 2 && update == UPDATES * 4 * 4);   // the fold is none of the three; the scan's bootstrap value is a critic launch too
        // the last rollout's fold: every env's episode was cut off once (T = 32, limit 20), none terminated
        int64_t events = 0;
        REQUIRE(ppo_env_truncations(algo->m_ctx, &events, nullptr, nullptr, 0) == PPO_OK);
        std::printf("truncation events: %lld\n", (long long)events);
        REQUIRE(events > 0 && events <= static_cast<int64_t>(N) * T);
        trained.resize(static_cast<size_t>(P));
        REQUIRE(ppo_params_get_h(algo->m_ctx, trained.data(), P) == PPO_OK);
        REQUIRE(trained[static_cast<size_t>(P - 1)] != 0.0f);   // log_std was stepped
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
        std::unique_ptr<PPO_ContinuousMountainCar> again;
        const std::string said = captured([&] { again = std::make_unique<PPO_ContinuousMountainCar>(); });
        REQUIRE(said.find("Loading model") != std::string::npos && said.find("ignoring it") == std::string::npos);
        std::vector<float> loaded(static_cast<size_t>(P));
        REQUIRE(ppo_param_count(again->m_ctx) == P && ppo_params_get_h(again->m_ctx, loaded.data(), P) == PPO_OK);
        REQUIRE(std::memcmp(loaded.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
    }
    {   // the host class against ppo_env_transition_f32: a raw action of 5 steps with the clipped force (like an action of 1) and pays the raw penalty
        MountainCarContinuous a(nullptr, 7, 0), b(nullptr, 7, 0);
        const std::vector<float> o0 = a.reset();
        REQUIRE(o0 == b.reset() && o0.size() == 2 && o0[0] >= -0.6f && o0[0] < -0.4f && o0[1] == 0.0f && a.state == o0);
        auto dev = std::make_shared<ppo::Device>(0);
        ppo::Tensor s = ppo::Tensor::from_host<float>(dev, o0, { 1, 2 }), act = ppo::Tensor::from_host<float>(dev, { 5.0f }, { 1, 1 });
        ppo::Tensor ns(dev, { 1, 2 }, ppo::DType::f32), ob(dev, { 1, 2 }, ppo::DType::f32), r(dev, { 1 }, ppo::DType::f32), t(dev, { 1 }, ppo::DType::i32);
        REQUIRE(ppo_env_transition_f32(PPO_ENV_MOUNTAINCAR_CONTINUOUS, s.data<float>(), act.data<float>(), 1, ns.data<float>(), ob.data<float>(), r.data<float>(),
                                       t.data<int32_t>(), dev->stream()) == PPO_OK);
        auto [oa, ra, ta, ua] = a.step({ 5.0f });
        auto [ob1, rb, tb, ub] = b.step({ 1.0f });
        REQUIRE(oa == ns.cpu<float>() && oa == ob.cpu<float>() && ra == r.item<float>() && ta == (t.item<int32_t>() != 0));
        REQUIRE(oa == ob1 && !ta && !tb && !ua && !ub && a.state == oa && a.episode_length == 1 && a.episode_reward == ra);
        REQUIRE(ra == -0.1f * (5.0f * 5.0f) && rb == -0.1f * (1.0f * 1.0f));   // the clipped force, the raw penalty
    }
    std::printf("host_mcc_test ok\n");
    return 0;
}
