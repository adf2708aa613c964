// PPO_DiscreteBlackjack (PPO/PPO_DiscreteBlackjack.h: a categorical policy on the device's Blackjack) on a GPU, driven by tests/test_gpu_blackjack_facade.py in
// a fresh directory: two iterations train, the rollout is none of the act launches, evaluate(8) returns ppo_evaluate's numbers on the same context and prints
// nothing, the checkpoint loads into a fresh object with bit-equal parameters, setBootstrapTruncated(true) throws the library's refusal, and the host-side
// Blackjack class steps every (t, ace, show) x both actions x n in 4..11 x two keys to the numbers of ppo_env_transition.
//
// The env part -- checkEnv(): the host class alone, no device, no library -- also builds as a program of its own with -DBLACKJACK_ENV_ONLY (and with
// -fsanitize=address,undefined: tests/test_blackjack_host_env.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../Environments/Blackjack.h"

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

// the two keys of the exhaustive rows (tests/test_gpu_blackjack.py uses the same): between them the dealer's play-outs take 0 and 7 cards
static const float KEYS[2][2] = { { 11259375.0f, 16777215.0f }, { 20927.0f, 3321251.0f } };

// every (t 2..31, ace, show 1..10) x both actions x n in 4..11 x two keys: 19 200 rows
static void exhaustiveRows(std::vector<float>& st, std::vector<int64_t>& act) {
    for (int key = 0; key < 2; key++)
        for (int n = 4; n < 12; n++)
            for (int t = 2; t < 32; t++)
                for (int ace = 0; ace < 2; ace++)
                    for (int show = 1; show <= 10; show++)
                        for (int a = 0; a < 2; a++) {
                            st.insert(st.end(), { static_cast<float>(t + 32 * ace + 64 * show), static_cast<float>(n), KEYS[key][0], KEYS[key][1] });
                            act.push_back(a);
                        }
}

// the host class alone: cards, the step's bookkeeping, the dealer's bound, foreign states, resets
static int checkEnv() {
    // thirteen buckets of a word: 1..9 once, 10 four times, at their exact boundaries ceil(b * 2^32 / 13)
    const int want[13] = { 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10, 10, 10 };
    for (int b = 0; b < 13; b++) {
        const uint64_t lo = ((static_cast<uint64_t>(b) << 32) + 12) / 13, hi = ((static_cast<uint64_t>(b + 1) << 32) + 12) / 13 - 1;
        REQUIRE(Blackjack::card(static_cast<uint32_t>(lo)) == want[b] && Blackjack::card(static_cast<uint32_t>(hi)) == want[b]);
        if (b) REQUIRE(Blackjack::card(static_cast<uint32_t>(lo - 1)) == want[b - 1]);
    }
    // Philox: the known-answer vector of Random123 (all-ones key and counter)
    const std::array<uint32_t, 4> kat = Blackjack::philox4x32_10(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
    REQUIRE(kat[0] == 0x408f276du && kat[1] == 0x41c83b0eu && kat[2] == 0xa20bc7c6u && kat[3] == 0x6d5451fdu);
    std::vector<float> st;
    std::vector<int64_t> act;
    exhaustiveRows(st, act);
    const int n = static_cast<int>(act.size());
    REQUIRE(n == 19200);
    int most = 0, none = 0, wins = 0, draws = 0, losses = 0;
    for (int k = 0; k < n; k++) {
        float s[4];
        std::memcpy(s, st.data() + 4 * k, sizeof(s));
        const int hand = static_cast<int>(s[0]), t = hand & 31, ace = (hand >> 5) & 1, show = hand >> 6, n0 = static_cast<int>(s[1]);
        bool term = false;
        int drew = -1;
        const float r = Blackjack::transition(s, static_cast<int>(act[static_cast<size_t>(k)]), term, &drew);
        const int h2 = static_cast<int>(s[0]), t2 = h2 & 31;
        REQUIRE(r == -1.0f || r == 0.0f || r == 1.0f);
        REQUIRE((h2 >> 6) == show && s[2] == st[4 * static_cast<size_t>(k) + 2] && s[3] == st[4 * static_cast<size_t>(k) + 3] && drew >= 0 && drew <= Blackjack::DEALER_DRAWS);
        if (t > 21) {
            REQUIRE(term && r == -1.0f && h2 == hand && static_cast<int>(s[1]) == n0 && drew == 0);
        } else if (act[static_cast<size_t>(k)] == 1) {
            const int c = Blackjack::cardAt(static_cast<uint32_t>(s[2]), static_cast<uint32_t>(s[3]), static_cast<uint32_t>(n0));
            REQUIRE(t2 == t + c && ((h2 >> 5) & 1) == (ace | (c == 1 ? 1 : 0)) && static_cast<int>(s[1]) == n0 + 1 && term == (t2 > 21) && r == (t2 > 21 ? -1.0f : 0.0f));
        } else {
            REQUIRE(term && h2 == hand && static_cast<int>(s[1]) == n0 + drew);
            most = drew > most ? drew : most;
            none += drew == 0 ? 1 : 0;
            wins += r > 0.0f; draws += r == 0.0f; losses += r < 0.0f;
        }
        float ob[Blackjack::OBS];
        Blackjack::observe(s, ob);
        float ones = 0.0f;
        for (float v : ob) ones += v;
        const int u = (((h2 >> 5) & 1) && t2 + 10 <= 21) ? 1 : 0;
        REQUIRE(ones == 3.0f && ob[t2 + 10 * u] == 1.0f && ob[32 + show] == 1.0f && ob[43 + u] == 1.0f);
    }
    std::printf("host Blackjack alone: %d rows, sticks won %d drew %d lost %d, dealer play-outs of 0 cards %d, longest %d\n", n, wins, draws, losses, none, most);
    REQUIRE(none > 0 && most >= 5 && wins > 0 && draws > 0 && losses > 0);
    // the dealer's bound over all 100 two-card starts: the longest line of play, depth first over the ten card values
    struct Rec {
        static int longest(int dt, bool dace) {
            if (dt + ((dace && dt + 10 <= 21) ? 10 : 0) >= 17) return 0;
            int best = 0;
            for (int c = 1; c <= 10; c++) { const int d = 1 + longest(dt + c, dace || c == 1); best = d > best ? d : best; }
            return best;
        }
    };
    int bound = 0;
    for (int s0 = 1; s0 <= 10; s0++)
        for (int h = 1; h <= 10; h++) { const int d = Rec::longest(s0 + h, s0 == 1 || h == 1); bound = d > bound ? d : bound; }
    REQUIRE(bound == Blackjack::DEALER_DRAWS);
    // foreign states: every component converted and clamped; nothing is read or written outside the 45 observations
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const float odd[6][4] = { { nan, -3.0f, 708.0f, 33554432.0f }, { 33554432.0f, nan, -3.0f, 708.0f }, { 708.0f, 33554432.0f, nan, -3.0f },
                              { -3.0f, 708.0f, 33554432.0f, nan }, { 0.0f, 1.5f, 3.99f, 0.0f }, { 65.9f, 16777215.0f, 1.0f, 2.0f } };
    for (const auto& row : odd)
        for (int a = -1; a <= 2; a++) {
            float s[4] = { row[0], row[1], row[2], row[3] }, ob[Blackjack::OBS];
            bool term = false;
            const float r = Blackjack::transition(s, a, term);
            REQUIRE((r == -1.0f || r == 0.0f || r == 1.0f) && s[0] >= 66.0f && s[0] <= 703.0f && s[1] >= 0.0f && s[1] <= 16777215.0f && s[2] <= 16777215.0f && s[3] <= 16777215.0f);
            Blackjack::observe(row, ob);
            float ones = 0.0f;
            for (float v : ob) ones += v;
            REQUIRE(ones == 3.0f);
        }
    // resets: the same (seed, env) deals the same hand; the next reset draws another key; n = 4
    Blackjack e1(7, 0), e2(7, 0);
    const std::vector<float> o0 = e1.reset();
    REQUIRE(o0 == e2.reset() && o0.size() == 45 && e1.episode_length == 0 && e1.episode_reward == 0.0f && e1.state[1] == 4.0f && e1.state == e2.state);
    const int t0 = static_cast<int>(e1.state[0]) & 31;
    REQUIRE(t0 >= 2 && t0 <= 20 && static_cast<int>(e1.state[0]) >> 6 >= 1);
    REQUIRE(t0 == Blackjack::cardAt(static_cast<uint32_t>(e1.state[2]), static_cast<uint32_t>(e1.state[3]), 0) +
                      Blackjack::cardAt(static_cast<uint32_t>(e1.state[2]), static_cast<uint32_t>(e1.state[3]), 1));
    e1.step(1);
    REQUIRE(e1.episode_length == 1 && e1.state[1] == 5.0f);
    (void)e1.reset();
    REQUIRE(e1.state[2] != e2.state[2] || e1.state[3] != e2.state[3]);
    // whole episodes end within 20 steps, whatever is played
    for (int e = 0; e < 200; e++) {
        Blackjack env(11, e);
        (void)env.reset();
        bool term = false;
        while (!term) {
            auto [obs, rew, t, trunc] = env.step(env.episode_length < 19 ? 1 : 0);
            (void)obs; (void)rew;
            term = t;
            REQUIRE(!trunc && env.episode_length <= 20);
        }
    }
    return 0;
}

#ifdef BLACKJACK_ENV_ONLY
int main() {
    if (checkEnv() != 0) return 1;
    std::printf("host_blackjack_env_test ok\n");
    return 0;
}
#else
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../PPO/PPO_DiscreteBlackjack.h"

namespace fs = std::filesystem;

static const int N = 64, T = 32, UPDATES = 2;

static void writeConfig(const std::string& extra) {
    std::ofstream f("PPOConfig.toml");
    f << "[environment]\nobs_size = 45\nmax_episode_steps = 20\n" << extra
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

// the host class against ppo_env_transition on the exhaustive rows
static int compareRows(const std::shared_ptr<ppo::Device>& dev, int& rows, int& differing) {
    std::vector<float> st;
    std::vector<int64_t> act;
    exhaustiveRows(st, act);
    const int n = static_cast<int>(act.size());
    ppo::Tensor s = ppo::Tensor::from_host<float>(dev, st, { n, 4 }), a = ppo::Tensor::from_host<int64_t>(dev, act, { n });
    ppo::Tensor ns(dev, { n, 4 }, ppo::DType::f32), r(dev, { n }, ppo::DType::f32), t(dev, { n }, ppo::DType::i32);
    REQUIRE(ppo_env_transition(PPO_ENV_BLACKJACK, s.data<float>(), a.data<int64_t>(), n, ns.data<float>(), r.data<float>(), t.data<int32_t>(), dev->stream()) == PPO_OK);
    const std::vector<float> dns = ns.cpu<float>(), dr = r.cpu<float>();
    const std::vector<int32_t> dt = t.cpu<int32_t>();
    for (int k = 0; k < n; k++) {
        Blackjack env(7, k);
        env.state.assign(st.begin() + 4 * k, st.begin() + 4 * k + 4);
        auto [obs, rew, term, trunc] = env.step(act[static_cast<size_t>(k)]);
        REQUIRE(obs.size() == 45);
        const bool eq = std::memcmp(env.state.data(), dns.data() + 4 * k, 4 * sizeof(float)) == 0 && rew == dr[static_cast<size_t>(k)] &&
                        term == (dt[static_cast<size_t>(k)] != 0) && !trunc;
        if (!eq) differing++;
    }
    rows += n;
    return 0;
}

int main() {
    if (checkEnv() != 0) return 1;
    writeConfig("");
    std::vector<float> trained;
    int64_t P = 0;
    {
        std::unique_ptr<PPO_DiscreteBlackjack> algo;
        captured([&] { algo = std::make_unique<PPO_DiscreteBlackjack>(); });
        ppo_config cfg{};
        REQUIRE(ppo_get_config(algo->m_ctx, &cfg) == PPO_OK);
        REQUIRE(cfg.env_kind == PPO_ENV_BLACKJACK && cfg.dist_kind == PPO_DIST_CATEGORICAL && (cfg.kernel_flags & PPO_KERNEL_CAT_FUSED) && cfg.max_episode_steps == 20 &&
                cfg.n_heads == 1 && cfg.head_dims[0] == 2 && cfg.obs_size == 45);
        REQUIRE(algo->m_obs_size == 45 && !algo->bootstrapTruncated() && algo->envKind() == PPO_ENV_BLACKJACK);
        P = ppo_param_count(algo->m_ctx);
        REQUIRE(P == 2 * (64 * 45 + 64 + 64 * 64 + 64) + (64 + 1) + 2 * (64 + 1));
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
        for (float v : dret) REQUIRE(v == -1.0f || v == 0.0f || v == 1.0f);   // a return is -1, 0 or +1
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
        REQUIRE(what.find("holds neither the card count nor the key") != std::string::npos && !algo->bootstrapTruncated());
    }
    const std::string ckpt = "./ModelCheckpoints/PPO_Agent_" + std::to_string(N * T * UPDATES) + "_steps.pt";
    REQUIRE(fs::exists(ckpt));
    {
        std::unique_ptr<PPO_DiscreteBlackjack> again;
        const std::string said = captured([&] { again = std::make_unique<PPO_DiscreteBlackjack>(); });
        REQUIRE(said.find("Loading model") != std::string::npos && said.find("ignoring it") == std::string::npos);
        std::vector<float> loaded(static_cast<size_t>(P));
        REQUIRE(ppo_param_count(again->m_ctx) == P && ppo_params_get_h(again->m_ctx, loaded.data(), P) == PPO_OK);
        REQUIRE(std::memcmp(loaded.data(), trained.data(), static_cast<size_t>(P) * sizeof(float)) == 0);
    }
    {
        auto dev = std::make_shared<ppo::Device>(0);
        int rows = 0, differing = 0;
        if (compareRows(dev, rows, differing) != 0) return 1;
        std::printf("host Blackjack against ppo_env_transition: %d of %d rows differ\n", differing, rows);
        REQUIRE(differing == 0 && rows == 19200);
    }
    std::printf("host_blackjack_test ok\n");
    return 0;
}
#endif
