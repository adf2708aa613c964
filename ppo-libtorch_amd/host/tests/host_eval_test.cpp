// evaluate() of the facade on a GPU: driven by tests/test_gpu_evaluate_facade.py, one mode per call, run in a fresh directory.
//   discrete   PPO_Discrete::evaluate(8) gives the numbers of ppo_evaluate on the same context (seed m_seed), greedy and sampled, prints nothing, and a
//              train() after it is the train() of an algorithm that never evaluated; Agent::getActionGreedy = getActionAndValueDiscrete with that action
//   hostenv    PPO_HostEnv<CartPole>::evaluate(8, factory) with factory(e) = CartPole(1000 + e): per episode the return and length of
//              PPO_Discrete::evaluate(1, true, 1000 + e) with the same parameters (a fresh CartPole(s)'s first reset is row 0 of stream s)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../Environments/CartPole.h"
#include "../PPO/PPO_Discrete.h"
#include "../PPO/PPO_HostEnv.h"

#define REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static void writeConfig() {
    std::ofstream("PPOConfig.toml") << "[environment]\nobs_size = 4\naction_size = 2\nmax_episode_steps = 40\n"
                                       "[general]\nseed = 3\ntotal_timesteps = 1536\nuse_cuda = true\ncheckpoint_updates = 1000\n"
                                       "[ppo]\nlearning_rate = 0.001\nnum_envs = 16\nnum_steps = 32\nanneal_lr = true\nuse_gae = true\ngamma = 0.98\n"
                                       "gae_lambda = 0.95\nnum_minibatches = 4\nupdate_epochs = 4\nnorm_adv = true\nclip_coef = 0.2\nclip_vloss = true\n"
                                       "ent_coef = 0.0\nvf_coef = 0.5\nmax_grad_norm = 0.5\n";
}

template <class Algo> static std::string trainQuietly(Algo& algo) {
    std::stringstream out;
    std::streambuf* old = std::cout.rdbuf(out.rdbuf());
    algo.train();
    std::cout.rdbuf(old);
    return out.str();
}

static bool sameStats(const ppo_eval_stats& a, const ppo_eval_stats& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    try {
        writeConfig();
        if (mode == "discrete") {
            PPO_Discrete algo, plain;
            std::stringstream out;
            std::streambuf* old = std::cout.rdbuf(out.rdbuf());
            const EvalResult g = algo.evaluate(8), s = algo.evaluate(8, false);
            std::cout.rdbuf(old);
            REQUIRE(out.str().empty());   // evaluate() prints nothing
            for (int greedy = 1; greedy >= 0; greedy--) {
                const EvalResult& r = greedy ? g : s;
                ppo_eval_stats st{};
                REQUIRE(ppo_evaluate(algo.m_ctx, 8, algo.m_seed, greedy, nullptr, nullptr, &st) == PPO_OK);
                REQUIRE(sameStats(st, r.stats));
                REQUIRE(r.returns.size() == 8 && r.lengths.size() == 8 && r.stats.episodes == 8);
                const ppo_eval_stats again = PPOAlgorithm::summarizeEpisodes(r.returns, r.lengths, algo.m_max_episode_steps);
                REQUIRE(sameStats(again, r.stats));
                std::printf("%s: return_mean %a length_mean %a truncated %lld\n", greedy ? "greedy" : "sampled", st.return_mean, st.length_mean, (long long)st.truncated);
            }
            // the greedy action through the Agent, and the log-prob the reference's entry point gives for it
            const ppo::Tensor x = ppo::Tensor::from_host<float>(algo.m_device, { 0.01f, -0.02f, 0.03f, 0.04f, -0.01f, 0.5f, 0.02f, -0.3f }, { 2, 4 });
            const AgentOutput ga = algo.m_agent->getActionGreedy(x);
            const AgentOutput fa = algo.m_agent->getActionAndValueDiscrete(x, ga.action);
            REQUIRE(ga.logprob.cpu<float>() == fa.logprob.cpu<float>() && ga.value.cpu<float>() == fa.value.cpu<float>());
            REQUIRE(ga.action.cpu<int64_t>() == algo.m_agent->getActionGreedy(x).action.cpu<int64_t>());
            // training after evaluating = training without (console table aside from its clock columns, final parameters)
            const std::string a = trainQuietly(algo), b = trainQuietly(plain);
            REQUIRE(algo.m_agent->parameters() == plain.m_agent->parameters());
            REQUIRE(!a.empty() && !b.empty());
            const EvalResult after = algo.evaluate(8);
            std::printf("after train(): return_mean %a\n", after.stats.return_mean);
        } else if (mode == "hostenv") {
            PPO_Discrete dev;
            trainQuietly(dev);
            PPO_HostEnv<CartPole> host;
            host.m_agent->setParameters(dev.m_agent->parameters());
            const uint64_t steps_before = host.m_global_step;
            const EvalResult h = host.evaluate(8, [](int64_t e) { return std::make_shared<CartPole>(1000 + e); });
            REQUIRE(h.returns.size() == 8 && h.stats.episodes == 8);
            for (int64_t e = 0; e < 8; e++) {
                const EvalResult d = dev.evaluate(1, true, 1000 + e);
                std::printf("episode %lld: host %a / %d  device %a / %d\n", (long long)e, h.returns[e], h.lengths[e], d.returns[0], d.lengths[0]);
                REQUIRE(std::memcmp(&h.returns[e], &d.returns[0], sizeof(float)) == 0 && h.lengths[e] == d.lengths[0]);
            }
            // more episodes than envs in flight: 40 episodes over 16 envs; the first 8 are unchanged
            const EvalResult h40 = host.evaluate(40, [](int64_t e) { return std::make_shared<CartPole>(1000 + e); });
            REQUIRE(h40.stats.episodes == 40 && h40.stats.env_steps > 0);
            for (size_t e = 0; e < 8; e++) REQUIRE(h40.returns[e] == h.returns[e] && h40.lengths[e] == h.lengths[e]);
            REQUIRE(host.m_global_step == steps_before);   // no training state moved
        } else {
            std::fprintf(stderr, "usage: host_eval_test discrete|hostenv\n");
            return 2;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    std::printf("host_eval_test %s ok\n", mode.c_str());
    return 0;
}
