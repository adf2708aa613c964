// PPO on the caller's own environments: the reference's custom-environment framework (README: "easily implement your own training environments").
// A reference user writes a class with reset() / step(action) / episode_length / episode_reward and puts it in place of CartPole in PPO_Discrete's
// m_envs; stepEnvs steps them on the thread pool (PPO_Discrete.cpp:365-483).  Here the same class is the template argument:
//
//     PPO_HostEnv<MyEnv> algo;                       // ./PPOConfig.toml as for PPO_Discrete (obs_size / action_size = MyEnv's)
//     algo.train();
//
// Env (duck type of the reference's CartPole): std::vector<float> reset(); std::tuple<std::vector<float>, float, bool, bool> step(const int64_t&);
// episode_length; episode_reward; and, when Masked, getActionMask() (any container of A values convertible to bool, or a ppo::Tensor of u8).
// The envs are made by a factory (default std::make_shared<Env>(m_seed), as the reference constructs its CartPoles).  Every env is stepped by one
// pool job at a time; envs must not share mutable state with each other (the facade's CartPole owns its Device: no shared HIP stream or context).
// The context (PPO_ENV_HOST) owns parameters, AdamW state, rollout buffers, sampler and episode statistics: include/ppo_hip.h ppo_host_*.
//
// Env groups (setEnvGroups(g), or `env_groups = g` in [environment] of PPOConfig.toml; default 1): with g > 1 the envs are cut into g equal contiguous
// groups (the remainder goes to the last) and the rollout is pipelined: while the pool steps group k, the main thread enqueues the policy call of the
// next group and collects its actions (ppo_host_group_*).  The GPU and host-link round trip of one group then hides behind the env stepping of
// another.  Training does not depend on g in a single bit.
//
// Time limits (setBootstrapTruncated(true), or `bootstrap_truncated = true` in [environment]; default false): the reference ends an episode that reaches
// max_episode_steps like one the env terminated (PPO_Discrete.cpp:443-452) and never reads the fourth value step() returns, its `truncated` flag.  With
// the option on, an episode ends when the env terminates, when the env itself reports truncated, or at max_episode_steps; one that ended without the
// env's `terminated` counts as truncated, the observation it ended on is kept, and the rollout's end bootstraps the value there (r + gamma V(final
// observation)) instead of treating the state as terminal (include/ppo_hip.h, "Time-limit truncations").  Off, stepEnvs is the reference's.
//
// Observation normalisation (setNormObs(true), or `norm_obs = true` in [environment]; default false): every batch of observations -- the reset
// observations, then each step's -- updates running mean / variance statistics on the device and is normalised and clipped to +-10 before the network or
// the rollout buffer sees it (include/ppo_hip.h, "Observation normalisation").  The statistics are saved beside every agent checkpoint
// ("<agent file>.obsnorm", ObsNormFile) and loaded with it when present.  Not with env groups: the constructor and the setters throw the ABI's message.
//
// Reward normalisation (setNormReward(true), or `norm_reward = true` in [environment]; default false): every step's rewards are divided by the running
// standard deviation of the discounted return and clipped to +-10 before the rollout buffer sees them; the episode statistics keep the raw reward
// (include/ppo_hip.h, "Reward normalisation").  Saved as "<agent file>.rewnorm" (RewardNormFile), loaded when present, refused with env groups likewise.
//
// `fused_categorical = true` in [environment] (default false) runs the context on the fused categorical 2 x 64 kernels (PPO_KERNEL_CAT_FUSED in ppo_hip.h:
// obs_size <= 64); ppo_gauss_fused_launches(m_ctx, ...), the family's counters, tells.  Same parameter order: checkpoints move between runs with and without the key.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "PPOAlgorithm.h"

template <class Env, bool Masked = false>
class PPO_HostEnv : public PPOAlgorithm {
  public:
    using EnvFactory = std::function<std::shared_ptr<Env>(int64_t env_index)>;

    explicit PPO_HostEnv(EnvFactory factory = nullptr)
        : PPOAlgorithm(PPO_ENV_HOST, Masked ? PPO_DIST_MASKED : PPO_DIST_CATEGORICAL, 4, 500) {
        getArgs();   // (reads the extension keys env_groups, bootstrap_truncated, norm_obs, norm_reward and fused_categorical too)
        construct();
        const bool norm_obs = m_norm_obs;   // the key; the member follows the context from here on (setNormObs)
        m_norm_obs = false;
        const bool norm_reward = m_norm_reward;   // likewise (setNormReward)
        m_norm_reward = false;
        setEnvGroups(m_env_groups);
        if (norm_obs) setNormObs(true);
        if (norm_reward) setNormReward(true);
        m_envs.reserve(static_cast<size_t>(m_num_envs));
        for (int64_t i = 0; i < m_num_envs; i++) m_envs.push_back(factory ? factory(i) : std::make_shared<Env>(m_seed));
        const size_t N = static_cast<size_t>(m_num_envs);
        m_next_obs.assign(N * static_cast<size_t>(m_obs_size), 0.0f);
        m_reward.assign(N, 0.0f);
        m_done.assign(N, 0);
        m_fin_len.assign(N, 0);
        m_fin_rew.assign(N, 0.0f);
        m_truncated.assign(N, 0);
        m_final_obs.assign(N * static_cast<size_t>(m_obs_size), 0.0f);
        m_action.assign(N, 0);
        if (Masked) m_mask.assign(N * static_cast<size_t>(m_action_size), 1);
    }

    std::vector<std::shared_ptr<Env>> m_envs;

    // g env groups for trainRollout's pipeline (1: the whole batch per call, as always)
    void setEnvGroups(int64_t g) {
        if (g < 1 || g > PPO_HOST_MAX_GROUPS || g > m_num_envs)
            throw std::runtime_error("env_groups = " + std::to_string(g) + ": expected 1 .. " + std::to_string(std::min<int64_t>(PPO_HOST_MAX_GROUPS, m_num_envs)));
        if (g > 1 && m_norm_obs) refuseGroupsWithNormObs(g);
        if (g > 1 && m_norm_reward) refuseGroupsWithNormReward(g);
        m_env_groups = g;
    }
    int64_t envGroups() const { return m_env_groups; }

    // running mean / variance normalisation of the observations (ppo_obs_norm_enable: update + apply, clip 10, eps 1e-8); false: raw observations.  The
    // statistics are kept when it is turned off.
    void setNormObs(bool on) {
        ppo::check(ppo_obs_norm_enable(m_ctx, on ? 1 : 0, 10.0f, 1e-8f), m_ctx, "norm_obs");
        m_norm_obs = on;
        if (on && m_env_groups > 1) {
            try { refuseGroupsWithNormObs(m_env_groups); }
            catch (...) { ppo_obs_norm_enable(m_ctx, 0, 10.0f, 1e-8f); m_norm_obs = false; throw; }
        }
    }
    bool normObs() const { return m_norm_obs; }

    // rewards divided by the running standard deviation of the discounted return (ppo_reward_norm_enable: update + apply, clip 10, eps 1e-8); false: raw
    // rewards.  The statistics are kept when it is turned off.
    void setNormReward(bool on) {
        ppo::check(ppo_reward_norm_enable(m_ctx, on ? 1 : 0, 10.0f, 1e-8f), m_ctx, "norm_reward");
        m_norm_reward = on;
        if (on && m_env_groups > 1) {
            try { refuseGroupsWithNormReward(m_env_groups); }
            catch (...) { ppo_reward_norm_enable(m_ctx, 0, 10.0f, 1e-8f); m_norm_reward = false; throw; }
        }
    }
    bool normReward() const { return m_norm_reward; }

    // bootstrap the value where a time limit (the env's own truncated flag, or max_episode_steps) cut an episode off; false: the reference's stepEnvs
    void setBootstrapTruncated(bool on) { m_bootstrap_truncated = on; }
    bool bootstrapTruncated() const { return m_bootstrap_truncated; }

    // initEnvs (:365-402): env 0 once for the obs-size check, then every env (env 0 twice, as the reference); NEXT_OBS = the reset observations
    ppo::Tensor initEnvs() {
        const std::vector<float> test_obs = m_envs[0]->reset();
        if (static_cast<int64_t>(test_obs.size()) != m_obs_size)
            throw std::runtime_error("The environment returned an observation of size " + std::to_string(test_obs.size()) +
                                     ", but your config defined the expected observation size to be " + std::to_string(m_obs_size) + ".\n" +
                                     "Have you properly defined your PPOConfig.toml file for your environment?");
        std::atomic<int64_t> bad_width{ -1 };
        for (int64_t i = 0; i < m_num_envs; i++)
            m_threadPool->queueJob([this, i, &bad_width]() {
                const std::vector<float> o = m_envs[static_cast<size_t>(i)]->reset();
                if (static_cast<int64_t>(o.size()) != m_obs_size) bad_width = static_cast<int64_t>(o.size());
                else copyObs(i, o);
            });
        m_threadPool->waitForJobsToFinish();
        if (bad_width >= 0) throw std::runtime_error("an environment returned an observation of size " + std::to_string(bad_width.load()) + " on reset");
        ppo::check(ppo_host_env_reset(m_ctx, m_next_obs.data()), m_ctx, "initEnvs");
        return bufferView(PPO_BUF_NEXT_OBS, { m_num_envs, m_obs_size }, ppo::DType::f32);
    }

    // stepEnvs (:413-483) on the pool: step, truncation at max_episode_steps, the finished episode's length / reward from the env itself, auto-reset.
    // Fills the host arrays ppo_host_observe takes.
    void stepEnvs(const std::vector<int64_t>& action) {
        std::atomic<int64_t> bad_width{ -1 };
        for (int64_t i = 0; i < m_num_envs; i++)
            m_threadPool->queueJob([this, i, &action, &bad_width]() { stepOne(i, action, bad_width); });
        m_threadPool->waitForJobsToFinish();
        throwBadWidth(bad_width);
    }

    // Held-out greedy evaluation on the caller's envs: episode e runs on a FRESH env factory(e) (never a training env: m_envs, their episode sums
    // and the context's rollout state stay as they are), up to num_envs episodes in flight on a thread pool, one ppo_policy_act_greedy launch per
    // step over the envs in flight, truncation at max_episode_steps as stepEnvs applies it.  An episode's return and length are the env's own
    // episode_reward / episode_length (:474-480).  Prints nothing.
    EvalResult evaluate(int64_t episodes, EnvFactory factory) {
        if (episodes <= 0 || !factory) throw std::runtime_error("PPO_HostEnv::evaluate needs episodes > 0 and an env factory");
        const size_t N = static_cast<size_t>(m_num_envs), O = static_cast<size_t>(m_obs_size), A = static_cast<size_t>(m_action_size);
        EvalResult r;
        r.returns.assign(static_cast<size_t>(episodes), 0.0f);
        r.lengths.assign(static_cast<size_t>(episodes), 0);
        std::vector<std::shared_ptr<Env>> envs;     // the episodes in flight, densely packed
        std::vector<int64_t> episode;
        std::vector<float> obs(N * O, 0.0f);
        std::vector<uint8_t> mask(Masked ? N * A : 0, 1);
        std::vector<char> finished(N, 0);
        ppo::Tensor d_obs(m_device, { m_num_envs, m_obs_size }, ppo::DType::f32), d_act(m_device, { m_num_envs, 1 }, ppo::DType::i64);
        ppo::Tensor d_mask;
        if (Masked) d_mask = ppo::Tensor(m_device, { m_num_envs, m_action_size }, ppo::DType::u8);
        // a pool of its own: m_threadPool runs only inside train() (which starts and stops it), and evaluate() may be called from train()'s m_on_update
        const int64_t hw = static_cast<int64_t>(std::thread::hardware_concurrency());
        ThreadPool pool(std::max<int64_t>(1, std::min<int64_t>(m_num_envs, hw)));
        pool.start();
        int64_t next = 0;
        std::atomic<int64_t> bad_width{ -1 };
        std::atomic<bool> failed{ false };
        auto put = [&](size_t k, const std::vector<float>& o) {
            if (o.size() != O) bad_width = static_cast<int64_t>(o.size());
            else std::memcpy(obs.data() + k * O, o.data(), sizeof(float) * O);
        };
        while (next < episodes || !envs.empty()) {
            while (envs.size() < N && next < episodes) {   // start further episodes, in index order
                envs.push_back(factory(next));
                episode.push_back(next++);
                put(envs.size() - 1, envs.back()->reset());
            }
            if (bad_width >= 0) throw std::runtime_error("an environment returned an observation of size " + std::to_string(bad_width.load()) + " on reset");
            const size_t k_live = envs.size();
            if constexpr (Masked) {
                for (size_t k = 0; k < k_live; k++) {
                    const auto m = envs[k]->getActionMask();
                    for (size_t a = 0; a < A; a++) mask[k * A + a] = maskAt(m, a) ? 1 : 0;
                }
                d_mask.copy_from_host(mask);
            }
            d_obs.copy_from_host(obs);
            ppo::check(ppo_policy_act_greedy(m_ctx, d_obs.template data<float>(), Masked ? d_mask.template data<uint8_t>() : nullptr, static_cast<int64_t>(k_live),
                                             d_act.template data<int64_t>(), nullptr, nullptr, nullptr),
                       m_ctx, "evaluate");
            ppo::check(ppo_sync(m_ctx), m_ctx, "sync");
            const std::vector<int64_t> action = d_act.template cpu<int64_t>();
            for (size_t k = 0; k < k_live; k++)
                pool.queueJob([&, k]() { try {
                    Env& env = *envs[k];
                    auto [o, reward, terminated, info] = env.step(action[k]);
                    (void)reward; (void)info;
                    if (static_cast<int64_t>(env.episode_length) == m_max_episode_steps) terminated = true;
                    finished[k] = terminated ? 1 : 0;
                    if (terminated) {
                        r.returns[static_cast<size_t>(episode[k])] = static_cast<float>(env.episode_reward);
                        r.lengths[static_cast<size_t>(episode[k])] = static_cast<int32_t>(env.episode_length);
                    } else {
                        put(k, o);
                    }
                } catch (...) { failed = true; } });   // (the pool swallows a job's exception: an episode that cannot step must not be stepped for ever)
            pool.waitForJobsToFinish();
            if (failed) throw std::runtime_error("PPO_HostEnv::evaluate: an environment's step threw");
            if (bad_width >= 0) throw std::runtime_error("an environment returned an observation of size " + std::to_string(bad_width.load()));
            size_t w = 0;   // drop the finished episodes, keep the rest packed
            for (size_t k = 0; k < k_live; k++) {
                if (finished[k]) continue;
                if (w != k) {
                    envs[w] = envs[k];
                    episode[w] = episode[k];
                    std::memcpy(obs.data() + w * O, obs.data() + k * O, sizeof(float) * O);
                }
                w++;
            }
            envs.resize(w);
            episode.resize(w);
        }
        r.stats = summarizeEpisodes(r.returns, r.lengths, m_max_episode_steps);
        return r;
    }

  protected:
    void trainInitEnvs() override { initEnvs(); }

    // the rollout of :524-548 with the caller's envs: one ppo_host_act (one kernel, one wait) and one stepEnvs per step; then values, advantages
    // and the update, enqueued by ppo_host_rollout_end
    void trainRollout() override {
        if (m_env_groups > 1) { trainRolloutGroups(); return; }
        ppo::check(ppo_host_rollout_begin(m_ctx), m_ctx, "rollout");
        for (int64_t t = 0; t < m_num_steps; t++) {
            if constexpr (Masked) gatherMasks();
            ppo::check(ppo_host_act(m_ctx, Masked ? m_mask.data() : nullptr, m_action.data()), m_ctx, "rollout");
            stepEnvs(m_action);
            if (m_bootstrap_truncated)
                ppo::check(ppo_host_observe_truncated(m_ctx, m_next_obs.data(), m_reward.data(), m_done.data(), m_fin_len.data(), m_fin_rew.data(),
                                                      m_truncated.data(), m_final_obs.data()),
                           m_ctx, "rollout");
            else
                ppo::check(ppo_host_observe(m_ctx, m_next_obs.data(), m_reward.data(), m_done.data(), m_fin_len.data(), m_fin_rew.data()), m_ctx, "rollout");
        }
        ppo::check(ppo_host_rollout_end(m_ctx), m_ctx, "update");
    }

  private:
    // norm_obs and env_groups > 1: the library refuses the grouped rollout; ask it now and throw its message (the refused call changes nothing)
    void refuseGroupsWithNormObs(int64_t g) {
        std::vector<int32_t> bounds(static_cast<size_t>(g) + 1);
        for (int64_t k = 0; k < g; k++) bounds[static_cast<size_t>(k)] = static_cast<int32_t>(k * (m_num_envs / g));
        bounds[static_cast<size_t>(g)] = static_cast<int32_t>(m_num_envs);
        ppo::check(ppo_host_rollout_begin_groups(m_ctx, static_cast<int32_t>(g), bounds.data()), m_ctx, "norm_obs with env_groups");
        throw std::runtime_error("norm_obs with env_groups = " + std::to_string(g) + " was not refused");
    }
    // norm_reward and env_groups > 1, likewise
    void refuseGroupsWithNormReward(int64_t g) {
        std::vector<int32_t> bounds(static_cast<size_t>(g) + 1);
        for (int64_t k = 0; k < g; k++) bounds[static_cast<size_t>(k)] = static_cast<int32_t>(k * (m_num_envs / g));
        bounds[static_cast<size_t>(g)] = static_cast<int32_t>(m_num_envs);
        ppo::check(ppo_host_rollout_begin_groups(m_ctx, static_cast<int32_t>(g), bounds.data()), m_ctx, "norm_reward with env_groups");
        throw std::runtime_error("norm_reward with env_groups = " + std::to_string(g) + " was not refused");
    }
    // one env's share of stepEnvs (a pool job: must not throw)
    void stepOne(int64_t i, const std::vector<int64_t>& action, std::atomic<int64_t>& bad_width) {
        const size_t k = static_cast<size_t>(i);
        Env& env = *m_envs[k];
        auto [obs, reward, terminated, info] = env.step(action[k]);
        if (m_bootstrap_truncated) {
            // the episode ends where the env terminates, where the env's own fourth value says truncated, or at max_episode_steps; it was truncated
            // when it ended without the env's `terminated`: its last observation is kept for the bootstrap
            const bool cut = !terminated && (info || static_cast<int64_t>(env.episode_length) == m_max_episode_steps);
            m_truncated[k] = cut ? 1 : 0;
            if (cut) {
                if (static_cast<int64_t>(obs.size()) != m_obs_size) { bad_width = static_cast<int64_t>(obs.size()); return; }
                std::memcpy(m_final_obs.data() + k * static_cast<size_t>(m_obs_size), obs.data(), sizeof(float) * static_cast<size_t>(m_obs_size));
                terminated = true;
            }
        } else {
            (void)info;
            if (static_cast<int64_t>(env.episode_length) == m_max_episode_steps) terminated = true;
        }
        m_fin_len[k] = 0;
        m_fin_rew[k] = 0.0f;
        if (terminated) {
            m_fin_len[k] = static_cast<int32_t>(env.episode_length);
            m_fin_rew[k] = static_cast<float>(env.episode_reward);
            obs = env.reset();
        }
        if (static_cast<int64_t>(obs.size()) != m_obs_size) bad_width = static_cast<int64_t>(obs.size());   // (pool jobs must not throw)
        else copyObs(i, obs);
        m_reward[k] = reward;
        m_done[k] = terminated ? 1 : 0;
    }
    void throwBadWidth(const std::atomic<int64_t>& bad_width) const {
        if (bad_width >= 0)
            throw std::runtime_error("The environment returned an observation of size " + std::to_string(bad_width.load()) +
                                     ", but your config defined the expected observation size to be " + std::to_string(m_obs_size) + ".");
    }

    // Jobs of ONE group still running.  The pool's waitForJobsToFinish waits for every job of every group, which would put the groups back in series.
    struct Latch {
        std::mutex mu;
        std::condition_variable cv;
        int64_t left = 0;
        void arm(int64_t n) { std::lock_guard<std::mutex> g(mu); left = n; }
        // notified with the mutex held: the waiter cannot return (and the latch go out of scope) until this job has let go of mutex and condition variable
        void done() { std::lock_guard<std::mutex> g(mu); --left; cv.notify_all(); }
        void wait() { std::unique_lock<std::mutex> g(mu); cv.wait(g, [this] { return left == 0; }); }
    };
    struct LatchDone {   // counts the job down however it ends (the pool swallows a job's exception)
        Latch& l;
        ~LatchDone() { l.done(); }
    };

    // The rollout as a pipeline over env groups.  Main thread, per group g in turn: read g's actions (waits for g's launch only), hand g's envs to the
    // pool, then finish the group whose envs were handed over before -- wait for ITS jobs, stage its observations, enqueue its next policy call.  So the
    // GPU and the host link serve one group while the pool steps another.  Group by group the calls are those of the ungrouped rollout, and the rollout
    // is the same in every bit (include/ppo_hip.h, "Env groups").
    void trainRolloutGroups() {
        const int64_t G = m_env_groups, N = m_num_envs, T = m_num_steps;
        std::vector<int32_t> bounds(static_cast<size_t>(G) + 1);
        for (int64_t g = 0; g < G; g++) bounds[static_cast<size_t>(g)] = static_cast<int32_t>(g * (N / G));
        bounds[static_cast<size_t>(G)] = static_cast<int32_t>(N);
        std::vector<Latch> latch(static_cast<size_t>(G));
        std::vector<int64_t> t_of(static_cast<size_t>(G), 0);
        std::atomic<int64_t> bad_width{ -1 };
        const size_t O = static_cast<size_t>(m_obs_size), A = static_cast<size_t>(m_action_size);
        auto act = [&](int64_t g) {
            const size_t b = static_cast<size_t>(bounds[static_cast<size_t>(g)]);
            if constexpr (Masked) gatherMasks(b, static_cast<size_t>(bounds[static_cast<size_t>(g) + 1]));
            ppo::check(ppo_host_group_act(m_ctx, static_cast<int32_t>(g), Masked ? m_mask.data() + b * A : nullptr), m_ctx, "rollout");
        };
        auto finish = [&](int64_t g) {   // the group's envs have been handed to the pool: wait for them, stage, enqueue the group's next step
            const size_t b = static_cast<size_t>(bounds[static_cast<size_t>(g)]);
            latch[static_cast<size_t>(g)].wait();
            if (bad_width >= 0) return;
            if (m_bootstrap_truncated)
                ppo::check(ppo_host_group_observe_truncated(m_ctx, static_cast<int32_t>(g), m_next_obs.data() + b * O, m_reward.data() + b, m_done.data() + b,
                                                            m_fin_len.data() + b, m_fin_rew.data() + b, m_truncated.data() + b, m_final_obs.data() + b * O),
                           m_ctx, "rollout");
            else
                ppo::check(ppo_host_group_observe(m_ctx, static_cast<int32_t>(g), m_next_obs.data() + b * O, m_reward.data() + b, m_done.data() + b,
                                                  m_fin_len.data() + b, m_fin_rew.data() + b),
                           m_ctx, "rollout");
            if (++t_of[static_cast<size_t>(g)] < T) act(g);
        };
        ppo::check(ppo_host_rollout_begin_groups(m_ctx, static_cast<int32_t>(G), bounds.data()), m_ctx, "rollout");
        for (int64_t g = 0; g < G; g++) act(g);
        int64_t stepping = -1;   // the group whose envs the pool is stepping
        try {
            for (int64_t t = 0; t < T; t++)
                for (int64_t g = 0; g < G; g++) {
                    const int64_t b0 = bounds[static_cast<size_t>(g)], b1 = bounds[static_cast<size_t>(g) + 1];
                    ppo::check(ppo_host_group_actions(m_ctx, static_cast<int32_t>(g), m_action.data() + b0), m_ctx, "rollout");
                    Latch& l = latch[static_cast<size_t>(g)];
                    l.arm(b1 - b0);
                    for (int64_t i = b0; i < b1; i++)
                        m_threadPool->queueJob([this, i, &l, &bad_width]() { LatchDone d{ l }; stepOne(i, m_action, bad_width); });
                    if (stepping >= 0) finish(stepping);
                    stepping = g;
                    throwBadWidth(bad_width);
                }
            finish(stepping);
            stepping = -1;
            throwBadWidth(bad_width);
        } catch (...) {
            m_threadPool->waitForJobsToFinish();   // no job may outlive the latches and bad_width it refers to
            throw;
        }
        ppo::check(ppo_host_rollout_end(m_ctx), m_ctx, "update");
    }

    void copyObs(int64_t i, const std::vector<float>& o) {
        std::memcpy(m_next_obs.data() + static_cast<size_t>(i * m_obs_size), o.data(), sizeof(float) * static_cast<size_t>(m_obs_size));
    }
    template <class M> static bool maskAt(const M& m, size_t a) {
        if constexpr (std::is_same<M, ppo::Tensor>::value) return m.template cpu<uint8_t>()[a] != 0;
        else return static_cast<bool>(m[a]);
    }
    void gatherMasks() { gatherMasks(0, m_envs.size()); }
    void gatherMasks(size_t i0, size_t i1) {
        const size_t A = static_cast<size_t>(m_action_size);
        for (size_t i = i0; i < i1; i++) {
            const auto m = m_envs[i]->getActionMask();
            for (size_t a = 0; a < A; a++) m_mask[i * A + a] = maskAt(m, a) ? 1 : 0;
        }
    }

    std::vector<float> m_next_obs, m_reward, m_fin_rew, m_final_obs;   // m_final_obs [k]: the observation env k's truncated episode ended on
    std::vector<int32_t> m_done, m_fin_len, m_truncated;
    std::vector<int64_t> m_action;
    std::vector<uint8_t> m_mask;
};
