// PPO on the caller's own environments with real-valued (Box) actions: the sibling of PPO_HostEnv (PPO_HostEnv.h) for diagonal-Gaussian policies
// (include/ppo_hip.h: PPO_DIST_GAUSSIAN).  The reference has no continuous policy; the class follows its custom-environment framework all the same:
//
//     PPO_HostEnvBox<MyEnv> algo;                    // ./PPOConfig.toml with [environment] obs_size and action_dim = MyEnv's
//     algo.train();
//
// Env: std::vector<float> reset(); std::tuple<std::vector<float>, float, bool, bool> step(const std::vector<float>& action); episode_length;
// episode_reward.  step() receives the policy's RAW sample mu + sigma * eps, D = action_dim values: an env with bounds clips its own copy (the rollout keeps
// the raw sample, whose log-prob it stored).  The envs are made by a factory (default std::make_shared<Env>(m_seed)); each is stepped by one pool job at a time.
// The extension keys of PPO_HostEnv work the same way: norm_obs, norm_reward (statistics beside every checkpoint), bootstrap_truncated.  Env groups are
// not built for Gaussian contexts: env_groups > 1 throws the library's message.  `fused_policy = true` in [environment] (default false) runs the context
// on the fused Gaussian kernels (PPO_KERNEL_GAUSS_FUSED in ppo_hip.h: obs_size <= 64, action_dim <= 32); ppo_gauss_fused_launches(m_ctx, ...) tells.  Checkpoints keep the reference's container with one more tensor, m_logStd
// (Utils/TorchArchive.h); no exchange of such files with the reference is claimed.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "PPOAlgorithm.h"

template <class Env>
class PPO_HostEnvBox : public PPOAlgorithm {
  public:
    using EnvFactory = std::function<std::shared_ptr<Env>(int64_t env_index)>;

    explicit PPO_HostEnvBox(EnvFactory factory = nullptr) : PPOAlgorithm(PPO_ENV_HOST, PPO_DIST_GAUSSIAN, 4, 500) {
        getArgs();   // (action_dim, and the extension keys env_groups, bootstrap_truncated, norm_obs, norm_reward)
        construct();
        const bool norm_obs = m_norm_obs, norm_reward = m_norm_reward;   // the keys; the members follow the context from here on
        m_norm_obs = m_norm_reward = false;
        setEnvGroups(m_env_groups);
        if (norm_obs) setNormObs(true);
        if (norm_reward) setNormReward(true);
        m_envs.reserve(static_cast<size_t>(m_num_envs));
        for (int64_t i = 0; i < m_num_envs; i++) m_envs.push_back(factory ? factory(i) : std::make_shared<Env>(m_seed));
        const size_t N = static_cast<size_t>(m_num_envs), O = static_cast<size_t>(m_obs_size), D = static_cast<size_t>(m_action_size);
        m_next_obs.assign(N * O, 0.0f);
        m_final_obs.assign(N * O, 0.0f);
        m_reward.assign(N, 0.0f);
        m_fin_rew.assign(N, 0.0f);
        m_done.assign(N, 0);
        m_fin_len.assign(N, 0);
        m_truncated.assign(N, 0);
        m_action.assign(N * D, 0.0f);
    }

    std::vector<std::shared_ptr<Env>> m_envs;

    int64_t actionDim() const { return m_action_size; }

    // env groups: 1 only.  g > 1: the library's refusal (ppo_host_rollout_begin_groups on a Gaussian context), thrown with its message
    void setEnvGroups(int64_t g) {
        if (g < 1 || g > PPO_HOST_MAX_GROUPS || g > m_num_envs)
            throw std::runtime_error("env_groups = " + std::to_string(g) + ": expected 1 .. " + std::to_string(std::min<int64_t>(PPO_HOST_MAX_GROUPS, m_num_envs)));
        if (g > 1) {
            std::vector<int32_t> bounds(static_cast<size_t>(g) + 1);
            for (int64_t k = 0; k < g; k++) bounds[static_cast<size_t>(k)] = static_cast<int32_t>(k * (m_num_envs / g));
            bounds[static_cast<size_t>(g)] = static_cast<int32_t>(m_num_envs);
            ppo::check(ppo_host_rollout_begin_groups(m_ctx, static_cast<int32_t>(g), bounds.data()), m_ctx, "env_groups");
            throw std::runtime_error("env_groups = " + std::to_string(g) + " on a Gaussian context was not refused");
        }
        m_env_groups = g;
    }
    void setNormObs(bool on) {
        ppo::check(ppo_obs_norm_enable(m_ctx, on ? 1 : 0, 10.0f, 1e-8f), m_ctx, "norm_obs");
        m_norm_obs = on;
    }
    bool normObs() const { return m_norm_obs; }
    void setNormReward(bool on) {
        ppo::check(ppo_reward_norm_enable(m_ctx, on ? 1 : 0, 10.0f, 1e-8f), m_ctx, "norm_reward");
        m_norm_reward = on;
    }
    bool normReward() const { return m_norm_reward; }
    void setBootstrapTruncated(bool on) { m_bootstrap_truncated = on; }
    bool bootstrapTruncated() const { return m_bootstrap_truncated; }

    // initEnvs (PPO_Discrete.cpp:365-402) as PPO_HostEnv runs it: the obs-size check on env 0, then every env's reset observation
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
        throwBadWidth(bad_width);
        ppo::check(ppo_host_env_reset(m_ctx, m_next_obs.data()), m_ctx, "initEnvs");
        return bufferView(PPO_BUF_NEXT_OBS, { m_num_envs, m_obs_size }, ppo::DType::f32);
    }

    // stepEnvs (:413-483) on the pool with action f32 [N, D]: step, the time limit, the finished episode's length / reward, auto-reset
    void stepEnvs(const std::vector<float>& action) {
        std::atomic<int64_t> bad_width{ -1 };
        for (int64_t i = 0; i < m_num_envs; i++)
            m_threadPool->queueJob([this, i, &action, &bad_width]() { stepOne(i, action, bad_width); });
        m_threadPool->waitForJobsToFinish();
        throwBadWidth(bad_width);
    }

  protected:
    void trainInitEnvs() override { initEnvs(); }

    // one ppo_host_act_f32 and one stepEnvs per step; then values, advantages and the update, enqueued by ppo_host_rollout_end
    void trainRollout() override {
        ppo::check(ppo_host_rollout_begin(m_ctx), m_ctx, "rollout");
        for (int64_t t = 0; t < m_num_steps; t++) {
            ppo::check(ppo_host_act_f32(m_ctx, m_action.data()), m_ctx, "rollout");
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
    // one env's share of stepEnvs (a pool job: must not throw)
    void stepOne(int64_t i, const std::vector<float>& action, std::atomic<int64_t>& bad_width) {
        const size_t k = static_cast<size_t>(i), O = static_cast<size_t>(m_obs_size), D = static_cast<size_t>(m_action_size);
        Env& env = *m_envs[k];
        const std::vector<float> a(action.begin() + static_cast<std::ptrdiff_t>(k * D), action.begin() + static_cast<std::ptrdiff_t>((k + 1) * D));
        auto [obs, reward, terminated, info] = env.step(a);
        if (m_bootstrap_truncated) {
            const bool cut = !terminated && (info || static_cast<int64_t>(env.episode_length) == m_max_episode_steps);
            m_truncated[k] = cut ? 1 : 0;
            if (cut) {
                if (obs.size() != O) { bad_width = static_cast<int64_t>(obs.size()); return; }
                std::memcpy(m_final_obs.data() + k * O, obs.data(), sizeof(float) * O);
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
        if (obs.size() != O) bad_width = static_cast<int64_t>(obs.size());
        else copyObs(i, obs);
        m_reward[k] = reward;
        m_done[k] = terminated ? 1 : 0;
    }
    void throwBadWidth(const std::atomic<int64_t>& bad_width) const {
        if (bad_width >= 0)
            throw std::runtime_error("The environment returned an observation of size " + std::to_string(bad_width.load()) +
                                     ", but your config defined the expected observation size to be " + std::to_string(m_obs_size) + ".");
    }
    void copyObs(int64_t i, const std::vector<float>& o) {
        std::memcpy(m_next_obs.data() + static_cast<size_t>(i * m_obs_size), o.data(), sizeof(float) * static_cast<size_t>(m_obs_size));
    }

    std::vector<float> m_next_obs, m_reward, m_fin_rew, m_final_obs, m_action;   // m_action [N, D]: the raw samples of the current step
    std::vector<int32_t> m_done, m_fin_len, m_truncated;
};
