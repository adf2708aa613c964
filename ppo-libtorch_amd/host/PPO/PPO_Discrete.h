// Drop-in for the reference's PPO/PPO_Discrete.h: PPO with a single categorical head on CartPole envs.
#pragma once
#include "PPOAlgorithm.h"
#include "../Environments/CartPole.h"

class PPO_Discrete : public PPOAlgorithm {
  public:
    PPO_Discrete();
    AgentOutput computeActionLogic(const ppo::Tensor& next_obs) const;   // PPO_Discrete.cpp:258-263
    ppo::Tensor initEnvs();                                              // :365-402
    // bootstrap the value where max_episode_steps cut an episode off (`bootstrap_truncated = true` in [environment]; default false): the rollout folds
    // gamma V(final observation) into the reward there instead of treating the state as terminal (include/ppo_hip.h, ppo_env_truncation_bootstrap);
    // false: the reference's stepEnvs (PPO_Discrete.cpp:443-452)
    void setBootstrapTruncated(bool on) { setEnvTruncationBootstrap(on); }
    bool bootstrapTruncated() const { return m_bootstrap_truncated; }
};
