// Drop-in for the reference's PPO/PPO_MultiDiscrete.h: masked (multi-)categorical heads on MountainCar envs.
// One extension key, `[network] hidden_size = H`, as in PPO_Discrete.h: two hidden layers of H on the generic engine (PPO_KERNEL_ENV_GENERIC); absent: 64 and
// today's kernels.  Depth other than 2 and bf16 storage stay with the C-ABI and the Python binding (the reference's archive names two hidden layers only).
// With the key present evaluate() and `bootstrap_truncated = true` / setBootstrapTruncated(true) throw the library's refusal, as in PPO_Discrete.h.
#pragma once
#include "PPOAlgorithm.h"
#include "../Environments/MountainCar.h"

class PPO_MultiDiscrete : public PPOAlgorithm {
  public:
    PPO_MultiDiscrete();
    AgentOutput computeActionLogic(const ppo::Tensor& next_obs, const ppo::Tensor& action_mask, const ppo::Tensor& action = ppo::Tensor());  // PPO_MultiDiscrete.cpp:271-277
    ppo::Tensor initEnvs(const ppo::Tensor& action_mask);                // :380-423 (fills the mask with ones)
    // bootstrap the value where max_episode_steps cut an episode off (`bootstrap_truncated = true` in [environment]; default false): the rollout folds
    // gamma V(final observation) into the reward there instead of treating the state as terminal (include/ppo_hip.h, ppo_env_truncation_bootstrap);
    // false: the reference's stepEnvs (PPO_MultiDiscrete.cpp, as PPO_Discrete.cpp:443-452)
    void setBootstrapTruncated(bool on) { setEnvTruncationBootstrap(on); }
    bool bootstrapTruncated() const { return m_bootstrap_truncated; }
};
