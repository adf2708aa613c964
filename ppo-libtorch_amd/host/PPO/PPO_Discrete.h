// Drop-in for the reference's PPO/PPO_Discrete.h: PPO with a single categorical head on CartPole envs.
// One extension key, `[network] hidden_size = H`: the two hidden layers are H wide (1 .. 2048) and the context runs on the generic engine
// (PPO_KERNEL_ENV_GENERIC, include/ppo_hip.h); checkpoints carry the width (TorchArchive's writeAgent / agentShapes take it) and load into an object with the
// same key.  Absent: 64, no flag, today's kernels and printout.  Depth other than 2 and bf16 storage stay with the C-ABI and the Python binding: the
// reference's archive names two hidden layers per net and no others.  With the key present two things the class offers are refused by the library, and the
// refusal is thrown as std::runtime_error with its message: evaluate() (the episode kernels hold the 2 x 64 network; step the episodes with
// ppo_policy_act_greedy + ppo_env_transition) and `bootstrap_truncated = true` / setBootstrapTruncated(true) (the fold is built on the reference-shape critic)
// -- the latter already in the constructor.
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
