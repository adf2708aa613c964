// PPO with a categorical policy on Acrobot-v1 on the device (include/ppo_hip.h: PPO_ENV_ACROBOT): the sibling of PPO_Discrete on the fused 2 x 64 kernels.
//
//     PPO_DiscreteAcrobot algo;   // ./PPOConfig.toml: [environment] obs_size = 6, max_episode_steps >= 1 (default 500, gym's)
//     algo.train();
//
// The context is created with PPO_KERNEL_CAT_FUSED -- the env exists on the fused categorical kernels only, so the class sets fused_categorical itself,
// whatever the file says -- and one head of three actions, the torque -1, 0 or +1.  An iteration is ppo_rollout (one launch for all T steps, two for the
// critic), the scan and the update.  evaluate() runs whole episodes in one launch (ppo_evaluate).  The observation of this env does not hold the angles, so
// the time-limit fold is not built for it: [environment] bootstrap_truncated = true throws the library's refusal, with its message.
// [environment] keep_cut_states = true creates the context with PPO_KERNEL_ENV_CUT_STATE: the rollout keeps the state of every cut-off episode, and
// bootstrap_truncated = true / setBootstrapTruncated(true) is served.
#pragma once
#include "PPOAlgorithm.h"
#include "../Environments/Acrobot.h"

class PPO_DiscreteAcrobot : public PPOAlgorithm {
  public:
    PPO_DiscreteAcrobot() : PPOAlgorithm(PPO_ENV_ACROBOT, PPO_DIST_CATEGORICAL, 6, 500) {
        getArgs();
        normRewardOnDeviceEnv();   // [environment] norm_reward = true: rewards divided by the running std of the discounted return
        m_fused_categorical = true;
        m_action_size = 3;
        construct();
        if (m_bootstrap_truncated) setEnvTruncationBootstrap(true);
    }
    ppo::Tensor initEnvs() { return initEnvsImpl(); }
    void setBootstrapTruncated(bool on) { setEnvTruncationBootstrap(on); }
    bool bootstrapTruncated() const { return m_bootstrap_truncated; }
};
