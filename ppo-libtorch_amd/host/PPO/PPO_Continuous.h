// PPO with a diagonal-Gaussian policy on the library's own continuous-action env, Pendulum-v1 on the device (include/ppo_hip.h: PPO_ENV_PENDULUM): the sibling
// of PPO_Discrete.  The reference has no continuous policy; the class keeps its shape all the same:
//
//     PPO_Continuous algo;          // ./PPOConfig.toml: [environment] obs_size = 3, max_episode_steps <= 290 (default 200)
//     algo.train();
//
// The context is created with PPO_KERNEL_GAUSS_FUSED -- the env exists on the fused Gaussian kernels only, so the class sets fused_policy itself, whatever
// the file says -- and one action dimension.  An iteration is what it is for the built-in discrete envs: ppo_rollout (one launch for all T steps, two for
// the critic), the scan and the update, enqueued by PPOAlgorithm::train().  Checkpoints go through the reference's container with one more tensor, m_logStd
// (Utils/TorchArchive.h).  evaluate() and bootstrap_truncated are not built for this env: the library's refusal is thrown with its message.
// [environment] keep_cut_states = true creates the context with PPO_KERNEL_ENV_CUT_STATE: the rollout keeps theta and theta_dot of every cut-off episode, and
// bootstrap_truncated = true / setBootstrapTruncated(true) is served -- on this env every episode ends at the limit, so every finished episode is bootstrapped.
#pragma once
#include "PPOAlgorithm.h"
#include "../Environments/Pendulum.h"

class PPO_Continuous : public PPOAlgorithm {
  public:
    PPO_Continuous() : PPOAlgorithm(PPO_ENV_PENDULUM, PPO_DIST_GAUSSIAN, 3, 200) {
        getArgs();
        normRewardOnDeviceEnv();   // [environment] norm_reward = true: rewards divided by the running std of the discounted return
        m_fused_policy = true;
        m_action_size = 1;
        construct();
        if (m_bootstrap_truncated) setEnvTruncationBootstrap(true);   // without keep_cut_states it throws: the fold from PPO_BUF_OBS is not built for this env
    }
    ppo::Tensor initEnvs() { return initEnvsImpl(); }
    void setBootstrapTruncated(bool on) { setEnvTruncationBootstrap(on); }
    bool bootstrapTruncated() const { return m_bootstrap_truncated; }
    int64_t actionDim() const { return m_action_size; }
};
