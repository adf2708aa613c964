// PPO with a diagonal-Gaussian policy on the library's second continuous-action env, MountainCarContinuous-v0 on the device (include/ppo_hip.h:
// PPO_ENV_MOUNTAINCAR_CONTINUOUS): the sibling of PPO_Continuous, with what that env adds.
//
//     PPO_ContinuousMountainCar algo;   // ./PPOConfig.toml: [environment] obs_size = 2, max_episode_steps >= 1 (default 999, gym's)
//     algo.train();
//
// The context is created with PPO_KERNEL_GAUSS_FUSED -- the env exists on the fused Gaussian kernels only, so the class sets fused_policy itself, whatever
// the file says -- and one action dimension, the force.  An iteration is PPO_Continuous's: ppo_rollout (one launch for all T steps, two for the critic), the
// scan and the update.  The observation of this env is its state, so the two things Pendulum refuses work here: [environment] bootstrap_truncated = true
// turns on the time-limit fold (one more launch behind the critic's; almost every episode of this env ends at the limit), and evaluate() runs whole episodes
// in one launch (ppo_evaluate).  [environment] keep_cut_states = true creates the context with PPO_KERNEL_ENV_CUT_STATE: the fold then reads the state the
// rollout kept instead of stepping PPO_BUF_OBS again -- the same events and rewards, bit for bit.
#pragma once
#include "PPOAlgorithm.h"
#include "../Environments/MountainCarContinuous.h"

class PPO_ContinuousMountainCar : public PPOAlgorithm {
  public:
    PPO_ContinuousMountainCar() : PPOAlgorithm(PPO_ENV_MOUNTAINCAR_CONTINUOUS, PPO_DIST_GAUSSIAN, 2, 999) {
        getArgs();
        normRewardOnDeviceEnv();   // [environment] norm_reward = true: rewards divided by the running std of the discounted return
        m_fused_policy = true;
        m_action_size = 1;
        construct();
        if (m_bootstrap_truncated) setEnvTruncationBootstrap(true);
    }
    ppo::Tensor initEnvs() { return initEnvsImpl(); }
    int64_t actionDim() const { return m_action_size; }
    void setBootstrapTruncated(bool on) { setEnvTruncationBootstrap(on); }
    bool bootstrapTruncated() const { return m_bootstrap_truncated; }
};
