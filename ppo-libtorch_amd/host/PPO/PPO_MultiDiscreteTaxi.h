// PPO with a masked categorical policy on Taxi-v3 on the device (include/ppo_hip.h: PPO_ENV_TAXI): the sibling of PPO_MultiDiscrete on the fused 2 x 64
// kernels, with an action mask that means something -- the env forms it on the chip, the rollout draws under it and stores it, the update reads it.
//
//     PPO_MultiDiscreteTaxi algo;   // ./PPOConfig.toml: [environment] obs_size = 19, max_episode_steps >= 1 (default 200, gym's)
//     algo.train();
//
// The context is created with PPO_DIST_MASKED and PPO_KERNEL_CAT_FUSED -- the env exists on the fused categorical kernels only, so the class sets
// fused_categorical itself, whatever the file says -- and one head of six actions (south, north, east, west, pickup, dropoff).  An iteration is ppo_rollout
// (one launch for all T steps, two for the critic), the scan and the update.  evaluate() runs whole episodes in one launch (ppo_evaluate).
// [environment] bootstrap_truncated = true turns the time-limit fold on (ppo_env_truncation_bootstrap: one more launch per rollout; an untrained policy hits
// the limit in most of its episodes here).  [environment] keep_cut_states = true creates the context with PPO_KERNEL_ENV_CUT_STATE: the fold then reads the
// state the rollout kept instead of decoding and stepping PPO_BUF_OBS again -- the same events and rewards, bit for bit.
#pragma once
#include "PPOAlgorithm.h"
#include "../Environments/Taxi.h"

class PPO_MultiDiscreteTaxi : public PPOAlgorithm {
  public:
    PPO_MultiDiscreteTaxi() : PPOAlgorithm(PPO_ENV_TAXI, PPO_DIST_MASKED, 19, 200) {
        getArgs();
        normRewardOnDeviceEnv();   // [environment] norm_reward = true: rewards divided by the running std of the discounted return
        m_fused_categorical = true;
        m_action_size = 6;
        construct();
        if (m_bootstrap_truncated) setEnvTruncationBootstrap(true);
    }
    ppo::Tensor initEnvs() { return initEnvsImpl(); }
    void setBootstrapTruncated(bool on) { setEnvTruncationBootstrap(on); }
    bool bootstrapTruncated() const { return m_bootstrap_truncated; }
};
