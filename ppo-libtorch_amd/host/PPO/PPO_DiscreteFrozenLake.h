// PPO with a categorical policy on FrozenLake-v1 / FrozenLake8x8-v1 (slippery) on the device (include/ppo_hip.h: PPO_ENV_FROZENLAKE, PPO_ENV_FROZENLAKE8X8):
// the sibling of PPO_DiscreteAcrobot on the fused 2 x 64 kernels, on the first device env whose transitions draw random numbers.
//
//     PPO_DiscreteFrozenLake algo;   // ./PPOConfig.toml: [environment] obs_size = 16 (the 4x4 map, the default) or 64 (the 8x8 map),
//     algo.train();                  //                   max_episode_steps in 1..16777215 (default 100, gym's for 4x4; gym's for 8x8 is 200)
//
// obs_size picks the env kind: 64 gives PPO_ENV_FROZENLAKE8X8, anything else PPO_ENV_FROZENLAKE (a width that is neither is refused by the library with the
// reference's obs-size message).  The context is created with PPO_KERNEL_CAT_FUSED -- the env exists on the fused categorical kernels only, so the class sets
// fused_categorical itself, whatever the file says -- and one head of four actions (left, down, right, up).  An iteration is ppo_rollout (one launch for all
// T steps, two for the critic), the scan and the update.  evaluate() runs whole episodes in one launch (ppo_evaluate).  The observation of this env holds
// neither the episode's step count nor its key, so the time-limit fold is not built for it: [environment] bootstrap_truncated = true, and
// setBootstrapTruncated(true), throw the library's refusal, with its message.
// [environment] keep_cut_states = true creates the context with PPO_KERNEL_ENV_CUT_STATE: the rollout keeps the state of every cut-off episode (the key and the
// count with it), and both are served.
#pragma once
#include "PPOAlgorithm.h"
#include "../Environments/FrozenLake.h"

class PPO_DiscreteFrozenLake : public PPOAlgorithm {
  public:
    PPO_DiscreteFrozenLake() : PPOAlgorithm(PPO_ENV_FROZENLAKE, PPO_DIST_CATEGORICAL, 16, 100) {
        getArgs();
        normRewardOnDeviceEnv();   // [environment] norm_reward = true: rewards divided by the running std of the discounted return
        if (m_obs_size == 64) m_env_kind = PPO_ENV_FROZENLAKE8X8;
        m_fused_categorical = true;
        m_action_size = 4;
        construct();
        if (m_bootstrap_truncated) setEnvTruncationBootstrap(true);
    }
    ppo::Tensor initEnvs() { return initEnvsImpl(); }
    void setBootstrapTruncated(bool on) { setEnvTruncationBootstrap(on); }
    bool bootstrapTruncated() const { return m_bootstrap_truncated; }
    int envKind() const { return m_env_kind; }
};
