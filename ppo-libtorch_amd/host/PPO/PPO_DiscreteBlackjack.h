// PPO with a categorical policy on Blackjack-v1 (natural = False, sab = False, the infinite deck) on the device (include/ppo_hip.h: PPO_ENV_BLACKJACK): the
// sibling of PPO_DiscreteFrozenLake on the fused 2 x 64 kernels, on the device env whose step draws a number of cards that depends on the data.
//
//     PPO_DiscreteBlackjack algo;    // ./PPOConfig.toml: [environment] obs_size = 45 (the default), max_episode_steps in 1..16777215 (default 100; an
//     algo.train();                  //                   episode takes at most 20 steps, so any limit from 20 on never cuts one off)
//
// The context is created with PPO_KERNEL_CAT_FUSED -- the env exists on the fused categorical kernels only, so the class sets fused_categorical itself,
// whatever the file says -- and one head of two actions (stick, hit).  An iteration is ppo_rollout (one launch for all T steps, two for the critic), the scan
// and the update.  evaluate() runs whole episodes in one launch (ppo_evaluate); a return is -1, 0 or +1.  The observation of this env holds neither the index
// of the next card nor the episode's key, so the time-limit fold is not built for it: [environment] bootstrap_truncated = true, and
// setBootstrapTruncated(true), throw the library's refusal, with its message.
// [environment] keep_cut_states = true creates the context with PPO_KERNEL_ENV_CUT_STATE: the rollout keeps the state of every cut-off episode (the key and the
// count with it), and both are served.
#pragma once
#include "PPOAlgorithm.h"
#include "../Environments/Blackjack.h"

class PPO_DiscreteBlackjack : public PPOAlgorithm {
  public:
    PPO_DiscreteBlackjack() : PPOAlgorithm(PPO_ENV_BLACKJACK, PPO_DIST_CATEGORICAL, Blackjack::OBS, 100) {
        getArgs();
        normRewardOnDeviceEnv();   // [environment] norm_reward = true: rewards divided by the running std of the discounted return
        m_fused_categorical = true;
        m_action_size = 2;
        construct();
        if (m_bootstrap_truncated) setEnvTruncationBootstrap(true);
    }
    ppo::Tensor initEnvs() { return initEnvsImpl(); }
    void setBootstrapTruncated(bool on) { setEnvTruncationBootstrap(on); }
    bool bootstrapTruncated() const { return m_bootstrap_truncated; }
    int envKind() const { return m_env_kind; }
};
