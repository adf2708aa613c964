// Shared implementation behind the two algorithm classes of the reference, which are near-verbatim copies of each other
// (PPO/PPO_Discrete.{h,cpp} and PPO/PPO_MultiDiscrete.{h,cpp}; their diff is the env type, the masked distribution, the
// action-mask buffer and max_episode_steps).  Public members keep the reference's names (PPO_Discrete.h:24-108).
#pragma once
#include <array>
#include <chrono>
#include <functional>
#include <iomanip>
#include <iostream>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "../Tensor.h"
#include "../Utils/ThreadPool.h"
#include "../Utils/Utils.h"
#include "Agent.h"

// What evaluate() returns: the summary ppo_evaluate forms (include/ppo_hip.h ppo_eval_stats) and the per-episode numbers it is formed from.
// The observation normaliser's statistics as they sit beside a checkpoint (PPO_HostEnv with norm_obs): "<agent file>.obsnorm", raw little-endian f64:
// O, count, mean[O], var[O] -- 8 * (2 + 2 O) bytes, what ppo_obs_norm_get_h returns and ppo_obs_norm_set_h takes.  The .pt archives stay the reference's.
struct ObsNormFile {
    double count = 0.0;
    std::vector<double> mean, var;
    static std::string pathFor(const std::string& agentFile) { return agentFile + ".obsnorm"; }
    void write(const std::string& path) const;          // throws std::runtime_error
    static ObsNormFile read(const std::string& path);   // throws std::runtime_error (missing, wrong size, O <= 0)
};

// The reward normaliser's statistics beside a checkpoint (PPO_HostEnv with norm_reward): "<agent file>.rewnorm", raw little-endian f64 count, mean, var --
// 24 bytes, what ppo_reward_norm_get_h returns and ppo_reward_norm_set_h takes.  The discounted-return accumulators are not saved: a resume resets the envs.
struct RewardNormFile {
    double count = 0.0, mean = 0.0, var = 1.0;
    static std::string pathFor(const std::string& agentFile) { return agentFile + ".rewnorm"; }
    void write(const std::string& path) const;             // throws std::runtime_error
    static RewardNormFile read(const std::string& path);   // throws std::runtime_error (missing, not 24 bytes, negative or non-finite numbers)
};

struct EvalResult {
    ppo_eval_stats stats{};
    std::vector<float> returns;
    std::vector<int32_t> lengths;
};

class PPOAlgorithm {
  public:
    virtual ~PPOAlgorithm();

    // Setup
    void getArgs();                       // ./PPOConfig.toml, sections [environment] [general] [ppo] (PPO_Discrete.cpp:107-255)
    void loadPolicyFromCheckpoint();      // newest file of ./ModelCheckpoints + ./OptimizerCheckpoints (:782-835)
    void setTargetKL(float target_kl);    // m_target_kl and the context's switch (ppo_target_kl_set); 0 = off

    // ALGO LOGIC
    std::array<ppo::Tensor, 2> calcAdvantage(const ppo::Tensor& next_obs, const ppo::Tensor& next_done) const;  // {returns, advantages}, :274-331
    ppo::Tensor getApproxKLAndClippedObj(const ppo::Tensor& ratio, const ppo::Tensor& logratio);                 // :343-356
    void train();                                                                                              // :485-690

    // Held-out evaluation of the current policy (not in the reference, whose only quality signal is the mean over the last 100 exploration episodes,
    // :474-480): `episodes` whole episodes of the context's device env in one launch (ppo_evaluate), greedy (Categorical::mode) or sampled, episode e
    // from start state e of `seed` (default m_seed).  Prints nothing and leaves the training state untouched.  PPO_HostEnv has its own evaluate().
    EvalResult evaluate(int64_t episodes, bool greedy = true) { return evaluate(episodes, greedy, m_seed); }
    EvalResult evaluate(int64_t episodes, bool greedy, int64_t seed);
    // the summary of per-episode returns / lengths as ppo_evaluate forms it (f64, index order; truncated = episodes of max_episode_steps steps)
    static ppo_eval_stats summarizeEpisodes(const std::vector<float>& returns, const std::vector<int32_t>& lengths, int64_t max_episode_steps);

    // Controlling Environments
    std::tuple<ppo::Tensor, ppo::Tensor, ppo::Tensor> stepEnvs(const ppo::Tensor& action);                      // :413-483

    // Printing results to console
    void printPPOResults(int64_t update, int64_t global_step, std::chrono::milliseconds fps, std::chrono::milliseconds time_elapsed,
                         ppo::Tensor& approx_kl, ppo::Tensor& entropy_loss, ppo::Tensor& explained_var, ppo::Tensor& loss, ppo::Tensor& pg_loss,
                         ppo::Tensor& v_loss);
    template <typename T> void printElement(T t, const int& width) {
        std::cout << std::left << std::setw(width) << std::setfill(' ') << t << std::right << "|\n";
    }

    // Hyperparameters (defaults PPO_Discrete.cpp:7-29)
    int64_t m_obs_size;
    int64_t m_action_size;
    float m_action_high, m_action_low;   // PPO_MultiDiscrete only, unused (PPO_MultiDiscrete.cpp:136-144)
    float m_learning_rate;
    int64_t m_seed;
    int64_t m_total_timesteps;
    bool m_use_cuda;                      // true = run on the GPU (there is no CPU path; false is rejected at construction)
    bool m_torch_deterministic;           // accepted for config compatibility; the HIP path is deterministic by construction
    int64_t m_num_envs;
    int64_t m_num_steps;
    bool m_anneal_lr;
    bool m_use_gae;
    float m_gamma;
    float m_gae_lambda;
    int64_t m_num_minibatches;
    int64_t m_update_epochs;
    bool m_norm_adv;
    float m_clip_coef;
    bool m_clip_vloss;
    float m_ent_coef;
    float m_vf_coef;
    float m_max_grad_norm;
    int64_t m_checkpoint_updates;
    int64_t m_max_episode_steps;
    int64_t m_env_groups = 1;            // extension ([environment] env_groups): PPO_HostEnv's env groups; the device-env algorithms have no use for it
    bool m_norm_obs = false;             // extension ([environment] norm_obs): PPO_HostEnv normalises observations with running statistics (ppo_obs_norm_*)
    bool m_fused_categorical = false;    // extension ([environment] fused_categorical): PPO_HostEnv's context runs the fused categorical 2 x 64 kernels (PPO_KERNEL_CAT_FUSED); on any other class the library refuses the context
    bool m_fused_policy = false;         // extension ([environment] fused_policy): PPO_HostEnvBox's context runs the fused Gaussian 2 x 64 kernels (PPO_KERNEL_GAUSS_FUSED); on any other class the library refuses the context
    bool m_norm_reward = false;          // extension ([environment] norm_reward): PPO_HostEnv divides rewards by the running std of the discounted return (ppo_reward_norm_*)
    // norm_reward on a fused device-env class (PPO_Continuous, PPO_ContinuousMountainCar, PPO_DiscreteAcrobot, PPO_MultiDiscreteTaxi, PPO_DiscreteFrozenLake,
    // PPO_DiscreteBlackjack): the class calls normRewardOnDeviceEnv() behind getArgs(), and construct() creates the context with PPO_KERNEL_ENV_REWARD_NORM and
    // turns the normaliser on.  PPO_Discrete and PPO_MultiDiscrete never set it (CartPole and MountainCar pay rewards of unit scale), nor does PPO_HostEnv
    bool m_env_norm_reward = false;
    void normRewardOnDeviceEnv() { m_env_norm_reward = m_norm_reward; }
    // extension ([environment] keep_cut_states; the fused device-env classes PPO_Continuous, PPO_ContinuousMountainCar, PPO_DiscreteAcrobot, PPO_MultiDiscreteTaxi,
    // PPO_DiscreteFrozenLake, PPO_DiscreteBlackjack): the context is created with PPO_KERNEL_ENV_CUT_STATE -- the rollout keeps the state a time limit cut an
    // episode off in, and bootstrap_truncated is served on every one of them; on any other class the library refuses the context
    bool m_keep_cut_states = false;
    bool m_bootstrap_truncated = false;  // extension ([environment] bootstrap_truncated): bootstrap the value where a time limit cut an episode off (every algorithm class; set it with setBootstrapTruncated)
    // extension ([network] hidden_size = H; PPO_Discrete and PPO_MultiDiscrete only): the two hidden layers are H wide and the context runs on the generic engine
    // (PPO_KERNEL_ENV_GENERIC).  Absent: 64, no flag, the reference-shape kernels, nothing printed.  Depth other than 2 and bf16 storage stay with the C-ABI and
    // the Python binding: the reference's archive has names for two hidden layers only (TorchArchive.h), so a checkpoint of another depth could not be written
    int64_t m_hidden_size = 64;
    bool m_hidden_size_given = false;
    float m_target_kl = 0.0f;            // extension ([ppo] target_kl): stop an update's optimizer steps once an epoch's last approx_kl exceeds it (ppo_target_kl_set); absent or 0: off

    int64_t m_batch_size;
    int64_t m_minibatch_size;

    std::shared_ptr<ppo::Device> m_device;
    std::shared_ptr<Agent> m_agent;
    ppo_ctx* m_ctx = nullptr;             // owns parameters, AdamW state (m_optimizer in the reference), envs and rollout buffers

    // Rollout buffers: views of the context's device buffers (time-major, PPO_Discrete.cpp:90-95)
    ppo::Tensor m_obs, m_actions, m_logprobs, m_rewards, m_dones, m_values, m_action_masks;

    std::vector<float> m_clipfracs;
    ppo_stats m_last_stats{};             // the statistics snapshot train() is printing (printPPOResults reads its learning rate from here, not from
    int64_t m_epochs_total = -1;          // train() with a target KL set on the context: the epochs its updates have applied so far, the table's n_updates row; else -1
    bool m_last_stats_valid = false;      // the context, which may already be an iteration ahead); false outside train(): the context is asked
    std::unique_ptr<CircularBuffer> m_episode_stats;
    uint64_t m_global_step;
    std::shared_ptr<ThreadPool> m_threadPool;
    // called by train() with every update's statistics as printPPOResults receives them (not in the reference: for logging and tests)
    std::function<void(int64_t update, const ppo_stats&)> m_on_update;

  protected:
    // train()'s env handling: the context's device envs here; PPO_HostEnv (PPO_HostEnv.h) steps the caller's envs instead
    virtual void trainInitEnvs();         // initEnvs before the first update (:492-494)
    virtual void trainRollout();          // rollout (:524-548), advantages (:554) and the update (:567-648) of one iteration, enqueued
    PPOAlgorithm(int env_kind, int dist_kind, int64_t default_obs, int64_t default_max_episode_steps);
    void construct();                     // second half of the reference's constructor: needs the final hyper-parameters
    void setEnvTruncationBootstrap(bool on);   // the device envs' switch (ppo_env_truncation_bootstrap) and m_bootstrap_truncated with it
    ppo::Tensor initEnvsImpl();
    AgentOutput actImpl(const ppo::Tensor& obs, const ppo::Tensor* mask, const ppo::Tensor& action) const;
    ppo::Tensor bufferView(int which, std::vector<int64_t> shape, ppo::DType dt) const;
    void saveCheckpoint(const std::string& agentFile, const std::string& optimizerFile);
    int m_env_kind, m_dist_kind;
    std::string m_tag;                    // "PPO_Agent_" / file naming
};
