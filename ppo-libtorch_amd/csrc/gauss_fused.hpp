// ppo-libtorch_amd/csrc/gauss_fused.hpp -- launchers of kernels_gauss_fused.hip (PPO_KERNEL_GAUSS_FUSED: Gaussian policies on a 2 x 64 f32 network)
#pragma once
#include "generic.hpp"

constexpr int GAUSS_FUSED_MAX_OBS = 64;      // the X image and W1 are sized by it (the LDS budget is at the head of kernels_gauss_fused.hip)
constexpr int GAUSS_FUSED_MAX_BLOCKS = 128;  // workgroups per net of the update kernel = partial slabs; a minibatch of more than 64 x this many rows gives a workgroup several tiles

bool gauss_fused_serves_shape(int obs, int hidden, int n_hidden, int D);
// floats between two partial slabs: the wider net's parameters (the actor's, with log_std behind them)
int64_t gauss_fused_slab_stride(const GenLayout& L);

// the rollout stores of one step (gen_gauss_store_step's): rows of step t; null: the stand-alone policy
struct GaussStepStores { const int32_t* done_prev; float* obs_t; float* act_t; float* lp_t; float* dones_t; };

// gen_forward (actor) + gen_gauss_heads (+ gen_gauss_store_step) in one launch; action / logprob / entropy may be null
hipError_t gauss_fused_act(const GenLayout& L, const float* params, const float* obs, const float* forced, int64_t n, int64_t seed, int64_t row_offset,
                           int64_t step_index, bool greedy, float* action, float* logprob, float* entropy, const GaussStepStores* st, hipStream_t s);
// the critic over n rows in one launch
hipError_t gauss_fused_values(const GenLayout& L, const float* params, const float* obs, int64_t n, float* value, hipStream_t s);
// ppo_dev_observe with truncation flags on either fused family (gauss_dev_fold_kernel): ONE launch of ceil(N / 256) workgroups finds the rows with
// truncated && done (ppo_internal.hpp: DevFoldArgs), runs gauss_fused_values' forward on those rows of final_obs [N, O] only -- v is that launch's value of
// the row, bit for bit -- and folds: rewards[t N + n] = f32(r + f32(gamma v)), (t N + n, v) into the event list, one atomicAdd per workgroup with events.
// A workgroup without a flagged row reads its 2 x 256 flags and returns; the critic's weights are staged only by workgroups that found one.
hipError_t gauss_fused_dev_fold(const GenLayout& L, const float* params, const DevFoldArgs& a, hipStream_t s);
// one minibatch step's gradient: gather through idx, forward, loss, backward (one launch, partial slabs [2][GAUSS_FUSED_MAX_BLOCKS][stride]) and the slab
// sums into grads [P] (a second launch); the five loss partials go to loss_part [GEN_LOSS_BLOCKS][8] for gen_loss_sums
hipError_t gauss_fused_fwd_bwd(const GenLayout& L, const LossParams& hp, const float* params, const float* obs, const float* actions, const float* oldlp,
                               const float* adv, const float* ret, const float* oldv, const int32_t* idx, int64_t M, double inv_global_M, double global_M,
                               const AdvStat* adv_stat, float* slab, double* loss_part, float* grads, hipStream_t s);

// PPO_KERNEL_CAT_FUSED: the same kernel family for categorical / masked multi-head policies (GenLayout with gauss = 0; A = L.act <= PPO_MAX_ACT logits in the
// place of the mean).  The critic is gauss_fused_values, the slab stride gauss_fused_slab_stride (no log_std behind the actor).
bool cat_fused_serves_shape(int obs, int hidden, int n_hidden, int A);
// the rollout stores of one step (gen_store_step's): rows of step t, every pointer at the first row of the launch; null: the stand-alone policy
struct CatStepStores { const int32_t* done_prev; float* obs_t; uint8_t* mask_t; int32_t* act_t; float* lp_t; float* dones_t; };
// gen_forward (actor) + gen_heads (+ gen_store_step) in one launch over n rows; every pointer names the first of them, row_offset is the sampler's row origin
// (env_offset + the slice's first row); mask u8 [n, A] or null, forced i64 [n, H] or null; action (i64 [n, H]) / logprob / entropy may be null
hipError_t cat_fused_act(const GenLayout& L, int dist_kind, const float* params, const float* obs, const uint8_t* mask, const int64_t* forced, int64_t n, int64_t seed,
                         int64_t row_offset, int64_t step_index, bool greedy, int64_t* action, float* logprob, float* entropy, const CatStepStores* st, hipStream_t s);
// gauss_fused_fwd_bwd for such a policy: actions i32 [B, H], masks u8 [B, A] (read for PPO_DIST_MASKED), both read in place through idx
hipError_t cat_fused_fwd_bwd(const GenLayout& L, const LossParams& hp, const float* params, const float* obs, const int32_t* actions, const uint8_t* masks,
                             const float* oldlp, const float* adv, const float* ret, const float* oldv, const int32_t* idx, int64_t M, double inv_global_M,
                             double global_M, const AdvStat* adv_stat, float* slab, double* loss_part, float* grads, hipStream_t s);

// The device envs with real-valued actions (PPO_ENV_PENDULUM, PPO_ENV_MOUNTAINCAR_CONTINUOUS; the traits are ppo_internal.hpp's GaussEnv*): the T steps of a
// rollout in one launch (gauss_rollout_kernel<Env>: one workgroup per 64 envs, the actor's weights resident, the env in wave 0's registers); the context's
// buffers, the teacher-forcing actions f32 [T, N, 1] or null.  The critic is not in it: two gauss_fused_values launches follow.
struct GaussRolloutArgs {
    const float* params;
    int N, T, max_episode_steps;
    int64_t seed, env_offset, step_base;
    float* env_state; int32_t* ep_len; float* ep_rew; int32_t* reset_count;
    float *obs, *actions, *logprobs, *rewards, *dones; int32_t* fin_len; float* fin_rew;
    float* next_obs; int32_t* next_done;
    const float* forced;
};
// by env kind: the launcher is a template over the trait like the kernel (hipErrorInvalidValue for an env without one)
hipError_t gauss_fused_rollout(int env_kind, const GenLayout& L, const GaussRolloutArgs& r, hipStream_t s);
// The envs' stand-alone kernels, one thread per env, on the rollout kernel's device functions (ppo_internal.hpp: GaussEnv*)
hipError_t launch_gauss_env_reset(int env_kind, int N, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew, int32_t* reset_count,
                                  float* next_obs, int32_t* next_done, hipStream_t s);
hipError_t launch_gauss_env_step(int env_kind, int N, int max_episode_steps, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew,
                                 int32_t* reset_count, const float* action, float* obs, float* reward, int32_t* done, hipStream_t s);
hipError_t launch_gauss_env_transition(int env_kind, const float* state_in, const float* action, int64_t n, float* next_state, float* obs_out, float* reward,
                                       int32_t* terminated, hipStream_t s);
hipError_t launch_gauss_env_obs(int env_kind, int N, const float* env_state, float* next_obs, hipStream_t s);

// ppo_env_truncation_bootstrap on a Gaussian device env whose observation is its state (PPO_ENV_MOUNTAINCAR_CONTINUOUS): ONE launch over the B = T * N stored
// samples (gauss_trunc_fold_kernel).  For every i with fin_len[i] == max_episode_steps the last transition is recomputed from obs[i] under actions[i] (f32, the
// raw action) with the env's own step; where the env terminated nothing happens, elsewhere v = Critic(final observation) -- gauss_values_kernel's forward, bit
// for bit -- is folded into rewards[i] (fold_store: two roundings) and (i, v) joins the event list.  A workgroup (256 samples) without such a row costs one
// pass over fin_len; the critic's weights are staged only by workgroups that found one.
struct GaussFoldArgs {
    const float* params;
    const float* obs;           // PPO_BUF_OBS [B, O]
    const float* actions;       // PPO_BUF_ACTIONS f32 [B, 1]
    const int32_t* fin_len;     // PPO_BUF_FIN_LEN [B]
    int64_t B;
    int max_episode_steps;      // > 0
    float gamma;
    float* rewards;             // PPO_BUF_REWARDS [B]
    int32_t* ev_count;          // the context's event list, cleared in front of the launch
    int32_t* ev_index;
    float* ev_value;
    int64_t ev_cap;
};
hipError_t gauss_fused_trunc_fold(int env_kind, const GenLayout& L, const GaussFoldArgs& a, hipStream_t s);

// ppo_evaluate on such an env: n_episodes whole episodes as ONE launch (gauss_eval_kernel: a workgroup owns 64 episodes, the actor's weights resident; episode
// e starts at reset 0 of env e under `seed`; greedy: the mean, else mu + sigma * eps keyed (seed, e, step of the episode, 0)); only the return (f32 sum in step
// order), the length and the truncated flag (the length reached max_episode_steps) leave the chip.
struct GaussEvalArgs {
    const float* params;
    int64_t n_episodes, seed;
    int max_episode_steps;      // >= 1
    int greedy;
    float* ep_return;           // [n_episodes]
    int32_t* ep_length;
    int32_t* ep_trunc;
};
hipError_t gauss_fused_evaluate(int env_kind, const GenLayout& L, const GaussEvalArgs& a, hipStream_t s);

// The device envs with integer actions (PPO_ENV_ACROBOT; the trait is ppo_internal.hpp's CatEnvAcrobot), on PPO_KERNEL_CAT_FUSED's forward: the T steps of a
// categorical rollout in one launch (cat_rollout_kernel<Env>: gauss_rollout_kernel's plan with cat_act_kernel's wave-0 work); the context's buffers, the
// teacher-forcing actions i64 [T, N, 1] or null.  PPO_BUF_MASKS is filled with ones.  The critic is not in it: two gauss_fused_values launches follow.
bool cat_fused_env_serves(int env_kind);
struct CatRolloutArgs {
    const float* params;
    int N, T, max_episode_steps;
    int64_t seed, env_offset, step_base;
    float* env_state; int32_t* ep_len; float* ep_rew; int32_t* reset_count;
    float* obs; uint8_t* masks; int32_t* actions; float *logprobs, *rewards, *dones; int32_t* fin_len; float* fin_rew;
    float* next_obs; int32_t* next_done;
    const int64_t* forced;
};
hipError_t cat_fused_rollout(int env_kind, int dist_kind, const GenLayout& L, const CatRolloutArgs& r, hipStream_t s);
// PPO_ENV_TAXI (CatEnvTaxi) is the env of this family that forms a mask (HAS_MASK): under dist_kind = PPO_DIST_MASKED a lane draws under the mask of its state
// and PPO_BUF_MASKS holds those masks; under PPO_DIST_CATEGORICAL it holds ones, as on PPO_ENV_ACROBOT.  Its observation holds its state (STATE_FROM_OBS), so
// it also has the time-limit fold (ppo_env_truncation_bootstrap): GaussFoldArgs' contract with i32 actions [B, 1], on cat_trunc_fold_kernel.
// PPO_ENV_FROZENLAKE / PPO_ENV_FROZENLAKE8X8 (CatEnvFrozenLake<4>, <8>) are the envs of this family whose step draws random numbers; the key and the count of
// the draw are words of the env state, so every entry point below serves them through the same arguments.  Their observation does not hold the state: no fold.
// PPO_ENV_BLACKJACK (CatEnvBlackjack) rides on the same mechanism with a number of draws per step that depends on the data (a hit one card, a stick the dealer's
// play-out, a reset the deal); no fold either.
bool cat_fused_env_folds(int env_kind);
struct CatFoldArgs {
    const float* params;
    const float* obs;
    const int32_t* actions;
    const int32_t* fin_len;
    int64_t B;
    int max_episode_steps;
    float gamma;
    float* rewards;
    int32_t* ev_count;
    int32_t* ev_index;
    float* ev_value;
    int64_t ev_cap;
};
hipError_t cat_fused_trunc_fold(int env_kind, const GenLayout& L, const CatFoldArgs& f, hipStream_t s);
// The env's stand-alone kernels, one thread per env, on the rollout kernel's device functions; env_state is [STATE, N]
hipError_t launch_cat_env_reset(int env_kind, int N, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew, int32_t* reset_count,
                                float* next_obs, int32_t* next_done, hipStream_t s);
hipError_t launch_cat_env_step(int env_kind, int N, int max_episode_steps, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew,
                               int32_t* reset_count, const int64_t* action, float* obs, float* reward, int32_t* done, hipStream_t s);
hipError_t launch_cat_env_transition(int env_kind, const float* state_in, const int64_t* action, int64_t n, float* next_state, float* reward, int32_t* terminated,
                                     hipStream_t s);
hipError_t launch_cat_env_obs(int env_kind, int N, const float* env_state, float* next_obs, hipStream_t s);
// ppo_evaluate on such an env: GaussEvalArgs' contract on cat_eval_kernel (greedy: the first-index argmax; else the draw keyed (seed, e, step of the episode, 0))
hipError_t cat_fused_evaluate(int env_kind, int dist_kind, const GenLayout& L, const GaussEvalArgs& a, hipStream_t s);
