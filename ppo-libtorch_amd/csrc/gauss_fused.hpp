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
// one minibatch step's gradient: gather through idx, forward, loss, backward (one launch, partial slabs [2][GAUSS_FUSED_MAX_BLOCKS][stride]) and the slab
// sums into grads [P] (a second launch); the five loss partials go to loss_part [GEN_LOSS_BLOCKS][8] for gen_loss_sums
hipError_t gauss_fused_fwd_bwd(const GenLayout& L, const LossParams& hp, const float* params, const float* obs, const float* actions, const float* oldlp,
                               const float* adv, const float* ret, const float* oldv, const int32_t* idx, int64_t M, double inv_global_M, double global_M,
                               const AdvStat* adv_stat, float* slab, double* loss_part, float* grads, hipStream_t s);

// PPO_ENV_PENDULUM: the T steps of a rollout in one launch (gauss_rollout_kernel: one workgroup per 64 envs, the actor's weights resident, the env in wave 0's
// registers); the context's buffers, the teacher-forcing actions f32 [T, N, 1] or null.  The critic is not in it: two gauss_fused_values launches follow.
struct GaussRolloutArgs {
    const float* params;
    int N, T, max_episode_steps;
    int64_t seed, env_offset, step_base;
    float* env_state; int32_t* ep_len; float* ep_rew; int32_t* reset_count;
    float *obs, *actions, *logprobs, *rewards, *dones; int32_t* fin_len; float* fin_rew;
    float* next_obs; int32_t* next_done;
    const float* forced;
};
hipError_t gauss_fused_rollout(const GenLayout& L, const GaussRolloutArgs& r, hipStream_t s);
// Pendulum's stand-alone env kernels, one thread per env, on the rollout kernel's device functions (ppo_internal.hpp: pendulum_step, pendulum_reset)
hipError_t launch_pendulum_reset(int N, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew, int32_t* reset_count, float* next_obs,
                                 int32_t* next_done, hipStream_t s);
hipError_t launch_pendulum_step(int N, int max_episode_steps, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew,
                                int32_t* reset_count, const float* action, float* obs, float* reward, int32_t* done, hipStream_t s);
hipError_t launch_pendulum_transition(const float* state_in, const float* action, int64_t n, float* next_state, float* obs_out, float* reward, int32_t* terminated,
                                      hipStream_t s);
hipError_t launch_pendulum_obs(int N, const float* env_state, float* next_obs, hipStream_t s);
