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
