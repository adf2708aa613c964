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

// ---- The device envs of the two fused families.  An env is a trait in ppo_internal.hpp (GaussEnv*: one real-valued action; CatEnv*: one head of integer
// actions), one line of its family's dispatcher and one row of the table in kernels_gauss_fused.hip; everything the C-ABI layer knows about an env it reads
// from the row.  The numbers of a row come from the trait. ----
enum FusedFamily { FUSED_GAUSS, FUSED_CAT };   // PPO_KERNEL_GAUSS_FUSED with dist_kind PPO_DIST_GAUSSIAN / PPO_KERNEL_CAT_FUSED with a categorical one
// the words in which ppo_ctx_create's refusals differ between envs: "takes <takes>", "has <head>", "max_episode_steps ... (<steps_why>)"; and what envt_state
// says of an env without the fold ("a <no_fold>: not built for this env"; null where it folds)
struct FusedEnvTexts { const char *takes, *head, *steps_why, *no_fold; };
// ppo_env_set_state_h on an env whose state words are integers: word w is an integer in 0..hi[w] that also passes word_ok (null: no further condition), and
// `words` describes the ranges; words = null: the state is not checked
struct FusedStateCheck { const char* words; int hi[4]; bool (*word_ok)(int word, int value); };
struct FusedEnvInfo {
    int env_kind;
    const char* name;            // "PPO_ENV_..."
    FusedFamily family;
    int obs, state, actions;     // Env::OBS, Env::STATE, Env::ACTIONS (FUSED_GAUSS: the action dimension, 1)
    unsigned dist_mask;          // bit d: dist_kind d is accepted (PPO_DIST_MASKED where the env forms a mask, Env::HAS_MASK)
    bool obs_is_state;           // Env::OBS_IS_STATE: ppo_env_set_state_h copies the state into PPO_BUF_NEXT_OBS; elsewhere launch_fused_env_obs forms it
    bool folds;                  // ppo_env_truncation_bootstrap: the stored observation holds the state (fused_env_trunc_fold)
    bool evaluates;              // ppo_evaluate (fused_env_evaluate)
    int max_steps;               // the upper bound of max_episode_steps; 0: none
    FusedEnvTexts text;
    FusedStateCheck check;
};
// the row of a device env of the fused families; null for every other env_kind
const FusedEnvInfo* fused_env_info(int env_kind);
// a family's rows by name, as ppo_ctx_create's refusals of PPO_DIST_GAUSSIAN and of PPO_KERNEL_CAT_FUSED on another env list them
const char* fused_env_names(FusedFamily family);

// The T steps of a rollout in one launch (gauss_rollout_kernel<Env> / cat_rollout_kernel<Env, DIST>: one workgroup per 64 envs, the actor's weights resident,
// the env in wave 0's registers); the context's buffers.  actions / forced (teacher forcing, or null) are f32 [T, N, 1] on a FUSED_GAUSS env, i32 / i64 [T, N, 1]
// on a FUSED_CAT one; masks is read by FUSED_CAT only: PPO_BUF_MASKS holds the masks of the env's states under PPO_DIST_MASKED, ones otherwise.  The critic is
// not in it: two gauss_fused_values launches follow.
struct FusedRolloutArgs {
    const float* params;
    int N, T, max_episode_steps;
    int64_t seed, env_offset, step_base;
    float* env_state; int32_t* ep_len; float* ep_rew; int32_t* reset_count;   // env_state is [STATE, N]
    float* obs; uint8_t* masks; void* actions; float *logprobs, *rewards, *dones; int32_t* fin_len; float* fin_rew;
    float* next_obs; int32_t* next_done;
    const void* forced;
    float* cut;   // a context with PPO_KERNEL_ENV_CUT_STATE: the cut-off record, f32 [STATE + 1, T * N] (the KEEP instantiation writes column t * N + env where
                  // that step's episode reached the limit: the pre-reset state, then 0.0f / 1.0f "the env itself terminated"); null: today's kernel
};
// by env kind: the launchers are templates over the trait like the kernels (hipErrorInvalidValue for an env without a row, or without the call)
hipError_t launch_fused_env_rollout(int env_kind, int dist_kind, const GenLayout& L, const FusedRolloutArgs& r, hipStream_t s);

// ppo_env_truncation_bootstrap on an env that folds: ONE launch over the B = T * N stored samples (gauss_trunc_fold_kernel / cat_trunc_fold_kernel).  For every
// i with fin_len[i] == max_episode_steps the last transition is recomputed from obs[i] (the state, or its one-hot groups decoded) under actions[i] with the env's
// own step; where the env terminated nothing happens, elsewhere v = Critic(final observation) -- gauss_values_kernel's forward, bit for bit -- is folded into
// rewards[i] (fold_store: two roundings) and (i, v) joins the event list.  A workgroup (256 samples) without such a row costs one pass over fin_len; the
// critic's weights are staged only by workgroups that found one.
struct FusedFoldArgs {
    const float* params;
    const float* obs;           // PPO_BUF_OBS [B, O]
    const void* actions;        // PPO_BUF_ACTIONS [B, 1]: f32, the raw action (FUSED_GAUSS) / i32 (FUSED_CAT)
    const int32_t* fin_len;     // PPO_BUF_FIN_LEN [B]
    int64_t B;
    int max_episode_steps;      // > 0
    float gamma;
    float* rewards;             // PPO_BUF_REWARDS [B]
    int32_t* ev_count;          // the context's event list, cleared in front of the launch
    int32_t* ev_index;
    float* ev_value;
    int64_t ev_cap;
    const float* cut;           // the cut-off record of a PPO_KERNEL_ENV_CUT_STATE context: EVERY fused env folds from it (cut_state_fold_kernel reads the final
                                // state there, forms Env::obs of it and replays nothing; obs and actions are not read); null: the two kernels above
};
hipError_t fused_env_trunc_fold(int env_kind, const GenLayout& L, const FusedFoldArgs& f, hipStream_t s);

// ppo_evaluate on an env that evaluates: n_episodes whole episodes as ONE launch (gauss_eval_kernel / cat_eval_kernel: a workgroup owns 64 episodes, the actor's
// weights resident; episode e starts at reset 0 of env e under `seed`; greedy: the mean / the first-index argmax, else the draw keyed (seed, e, step of the
// episode, 0)); only the return (f32 sum in step order), the length and the truncated flag (the length reached max_episode_steps) leave the chip.
struct FusedEvalArgs {
    const float* params;
    int64_t n_episodes, seed;
    int max_episode_steps;      // >= 1
    int greedy;
    float* ep_return;           // [n_episodes]
    int32_t* ep_length;
    int32_t* ep_trunc;
};
hipError_t fused_env_evaluate(int env_kind, int dist_kind, const GenLayout& L, const FusedEvalArgs& e, hipStream_t s);

// The envs' stand-alone kernels, one thread per env, on the rollout kernel's device functions.  The step and the transition take the family's action type, as
// the C ABI does (ppo_env_step / ppo_env_step_f32): each serves the envs of its family only.
hipError_t launch_fused_env_reset(int env_kind, int N, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew, int32_t* reset_count,
                                  float* next_obs, int32_t* next_done, hipStream_t s);
hipError_t launch_fused_env_obs(int env_kind, int N, const float* env_state, float* next_obs, hipStream_t s);
hipError_t launch_gauss_env_step(int env_kind, int N, int max_episode_steps, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew,
                                 int32_t* reset_count, const float* action, float* obs, float* reward, int32_t* done, hipStream_t s);
hipError_t launch_cat_env_step(int env_kind, int N, int max_episode_steps, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew,
                               int32_t* reset_count, const int64_t* action, float* obs, float* reward, int32_t* done, hipStream_t s);
hipError_t launch_gauss_env_transition(int env_kind, const float* state_in, const float* action, int64_t n, float* next_state, float* obs_out, float* reward,
                                       int32_t* terminated, hipStream_t s);
hipError_t launch_cat_env_transition(int env_kind, const float* state_in, const int64_t* action, int64_t n, float* next_state, float* reward, int32_t* terminated,
                                     hipStream_t s);
