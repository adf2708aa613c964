// ppo-libtorch_amd/csrc/kernels_gauss_fused.hip -- diagonal-Gaussian policies on a 2 x 64 f32 network (PPO_KERNEL_GAUSS_FUSED): the env step, the critic
// batch and the minibatch step as ONE launch each, in the place of the generic engine's per-layer products (kernels_gemm.hip pads every 64-wide product to
// 128-wide tiles and takes a launch per layer and direction).
//
// One workgroup = 4 waves = one 64-sample tile at a time.  The net's weights are resident in LDS for the whole launch, activations are [unit][sample] images of
// stride PPO_LDS_STRIDE (the model is fwd_bwd_body, kernels_update.hip); obs_size is a run-time value, padded with zeros to a multiple of 4 in LDS.  All three
// kernels go through gf_forward_tile, so an observation gets the same mean and the same value from every entry point, bit for bit: plain f32, every product an
// explicit fmaf in ascending k, bias first.  No reduced-precision operand anywhere.
//
// LDS (floats; obsP = obs rounded up to 4, outP = the output width rounded up to 4; the update kernel carves for the wider net, the actor):
//   W1 64 obsP | W2 4096 | W3 64 outP | b1 64 | b2 64 | b3 32 | log_std 32 | exp(-log_std) 32 | row index 64 | X obsP 68 | H1 64 68 | H2 64 68 | OUT outP 68
//   obs 64, D 32 (the largest shape served): 4096 + 4096 + 2048 + 288 + 4352 + 4352 + 4352 + 2176 = 25 760 floats = 103 040 bytes of 163 840.
//   obs 17, D 6: 1280 + 4096 + 512 + 288 + 1360 + 4352 + 4352 + 544 = 16 784 floats = 67 136 bytes: two workgroups per CU.
//   obs 3, D 1 (PPO_ENV_PENDULUM): 256 + 4096 + 256 + 288 + 272 + 4352 + 4352 + 272 = 14 144 floats = 56 576 bytes: two workgroups per CU.
//   obs 2, D 1 (PPO_ENV_MOUNTAINCAR_CONTINUOUS): the same carve, gf_carve(4, 4); rows 2 and 3 of the X image are zero padding.
//
// PPO_KERNEL_CAT_FUSED: the same family for categorical / masked multi-head policies of a caller-stepped context (the actor's output = up to 32 logits): the
// family depends on the distribution in two places only, what wave 0 does with the output tile in the act kernel (cat_act_kernel) and what the actor's
// loss lane does in the update kernel (cat_fwd_bwd_kernel = gf_fwd_bwd_body<DIST>, the body gauss_fwd_bwd_kernel instantiates for the Gaussian); the critic
// kernel is shared.  obs 17, 12 logits: 1280 + 4096 + 768 + 288 + 1360 + 4352 + 4352 + 816 = 17 312 floats = 69 248 bytes.
//
// The device envs with real-valued actions (ppo_internal.hpp: GaussEnvPendulum, GaussEnvMountainCarContinuous) add kernels on the same forward, each a
// template over the env trait: gauss_rollout_kernel, the T steps of a rollout in one launch with the env in registers (below); the envs' small stand-alone
// kernels; and, for an env whose observation is its state, gauss_trunc_fold_kernel (ppo_env_truncation_bootstrap) and gauss_eval_kernel (ppo_evaluate).
//
// The device env with integer actions (ppo_internal.hpp: CatEnvAcrobot, PPO_ENV_ACROBOT) adds the categorical twins on the same forward: cat_rollout_kernel
// (gauss_rollout_kernel's plan with cat_act_kernel's wave-0 work; obs 6, 3 logits: gf_carve(8, 4) = 14 672 floats = 58 688 bytes, two workgroups per CU), its
// stand-alone env kernels and cat_eval_kernel (ppo_evaluate); the lanes keep the env's STATE, so the observation need not be the state.
// PPO_ENV_TAXI (CatEnvTaxi) instantiates the same kernels for an env whose mask means something (HAS_MASK: under PPO_DIST_MASKED a lane forms the mask of its
// state, draws under it, and waves 1 .. 3 store it), whose observation is 19 wide (OBS_ONE_HOT: the lane moves four ones in the X image; gf_carve(20, 8) =
// 16 784 floats = 67 136 bytes, above 64 KB: the attribute is asked for, two workgroups per CU still fit in 160 KB -- arithmetic, not a measurement) and holds
// the state (STATE_FROM_OBS: cat_trunc_fold_kernel, the time-limit fold).  The traits are compile-time: the Acrobot instantiations are what they were.
// PPO_ENV_FROZENLAKE / PPO_ENV_FROZENLAKE8X8 (CatEnvFrozenLake<4>, <8>) instantiate them for an env whose step draws random numbers.  No trait says so: the key
// and the step count of the draw are state words (ppo_internal.hpp), so Env::step(st, a) is as pure here as Taxi's and the kernels did not change for it.  What
// did is the observation width, 16 and 64: gf_carve(16, 4) = 15 728 floats = 62 912 bytes, two workgroups per CU; gf_carve(64, 4) = 22 064 floats =
// 88 256 bytes, above 64 KB (the attribute is asked for) and ONE workgroup per CU of 160 KB -- arithmetic, not a measurement.
// PPO_ENV_BLACKJACK (CatEnvBlackjack) instantiates them for an env whose step draws a NUMBER of cards that depends on the data: a hit one, a stick the dealer's
// play-out of up to ten, a reset four.  Again no trait says so and the kernels did not change: the draws are inside Env::step / Env::reset, keyed by state
// words, and the dealer's loop has a compile-time bound.  gf_carve(48, 4) = 19 952 floats = 79 808 bytes: the attribute, and two workgroups per CU still fit.
//
// Caller-stepped contexts of either family fold time-limit truncations per step in gauss_dev_fold_kernel (ppo_dev_observe with flags): the critic kernel's
// forward on the flagged rows of the step, found on the device.
#include <algorithm>

#include "generic.hpp"
#include "gauss_dist.hpp"
#include "gauss_fused.hpp"

namespace {

constexpr int GF_THREADS = 256;
constexpr int GF_S = PPO_LDS_STRIDE;

// what the kernels need of GenLayout: offsets (floats, into the flat parameter vector) of {W1, b1, W2, b2, W3, b3} per net, log_std behind the actor
struct GfShape {
    int obs, D;              // D: the Gaussian action width; 0 for a categorical policy (no log_std is read then)
    int A;                   // the actor's output width: D, or the sum of the categorical heads' widths
    int n_heads;
    int head_dims[PPO_MAX_HEADS];
    int off[2][6];
    int logstd_off;
};

GfShape gf_shape(const GenLayout& L) {
    GfShape sh{};
    sh.obs = L.obs; sh.D = L.gauss; sh.A = L.act; sh.n_heads = L.n_heads;
    for (int h = 0; h < L.n_heads; h++) sh.head_dims[h] = L.head_dims[h];
    for (int net = 0; net < 2; net++)
        for (int l = 0; l < 3; l++) { sh.off[net][2 * l] = L.w_off[net][l]; sh.off[net][2 * l + 1] = L.b_off[net][l]; }
    sh.logstd_off = L.logstd_off;
    return sh;
}

struct GfLds {
    float *w1, *w2, *w3, *b1, *b2, *b3, *ls, *inv;
    int* ridx;
    float *x, *h1, *h2, *o;
    int obsP, outP;
};

__host__ __device__ inline int gf_pad4(int v) { return (v + 3) & ~3; }
__host__ __device__ inline int gf_lds_floats(int obsP, int outP) { return 64 * obsP + 4096 + 64 * outP + 64 + 64 + 32 + 32 + 32 + 64 + obsP * GF_S + 64 * GF_S + 64 * GF_S + outP * GF_S; }

__device__ __forceinline__ GfLds gf_carve(float* base, int obsP, int outP) {
    GfLds m;
    m.obsP = obsP; m.outP = outP;
    float* p = base;
    m.w1 = p; p += 64 * obsP;
    m.w2 = p; p += 4096;
    m.w3 = p; p += 64 * outP;
    m.b1 = p; p += 64;
    m.b2 = p; p += 64;
    m.b3 = p; p += 32;
    m.ls = p; p += 32;
    m.inv = p; p += 32;
    m.ridx = reinterpret_cast<int*>(p); p += 64;
    m.x = p; p += obsP * GF_S;
    m.h1 = p; p += 64 * GF_S;
    m.h2 = p; p += 64 * GF_S;
    m.o = p;
    return m;
}

// one net's weights into LDS (zero padded), log_std and exp(-log_std); every thread of the workgroup calls it; the caller's next barrier publishes it
__device__ __forceinline__ void gf_stage_weights(const GfLds& m, const GfShape& sh, const float* __restrict__ params, int net, int tid) {
    const int obs = sh.obs, obsP = m.obsP, out = net == 0 ? 1 : sh.A;
    const float* W1 = params + sh.off[net][0];
    const float* W2 = params + sh.off[net][2];
    const float* W3 = params + sh.off[net][4];
    for (int i = tid; i < 64 * obsP; i += GF_THREADS) {
        const int u = i / obsP, k = i - u * obsP;
        m.w1[i] = k < obs ? W1[u * obs + k] : 0.0f;
    }
    for (int i = tid; i < 4096; i += GF_THREADS) m.w2[i] = W2[i];
    for (int i = tid; i < 64 * m.outP; i += GF_THREADS) m.w3[i] = (i >> 6) < out ? W3[i] : 0.0f;
    if (tid < 64) { m.b1[tid] = params[sh.off[net][1] + tid]; m.b2[tid] = params[sh.off[net][3] + tid]; }
    if (tid < 32) {
        m.b3[tid] = tid < out ? params[sh.off[net][5] + tid] : 0.0f;
        const float ls = tid < sh.D ? params[sh.logstd_off + tid] : 0.0f;
        m.ls[tid] = ls;
        m.inv[tid] = expf(-ls);
    }
}

// the tile's observations as the [k][sample] image: row m.ridx[s] of obs [., O], zeros for a sample without a row (ridx < 0) and for k >= O
__device__ __forceinline__ void gf_load_x(const GfLds& m, const float* __restrict__ obs, int O, int tid) {
    const int obsP = m.obsP;
    for (int i = tid; i < 64 * obsP; i += GF_THREADS) {
        const int s = i / obsP, k = i - s * obsP;
        const int r = m.ridx[s];
        m.x[k * GF_S + s] = (k < O && r >= 0) ? obs[(int64_t)r * O + k] : 0.0f;
    }
}

// a hidden layer: out[u][s] = tanh(b[u] + sum_k W[u][k] in[k][s]), k ascending; lane = sample, wave w owns units 16 w .. 16 w + 15; K a multiple of 4
__device__ __forceinline__ void gf_hidden_layer(const float* __restrict__ W, const float* __restrict__ b, const float* __restrict__ in, float* __restrict__ out, int K,
                                                int s, int w) {
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = b[16 * w + i];
    for (int k = 0; k < K; k += 4) {
        const float x0 = in[(k + 0) * GF_S + s], x1 = in[(k + 1) * GF_S + s], x2 = in[(k + 2) * GF_S + s], x3 = in[(k + 3) * GF_S + s];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const float4 wv = *reinterpret_cast<const float4*>(&W[(16 * w + i) * K + k]);
            acc[i] = __builtin_fmaf(wv.x, x0, acc[i]);
            acc[i] = __builtin_fmaf(wv.y, x1, acc[i]);
            acc[i] = __builtin_fmaf(wv.z, x2, acc[i]);
            acc[i] = __builtin_fmaf(wv.w, x3, acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[(16 * w + i) * GF_S + s] = tanh_fast(acc[i]);
}

// THE forward pass of all three kernels: the tile in m.x through obs -> 64 -> 64 -> out; leaves H1, H2 (post-tanh) and OUT rows 0 .. out - 1.
// Every thread of the workgroup calls it; barriers: one at entry (m.x and the weights are complete), one behind every layer.
__device__ __forceinline__ void gf_forward_tile(const GfLds& m, int out, int tid) {
    const int s = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    __syncthreads();
    gf_hidden_layer(m.w1, m.b1, m.x, m.h1, m.obsP, s, w);
    __syncthreads();
    gf_hidden_layer(m.w2, m.b2, m.h1, m.h2, 64, s, w);
    __syncthreads();
    {   // output layer: wave w owns units w, w + 4, ... (< out <= 32)
        const int nu = (out - w + 3) >> 2;
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; i++) acc[i] = m.b3[(4 * i + w) & 31];
        for (int k = 0; k < 64; k += 4) {
            const float x0 = m.h2[(k + 0) * GF_S + s], x1 = m.h2[(k + 1) * GF_S + s], x2 = m.h2[(k + 2) * GF_S + s], x3 = m.h2[(k + 3) * GF_S + s];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                if (i < nu) {
                    const float4 wv = *reinterpret_cast<const float4*>(&m.w3[(4 * i + w) * 64 + k]);
                    acc[i] = __builtin_fmaf(wv.x, x0, acc[i]);
                    acc[i] = __builtin_fmaf(wv.y, x1, acc[i]);
                    acc[i] = __builtin_fmaf(wv.z, x2, acc[i]);
                    acc[i] = __builtin_fmaf(wv.w, x3, acc[i]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++) if (i < nu) m.o[(4 * i + w) * GF_S + s] = acc[i];
    }
    __syncthreads();
}

// rows row0 .. row0 + 63 of a dense batch of n
__device__ __forceinline__ void gf_dense_rows(const GfLds& m, int64_t row0, int64_t n, int tid) {
    if (tid < 64) m.ridx[tid] = row0 + tid < n ? (int)(row0 + tid) : -1;
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------
// gauss_act_kernel: actor forward + gauss_heads_kernel's sample / log-prob / entropy (the same device functions, gauss_dist.hpp) + the rollout stores of
// the step (gauss_store_step_kernel's; st.obs_t == nullptr: the stand-alone policy, none)
// ---------------------------------------------------------------------------------------------------------
struct GfStepStores { const int32_t* done_prev; float* obs_t; float* act_t; float* lp_t; float* dones_t; };

template <bool GREEDY>
__global__ __launch_bounds__(GF_THREADS) void gauss_act_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs,
                                                               const float* __restrict__ forced, int64_t n, int64_t seed, int64_t row_offset, int64_t step_index,
                                                               float* action, float* logprob, float* entropy, GfStepStores st) {
    extern __shared__ __attribute__((aligned(16))) float gf_lds[];
    const int tid = threadIdx.x, D = sh.D, O = sh.obs;
    const GfLds m = gf_carve(gf_lds, gf_pad4(O), gf_pad4(D));
    gf_stage_weights(m, sh, params, 1, tid);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(m, row0, n, tid);
        gf_load_x(m, obs, O, tid);
        gf_forward_tile(m, D, tid);
        const int64_t r = row0 + (tid & 63);
        if (tid < 64) {
            if (r < n) {
                double lp = 0.0, en = 0.0;
                for (int k4 = 0; k4 < D; k4 += 4) {
                    float eps[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                    if (!GREEDY && !forced) gauss_eps4(seed, row_offset + r, step_index, k4, eps);
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int k = k4 + j;
                        if (k < D) {
                            const float mu = m.o[k * GF_S + tid], ls = m.ls[k];
                            float a;
                            if (GREEDY) a = mu;
                            else if (forced) a = forced[r * D + k];
                            else a = gauss_sample(mu, ls, eps[j]);
                            if (action) action[r * D + k] = a;
                            if (st.act_t) st.act_t[r * D + k] = a;
                            lp += gauss_logp(gauss_z(a, mu, expf(-ls)), ls);
                            en += gauss_entropy(ls);
                        }
                    }
                }
                if (logprob) logprob[r] = (float)lp;
                if (st.lp_t) st.lp_t[r] = (float)lp;
                if (entropy) entropy[r] = (float)en;
            }
        } else if (st.obs_t) {   // waves 1 .. 3: the step's other stores
            const int64_t rows = n - row0 < 64 ? n - row0 : 64;
            for (int64_t i = tid - 64; i < rows * O; i += GF_THREADS - 64) st.obs_t[row0 * O + i] = obs[row0 * O + i];
            if (tid < 128 && r < n) st.dones_t[r] = (float)st.done_prev[r];
        }
        __syncthreads();   // OUT and the row list are read: the next tile may overwrite them
    }
}

// gauss_values_kernel: the critic over n rows
__global__ __launch_bounds__(GF_THREADS) void gauss_values_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs, int64_t n,
                                                                  float* __restrict__ value) {
    extern __shared__ __attribute__((aligned(16))) float gf_lds[];
    const int tid = threadIdx.x, O = sh.obs;
    const GfLds m = gf_carve(gf_lds, gf_pad4(O), 4);
    gf_stage_weights(m, sh, params, 0, tid);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(m, row0, n, tid);
        gf_load_x(m, obs, O, tid);
        gf_forward_tile(m, 1, tid);
        if (tid < 64 && row0 + tid < n) value[row0 + tid] = m.o[tid];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------
// cat_act_kernel (PPO_KERNEL_CAT_FUSED): gauss_act_kernel's plan for a categorical / masked multi-head policy.  The forward leaves the logits [A][sample] in
// OUT; wave 0, lane = row, then does what heads_kernel (kernels_generic.hip) does with a row of logits, on the same device functions (categorical_head,
// sample_head, the same Philox keying), so equal logits give equal action, log-prob and entropy bits.  The row's logits stay where they are: z is the lane's
// column of OUT (log-probs in place), p the lane's column of the H1 image, which nobody reads behind the forward's last barrier -- run-time head offsets index
// LDS, no per-lane array exists.  Waves 1 .. 3 do the step's other stores meanwhile (store_step_kernel's: OBS[t], MASKS[t] -- all ones without a mask --
// and DONES[t] from the previous done flags).  Every pointer names the first of the launch's n rows (an env group's slice: row_offset carries its origin).
// ---------------------------------------------------------------------------------------------------------
struct CfStepStores { const int32_t* done_prev; float* obs_t; uint8_t* mask_t; int32_t* act_t; float* lp_t; float* dones_t; };

template <int DIST, bool GREEDY>
__global__ __launch_bounds__(GF_THREADS) void cat_act_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs,
                                                             const uint8_t* __restrict__ mask, const int64_t* __restrict__ forced, int64_t n, int64_t seed,
                                                             int64_t row_offset, int64_t step_index, int64_t* action, float* logprob, float* entropy, CfStepStores st) {
    extern __shared__ __attribute__((aligned(16))) float gf_lds[];
    const int tid = threadIdx.x, A = sh.A, O = sh.obs, H = sh.n_heads;
    const GfLds m = gf_carve(gf_lds, gf_pad4(O), gf_pad4(A));
    gf_stage_weights(m, sh, params, 1, tid);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(m, row0, n, tid);
        gf_load_x(m, obs, O, tid);
        gf_forward_tile(m, A, tid);
        const int64_t r = row0 + (tid & 63);
        if (tid < 64) {
            if (r < n) {
                float lp_sum = 0.0f, en_sum = 0.0f;
                int off = 0;
                for (int h = 0; h < H; h++) {
                    const int Ah = sh.head_dims[h];
                    float* z = m.o + off * GF_S + tid;
                    float* p = m.h1 + off * GF_S + tid;
                    const uint8_t* mrow = (DIST == PPO_DIST_MASKED && mask) ? mask + r * A + off : nullptr;
                    const float en = categorical_head<DIST, GF_S>(z, p, mrow, Ah);
                    int a;
                    if constexpr (GREEDY) {
                        a = 0;
                        for (int k = 1; k < Ah; k++) if (p[k * GF_S] > p[a * GF_S]) a = k;
                    } else if (forced) {
                        a = (int)forced[r * H + h];
                    } else {
                        const uint4 w = philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)(row_offset + r), (uint32_t)(step_index >> 2), (uint32_t)h, 0u);
                        const uint32_t ws = (step_index & 3) == 0 ? w.x : ((step_index & 3) == 1 ? w.y : ((step_index & 3) == 2 ? w.z : w.w));
                        a = sample_head<GF_S>(p, Ah, (float)(ws >> 8) * 0x1p-24f);
                    }
                    if (action) action[r * H + h] = a;
                    if (st.act_t) st.act_t[r * H + h] = a;
                    float lp = 0.0f;
                    for (int k = 0; k < Ah; k++) if (k == a) lp = z[k * GF_S];
                    if (h == 0) { lp_sum = lp; en_sum = en; } else { lp_sum += lp; en_sum += en; }   // stack(...).sum(0), Agent.cpp:165-168
                    off += Ah;
                }
                if (logprob) logprob[r] = lp_sum;
                if (st.lp_t) st.lp_t[r] = lp_sum;
                if (entropy) entropy[r] = en_sum;
            }
        } else if (st.obs_t) {   // waves 1 .. 3: the step's other stores
            const int64_t rows = n - row0 < 64 ? n - row0 : 64;
            for (int64_t i = tid - 64; i < rows * O; i += GF_THREADS - 64) st.obs_t[row0 * O + i] = obs[row0 * O + i];
            for (int64_t i = tid - 64; i < rows * A; i += GF_THREADS - 64) st.mask_t[row0 * A + i] = mask ? mask[row0 * A + i] : (uint8_t)1;
            if (tid < 128 && r < n) st.dones_t[r] = (float)st.done_prev[r];
        }
        __syncthreads();   // OUT, the H1 columns and the row list are read: the next tile may overwrite them
    }
}

// ---------------------------------------------------------------------------------------------------------
// gauss_fwd_bwd_kernel: one minibatch step of one net per workgroup column (blockIdx.y = net): gather through the index list, forward, PPO loss
// (gauss_loss_kernel's arithmetic), backward.  Gradients accumulate in registers over the workgroup's tiles and leave as one partial slab.
// ---------------------------------------------------------------------------------------------------------
struct GfUpdArgs {
    GfShape sh;
    LossParams hp;
    const float* params;
    const float* obs;        // [B, O] and the other flattened rollout buffers, read in place through idx
    const float* actions;    // [B, D]; a categorical policy: the i32 actions [B, H] behind the same pointer
    const uint8_t* masks;    // [B, A] (PPO_DIST_MASKED), else null
    const float* oldlp;
    const float* adv;
    const float* ret;
    const float* oldv;
    const int32_t* idx;      // [M]
    int M;
    float invM;              // 1 / rows of the global minibatch
    const AdvStat* adv_stat; // PPO_ADV_PARTS partial sums, or null (norm_adv off)
    double global_M;
    float* slab;             // [2][nb][slab_stride]
    int slab_stride, nb;
    double* loss_part;       // [GEN_LOSS_BLOCKS][8]
};

// dW[4 ub + i][4 kb + j] += sum_s dz[4 ub + i][s] in[4 kb + j][s], db[4 ub + i] += sum_s dz[4 ub + i][s]: the tile's sum from zero in ascending s, then
// added to the running sum (the workgroup's tiles in order)
__device__ __forceinline__ void gf_dw_tile(const float* __restrict__ dz, const float* __restrict__ in, int ub, int kb, float* acc, float* accb) {
    float t[16], tb[4];
#pragma unroll
    for (int i = 0; i < 16; i++) t[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) tb[i] = 0.0f;
    for (int s4 = 0; s4 < 64; s4 += 4) {
        float4 d[4], h[4];
#pragma unroll
        for (int i = 0; i < 4; i++) d[i] = *reinterpret_cast<const float4*>(&dz[(4 * ub + i) * GF_S + s4]);
#pragma unroll
        for (int j = 0; j < 4; j++) h[j] = *reinterpret_cast<const float4*>(&in[(4 * kb + j) * GF_S + s4]);
#pragma unroll
        for (int i = 0; i < 4; i++) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float v = t[i * 4 + j];
                v = __builtin_fmaf(d[i].x, h[j].x, v);
                v = __builtin_fmaf(d[i].y, h[j].y, v);
                v = __builtin_fmaf(d[i].z, h[j].z, v);
                v = __builtin_fmaf(d[i].w, h[j].w, v);
                t[i * 4 + j] = v;
            }
            tb[i] = (((tb[i] + d[i].x) + d[i].y) + d[i].z) + d[i].w;
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] += t[i];
#pragma unroll
    for (int i = 0; i < 4; i++) accb[i] += tb[i];
}

// h[k][s] <- (sum_o W[o][k] dout[o][s]) (1 - h[k][s]^2), o ascending below n_out: d(pre-activation) of the layer under `dout`, in the activation's place.
// lane = sample, wave w owns k = 16 w .. 16 w + 15; a thread reads and writes only its own elements of h
__device__ __forceinline__ void gf_dz_tile(const float* __restrict__ dout, int n_out, const float* __restrict__ W, float* h, int s, int w) {
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.0f;
    for (int o = 0; o < n_out; o++) {
        const float d = dout[o * GF_S + s];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float4 wv = *reinterpret_cast<const float4*>(&W[o * 64 + 16 * w + 4 * q]);
            acc[4 * q + 0] = __builtin_fmaf(wv.x, d, acc[4 * q + 0]);
            acc[4 * q + 1] = __builtin_fmaf(wv.y, d, acc[4 * q + 1]);
            acc[4 * q + 2] = __builtin_fmaf(wv.z, d, acc[4 * q + 2]);
            acc[4 * q + 3] = __builtin_fmaf(wv.w, d, acc[4 * q + 3]);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const float a = h[(16 * w + i) * GF_S + s];
        h[(16 * w + i) * GF_S + s] = acc[i] * (1.0f - a * a);
    }
}

constexpr int AM = PPO_MAX_ACT;

// The actor's loss lane of a categorical policy (cat_fwd_bwd_kernel): loss_kernel's arithmetic (kernels_generic.hip) on one row, whose logits arrive in z.
// Every array is indexed by an unrolled k: a logit takes part in head h's pass when off <= k < off + head_dims[h], a wave-uniform predicate, so the arrays
// stay in registers.  Leaves p = m_probs and q[k] = -p_k (log p_k + H_head(k)), the entropy's derivative (PPO_DIST_MASKED); `valid` = the mask bits (all
// ones without a mask); returns the summed log-prob of the stored actions and the summed entropy.
template <int DIST>
__device__ __forceinline__ float cat_row_heads(const GfShape& sh, float (&z)[PPO_MAX_ACT], float (&p)[PPO_MAX_ACT], float (&q)[PPO_MAX_ACT], uint32_t valid,
                                               const int32_t* __restrict__ act_row, uint32_t& chosen, float& ent_out) {
    float nlp = 0.0f, ent = 0.0f;
    int off = 0;
    chosen = 0u;
    for (int h = 0; h < sh.n_heads; h++) {
        const int Ah = sh.head_dims[h], end = off + Ah;
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < PPO_MAX_ACT; k++) {
            if (k >= off && k < end) {
                if (DIST == PPO_DIST_MASKED && !((valid >> k) & 1u)) z[k] = -1e8f;
                mx = z[k] > mx ? z[k] : mx;
            }
        }
        float se = 0.0f;
#pragma unroll
        for (int k = 0; k < PPO_MAX_ACT; k++) if (k >= off && k < end) { p[k] = expf(z[k] - mx); se += p[k]; }
        const float lse = logf(se) + mx;
        float e = 0.0f;
#pragma unroll
        for (int k = 0; k < PPO_MAX_ACT; k++) {
            if (k >= off && k < end) {
                z[k] = z[k] - lse;
                p[k] = p[k] / se;
                if (DIST == PPO_DIST_CATEGORICAL) {
                    const float l = z[k] > 1.17549435e-38f ? z[k] : 1.17549435e-38f;   // torch::clamp(m_logits, FLT_MIN), Categorical.cpp:115
                    e += l * p[k];
                } else {
                    const float plp = z[k] * p[k];
                    e += ((valid >> k) & 1u) ? plp : 0.0f;
                }
            }
        }
        const float headH = -e;
        const int a = off + act_row[h];
        float lp = 0.0f;
#pragma unroll
        for (int k = 0; k < PPO_MAX_ACT; k++) {
            if (k >= off && k < end) {
                if (k == a) { lp = z[k]; chosen |= 1u << k; }
                q[k] = -p[k] * (z[k] + headH);
            }
        }
        if (h == 0) { nlp = lp; ent = headH; } else { nlp += lp; ent += headH; }
        off = end;
    }
    ent_out = ent;
    return nlp;
}

// DIST: PPO_DIST_GAUSSIAN (gauss_fwd_bwd_kernel) or PPO_DIST_CATEGORICAL / PPO_DIST_MASKED (cat_fwd_bwd_kernel); only the actor's loss lane and the
// log_std gradient depend on it
template <int DIST>
__device__ __forceinline__ void gf_fwd_bwd_body(const GfUpdArgs& a, float* gf_lds) {
    constexpr bool GAUSS = DIST == PPO_DIST_GAUSSIAN;
    const int tid = threadIdx.x, D = a.sh.D, O = a.sh.obs;
    const int net = blockIdx.y, b = blockIdx.x, nb = a.nb;
    const int out = net == 0 ? 1 : a.sh.A, outP = gf_pad4(out);
    const GfLds m = gf_carve(gf_lds, gf_pad4(O), gf_pad4(a.sh.A));
    const int obsP = m.obsP;
    gf_stage_weights(m, a.sh, a.params, net, tid);
    const int s = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ub = tid >> 4, kb = tid & 15;
    const LossParams hp = a.hp;
    const float invM = a.invM;

    float gW1[16], gW2[16], gW3[16], gb1[4], gb2[4], gb3[4];
#pragma unroll
    for (int i = 0; i < 16; i++) gW1[i] = gW2[i] = gW3[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) gb1[i] = gb2[i] = gb3[i] = 0.0f;
    float dls[AM];
#pragma unroll
    for (int k = 0; k < AM; k++) dls[k] = 0.0f;
    double sums[5] = { 0, 0, 0, 0, 0 };

    // mean and 1 / (Bessel std + 1e-8) of the (global) minibatch's advantages from the PPO_ADV_PARTS partial sums: gauss_loss_kernel's arithmetic
    float mean_f = 0.0f, std_f = 0.0f;
    if (a.adv_stat && net == 1 && w == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int i = 0; i < PPO_ADV_PARTS; i++) { t1 += a.adv_stat[i].s1; t2 += a.adv_stat[i].s2; }
        const double mean_a = t1 / a.global_M;
        const double var = (t2 - t1 * mean_a) / (a.global_M - 1.0);
        mean_f = (float)mean_a;
        std_f = (float)sqrt(var < 0.0 ? 0.0 : var);
    }
    const float inv_std = 1.0f / (std_f + 1e-8f);
    const float clip = hp.clip_coef, lo = 1 - clip, hi_c = 1 + clip;

    const int tiles = (a.M + 63) / 64;
    for (int tile = b; tile < tiles; tile += nb) {
        if (tid < 64) m.ridx[tid] = tile * 64 + tid < a.M ? a.idx[tile * 64 + tid] : -1;
        __syncthreads();
        gf_load_x(m, a.obs, O, tid);
        gf_forward_tile(m, out, tid);
        // ---- loss: wave 0, lane = sample; d(loss)/d(output) replaces the output in OUT (zero for a sample without a row and for rows out .. outP - 1) ----
        if (w == 0) {
            const int r = m.ridx[s];
            if (net == 1 && !GAUSS) {
                // categorical heads: new log-prob and entropy from the row's logits, its stored actions and (masked) its mask row; d(loss)/d(logits) -> OUT
                float z[AM], p[AM], q[AM];
                float g_nlp = 0.0f, g_ent = 0.0f;
                uint32_t valid = 0xffffffffu, chosen = 0u;
                if (r >= 0) {
#pragma unroll
                    for (int k = 0; k < AM; k++) z[k] = k < out ? m.o[k * GF_S + s] : 0.0f;
                    if (DIST == PPO_DIST_MASKED && a.masks) {
                        const uint8_t* mrow = a.masks + (int64_t)r * out;
#pragma unroll
                        for (int k = 0; k < AM; k++) if (k < out && mrow[k] == 0) valid &= ~(1u << k);
                    }
                    float ent;
                    const float nlp = cat_row_heads<DIST>(a.sh, z, p, q, valid, reinterpret_cast<const int32_t*>(a.actions) + (int64_t)r * a.sh.n_heads, chosen, ent);
                    const float logratio = nlp - a.oldlp[r];
                    const float ratio = expf(logratio);
                    float adv = a.adv[r];
                    if (hp.norm_adv) adv = (adv - mean_f) * inv_std;
                    const float rc = ratio < lo ? lo : (ratio > hi_c ? hi_c : ratio);
                    const float l1 = -adv * ratio, l2 = -adv * rc;
                    const bool inside = (ratio >= lo && ratio <= hi_c);
                    float d_ratio;
                    if (l1 > l2) d_ratio = -adv;
                    else if (l1 < l2) d_ratio = inside ? -adv : 0.0f;
                    else d_ratio = 0.5f * -adv + (inside ? 0.5f * -adv : 0.0f);   // torch::max splits ties half/half
                    g_nlp = invM * d_ratio * ratio;
                    g_ent = -hp.ent_coef * invM;
                    sums[0] += (double)(l1 > l2 ? l1 : l2);
                    sums[1] += (double)ent;
                    sums[2] += (double)((ratio - 1.0f) - logratio);
                    sums[3] += (fabsf(ratio - 1.0f) > clip) ? 1.0 : 0.0;
                }
#pragma unroll
                for (int k = 0; k < AM; k++) {
                    if (k < outP) {
                        float d = 0.0f;
                        if (r >= 0 && k < out) {
                            d = g_nlp * ((((chosen >> k) & 1u) ? 1.0f : 0.0f) - p[k]);
                            // CategoricalMasked's entropy is the true entropy: dH/dz_k = -p_k (log p_k + H); the plain Categorical's clamped form has none
                            if (DIST == PPO_DIST_MASKED) d += g_ent * q[k];
                            d = ((valid >> k) & 1u) ? d : 0.0f;
                        }
                        m.o[k * GF_S + s] = d;
                    }
                }
            } else if (net == 1) {
                float z[AM];
                float g_nlp = 0.0f, g_ent = 0.0f;
                if (r >= 0) {
                    double ent_d = 0.0;   // the same on every row
#pragma unroll
                    for (int k = 0; k < AM; k++) if (k < D) ent_d += gauss_entropy(m.ls[k]);
                    const float ent = (float)ent_d;
                    double nlp_d = 0.0;
#pragma unroll
                    for (int k = 0; k < AM; k++) {
                        z[k] = 0.0f;
                        if (k < D) {
                            z[k] = gauss_z(a.actions[(int64_t)r * D + k], m.o[k * GF_S + s], m.inv[k]);
                            nlp_d += gauss_logp(z[k], m.ls[k]);
                        }
                    }
                    const float logratio = (float)(nlp_d - (double)a.oldlp[r]);
                    const float ratio = expf(logratio);
                    float adv = a.adv[r];
                    if (hp.norm_adv) adv = (adv - mean_f) * inv_std;
                    const float rc = ratio < lo ? lo : (ratio > hi_c ? hi_c : ratio);
                    const float l1 = -adv * ratio, l2 = -adv * rc;
                    const bool inside = (ratio >= lo && ratio <= hi_c);
                    float d_ratio;
                    if (l1 > l2) d_ratio = -adv;
                    else if (l1 < l2) d_ratio = inside ? -adv : 0.0f;
                    else d_ratio = 0.5f * -adv + (inside ? 0.5f * -adv : 0.0f);   // torch::max splits ties half/half
                    g_nlp = invM * d_ratio * ratio;
                    g_ent = -hp.ent_coef * invM;
                    sums[0] += (double)(l1 > l2 ? l1 : l2);
                    sums[1] += (double)ent;
                    sums[2] += (double)((ratio - 1.0f) - logratio);
                    sums[3] += (fabsf(ratio - 1.0f) > clip) ? 1.0 : 0.0;
                }
#pragma unroll
                for (int k = 0; k < AM; k++) {
                    if (k < outP) {
                        float dm = 0.0f;
                        if (r >= 0 && k < D) {
                            dm = g_nlp * z[k] * m.inv[k];
                            dls[k] += g_nlp * (z[k] * z[k] - 1.0f) + g_ent;
                        }
                        m.o[k * GF_S + s] = dm;
                    }
                }
            } else {
                float g_v = 0.0f;
                if (r >= 0) {   // value loss (PPO_Discrete.cpp:603-625)
                    const float v = m.o[s], R = a.ret[r], vold = a.oldv[r];
                    const float un = (v - R) * (v - R);
                    float lossv;
                    if (hp.clip_vloss) {
                        const float dv = v - vold;
                        const float dvc = dv < -clip ? -clip : (dv > clip ? clip : dv);
                        const float vc = vold + dvc;
                        const float cl = (vc - R) * (vc - R);
                        lossv = un > cl ? un : cl;
                        const bool vin = (dv >= -clip && dv <= clip);
                        const float d_un = 2.0f * (v - R), d_cl = vin ? 2.0f * (vc - R) : 0.0f;
                        const float d = un > cl ? d_un : (un < cl ? d_cl : 0.5f * d_un + 0.5f * d_cl);
                        g_v = hp.vf_coef * 0.5f * invM * d;
                    } else {
                        lossv = un;
                        g_v = hp.vf_coef * 0.5f * invM * 2.0f * (v - R);
                    }
                    sums[4] += (double)lossv;
                }
                m.o[s] = g_v;
                m.o[1 * GF_S + s] = 0.0f; m.o[2 * GF_S + s] = 0.0f; m.o[3 * GF_S + s] = 0.0f;
            }
        }
        __syncthreads();
        // ---- backward ----
        if (4 * ub < outP) gf_dw_tile(m.o, m.h2, ub, kb, gW3, gb3);     // dW3 = dOUT H2^T, db3
        __syncthreads();                                                // ... has read H2
        gf_dz_tile(m.o, out, m.w3, m.h2, s, w);                         // H2 <- dZ2
        __syncthreads();
        gf_dw_tile(m.h2, m.h1, ub, kb, gW2, gb2);                       // dW2 = dZ2 H1^T, db2
        __syncthreads();                                                // ... has read H1
        gf_dz_tile(m.h2, 64, m.w2, m.h1, s, w);                         // H1 <- dZ1
        __syncthreads();
        if (4 * kb < obsP) gf_dw_tile(m.h1, m.x, ub, kb, gW1, gb1);     // dW1 = dZ1 X^T, db1 (the threads of kb = 0 are always among them)
        __syncthreads();                                                // the images are free for the next tile
    }

    // ---- the workgroup's partial slab, in the net's own parameter order: W1 b1 W2 b2 W3 b3 (actor: then log_std, which sits behind it in the flat vector) ----
    float* slab = a.slab + ((size_t)net * nb + b) * a.slab_stride;
    const int base = a.sh.off[net][0];
    {
        float* dW1 = slab + (a.sh.off[net][0] - base);
        float* dW2 = slab + (a.sh.off[net][2] - base);
        float* dW3 = slab + (a.sh.off[net][4] - base);
#pragma unroll
        for (int i = 0; i < 4; i++) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int u = 4 * ub + i, k = 4 * kb + j;
                if (k < O) dW1[u * O + k] = gW1[i * 4 + j];
                dW2[u * 64 + k] = gW2[i * 4 + j];
                if (u < out) dW3[u * 64 + k] = gW3[i * 4 + j];
            }
        }
        if (kb == 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int u = 4 * ub + i;
                slab[a.sh.off[net][1] - base + u] = gb1[i];
                slab[a.sh.off[net][3] - base + u] = gb2[i];
                if (u < out) slab[a.sh.off[net][5] - base + u] = gb3[i];
            }
        }
    }
    if (w == 0) {
        if (GAUSS && net == 1) {
#pragma unroll
            for (int k = 0; k < AM; k++) {
                if (k < D) {
                    const float t = wave_sum(dls[k]);
                    if (s == 0) slab[a.sh.logstd_off - base + k] = t;
                }
            }
        }
        // loss partials in gen_loss_sums's layout: the actor's workgroup b writes columns 0 .. 3 (and the padding 5 .. 7), the critic's column 4, of row b;
        // together the nb workgroups of a net write ALL GEN_LOSS_BLOCKS rows, the rows without a workgroup as zeros
        double t[5];
#pragma unroll
        for (int k = 0; k < 5; k++) t[k] = wave_sum_d_dpp(sums[k]);
        if (s < 8 && (net == 1 ? s != 4 : s == 4)) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 5; k++) v = s == k ? t[k] : v;
            for (int row = b; row < GEN_LOSS_BLOCKS; row += nb) a.loss_part[row * 8 + s] = row == b ? v : 0.0;
        }
    }
}

__global__ __launch_bounds__(GF_THREADS) void gauss_fwd_bwd_kernel(GfUpdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gf_lds[];
    gf_fwd_bwd_body<PPO_DIST_GAUSSIAN>(a, gf_lds);
}
// cat_fwd_bwd_kernel (PPO_KERNEL_CAT_FUSED): the same plan for a categorical / masked multi-head policy; there is no log_std tensor
template <int DIST>
__global__ __launch_bounds__(GF_THREADS) void cat_fwd_bwd_kernel(GfUpdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gf_lds[];
    gf_fwd_bwd_body<DIST>(a, gf_lds);
}

// grads[i] = the slabs' elements in workgroup order (one thread per element; the actor's range runs on through log_std)
__global__ __launch_bounds__(256) void gauss_slab_reduce_kernel(const float* __restrict__ slab, int slab_stride, int nb, int net1_off, int P, float* __restrict__ grads) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int net = i >= net1_off ? 1 : 0;
    const float* p = slab + (size_t)net * nb * slab_stride + (i - (net ? net1_off : 0));
    float acc = 0.0f;
    for (int k = 0; k < nb; k++) acc += p[(size_t)k * slab_stride];
    grads[i] = acc;
}

// ---------------------------------------------------------------------------------------------------------
// gauss_rollout_kernel<Env> (PPO_ENV_PENDULUM, PPO_ENV_MOUNTAINCAR_CONTINUOUS): the T steps of a rollout as ONE launch.  A workgroup owns one tile of 64 envs for the whole rollout; the actor's
// weights are staged once.  Lanes 0 .. 63 of wave 0 keep their env (state, episode sums, reset count, previous done flag, the current observation) in
// registers and do, per step, what gauss_act_kernel's wave 0 does behind the same forward -- the same draw, sample and log-prob expressions, so a stepwise
// loop of ppo_policy_act_f32 + ppo_env_step_f32 reproduces every stored bit -- then the env step (Env::step_episode).  Waves 1 .. 3 store the step's
// observation and done flag from LDS meanwhile (the done flag rides in the row-index words, which this kernel does not need as indices).
// Barriers per step: gf_forward_tile's four and one behind the stores (X and the done words are rewritten for the next step); every thread runs every
// barrier, a short tile masks its stores only.  No workgroup talks to another.  LDS: gf_lds_floats(4, 4) = 14 144 floats = 56 576 bytes, two workgroups per CU
// (Env::OBS <= 4: rows Env::OBS .. 3 of the X image are zero padding, written once).
// KEEP (a context with PPO_KERNEL_ENV_CUT_STATE; false: the kernel as it is without the parameter, which every other context launches): the owning lane runs
// step_episode_keep<Env> (ppo_internal.hpp) in the place of Env::step_episode -- the same step, bookkeeping and reset, and where the episode's length
// reaches the limit on this step, Env::STATE + 1 stores of the pre-reset state and the terminated word into column t N + env of the record a.cut
// [STATE + 1, T N].  No store at any other sample; cut_state_fold_kernel (below) reads the record.
// ---------------------------------------------------------------------------------------------------------
struct GfRolloutArgs {
    GfShape sh;
    const float* params;
    int N, T, max_episode_steps;
    int64_t seed, env_offset, step_base;
    float* env_state;        // [2, N]
    int32_t* ep_len;
    float* ep_rew;
    int32_t* reset_count;
    float* obs;              // [T, N, Env::OBS]
    float* actions;          // [T, N, 1]
    float* logprobs;
    float* rewards;
    float* dones;
    int32_t* fin_len;
    float* fin_rew;
    float* next_obs;         // [N, Env::OBS]
    int32_t* next_done;
    const float* forced;     // [T, N, 1] or null
    float* cut;              // KEEP: the cut-off record [Env::STATE + 1, T * N]; null otherwise
};

template <class Env, bool KEEP>
__global__ __launch_bounds__(GF_THREADS) void gauss_rollout_kernel(GfRolloutArgs a) {
    constexpr int OBS = Env::OBS;
    static_assert(OBS <= 4 && Env::STATE == 2, "the rollout kernel carves its LDS for an observation of at most 4 floats and keeps a state of 2 in registers");
    extern __shared__ __attribute__((aligned(16))) float gf_lds[];
    const int tid = threadIdx.x, N = a.N;
    const GfLds m = gf_carve(gf_lds, 4, 4);
    gf_stage_weights(m, a.sh, a.params, 1, tid);
    const int row0 = blockIdx.x * 64;
    const int env = row0 + (tid & 63);
    const bool owner = tid < 64 && env < N;
    const int64_t env_global = a.env_offset + env;
    float st[2] = { 0.0f, 0.0f }, ob[OBS], ep_rew = 0.0f;
#pragma unroll
    for (int k = 0; k < OBS; k++) ob[k] = 0.0f;
    int ep_len = 0, resets = 0, done = 0;
    if (owner) {
        st[0] = a.env_state[env];
        st[1] = a.env_state[(size_t)N + env];
        ep_len = a.ep_len[env];
        ep_rew = a.ep_rew[env];
        resets = a.reset_count[env];
        done = a.next_done[env];
        Env::obs(st, ob);
    }
    if (tid < 64) {   // the padding rows of the observation image, once
#pragma unroll
        for (int k = OBS; k < 4; k++) m.x[k * GF_S + tid] = 0.0f;
    }
    const int rows = N - row0 < 64 ? N - row0 : 64;
    for (int t = 0; t < a.T; t++) {
        const size_t tn = (size_t)t * N;
        if (tid < 64) {
#pragma unroll
            for (int k = 0; k < OBS; k++) m.x[k * GF_S + tid] = ob[k];
            m.ridx[tid] = done;
        }
        gf_forward_tile(m, 1, tid);
        if (tid < 64) {
            if (owner) {
                const float mu = m.o[tid], ls = m.ls[0];
                float eps[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                if (!a.forced) gauss_eps4(a.seed, env_global, a.step_base + t, 0, eps);
                const float act = a.forced ? a.forced[tn + env] : gauss_sample(mu, ls, eps[0]);
                double lp = 0.0;
                lp += gauss_logp(gauss_z(act, mu, expf(-ls)), ls);
                int fin_len;
                float fin_rew;
                float r;
                if constexpr (KEEP)
                    r = step_episode_keep<Env>(st, act, a.max_episode_steps, a.seed, env_global, ep_len, ep_rew, resets, done, fin_len, fin_rew, a.cut + tn + env,
                                               (size_t)a.T * N);
                else
                    r = Env::step_episode(st, act, a.max_episode_steps, a.seed, env_global, ep_len, ep_rew, resets, done, fin_len, fin_rew);
                Env::obs(st, ob);
                a.actions[tn + env] = act;
                a.logprobs[tn + env] = (float)lp;
                a.rewards[tn + env] = r;
                a.fin_len[tn + env] = fin_len;
                a.fin_rew[tn + env] = fin_rew;
            }
        } else {   // waves 1 .. 3: the step's observation rows and done flags, out of LDS
            float* obs_t = a.obs + (tn + row0) * OBS;
            for (int i = tid - 64; i < rows * OBS; i += GF_THREADS - 64) {
                const int s = i / OBS, k = i - OBS * s;
                obs_t[i] = m.x[k * GF_S + s];
            }
            if (tid < 128 && env < N) a.dones[tn + env] = (float)m.ridx[tid & 63];
        }
        __syncthreads();   // X and the done words are read: wave 0 may write the next step's
    }
    if (owner) {
#pragma unroll
        for (int k = 0; k < OBS; k++) a.next_obs[(size_t)env * OBS + k] = ob[k];
        a.next_done[env] = done;
        a.env_state[env] = st[0];
        a.env_state[(size_t)N + env] = st[1];
        a.ep_len[env] = ep_len;
        a.ep_rew[env] = ep_rew;
        a.reset_count[env] = resets;
    }
}

// ---- the envs' stand-alone kernels: one thread per env, on the device functions the rollout kernel uses (ppo_internal.hpp: GaussEnv*) ----
// ppo_env_reset: env_reset_kernel's bookkeeping (global env 0 takes reset 1: initEnvs probes it once before it resets everybody)
template <class Env>
__global__ void gauss_env_reset_kernel(int N, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew, int32_t* reset_count,
                                       float* next_obs, int32_t* next_done) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int k = (env_offset + i == 0) ? 1 : 0;
    float st[2], ob[Env::OBS];
    Env::reset(st, k, seed, env_offset + i);
    Env::obs(st, ob);
    env_state[i] = st[0];
    env_state[(size_t)N + i] = st[1];
    for (int j = 0; j < Env::OBS; j++) next_obs[(size_t)i * Env::OBS + j] = ob[j];
    ep_len[i] = 0;
    ep_rew[i] = 0.0f;
    reset_count[i] = k + 1;
    next_done[i] = 0;
}
// ppo_env_step_f32: action f32 [N, 1]
template <class Env>
__global__ void gauss_env_step_kernel(int N, int max_episode_steps, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew,
                                      int32_t* reset_count, const float* __restrict__ action, float* obs, float* reward, int32_t* done) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float st[2] = { env_state[i], env_state[(size_t)N + i] }, ob[Env::OBS];
    int len = ep_len[i], resets = reset_count[i], d, fin_len;
    float rew = ep_rew[i], fin_rew;
    const float r = Env::step_episode(st, action[i], max_episode_steps, seed, env_offset + i, len, rew, resets, d, fin_len, fin_rew);
    Env::obs(st, ob);
    env_state[i] = st[0];
    env_state[(size_t)N + i] = st[1];
    ep_len[i] = len;
    ep_rew[i] = rew;
    reset_count[i] = resets;
    for (int j = 0; j < Env::OBS; j++) obs[(size_t)i * Env::OBS + j] = ob[j];
    reward[i] = r;
    done[i] = d;
}
// ppo_env_transition_f32: stateless; state [n, 2], action [n, 1], obs_out [n, Env::OBS] or null
template <class Env>
__global__ void gauss_env_transition_kernel(const float* __restrict__ state_in, const float* __restrict__ action, int64_t n, float* next_state, float* obs_out,
                                            float* reward, int32_t* terminated) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float st[2] = { state_in[i * 2], state_in[i * 2 + 1] };
    int term;
    const float r = Env::step(st, action[i], term);
    next_state[i * 2] = st[0];
    next_state[i * 2 + 1] = st[1];
    if (obs_out) {
        float ob[Env::OBS];
        Env::obs(st, ob);
        for (int j = 0; j < Env::OBS; j++) obs_out[i * Env::OBS + j] = ob[j];
    }
    reward[i] = r;
    terminated[i] = term;
}
// ppo_env_set_state_h: NEXT_OBS from the injected states
template <class Env>
__global__ void gauss_env_obs_kernel(int N, const float* __restrict__ env_state, float* next_obs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float st[2] = { env_state[i], env_state[(size_t)N + i] };
    float ob[Env::OBS];
    Env::obs(st, ob);
    for (int j = 0; j < Env::OBS; j++) next_obs[(size_t)i * Env::OBS + j] = ob[j];
}

// ---------------------------------------------------------------------------------------------------------
// gauss_trunc_fold_kernel<Env> (ppo_env_truncation_bootstrap on an env whose observation is its state): env_trunc_fold_mfma_kernel's plan (kernels_update_mfma.hip)
// on this file's critic.  A 256-thread workgroup owns 256 consecutive flat samples.  Every thread reads FIN_LEN[i]; a lane whose episode reached the limit
// recomputes the step (Env::step on OBS[i] under the raw action ACTIONS[i]: divergent code without a barrier) and keeps the sample unless the env terminated
// on it.  ONE compaction (fold_compact), on the kept samples; a workgroup that keeps none -- the common case, one pass over FIN_LEN -- returns before it
// loads a weight (the count is the same in every thread, so the return is uniform).  The kept samples' final observations wait in LDS in list order
// (ascending); the critic's weights are staged, and the workgroup runs gf_forward_tile on the list in tiles of 64 -- gauss_values_kernel's forward on the same
// carve, so v is that kernel's value of the final observation, bit for bit.  Lane k of wave 0 folds row k of the tile (fold_store).
// LDS: gf_lds_floats(4, 4) dynamic + 256 * OBS floats + 264 ints static = 59 680 bytes for OBS 2: no attribute needed, two workgroups per CU.
// ---------------------------------------------------------------------------------------------------------
struct GfFoldArgs {
    GfShape sh;
    const float* params;
    const float* obs;
    const float* actions;
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

template <class Env>
__global__ __launch_bounds__(DEV_FOLD_THREADS) void gauss_trunc_fold_kernel(GfFoldArgs a) {
    constexpr int OBS = Env::OBS;
    static_assert(Env::OBS_IS_STATE && OBS == Env::STATE && OBS <= 4, "the fold steps the env from a stored observation");
    static_assert(DEV_FOLD_THREADS == GF_THREADS, "fold_compact and gf_forward_tile are written for the same workgroup");
    extern __shared__ __attribute__((aligned(16))) float gf_lds[];
    __shared__ float fobs[DEV_FOLD_THREADS * OBS];
    __shared__ int list[DEV_FOLD_THREADS], wtot[8];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * DEV_FOLD_THREADS + tid;
    bool keep = false;
    float st[OBS];
#pragma unroll
    for (int j = 0; j < OBS; j++) st[j] = 0.0f;
    if (i < a.B && a.fin_len[i] == a.max_episode_steps) {
#pragma unroll
        for (int j = 0; j < OBS; j++) st[j] = a.obs[i * OBS + j];
        int terminated;
        (void)Env::step(st, a.actions[i], terminated);
        keep = terminated == 0;
    }
    int pos;
    const int cnt = fold_compact(keep, (int)i, a.ev_count, list, wtot, pos);
    if (cnt == 0) return;
    const int base = wtot[4];
    if (keep) {
#pragma unroll
        for (int j = 0; j < OBS; j++) fobs[pos * OBS + j] = st[j];
    }
    const GfLds m = gf_carve(gf_lds, 4, 4);
    gf_stage_weights(m, a.sh, a.params, 0, tid);
    if (tid < 64) {   // the padding rows of the observation image, once
#pragma unroll
        for (int k = OBS; k < 4; k++) m.x[k * GF_S + tid] = 0.0f;
    }
    __syncthreads();   // fobs is complete
    for (int k0 = 0; k0 < cnt; k0 += 64) {
        const int k = k0 + tid;   // tid < 64: this lane's place in the list
        if (tid < 64) {
#pragma unroll
            for (int j = 0; j < OBS; j++) m.x[j * GF_S + tid] = k < cnt ? fobs[k * OBS + j] : 0.0f;
        }
        gf_forward_tile(m, 1, tid);
        if (tid < 64 && k < cnt) fold_store(a.rewards, a.gamma, a.ev_index, a.ev_value, a.ev_cap, (int64_t)base + k, list[k], m.o[tid]);
        __syncthreads();   // X and OUT are read: the next tile may overwrite them
    }
}

// ---------------------------------------------------------------------------------------------------------
// gauss_dev_fold_kernel (ppo_dev_observe with truncation flags on a PPO_KERNEL_GAUSS_FUSED / PPO_KERNEL_CAT_FUSED context): dev_fold_mfma_kernel's front end
// (ppo_internal.hpp: DevFoldArgs, dev_fold_compact) on this file's critic.  A 256-thread workgroup owns env rows [256 b, 256 b + 256); every thread reads
// truncated[n] and done[n], ONE compaction, and a workgroup without a flagged row -- the common step, one pass over 2 N int32 -- returns before it loads a
// weight (the count is the same in every thread, so the return is uniform).  Otherwise the critic's weights are staged on gauss_values_kernel's carve and the
// workgroup walks its list (ascending, up to 256 rows) in tiles of 64: the list's row numbers, or -1, are the tile's row indices, gf_load_x reads those rows
// of final_obs [N, O] and no other (an unflagged row may hold anything), gf_forward_tile is gauss_values_kernel's forward, so v is that kernel's value of
// the row, bit for bit.  Lane k of wave 0 folds row k of the tile (dev_fold_store).
// LDS: all dynamic -- gf_lds_floats(obsP, 4) floats and, behind them, the row list [256] and the waves' totals [8]: 54 464 + 528 obsP + 1 056 bytes, which
// passes 64 KB between obs 16 and obs 17 .. 20; the launcher decides on the attribute from this sum, so no static LDS sits outside what it counted.
// ---------------------------------------------------------------------------------------------------------
constexpr int GF_DEV_FOLD_LIST_INTS = DEV_FOLD_THREADS + 8;

__global__ __launch_bounds__(DEV_FOLD_THREADS) void gauss_dev_fold_kernel(GfShape sh, const float* __restrict__ params, DevFoldArgs a) {
    static_assert(DEV_FOLD_THREADS == GF_THREADS, "fold_compact and gf_forward_tile are written for the same workgroup");
    extern __shared__ __attribute__((aligned(16))) float gf_lds[];
    const int tid = threadIdx.x, O = sh.obs, obsP = gf_pad4(O);
    int* list = reinterpret_cast<int*>(gf_lds + gf_lds_floats(obsP, 4));
    int* wtot = list + DEV_FOLD_THREADS;
    const int cnt = dev_fold_compact(a, list, wtot);
    if (cnt == 0) return;
    const int base = wtot[4];
    const GfLds m = gf_carve(gf_lds, obsP, 4);
    gf_stage_weights(m, sh, params, 0, tid);
    for (int k0 = 0; k0 < cnt; k0 += 64) {
        const int k = k0 + tid;   // tid < 64: this lane's place in the list
        if (tid < 64) m.ridx[tid] = k < cnt ? list[k] : -1;
        __syncthreads();
        gf_load_x(m, a.final_obs, O, tid);
        gf_forward_tile(m, 1, tid);
        if (tid < 64 && k < cnt) dev_fold_store(a, base, k, list[k], m.o[tid]);
        __syncthreads();   // OUT and the row indices are read: the next tile may overwrite them
    }
}

// ---------------------------------------------------------------------------------------------------------
// gauss_eval_kernel<Env> (ppo_evaluate on an env whose observation is its state): whole episodes in ONE launch.  A workgroup owns 64 episodes for their whole
// length with the actor's weights resident, as in gauss_rollout_kernel: lane l of wave 0 keeps episode 64 b + l (state, return, length) in registers, writes
// its observation into the X image, every thread runs gf_forward_tile, and wave 0 takes the mean (greedy) or mu + sigma * eps with eps keyed (seed, episode,
// step of the episode, 0) -- gauss_act_kernel's expressions -- and steps the env (Env::step).  An episode ends where the env terminates or its length reaches
// max_episode_steps; a finished lane keeps feeding its last observation through the forward and ignores the result.
// The step loop's exit must be uniform across the workgroup (every thread runs the forward's barriers): wave 0 ballots its live lanes and publishes the count
// in the row-index words, which this kernel does not need as indices; the step's closing barrier, which every thread runs, hands it to the other waves.
// The loop ends after at most max_episode_steps steps.  Nothing depends on the tile an episode sits in.
// ---------------------------------------------------------------------------------------------------------
struct GfEvalArgs {
    GfShape sh;
    const float* params;
    int64_t n_episodes, seed;
    int max_episode_steps, greedy;
    float* ep_return;
    int32_t* ep_length;
    int32_t* ep_trunc;
};

template <class Env>
__global__ __launch_bounds__(GF_THREADS) void gauss_eval_kernel(GfEvalArgs a) {
    constexpr int OBS = Env::OBS;
    static_assert(Env::OBS_IS_STATE && OBS <= 4 && Env::STATE == 2, "as gauss_rollout_kernel");
    extern __shared__ __attribute__((aligned(16))) float gf_lds[];
    const int tid = threadIdx.x;
    const GfLds m = gf_carve(gf_lds, 4, 4);
    gf_stage_weights(m, a.sh, a.params, 1, tid);
    const int64_t ep = (int64_t)blockIdx.x * 64 + (tid & 63);
    bool alive = tid < 64 && ep < a.n_episodes;
    const bool owner = alive;
    float st[2] = { 0.0f, 0.0f }, ob[OBS], ep_rew = 0.0f;
#pragma unroll
    for (int k = 0; k < OBS; k++) ob[k] = 0.0f;
    int ep_len = 0, trunc = 0;
    if (owner) {
        Env::reset(st, 0, a.seed, ep);
        Env::obs(st, ob);
    }
    if (tid < 64) {
#pragma unroll
        for (int k = OBS; k < 4; k++) m.x[k * GF_S + tid] = 0.0f;
    }
    for (;;) {
        if (tid < 64) {
#pragma unroll
            for (int k = 0; k < OBS; k++) m.x[k * GF_S + tid] = ob[k];
        }
        gf_forward_tile(m, 1, tid);
        if (tid < 64) {
            if (alive) {
                const float mu = m.o[tid], ls = m.ls[0];
                float eps[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                if (!a.greedy) gauss_eps4(a.seed, ep, (int64_t)ep_len, 0, eps);
                const float act = a.greedy ? mu : gauss_sample(mu, ls, eps[0]);
                int term;
                const float r = Env::step(st, act, term);
                ep_len += 1;
                ep_rew += r;
                trunc = ep_len == a.max_episode_steps ? 1 : 0;
                if (term || trunc) alive = false;
                Env::obs(st, ob);
            }
            const unsigned long long live = __ballot(alive);
            if (tid == 0) m.ridx[0] = __popcll(live);
        }
        __syncthreads();   // the live count is published; OUT is read
        if (m.ridx[0] == 0) break;
        // the next write of the count is behind the next forward's four barriers: every wave has read this one by then
    }
    if (owner) {
        a.ep_return[ep] = ep_rew;
        a.ep_length[ep] = ep_len;
        a.ep_trunc[ep] = trunc;
    }
}

// ---------------------------------------------------------------------------------------------------------
// cat_rollout_kernel<Env, DIST> (PPO_ENV_ACROBOT, PPO_ENV_TAXI): gauss_rollout_kernel's plan with cat_act_kernel's wave-0 work -- the T steps of a categorical rollout as ONE
// launch.  A workgroup owns one tile of 64 envs for the whole rollout; the actor's weights are staged once.  Lanes 0 .. 63 of wave 0 keep their env (state,
// episode sums, reset count, previous done flag, the current observation) in registers and do, per step, what cat_act_kernel<PPO_DIST_CATEGORICAL>'s wave 0
// does behind the same forward -- categorical_head and sample_head on the lane's columns of OUT and H1, the same Philox key (seed, env_offset + env,
// (step_base + t) >> 2, head 0) and word select (step_base + t) & 3 -- so a stepwise loop of ppo_policy_act + ppo_env_step reproduces every stored bit; then
// the env step (Env::step_episode under head 0's action).  Waves 1 .. 3 store the step's observation, its mask row (all ones: PPO_BUF_MASKS as a host-fed
// context without a mask holds it) and the done flag meanwhile (the flag rides in the row-index words).  Barriers per step: gf_forward_tile's four and one
// behind the stores; every thread runs every barrier, a short tile masks its stores only.  No workgroup talks to another.
// LDS: gf_carve(8, 4) for PPO_ENV_ACROBOT (OBS 6, 3 logits) = 14 672 floats = 58 688 bytes, two workgroups per CU; rows OBS .. obsP - 1 of the X image are zero
// padding, written once.  The policy has ONE head (ppo_ctx_create), of Env::ACTIONS logits.
// PPO_ENV_TAXI: gf_carve(20, 8) = 16 784 floats = 67 136 bytes (the launcher asks for the attribute through gf_allow).  Env::HAS_MASK and DIST = PPO_DIST_MASKED:
// the lane forms the mask bits of its state in front of the forward, publishes them next to the done flag in the row-index words (bit 0 the flag, bits 1 ..
// the mask), and behind the forward draws under them with cat_act_kernel<PPO_DIST_MASKED>'s expressions (categorical_head<PPO_DIST_MASKED, GF_S> on the lane's
// columns, the same key and word select), so ppo_policy_act(obs, mask, step_index) + ppo_env_step reproduces every stored bit; waves 1 .. 3 store the real mask
// rows meanwhile.  DIST = PPO_DIST_CATEGORICAL on such an env: ones, and an unmasked draw -- Acrobot's rule.  Env::OBS_ONE_HOT: the lane keeps no observation;
// its column of the X image is zeroed once and per step the HOT old ones are cleared and the HOT new ones set -- 8 LDS stores at computed rows (and about as
// many address computations) against 19 compares, 19 selects and 19 stores for writing the column out: the smaller instruction count, chosen for that.
// PPO_ENV_FROZENLAKE / PPO_ENV_FROZENLAKE8X8 (OBS 16 / 64, 4 logits, HOT 1): gf_carve(16, 4) = 15 728 floats = 62 912 bytes; gf_carve(64, 4) = 22 064 floats =
// 88 256 bytes (the attribute; one workgroup per CU).  The env's slip is drawn inside Env::step_episode, in wave 0's lane right behind the action draw: one
// Philox call keyed by the state's own words (k0, k1) at counter (j >> 2, 0, 0, 0x20), every step -- the definition's bits by construction, since it IS the
// definition the stand-alone step and the stateless transition run.  Waves 1 .. 3 store the step's observation rows from the X image as on the other envs: at
// OBS 64 that is 16 KB per workgroup and step.
// PPO_ENV_BLACKJACK (OBS 45, 2 logits, HOT 3): gf_carve(48, 4) = 79 808 bytes (the attribute).  What differs between the lanes of wave 0 here is the WORK of a
// step: a hit is one Philox call, a stick the call of the hidden card, the dealer's (one more, seldom two) and the two of the reset that follows -- lanes that
// hit wait for lanes that stick, the wave pays the longest lane's path each step.
// KEEP: as in gauss_rollout_kernel -- step_episode_keep<Env> in the place of Env::step_episode, the record a.cut [STATE + 1, T N]; false is the kernel as it was.
// ---------------------------------------------------------------------------------------------------------
struct CfRolloutArgs {
    GfShape sh;
    const float* params;
    int N, T, max_episode_steps;
    int64_t seed, env_offset, step_base;
    float* env_state;        // [Env::STATE, N]
    int32_t* ep_len;
    float* ep_rew;
    int32_t* reset_count;
    float* obs;              // [T, N, Env::OBS]
    uint8_t* masks;          // [T, N, Env::ACTIONS]
    int32_t* actions;        // [T, N, 1]
    float* logprobs;
    float* rewards;
    float* dones;
    int32_t* fin_len;
    float* fin_rew;
    float* next_obs;         // [N, Env::OBS]
    int32_t* next_done;
    const int64_t* forced;   // [T, N, 1] or null
    float* cut;              // KEEP: the cut-off record [Env::STATE + 1, T * N]; null otherwise
};

// wave 0's lane behind the forward: the row's head on the lane's columns (z: OUT, log-probs in place; p: H1), the action (GREEDY: the first-index argmax of
// the probabilities; forced; or the draw with uniform word `ws`) and its log-prob -- cat_act_kernel<DIST>'s expressions for one head.  PPO_DIST_MASKED:
// bit k of `allowed` is the row's mask byte k (the lane formed it from its env's state; a masked-out logit becomes -1e8f, its probability 0)
template <int DIST, bool GREEDY>
__device__ __forceinline__ int cat_lane_head(const GfLds& m, int lane, int Ah, uint32_t allowed, bool has_forced, int forced, uint32_t ws, float& lp) {
    float* z = m.o + lane;
    float* p = m.h1 + lane;
    if constexpr (DIST == PPO_DIST_MASKED) {
        uint8_t mrow[8];
#pragma unroll
        for (int k = 0; k < 8; k++) mrow[k] = (uint8_t)((allowed >> k) & 1u);
        (void)categorical_head<PPO_DIST_MASKED, GF_S>(z, p, mrow, Ah);
    } else {
        (void)categorical_head<PPO_DIST_CATEGORICAL, GF_S>(z, p, nullptr, Ah);
    }
    int a;
    if constexpr (GREEDY) {
        a = 0;
        for (int k = 1; k < Ah; k++) if (p[k * GF_S] > p[a * GF_S]) a = k;
    } else if (has_forced) {
        a = forced;
    } else {
        a = sample_head<GF_S>(p, Ah, (float)(ws >> 8) * 0x1p-24f);
    }
    lp = 0.0f;
    for (int k = 0; k < Ah; k++) if (k == a) lp = z[k * GF_S];
    return a;
}
// a caller's i64 action as the env's int: saturated, not truncated, so that an env that clamps its action clamps the caller's number
__device__ __forceinline__ int cat_action_int(int64_t a) { return a < -2147483647ll ? -2147483647 : (a > 2147483647ll ? 2147483647 : (int)a); }
__device__ __forceinline__ uint32_t cat_draw_word(int64_t seed, int64_t row, int64_t step_index) {
    const uint4 w = philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)row, (uint32_t)(step_index >> 2), 0u, 0u);
    return (step_index & 3) == 0 ? w.x : ((step_index & 3) == 1 ? w.y : ((step_index & 3) == 2 ? w.z : w.w));
}

template <class Env, int DIST, bool KEEP>
__global__ __launch_bounds__(GF_THREADS) void cat_rollout_kernel(CfRolloutArgs a) {
    constexpr int OBS = Env::OBS, ST = Env::STATE, A = Env::ACTIONS, OBSP = (OBS + 3) & ~3, OUTP = (A + 3) & ~3;
    constexpr bool MASKED = Env::HAS_MASK && DIST == PPO_DIST_MASKED;   // the env's mask is drawn under and stored; otherwise PPO_BUF_MASKS holds ones
    static_assert(OBS <= 64 && A <= 8, "the rollout kernel carves its LDS for an observation of at most 64 floats and a head of at most 8 logits");
    static_assert(DIST == PPO_DIST_CATEGORICAL || Env::HAS_MASK, "a masked policy needs an env that forms a mask");
    extern __shared__ __attribute__((aligned(16))) float gf_lds[];
    const int tid = threadIdx.x, N = a.N;
    const GfLds m = gf_carve(gf_lds, OBSP, OUTP);
    gf_stage_weights(m, a.sh, a.params, 1, tid);
    const int row0 = blockIdx.x * 64;
    const int env = row0 + (tid & 63);
    const bool owner = tid < 64 && env < N;
    const int64_t env_global = a.env_offset + env;
    // a one-hot env keeps no observation: its lane moves the ones in the X image (hot: the rows that hold them)
    float st[ST], ob[Env::OBS_ONE_HOT ? 1 : OBS], ep_rew = 0.0f;
    int hot[Env::OBS_ONE_HOT ? Env::HOT : 1];
#pragma unroll
    for (int k = 0; k < ST; k++) st[k] = 0.0f;
    if constexpr (!Env::OBS_ONE_HOT) {
#pragma unroll
        for (int k = 0; k < OBS; k++) ob[k] = 0.0f;
    }
    int ep_len = 0, resets = 0, done = 0;
    if (owner) {
#pragma unroll
        for (int k = 0; k < ST; k++) st[k] = a.env_state[(size_t)k * N + env];
        ep_len = a.ep_len[env];
        ep_rew = a.ep_rew[env];
        resets = a.reset_count[env];
        done = a.next_done[env];
        if constexpr (!Env::OBS_ONE_HOT) Env::obs(st, ob);
    }
    if (tid < 64) {
        if constexpr (Env::OBS_ONE_HOT) {   // the whole column of the observation image, once: per step 2 HOT stores move the ones (19 selects and stores otherwise)
#pragma unroll
            for (int k = 0; k < OBSP; k++) m.x[k * GF_S + tid] = 0.0f;
            Env::hot(st, hot);   // a lane without an env: the all-zero state, whose rows are inside the image like any other's
        } else {   // the padding rows of the observation image, once
#pragma unroll
            for (int k = OBS; k < OBSP; k++) m.x[k * GF_S + tid] = 0.0f;
        }
    }
    const int rows = N - row0 < 64 ? N - row0 : 64;
    for (int t = 0; t < a.T; t++) {
        const size_t tn = (size_t)t * N;
        uint32_t allowed = 0xffu;
        if (tid < 64) {
            if constexpr (Env::OBS_ONE_HOT) {
#pragma unroll
                for (int k = 0; k < Env::HOT; k++) m.x[hot[k] * GF_S + tid] = 0.0f;   // the previous step's ones (the first step: zeros over zeros)
                Env::hot(st, hot);
#pragma unroll
                for (int k = 0; k < Env::HOT; k++) m.x[hot[k] * GF_S + tid] = 1.0f;
            } else {
#pragma unroll
                for (int k = 0; k < OBS; k++) m.x[k * GF_S + tid] = ob[k];
            }
            if constexpr (MASKED) {   // the mask of the state the action is drawn in rides next to the done flag: waves 1 .. 3 store its row
                allowed = Env::mask_bits(st);
                m.ridx[tid] = done | (int)(allowed << 1);
            } else {
                m.ridx[tid] = done;
            }
        }
        gf_forward_tile(m, A, tid);
        if (tid < 64) {
            if (owner) {
                const int64_t step_index = a.step_base + t;
                const uint32_t ws = a.forced ? 0u : cat_draw_word(a.seed, env_global, step_index);
                float lp;
                const int act = cat_lane_head<MASKED ? PPO_DIST_MASKED : PPO_DIST_CATEGORICAL, false>(m, tid, A, allowed, a.forced != nullptr,
                                                                                                      a.forced ? cat_action_int(a.forced[tn + env]) : 0, ws, lp);
                int fin_len;
                float fin_rew;
                float r;
                if constexpr (KEEP)
                    r = step_episode_keep<Env>(st, act, a.max_episode_steps, a.seed, env_global, ep_len, ep_rew, resets, done, fin_len, fin_rew, a.cut + tn + env,
                                               (size_t)a.T * N);
                else
                    r = Env::step_episode(st, act, a.max_episode_steps, a.seed, env_global, ep_len, ep_rew, resets, done, fin_len, fin_rew);
                if constexpr (!Env::OBS_ONE_HOT) Env::obs(st, ob);
                a.actions[tn + env] = act;
                a.logprobs[tn + env] = lp;
                a.rewards[tn + env] = r;
                a.fin_len[tn + env] = fin_len;
                a.fin_rew[tn + env] = fin_rew;
            }
        } else {   // waves 1 .. 3: the step's observation rows, mask rows and done flags; X and the done words are not touched by wave 0's head work
            float* obs_t = a.obs + (tn + row0) * OBS;
            for (int i = tid - 64; i < rows * OBS; i += GF_THREADS - 64) {
                const int s = i / OBS, k = i - OBS * s;
                obs_t[i] = m.x[k * GF_S + s];
            }
            uint8_t* mask_t = a.masks + (tn + row0) * A;
            if constexpr (MASKED) {
                for (int i = tid - 64; i < rows * A; i += GF_THREADS - 64) {
                    const int s = i / A, k = i - A * s;
                    mask_t[i] = (uint8_t)((m.ridx[s] >> (1 + k)) & 1);
                }
                if (tid < 128 && env < N) a.dones[tn + env] = (float)(m.ridx[tid & 63] & 1);
            } else {
                for (int i = tid - 64; i < rows * A; i += GF_THREADS - 64) mask_t[i] = (uint8_t)1;
                if (tid < 128 && env < N) a.dones[tn + env] = (float)m.ridx[tid & 63];
            }
        }
        __syncthreads();   // X, OUT, the H1 columns and the done words are read: wave 0 may write the next step's
    }
    if (owner) {
        if constexpr (Env::OBS_ONE_HOT) {
            float fo[OBS];
            Env::obs(st, fo);
#pragma unroll
            for (int k = 0; k < OBS; k++) a.next_obs[(size_t)env * OBS + k] = fo[k];
        } else {
#pragma unroll
            for (int k = 0; k < OBS; k++) a.next_obs[(size_t)env * OBS + k] = ob[k];
        }
        a.next_done[env] = done;
#pragma unroll
        for (int k = 0; k < ST; k++) a.env_state[(size_t)k * N + env] = st[k];
        a.ep_len[env] = ep_len;
        a.ep_rew[env] = ep_rew;
        a.reset_count[env] = resets;
    }
}

// ---- the stand-alone kernels of a device env with integer actions: one thread per env, on the device functions the rollout kernel uses (CatEnv*) ----
template <class Env>
__global__ void cat_env_reset_kernel(int N, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew, int32_t* reset_count,
                                     float* next_obs, int32_t* next_done) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int k = (env_offset + i == 0) ? 1 : 0;   // global env 0 takes reset 1, as elsewhere (env_reset_kernel)
    float st[Env::STATE], ob[Env::OBS];
    Env::reset(st, k, seed, env_offset + i);
    Env::obs(st, ob);
    for (int j = 0; j < Env::STATE; j++) env_state[(size_t)j * N + i] = st[j];
    for (int j = 0; j < Env::OBS; j++) next_obs[(size_t)i * Env::OBS + j] = ob[j];
    ep_len[i] = 0;
    ep_rew[i] = 0.0f;
    reset_count[i] = k + 1;
    next_done[i] = 0;
}
// ppo_env_step: action i64 [N, 1]
template <class Env>
__global__ void cat_env_step_kernel(int N, int max_episode_steps, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew,
                                    int32_t* reset_count, const int64_t* __restrict__ action, float* obs, float* reward, int32_t* done) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float st[Env::STATE], ob[Env::OBS];
    for (int j = 0; j < Env::STATE; j++) st[j] = env_state[(size_t)j * N + i];
    int len = ep_len[i], resets = reset_count[i], d, fin_len;
    float rew = ep_rew[i], fin_rew;
    const float r = Env::step_episode(st, cat_action_int(action[i]), max_episode_steps, seed, env_offset + i, len, rew, resets, d, fin_len, fin_rew);
    Env::obs(st, ob);
    for (int j = 0; j < Env::STATE; j++) env_state[(size_t)j * N + i] = st[j];
    ep_len[i] = len;
    ep_rew[i] = rew;
    reset_count[i] = resets;
    for (int j = 0; j < Env::OBS; j++) obs[(size_t)i * Env::OBS + j] = ob[j];
    reward[i] = r;
    done[i] = d;
}
// ppo_env_transition: stateless; state [n, Env::STATE], action i64 [n]
template <class Env>
__global__ void cat_env_transition_kernel(const float* __restrict__ state_in, const int64_t* __restrict__ action, int64_t n, float* next_state, float* reward,
                                          int32_t* terminated) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float st[Env::STATE];
    for (int j = 0; j < Env::STATE; j++) st[j] = state_in[i * Env::STATE + j];
    int term;
    const float r = Env::step(st, cat_action_int(action[i]), term);
    for (int j = 0; j < Env::STATE; j++) next_state[i * Env::STATE + j] = st[j];
    reward[i] = r;
    terminated[i] = term;
}
// ppo_env_set_state_h: NEXT_OBS from the injected states ([Env::STATE, N])
template <class Env>
__global__ void cat_env_obs_kernel(int N, const float* __restrict__ state, float* obs_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float st[Env::STATE], ob[Env::OBS];
    for (int j = 0; j < Env::STATE; j++) st[j] = state[(size_t)j * N + i];
    Env::obs(st, ob);
    for (int j = 0; j < Env::OBS; j++) obs_out[(size_t)i * Env::OBS + j] = ob[j];
}

// ---------------------------------------------------------------------------------------------------------
// cat_eval_kernel<Env, DIST> (ppo_evaluate on PPO_ENV_ACROBOT, PPO_ENV_TAXI, PPO_ENV_FROZENLAKE, PPO_ENV_FROZENLAKE8X8, PPO_ENV_BLACKJACK): gauss_eval_kernel's plan with a categorical head.  A workgroup owns 64 episodes for their whole
// length with the actor's weights resident: lane l of wave 0 keeps episode 64 b + l (state, return, length) in registers -- the STATE, not the observation:
// nothing here needs an observation to be a state -- writes its observation into the X image, every thread runs gf_forward_tile, and wave 0 takes the
// first-index argmax of the probabilities (greedy: ppo_policy_act_greedy's) or the draw keyed (seed, episode, step of the episode, head 0) --
// ppo_policy_act(step_index = step) on row `episode` -- and steps the env (Env::step).  The loop's exit is uniform: wave 0 publishes its live count in the
// row-index words, the step's closing barrier hands it to the other waves (gauss_eval_kernel).  At most max_episode_steps steps.
// PPO_ENV_TAXI under PPO_DIST_MASKED: the same widening and the same masked head as cat_rollout_kernel; greedy is the first-index argmax of the MASKED
// probabilities (a masked-out action has probability 0 and is never chosen: an allowed one has a positive probability, and the comparison is strict).
// PPO_ENV_BLACKJACK: the rollout's carve (79 808 bytes); an episode's cards come from the key its reset drew from (seed, e), as FrozenLake's slips do.
// PPO_ENV_FROZENLAKE / PPO_ENV_FROZENLAKE8X8: the rollout's carves (62 912 and 88 256 bytes).  Episode e's slips come from the key its reset drew from (seed, e)
// and from its own step count, both in the lane's state: the episode is a pure function of (parameters, seed, e), whatever its neighbours do.
// ---------------------------------------------------------------------------------------------------------
template <class Env, int DIST>
__global__ __launch_bounds__(GF_THREADS) void cat_eval_kernel(GfEvalArgs a) {
    constexpr int OBS = Env::OBS, ST = Env::STATE, A = Env::ACTIONS, OBSP = (OBS + 3) & ~3, OUTP = (A + 3) & ~3;
    constexpr bool MASKED = Env::HAS_MASK && DIST == PPO_DIST_MASKED;
    constexpr int HEAD = MASKED ? PPO_DIST_MASKED : PPO_DIST_CATEGORICAL;
    static_assert(OBS <= 64 && A <= 8, "as cat_rollout_kernel");
    static_assert(DIST == PPO_DIST_CATEGORICAL || Env::HAS_MASK, "a masked policy needs an env that forms a mask");
    extern __shared__ __attribute__((aligned(16))) float gf_lds[];
    const int tid = threadIdx.x;
    const GfLds m = gf_carve(gf_lds, OBSP, OUTP);
    gf_stage_weights(m, a.sh, a.params, 1, tid);
    const int64_t ep = (int64_t)blockIdx.x * 64 + (tid & 63);
    bool alive = tid < 64 && ep < a.n_episodes;
    const bool owner = alive;
    float st[ST], ob[Env::OBS_ONE_HOT ? 1 : OBS], ep_rew = 0.0f;
    int hot[Env::OBS_ONE_HOT ? Env::HOT : 1];
#pragma unroll
    for (int k = 0; k < ST; k++) st[k] = 0.0f;
    if constexpr (!Env::OBS_ONE_HOT) {
#pragma unroll
        for (int k = 0; k < OBS; k++) ob[k] = 0.0f;
    }
    int ep_len = 0, trunc = 0;
    if (owner) {
        Env::reset(st, 0, a.seed, ep);
        if constexpr (!Env::OBS_ONE_HOT) Env::obs(st, ob);
    }
    if (tid < 64) {
        if constexpr (Env::OBS_ONE_HOT) {   // as cat_rollout_kernel: the column is zeroed once and the ones move
#pragma unroll
            for (int k = 0; k < OBSP; k++) m.x[k * GF_S + tid] = 0.0f;
            Env::hot(st, hot);
        } else {
#pragma unroll
            for (int k = OBS; k < OBSP; k++) m.x[k * GF_S + tid] = 0.0f;
        }
    }
    for (;;) {
        if (tid < 64) {
            if constexpr (Env::OBS_ONE_HOT) {
#pragma unroll
                for (int k = 0; k < Env::HOT; k++) m.x[hot[k] * GF_S + tid] = 0.0f;
                Env::hot(st, hot);
#pragma unroll
                for (int k = 0; k < Env::HOT; k++) m.x[hot[k] * GF_S + tid] = 1.0f;
            } else {
#pragma unroll
                for (int k = 0; k < OBS; k++) m.x[k * GF_S + tid] = ob[k];
            }
        }
        gf_forward_tile(m, A, tid);
        if (tid < 64) {
            if (alive) {
                uint32_t allowed = 0xffu;
                if constexpr (MASKED) allowed = Env::mask_bits(st);
                float lp;
                int act;
                if (a.greedy) act = cat_lane_head<HEAD, true>(m, tid, A, allowed, false, 0, 0u, lp);
                else act = cat_lane_head<HEAD, false>(m, tid, A, allowed, false, 0, cat_draw_word(a.seed, ep, (int64_t)ep_len), lp);
                int term;
                const float r = Env::step(st, act, term);
                ep_len += 1;
                ep_rew += r;
                trunc = ep_len == a.max_episode_steps ? 1 : 0;
                if (term || trunc) alive = false;
                if constexpr (!Env::OBS_ONE_HOT) Env::obs(st, ob);
            }
            const unsigned long long live = __ballot(alive);
            if (tid == 0) m.ridx[0] = __popcll(live);
        }
        __syncthreads();   // the live count is published; OUT and the H1 columns are read
        if (m.ridx[0] == 0) break;
        // the next write of the count is behind the next forward's four barriers: every wave has read this one by then
    }
    if (owner) {
        a.ep_return[ep] = ep_rew;
        a.ep_length[ep] = ep_len;
        a.ep_trunc[ep] = trunc;
    }
}

// ---------------------------------------------------------------------------------------------------------
// cat_trunc_fold_kernel<Env> (ppo_env_truncation_bootstrap on an env with STATE_FROM_OBS: PPO_ENV_TAXI): gauss_trunc_fold_kernel's plan for an env whose
// observation is not its state but holds it.  A 256-thread workgroup owns 256 consecutive flat samples.  A lane whose episode reached the limit
// (FIN_LEN[i] == max_episode_steps) decodes OBS[i] to the state (Env::state_of), steps it under ACTIONS[i, 0] (i32; divergent code without a barrier) and
// keeps the sample unless the env terminated on that step.  ONE compaction (fold_compact); a workgroup that keeps none returns before it loads a weight (the
// count is the same in every thread, so the return is uniform).  The kept samples' final STATES (Env::STATE words, not Env::OBS) wait in LDS in list order;
// the critic's weights are staged on gauss_values_kernel's carve, and a tile's X image is the observations of 64 of those states, expanded as it is written.
// gf_forward_tile is gauss_values_kernel's forward, so v is that kernel's value of the final observation, bit for bit -- the critic that fills PPO_BUF_VALUES
// on this family.  Lane k of wave 0 folds row k of the tile (fold_store: two roundings).
// LDS: all dynamic, counted by the launcher (cat_fold_lds_bytes) -- gf_lds_floats(obsP, 4) floats, behind them the kept states [256][STATE] and the row list
// [256] with the waves' totals [8]: 65 024 + 4 096 + 1 056 = 70 176 bytes for PPO_ENV_TAXI, above 64 KB: the attribute is asked for (gf_allow).
// ---------------------------------------------------------------------------------------------------------
struct CfFoldArgs {
    GfShape sh;
    const float* params;
    const float* obs;          // [B, Env::OBS]
    const int32_t* actions;    // [B, 1]
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

template <class Env>
int cat_fold_lds_bytes() {   // every byte of LDS the kernel uses: the attribute is decided on this sum
    return (gf_lds_floats(gf_pad4(Env::OBS), 4) + DEV_FOLD_THREADS * Env::STATE) * (int)sizeof(float) + GF_DEV_FOLD_LIST_INTS * (int)sizeof(int);
}

template <class Env>
__global__ __launch_bounds__(DEV_FOLD_THREADS) void cat_trunc_fold_kernel(CfFoldArgs a) {
    constexpr int OBS = Env::OBS, ST = Env::STATE, OBSP = (OBS + 3) & ~3;
    static_assert(Env::STATE_FROM_OBS, "the fold steps the env from the state behind a stored observation");
    static_assert(DEV_FOLD_THREADS == GF_THREADS, "fold_compact and gf_forward_tile are written for the same workgroup");
    extern __shared__ __attribute__((aligned(16))) float gf_lds[];
    float* fst = gf_lds + gf_lds_floats(OBSP, 4);
    int* list = reinterpret_cast<int*>(fst + DEV_FOLD_THREADS * ST);
    int* wtot = list + DEV_FOLD_THREADS;
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * DEV_FOLD_THREADS + tid;
    bool keep = false;
    float st[ST];
#pragma unroll
    for (int j = 0; j < ST; j++) st[j] = 0.0f;
    if (i < a.B && a.fin_len[i] == a.max_episode_steps) {
        float ob[OBS];
#pragma unroll
        for (int j = 0; j < OBS; j++) ob[j] = a.obs[i * OBS + j];
        Env::state_of(ob, st);
        int terminated;
        (void)Env::step(st, a.actions[i], terminated);
        keep = terminated == 0;
    }
    int pos;
    const int cnt = fold_compact(keep, (int)i, a.ev_count, list, wtot, pos);
    if (cnt == 0) return;
    const int base = wtot[4];
    if (keep) {
#pragma unroll
        for (int j = 0; j < ST; j++) fst[pos * ST + j] = st[j];
    }
    const GfLds m = gf_carve(gf_lds, OBSP, 4);
    gf_stage_weights(m, a.sh, a.params, 0, tid);
    if (tid < 64) {   // the padding rows of the observation image, once
#pragma unroll
        for (int k = OBS; k < OBSP; k++) m.x[k * GF_S + tid] = 0.0f;
    }
    __syncthreads();   // the kept states are complete
    for (int k0 = 0; k0 < cnt; k0 += 64) {
        const int k = k0 + tid;   // tid < 64: this lane's place in the list
        if (tid < 64) {
            float ob[OBS];
#pragma unroll
            for (int j = 0; j < OBS; j++) ob[j] = 0.0f;
            if (k < cnt) {
                float fs[ST];
#pragma unroll
                for (int j = 0; j < ST; j++) fs[j] = fst[k * ST + j];
                Env::obs(fs, ob);
            }
#pragma unroll
            for (int j = 0; j < OBS; j++) m.x[j * GF_S + tid] = ob[j];
        }
        gf_forward_tile(m, 1, tid);
        if (tid < 64 && k < cnt) fold_store(a.rewards, a.gamma, a.ev_index, a.ev_value, a.ev_cap, (int64_t)base + k, list[k], m.o[tid]);
        __syncthreads();   // X and OUT are read: the next tile may overwrite them
    }
}

// ---------------------------------------------------------------------------------------------------------
// cut_state_fold_kernel<Env> (ppo_env_truncation_bootstrap on a context with PPO_KERNEL_ENV_CUT_STATE, every GaussEnv* and CatEnv* trait): cat_trunc_fold_kernel's
// plan on the record the KEEP rollout wrote (step_episode_keep), so nothing is replayed and no action is read.  A 256-thread workgroup owns 256 consecutive
// flat samples.  Every thread reads FIN_LEN[i]; a lane whose episode reached the limit reads column i of the record [STATE + 1, B] -- written by this rollout
// at exactly these samples, so a stale column is never read -- and keeps the sample unless the terminated word is set.  ONE compaction (fold_compact); a
// workgroup that keeps none returns before it loads a weight (the count is the same in every thread, so the return is uniform).  The kept STATES wait in LDS
// in list order; the critic's weights are staged on gauss_values_kernel's carve, and per tile of 64 wave 0's lanes write Env::obs(state) into the X image --
// on an OBS_ONE_HOT env the lane's column is zeroed and the HOT ones set -- so 256 observations are never held.  gf_forward_tile is gauss_values_kernel's
// forward, so v is that kernel's value of the final observation, bit for bit.  Lane k of wave 0 folds row k of the tile (fold_store: two roundings).
// LDS: all dynamic, counted by the launcher (cut_fold_lds_bytes) -- gf_lds_floats(obsP, 4) floats, the kept states [256][STATE], the row list [256] and the
// waves' totals [8]: 54 464 + 528 obsP + 1 024 STATE + 1 056 bytes.  Observation 2 and 3 (STATE 2): 59 680; 6: 63 840; 16: 68 064; 19: 70 176; 45: 84 960;
// 64: 93 408 -- above 64 KB from 16 on: the attribute is asked for (gf_allow).
// ---------------------------------------------------------------------------------------------------------
struct CutFoldArgs {
    GfShape sh;
    const float* params;
    const float* cut;          // [Env::STATE + 1, B]
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

template <class Env>
int cut_fold_lds_bytes() {   // every byte of LDS the kernel uses: the attribute is decided on this sum
    return (gf_lds_floats(gf_pad4(Env::OBS), 4) + DEV_FOLD_THREADS * Env::STATE) * (int)sizeof(float) + GF_DEV_FOLD_LIST_INTS * (int)sizeof(int);
}

template <class Env, bool = Env::OBS_ONE_HOT>
struct CutFoldObs {   // lane `tid` of wave 0 writes the observation of `fs` (valid) or zeros into its column of the X image; padding rows are zero already
    __device__ static __forceinline__ void write(const GfLds& m, int tid, bool valid, const float* fs) {
        float ob[Env::OBS];
#pragma unroll
        for (int j = 0; j < Env::OBS; j++) ob[j] = 0.0f;
        if (valid) Env::obs(fs, ob);
#pragma unroll
        for (int j = 0; j < Env::OBS; j++) m.x[j * GF_S + tid] = ob[j];
    }
};
template <class Env>
struct CutFoldObs<Env, true> {   // one-hot: Env::HOT ones over zeros (Env::hot clamps the state's words, so the rows are inside the image)
    __device__ static __forceinline__ void write(const GfLds& m, int tid, bool valid, const float* fs) {
#pragma unroll
        for (int j = 0; j < Env::OBS; j++) m.x[j * GF_S + tid] = 0.0f;
        if (valid) {
            int rows[Env::HOT];
            Env::hot(fs, rows);
#pragma unroll
            for (int j = 0; j < Env::HOT; j++) m.x[rows[j] * GF_S + tid] = 1.0f;
        }
    }
};

template <class Env>
__global__ __launch_bounds__(DEV_FOLD_THREADS) void cut_state_fold_kernel(CutFoldArgs a) {
    constexpr int OBS = Env::OBS, ST = Env::STATE, OBSP = (OBS + 3) & ~3;
    static_assert(DEV_FOLD_THREADS == GF_THREADS, "fold_compact and gf_forward_tile are written for the same workgroup");
    extern __shared__ __attribute__((aligned(16))) float gf_lds[];
    float* fst = gf_lds + gf_lds_floats(OBSP, 4);
    int* list = reinterpret_cast<int*>(fst + DEV_FOLD_THREADS * ST);
    int* wtot = list + DEV_FOLD_THREADS;
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * DEV_FOLD_THREADS + tid;
    bool keep = false;
    float st[ST];
#pragma unroll
    for (int j = 0; j < ST; j++) st[j] = 0.0f;
    if (i < a.B && a.fin_len[i] == a.max_episode_steps) {
#pragma unroll
        for (int j = 0; j < ST; j++) st[j] = a.cut[(int64_t)j * a.B + i];
        keep = a.cut[(int64_t)ST * a.B + i] == 0.0f;
    }
    int pos;
    const int cnt = fold_compact(keep, (int)i, a.ev_count, list, wtot, pos);
    if (cnt == 0) return;
    const int base = wtot[4];
    if (keep) {
#pragma unroll
        for (int j = 0; j < ST; j++) fst[pos * ST + j] = st[j];
    }
    const GfLds m = gf_carve(gf_lds, OBSP, 4);
    gf_stage_weights(m, a.sh, a.params, 0, tid);
    if (tid < 64) {   // the padding rows of the observation image, once
#pragma unroll
        for (int k = OBS; k < OBSP; k++) m.x[k * GF_S + tid] = 0.0f;
    }
    __syncthreads();   // the kept states are complete
    for (int k0 = 0; k0 < cnt; k0 += 64) {
        const int k = k0 + tid;   // tid < 64: this lane's place in the list
        if (tid < 64) {
            float fs[ST];
#pragma unroll
            for (int j = 0; j < ST; j++) fs[j] = k < cnt ? fst[k * ST + j] : 0.0f;
            CutFoldObs<Env>::write(m, tid, k < cnt, fs);
        }
        gf_forward_tile(m, 1, tid);
        if (tid < 64 && k < cnt) fold_store(a.rewards, a.gamma, a.ev_index, a.ev_value, a.ev_cap, (int64_t)base + k, list[k], m.o[tid]);
        __syncthreads();   // X and OUT are read: the next tile may overwrite them
    }
}

template <typename K>
hipError_t gf_allow(std::atomic<unsigned long long>& done, K kernel, int bytes) {
    return bytes > 64 * 1024 ? allow_dynamic_lds(done, reinterpret_cast<const void*>(kernel)) : hipSuccess;
}

}  // namespace

bool gauss_fused_serves_shape(int obs, int hidden, int n_hidden, int D) { return hidden == 64 && n_hidden == 2 && D >= 1 && D <= PPO_MAX_ACT && obs >= 1 && obs <= GAUSS_FUSED_MAX_OBS; }

int64_t gauss_fused_slab_stride(const GenLayout& L) { return ((int64_t)std::max(L.net_size[0], L.net_size[1] + L.gauss) + 3) & ~3ll; }

hipError_t gauss_fused_act(const GenLayout& L, const float* params, const float* obs, const float* forced, int64_t n, int64_t seed, int64_t row_offset,
                           int64_t step_index, bool greedy, float* action, float* logprob, float* entropy, const GaussStepStores* st, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const GfShape sh = gf_shape(L);
    const int bytes = gf_lds_floats(gf_pad4(L.obs), gf_pad4(L.gauss)) * 4;
    const int64_t tiles = (n + 63) / 64;
    const dim3 grid((unsigned)std::min<int64_t>(tiles, 1024)), block(GF_THREADS);
    GfStepStores ss{};
    if (st) ss = GfStepStores{ st->done_prev, st->obs_t, st->act_t, st->lp_t, st->dones_t };
    static std::atomic<unsigned long long> done_g{ 0 }, done_s{ 0 };
    if (greedy) {
        const hipError_t e = gf_allow(done_g, gauss_act_kernel<true>, bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(gauss_act_kernel<true>, grid, block, bytes, s, sh, params, obs, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss);
    } else {
        const hipError_t e = gf_allow(done_s, gauss_act_kernel<false>, bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(gauss_act_kernel<false>, grid, block, bytes, s, sh, params, obs, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss);
    }
    return hipGetLastError();
}

hipError_t gauss_fused_values(const GenLayout& L, const float* params, const float* obs, int64_t n, float* value, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const GfShape sh = gf_shape(L);
    const int bytes = gf_lds_floats(gf_pad4(L.obs), 4) * 4;
    const int64_t tiles = (n + 63) / 64;
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, gauss_values_kernel, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gauss_values_kernel, dim3((unsigned)std::min<int64_t>(tiles, 1024)), dim3(GF_THREADS), bytes, s, sh, params, obs, n, value);
    return hipGetLastError();
}

hipError_t gauss_fused_dev_fold(const GenLayout& L, const float* params, const DevFoldArgs& a, hipStream_t s) {
    if (a.N <= 0) return hipSuccess;
    const GfShape sh = gf_shape(L);
    // the row list and the waves' totals are part of the dynamic allocation: the attribute is decided on every byte of LDS the kernel uses
    const int bytes = gf_lds_floats(gf_pad4(L.obs), 4) * 4 + GF_DEV_FOLD_LIST_INTS * (int)sizeof(int);
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, gauss_dev_fold_kernel, bytes);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)(((int64_t)a.N + DEV_FOLD_THREADS - 1) / DEV_FOLD_THREADS);
    hipLaunchKernelGGL(gauss_dev_fold_kernel, dim3(grid), dim3(DEV_FOLD_THREADS), bytes, s, sh, params, a);
    return hipGetLastError();
}

hipError_t gauss_fused_fwd_bwd(const GenLayout& L, const LossParams& hp, const float* params, const float* obs, const float* actions, const float* oldlp,
                               const float* adv, const float* ret, const float* oldv, const int32_t* idx, int64_t M, double inv_global_M, double global_M,
                               const AdvStat* adv_stat, float* slab, double* loss_part, float* grads, hipStream_t s) {
    if (M < 1 || M >= (1ll << 31) - 64 || !slab || !loss_part) return hipErrorInvalidValue;
    GfUpdArgs a{};
    a.sh = gf_shape(L);
    a.hp = hp;
    a.params = params; a.obs = obs; a.actions = actions; a.oldlp = oldlp; a.adv = adv; a.ret = ret; a.oldv = oldv; a.idx = idx;
    a.M = (int)M;
    a.invM = (float)inv_global_M;
    a.adv_stat = (adv_stat && hp.norm_adv) ? adv_stat : nullptr;
    a.global_M = global_M;
    a.slab = slab;
    a.slab_stride = (int)gauss_fused_slab_stride(L);
    a.nb = (int)std::min<int64_t>((M + 63) / 64, GAUSS_FUSED_MAX_BLOCKS);
    a.loss_part = loss_part;
    const int bytes = gf_lds_floats(gf_pad4(L.obs), gf_pad4(L.gauss)) * 4;
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, gauss_fwd_bwd_kernel, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gauss_fwd_bwd_kernel, dim3(a.nb, 2), dim3(GF_THREADS), bytes, s, a);
    hipLaunchKernelGGL(gauss_slab_reduce_kernel, dim3((L.P + 255) / 256), dim3(256), 0, s, slab, a.slab_stride, a.nb, L.net_off[1], L.P, grads);
    return hipGetLastError();
}

// ---- PPO_KERNEL_CAT_FUSED: categorical / masked multi-head policies on the same forward (the critic is gauss_fused_values: with L.gauss = 0 no log_std is read) ----
bool cat_fused_serves_shape(int obs, int hidden, int n_hidden, int A) { return hidden == 64 && n_hidden == 2 && A >= 1 && A <= PPO_MAX_ACT && obs >= 1 && obs <= GAUSS_FUSED_MAX_OBS; }

template <int DIST, bool GREEDY>
static hipError_t cat_fused_act_launch(const GfShape& sh, int bytes, dim3 grid, const float* params, const float* obs, const uint8_t* mask, const int64_t* forced, int64_t n,
                                       int64_t seed, int64_t row_offset, int64_t step_index, int64_t* action, float* logprob, float* entropy, const CfStepStores& ss,
                                       hipStream_t s) {
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, cat_act_kernel<DIST, GREEDY>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((cat_act_kernel<DIST, GREEDY>), grid, dim3(GF_THREADS), bytes, s, sh, params, obs, mask, forced, n, seed, row_offset, step_index, action, logprob,
                       entropy, ss);
    return hipGetLastError();
}

hipError_t cat_fused_act(const GenLayout& L, int dist_kind, const float* params, const float* obs, const uint8_t* mask, const int64_t* forced, int64_t n, int64_t seed,
                         int64_t row_offset, int64_t step_index, bool greedy, int64_t* action, float* logprob, float* entropy, const CatStepStores* st, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (L.gauss || (dist_kind != PPO_DIST_CATEGORICAL && dist_kind != PPO_DIST_MASKED)) return hipErrorInvalidValue;
    const GfShape sh = gf_shape(L);
    const int bytes = gf_lds_floats(gf_pad4(L.obs), gf_pad4(L.act)) * 4;
    const dim3 grid((unsigned)std::min<int64_t>((n + 63) / 64, 1024));
    CfStepStores ss{};
    if (st) ss = CfStepStores{ st->done_prev, st->obs_t, st->mask_t, st->act_t, st->lp_t, st->dones_t };
    const bool masked = dist_kind == PPO_DIST_MASKED;
    if (greedy)
        return masked ? cat_fused_act_launch<PPO_DIST_MASKED, true>(sh, bytes, grid, params, obs, mask, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss, s)
                      : cat_fused_act_launch<PPO_DIST_CATEGORICAL, true>(sh, bytes, grid, params, obs, mask, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss, s);
    return masked ? cat_fused_act_launch<PPO_DIST_MASKED, false>(sh, bytes, grid, params, obs, mask, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss, s)
                  : cat_fused_act_launch<PPO_DIST_CATEGORICAL, false>(sh, bytes, grid, params, obs, mask, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss, s);
}

hipError_t cat_fused_fwd_bwd(const GenLayout& L, const LossParams& hp, const float* params, const float* obs, const int32_t* actions, const uint8_t* masks,
                             const float* oldlp, const float* adv, const float* ret, const float* oldv, const int32_t* idx, int64_t M, double inv_global_M,
                             double global_M, const AdvStat* adv_stat, float* slab, double* loss_part, float* grads, hipStream_t s) {
    if (M < 1 || M >= (1ll << 31) - 64 || !slab || !loss_part || L.gauss) return hipErrorInvalidValue;
    if (hp.dist_kind != PPO_DIST_CATEGORICAL && hp.dist_kind != PPO_DIST_MASKED) return hipErrorInvalidValue;
    GfUpdArgs a{};
    a.sh = gf_shape(L);
    a.hp = hp;
    a.params = params; a.obs = obs; a.actions = reinterpret_cast<const float*>(actions); a.oldlp = oldlp; a.adv = adv; a.ret = ret; a.oldv = oldv; a.idx = idx;
    a.masks = hp.dist_kind == PPO_DIST_MASKED ? masks : nullptr;
    a.M = (int)M;
    a.invM = (float)inv_global_M;
    a.adv_stat = (adv_stat && hp.norm_adv) ? adv_stat : nullptr;
    a.global_M = global_M;
    a.slab = slab;
    a.slab_stride = (int)gauss_fused_slab_stride(L);
    a.nb = (int)std::min<int64_t>((M + 63) / 64, GAUSS_FUSED_MAX_BLOCKS);
    a.loss_part = loss_part;
    const int bytes = gf_lds_floats(gf_pad4(L.obs), gf_pad4(L.act)) * 4;
    static std::atomic<unsigned long long> done_c{ 0 }, done_m{ 0 };
    if (hp.dist_kind == PPO_DIST_MASKED) {
        const hipError_t e = gf_allow(done_m, cat_fwd_bwd_kernel<PPO_DIST_MASKED>, bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(cat_fwd_bwd_kernel<PPO_DIST_MASKED>, dim3(a.nb, 2), dim3(GF_THREADS), bytes, s, a);
    } else {
        const hipError_t e = gf_allow(done_c, cat_fwd_bwd_kernel<PPO_DIST_CATEGORICAL>, bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(cat_fwd_bwd_kernel<PPO_DIST_CATEGORICAL>, dim3(a.nb, 2), dim3(GF_THREADS), bytes, s, a);
    }
    hipLaunchKernelGGL(gauss_slab_reduce_kernel, dim3((L.P + 255) / 256), dim3(256), 0, s, slab, a.slab_stride, a.nb, L.net_off[1], L.P, grads);
    return hipGetLastError();
}

// ---- the device envs of the two fused families (gauss_fused.hpp; the context's shape is fixed by ppo_ctx_create from the env's row: obs Env::OBS, one head of
// Env::ACTIONS logits, or D = 1) ----
// env_kind -> trait: f is called with a value of the env's trait type; an env without one gives hipErrorInvalidValue
template <class F>
static hipError_t gauss_env_dispatch(int env_kind, F f) {
    if (env_kind == PPO_ENV_PENDULUM) return f(GaussEnvPendulum{});
    if (env_kind == PPO_ENV_MOUNTAINCAR_CONTINUOUS) return f(GaussEnvMountainCarContinuous{});
    return hipErrorInvalidValue;
}
template <class F>
static hipError_t cat_env_dispatch(int env_kind, F f) {
    if (env_kind == PPO_ENV_ACROBOT) return f(CatEnvAcrobot{});
    if (env_kind == PPO_ENV_TAXI) return f(CatEnvTaxi{});
    if (env_kind == PPO_ENV_FROZENLAKE) return f(CatEnvFrozenLake<4>{});
    if (env_kind == PPO_ENV_FROZENLAKE8X8) return f(CatEnvFrozenLake<8>{});
    if (env_kind == PPO_ENV_BLACKJACK) return f(CatEnvBlackjack{});
    return hipErrorInvalidValue;
}

// One row per line of the two dispatchers.  A Gaussian env folds and evaluates where its observation is its state; a categorical env folds where the
// observation holds the state, and every one evaluates.
template <class Env>
static constexpr FusedEnvInfo gauss_env_row(int kind, const char* name, int max_steps, FusedEnvTexts t) {
    return { kind, name, FUSED_GAUSS, Env::OBS, Env::STATE, 1, 1u << PPO_DIST_GAUSSIAN, Env::OBS_IS_STATE, Env::OBS_IS_STATE, Env::OBS_IS_STATE, max_steps,
             t, {} };
}
template <class Env>
static constexpr FusedEnvInfo cat_env_row(int kind, const char* name, int max_steps, FusedEnvTexts t, FusedStateCheck c = {}) {
    static_assert(Env::STATE == 4, "FusedStateCheck::hi");
    return { kind, name, FUSED_CAT, Env::OBS, Env::STATE, Env::ACTIONS, 1u << PPO_DIST_CATEGORICAL | (Env::HAS_MASK ? 1u << PPO_DIST_MASKED : 0u),
             Env::OBS_IS_STATE, Env::STATE_FROM_OBS, true, max_steps, t, c };
}
// hand = t + 32 * ace + 64 * show: t in 2..31, show in 1..10; no bits above: hand <= BLACKJACK_HAND_MAX
static bool blackjack_word_ok(int word, int value) { return word != 0 || ((value & 31) >= 2 && (value >> 6) >= 1); }
static_assert(FROZENLAKE_WORD_MAX == 16777215 && BLACKJACK_WORD_MAX == 16777215, "the rows' FusedStateCheck::words");

static const FusedEnvInfo fused_env_rows[] = {
    gauss_env_row<GaussEnvPendulum>(PPO_ENV_PENDULUM, "PPO_ENV_PENDULUM", PENDULUM_MAX_EPISODE_STEPS,
        { "one real-valued action", "one action dimension, the torque", "the angle is not wrapped and the device sinf / cosf hold for |theta| < 120",
          "PPO_ENV_PENDULUM observation (cos, sin, theta_dot) does not hold theta" }),
    gauss_env_row<GaussEnvMountainCarContinuous>(PPO_ENV_MOUNTAINCAR_CONTINUOUS, "PPO_ENV_MOUNTAINCAR_CONTINUOUS", 0,
        { "one real-valued action", "one action dimension, the force", "an episode that never reaches the goal ends at the time limit only", nullptr }),
    cat_env_row<CatEnvAcrobot>(PPO_ENV_ACROBOT, "PPO_ENV_ACROBOT", 0,
        { "one of three discrete actions without a mask", "one head of three actions, the torque -1, 0 or +1",
          "an episode that never swings up ends at the time limit only",
          "PPO_ENV_ACROBOT observation (cos, sin of two angles, two velocities) does not hold the angles" }),
    cat_env_row<CatEnvTaxi>(PPO_ENV_TAXI, "PPO_ENV_TAXI", 0,
        { "one of six discrete actions, drawn under the env's action mask or without it", "one head of six actions (south, north, east, west, pickup, dropoff)",
          "an episode that never delivers the passenger ends at the time limit only", nullptr },
        { "PPO_ENV_TAXI: row, col, pass in 0..4, dest in 0..3", { 4, 4, 4, 3 }, nullptr }),
    // both maps say "PPO_ENV_FROZENLAKE" where they speak of the observation and of the state
    cat_env_row<CatEnvFrozenLake<4>>(PPO_ENV_FROZENLAKE, "PPO_ENV_FROZENLAKE", FROZENLAKE_WORD_MAX,
        { "one of four discrete actions without a mask", "one head of four actions (left, down, right, up)",
          "the episode's step count is a state word held exactly in f32, and it keys the env's draws",
          "PPO_ENV_FROZENLAKE observation (the one-hot of the cell) holds neither the step count nor the key the env's slip is drawn from" },
        { "PPO_ENV_FROZENLAKE: cell in 0..15; j, k0, k1 in 0..16777215", { CatEnvFrozenLake<4>::OBS - 1, FROZENLAKE_WORD_MAX, FROZENLAKE_WORD_MAX, FROZENLAKE_WORD_MAX },
          nullptr }),
    cat_env_row<CatEnvFrozenLake<8>>(PPO_ENV_FROZENLAKE8X8, "PPO_ENV_FROZENLAKE8X8", FROZENLAKE_WORD_MAX,
        { "one of four discrete actions without a mask", "one head of four actions (left, down, right, up)",
          "the episode's step count is a state word held exactly in f32, and it keys the env's draws",
          "PPO_ENV_FROZENLAKE observation (the one-hot of the cell) holds neither the step count nor the key the env's slip is drawn from" },
        { "PPO_ENV_FROZENLAKE: cell in 0..63; j, k0, k1 in 0..16777215", { CatEnvFrozenLake<8>::OBS - 1, FROZENLAKE_WORD_MAX, FROZENLAKE_WORD_MAX, FROZENLAKE_WORD_MAX },
          nullptr }),
    cat_env_row<CatEnvBlackjack>(PPO_ENV_BLACKJACK, "PPO_ENV_BLACKJACK", BLACKJACK_WORD_MAX,
        { "one of two discrete actions without a mask", "one head of two actions (stick, hit)",
          "as on PPO_ENV_FROZENLAKE: the state's words are integers held exactly in f32",
          "PPO_ENV_BLACKJACK observation (the player's sum, the dealer's showing card, the usable ace) holds neither the card count nor the key the env's cards "
          "are drawn from" },
        { "PPO_ENV_BLACKJACK: hand = t + 32 * ace + 64 * show with t in 2..31, ace in 0..1, show in 1..10; n, k0, k1 in 0..16777215",
          { BLACKJACK_HAND_MAX, BLACKJACK_WORD_MAX, BLACKJACK_WORD_MAX, BLACKJACK_WORD_MAX }, blackjack_word_ok }),
};
const char* fused_env_names(FusedFamily family) {
    return family == FUSED_GAUSS ? "PPO_ENV_PENDULUM and PPO_ENV_MOUNTAINCAR_CONTINUOUS"
                                 : "PPO_ENV_ACROBOT, PPO_ENV_TAXI, the two PPO_ENV_FROZENLAKE kinds and PPO_ENV_BLACKJACK";
}

const FusedEnvInfo* fused_env_info(int env_kind) {
    for (const FusedEnvInfo& e : fused_env_rows)
        if (e.env_kind == env_kind) return &e;
    return nullptr;
}

// the family's dispatcher: fg is called with a GaussEnv* trait, fc with a CatEnv* one
template <class FG, class FC>
static hipError_t fused_env_dispatch(int env_kind, FG fg, FC fc) {
    const FusedEnvInfo* e = fused_env_info(env_kind);
    if (!e) return hipErrorInvalidValue;
    return e->family == FUSED_GAUSS ? gauss_env_dispatch(env_kind, fg) : cat_env_dispatch(env_kind, fc);
}

template <class Env>
static bool gauss_env_shape_ok(const GenLayout& L) { return L.obs == Env::OBS && L.gauss == 1; }
template <class Env>
static bool cat_env_shape_ok(const GenLayout& L) { return L.obs == Env::OBS && L.gauss == 0 && L.n_heads == 1 && L.act == Env::ACTIONS; }
// a masked policy runs on an env that forms a mask, and on no other (ppo_ctx_create)
template <class Env>
static bool cat_env_dist_ok(int dist_kind) { return dist_kind == PPO_DIST_CATEGORICAL || (dist_kind == PPO_DIST_MASKED && Env::HAS_MASK); }
template <class Env>
static int cat_env_lds_bytes() { return gf_lds_floats(gf_pad4(Env::OBS), gf_pad4(Env::ACTIONS)) * 4; }

// the kernels' argument structs from the launchers' (GfRolloutArgs / CfRolloutArgs, GfFoldArgs / CfFoldArgs: the same fields, the family's action types)
template <class KernelArgs>
static KernelArgs rollout_kernel_args(const GenLayout& L, const FusedRolloutArgs& r) {
    KernelArgs a{};
    a.sh = gf_shape(L);
    a.params = r.params;
    a.N = r.N; a.T = r.T; a.max_episode_steps = r.max_episode_steps;
    a.seed = r.seed; a.env_offset = r.env_offset; a.step_base = r.step_base;
    a.env_state = r.env_state; a.ep_len = r.ep_len; a.ep_rew = r.ep_rew; a.reset_count = r.reset_count;
    a.obs = r.obs; a.actions = static_cast<decltype(a.actions)>(r.actions); a.logprobs = r.logprobs; a.rewards = r.rewards; a.dones = r.dones;
    a.fin_len = r.fin_len; a.fin_rew = r.fin_rew;
    a.next_obs = r.next_obs; a.next_done = r.next_done; a.forced = static_cast<decltype(a.forced)>(r.forced);
    a.cut = r.cut;
    return a;
}
template <class KernelArgs>
static KernelArgs fold_kernel_args(const GenLayout& L, const FusedFoldArgs& f) {
    KernelArgs a{};
    a.sh = gf_shape(L);
    a.params = f.params; a.obs = f.obs; a.actions = static_cast<decltype(a.actions)>(f.actions); a.fin_len = f.fin_len;
    a.B = f.B; a.max_episode_steps = f.max_episode_steps; a.gamma = f.gamma;
    a.rewards = f.rewards; a.ev_count = f.ev_count; a.ev_index = f.ev_index; a.ev_value = f.ev_value; a.ev_cap = f.ev_cap;
    return a;
}
static GfEvalArgs eval_kernel_args(const GenLayout& L, const FusedEvalArgs& e) {
    GfEvalArgs a{};
    a.sh = gf_shape(L);
    a.params = e.params;
    a.n_episodes = e.n_episodes; a.seed = e.seed;
    a.max_episode_steps = e.max_episode_steps; a.greedy = e.greedy != 0;
    a.ep_return = e.ep_return; a.ep_length = e.ep_length; a.ep_trunc = e.ep_trunc;
    return a;
}

template <class Env, bool KEEP>
static hipError_t gauss_rollout_launch(const GenLayout& L, const FusedRolloutArgs& r, hipStream_t s) {
    if (!gauss_env_shape_ok<Env>(L)) return hipErrorInvalidValue;
    const GfRolloutArgs a = rollout_kernel_args<GfRolloutArgs>(L, r);
    const int bytes = gf_lds_floats(4, 4) * 4;
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, gauss_rollout_kernel<Env, KEEP>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((gauss_rollout_kernel<Env, KEEP>), dim3((unsigned)((r.N + 63) / 64)), dim3(GF_THREADS), bytes, s, a);
    return hipGetLastError();
}
// cat_rollout_kernel<Env, DIST> for the context's distribution; the attribute where the carve passes 64 KB (PPO_ENV_TAXI: 67 136 bytes; PPO_ENV_FROZENLAKE8X8: 88 256; PPO_ENV_BLACKJACK: 79 808)
// KEEP (a context with PPO_KERNEL_ENV_CUT_STATE): the instantiation that also writes the cut-off record; a.cut is null exactly where KEEP is false
template <class Env, int DIST, bool KEEP>
static hipError_t cat_rollout_launch_keep(const CfRolloutArgs& a, int N, hipStream_t s) {
    const int bytes = cat_env_lds_bytes<Env>();
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, cat_rollout_kernel<Env, DIST, KEEP>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((cat_rollout_kernel<Env, DIST, KEEP>), dim3((unsigned)((N + 63) / 64)), dim3(GF_THREADS), bytes, s, a);
    return hipGetLastError();
}
template <class Env, int DIST>
static hipError_t cat_rollout_launch(const CfRolloutArgs& a, int N, hipStream_t s) {
    return a.cut ? cat_rollout_launch_keep<Env, DIST, true>(a, N, s) : cat_rollout_launch_keep<Env, DIST, false>(a, N, s);
}
template <class Env, int DIST>
static hipError_t cat_eval_launch(const GfEvalArgs& a, hipStream_t s) {
    const int bytes = cat_env_lds_bytes<Env>();
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, cat_eval_kernel<Env, DIST>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((cat_eval_kernel<Env, DIST>), dim3((unsigned)((a.n_episodes + 63) / 64)), dim3(GF_THREADS), bytes, s, a);
    return hipGetLastError();
}

hipError_t launch_fused_env_rollout(int env_kind, int dist_kind, const GenLayout& L, const FusedRolloutArgs& r, hipStream_t s) {
    if (r.N <= 0 || r.T <= 0) return hipSuccess;
    return fused_env_dispatch(env_kind, [&](auto env) {
        return r.cut ? gauss_rollout_launch<decltype(env), true>(L, r, s) : gauss_rollout_launch<decltype(env), false>(L, r, s);
    }, [&](auto env) {
        using Env = decltype(env);
        if (!cat_env_shape_ok<Env>(L) || !cat_env_dist_ok<Env>(dist_kind)) return hipErrorInvalidValue;
        CfRolloutArgs a = rollout_kernel_args<CfRolloutArgs>(L, r);
        a.masks = r.masks;
        if constexpr (Env::HAS_MASK) {
            if (dist_kind == PPO_DIST_MASKED) return cat_rollout_launch<Env, PPO_DIST_MASKED>(a, r.N, s);
        }
        return cat_rollout_launch<Env, PPO_DIST_CATEGORICAL>(a, r.N, s);
    });
}

// the fold exists for the envs whose stored observation holds the state
hipError_t fused_env_trunc_fold(int env_kind, const GenLayout& L, const FusedFoldArgs& f, hipStream_t s) {
    if (f.B <= 0 || f.max_episode_steps <= 0) return hipSuccess;   // no limit: no episode is ever cut off
    if (f.B >= (1ll << 31)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((f.B + DEV_FOLD_THREADS - 1) / DEV_FOLD_THREADS);
    if (f.cut) {   // PPO_KERNEL_ENV_CUT_STATE: every env of either family folds from the record its rollout kept
        auto from_record = [&](auto env, bool shape_ok) {
            using Env = decltype(env);
            if (!shape_ok) return hipErrorInvalidValue;
            CutFoldArgs a{};
            a.sh = gf_shape(L);
            a.params = f.params; a.cut = f.cut; a.fin_len = f.fin_len;
            a.B = f.B; a.max_episode_steps = f.max_episode_steps; a.gamma = f.gamma;
            a.rewards = f.rewards; a.ev_count = f.ev_count; a.ev_index = f.ev_index; a.ev_value = f.ev_value; a.ev_cap = f.ev_cap;
            const int bytes = cut_fold_lds_bytes<Env>();
            static std::atomic<unsigned long long> done{ 0 };
            const hipError_t e = gf_allow(done, cut_state_fold_kernel<Env>, bytes);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(cut_state_fold_kernel<Env>, dim3(grid), dim3(DEV_FOLD_THREADS), bytes, s, a);
            return hipGetLastError();
        };
        return fused_env_dispatch(env_kind, [&](auto env) { return from_record(env, gauss_env_shape_ok<decltype(env)>(L)); },
                                  [&](auto env) { return from_record(env, cat_env_shape_ok<decltype(env)>(L)); });
    }
    return fused_env_dispatch(env_kind, [&](auto env) {
        using Env = decltype(env);
        if constexpr (Env::OBS_IS_STATE) {
            if (!gauss_env_shape_ok<Env>(L)) return hipErrorInvalidValue;
            const int bytes = gf_lds_floats(4, 4) * 4;
            hipLaunchKernelGGL(gauss_trunc_fold_kernel<Env>, dim3(grid), dim3(DEV_FOLD_THREADS), bytes, s, fold_kernel_args<GfFoldArgs>(L, f));
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }, [&](auto env) {
        using Env = decltype(env);
        if constexpr (Env::STATE_FROM_OBS) {
            if (!cat_env_shape_ok<Env>(L)) return hipErrorInvalidValue;
            const int bytes = cat_fold_lds_bytes<Env>();
            static std::atomic<unsigned long long> done{ 0 };
            const hipError_t e = gf_allow(done, cat_trunc_fold_kernel<Env>, bytes);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(cat_trunc_fold_kernel<Env>, dim3(grid), dim3(DEV_FOLD_THREADS), bytes, s, fold_kernel_args<CfFoldArgs>(L, f));
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    });
}

// the Gaussian evaluation exists for the envs whose observation is their state
hipError_t fused_env_evaluate(int env_kind, int dist_kind, const GenLayout& L, const FusedEvalArgs& e, hipStream_t s) {
    if (e.n_episodes <= 0) return hipSuccess;
    if (e.max_episode_steps < 1 || e.n_episodes >= (1ll << 31) * 64 || !e.ep_return || !e.ep_length || !e.ep_trunc) return hipErrorInvalidValue;
    return fused_env_dispatch(env_kind, [&](auto env) {
        using Env = decltype(env);
        if constexpr (Env::OBS_IS_STATE) {
            if (!gauss_env_shape_ok<Env>(L)) return hipErrorInvalidValue;
            const int bytes = gf_lds_floats(4, 4) * 4;
            hipLaunchKernelGGL(gauss_eval_kernel<Env>, dim3((unsigned)((e.n_episodes + 63) / 64)), dim3(GF_THREADS), bytes, s, eval_kernel_args(L, e));
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }, [&](auto env) {
        using Env = decltype(env);
        if (!cat_env_shape_ok<Env>(L) || !cat_env_dist_ok<Env>(dist_kind)) return hipErrorInvalidValue;
        const GfEvalArgs a = eval_kernel_args(L, e);
        if constexpr (Env::HAS_MASK) {
            if (dist_kind == PPO_DIST_MASKED) return cat_eval_launch<Env, PPO_DIST_MASKED>(a, s);
        }
        return cat_eval_launch<Env, PPO_DIST_CATEGORICAL>(a, s);
    });
}

hipError_t launch_fused_env_reset(int env_kind, int N, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew, int32_t* reset_count,
                                  float* next_obs, int32_t* next_done, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    return fused_env_dispatch(env_kind, [&](auto env) {
        hipLaunchKernelGGL(gauss_env_reset_kernel<decltype(env)>, dim3((N + 255) / 256), dim3(256), 0, s, N, seed, env_offset, env_state, ep_len, ep_rew, reset_count,
                           next_obs, next_done);
        return hipGetLastError();
    }, [&](auto env) {
        hipLaunchKernelGGL(cat_env_reset_kernel<decltype(env)>, dim3((N + 255) / 256), dim3(256), 0, s, N, seed, env_offset, env_state, ep_len, ep_rew, reset_count,
                           next_obs, next_done);
        return hipGetLastError();
    });
}
hipError_t launch_fused_env_obs(int env_kind, int N, const float* env_state, float* next_obs, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    return fused_env_dispatch(env_kind, [&](auto env) {
        hipLaunchKernelGGL(gauss_env_obs_kernel<decltype(env)>, dim3((N + 255) / 256), dim3(256), 0, s, N, env_state, next_obs);
        return hipGetLastError();
    }, [&](auto env) {
        hipLaunchKernelGGL(cat_env_obs_kernel<decltype(env)>, dim3((N + 255) / 256), dim3(256), 0, s, N, env_state, next_obs);
        return hipGetLastError();
    });
}
hipError_t launch_gauss_env_step(int env_kind, int N, int max_episode_steps, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew,
                                 int32_t* reset_count, const float* action, float* obs, float* reward, int32_t* done, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    return gauss_env_dispatch(env_kind, [&](auto env) {
        hipLaunchKernelGGL(gauss_env_step_kernel<decltype(env)>, dim3((N + 255) / 256), dim3(256), 0, s, N, max_episode_steps, seed, env_offset, env_state, ep_len,
                           ep_rew, reset_count, action, obs, reward, done);
        return hipGetLastError();
    });
}
hipError_t launch_cat_env_step(int env_kind, int N, int max_episode_steps, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew,
                               int32_t* reset_count, const int64_t* action, float* obs, float* reward, int32_t* done, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    return cat_env_dispatch(env_kind, [&](auto env) {
        hipLaunchKernelGGL(cat_env_step_kernel<decltype(env)>, dim3((N + 255) / 256), dim3(256), 0, s, N, max_episode_steps, seed, env_offset, env_state, ep_len,
                           ep_rew, reset_count, action, obs, reward, done);
        return hipGetLastError();
    });
}
hipError_t launch_gauss_env_transition(int env_kind, const float* state_in, const float* action, int64_t n, float* next_state, float* obs_out, float* reward,
                                       int32_t* terminated, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n >= (1ll << 31) * 256) return hipErrorInvalidValue;
    return gauss_env_dispatch(env_kind, [&](auto env) {
        hipLaunchKernelGGL(gauss_env_transition_kernel<decltype(env)>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, state_in, action, n, next_state, obs_out,
                           reward, terminated);
        return hipGetLastError();
    });
}
hipError_t launch_cat_env_transition(int env_kind, const float* state_in, const int64_t* action, int64_t n, float* next_state, float* reward, int32_t* terminated,
                                     hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n >= (1ll << 31) * 256) return hipErrorInvalidValue;
    return cat_env_dispatch(env_kind, [&](auto env) {
        hipLaunchKernelGGL(cat_env_transition_kernel<decltype(env)>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, state_in, action, n, next_state, reward,
                           terminated);
        return hipGetLastError();
    });
}
