// ppo-libtorch_amd/csrc/gauss_fused_dev.hpp -- the device functions of the fused 2 x 64 family (PPO_KERNEL_GAUSS_FUSED / PPO_KERNEL_CAT_FUSED) that its two
// kernel files share: kernels_gauss_fused.hip (W1 and the whole X image resident in LDS, obs_size <= GAUSS_FUSED_MAX_OBS) and kernels_fused_wide.hip
// (PPO_KERNEL_FUSED_WIDE_OBS: layer 1 streamed in K-chunks).  The carve, the weight staging, the layers, the heads' and the loss lanes' arithmetic and the
// backward's tile functions are written once, here; a kernel file adds its kernels and launchers.  Included by those two files and by
// kernels_fused_matrix.hip (PPO_KERNEL_FUSED_MATRIX: the same plan with the 64-wide products on the matrix cores) and, through fused_matrix_dev.hpp, by
// kernels_env_matrix.hip (PPO_KERNEL_ENV_MATRIX: the device envs' one-launch rollouts behind that forward).
#pragma once
#include <algorithm>

#include "generic.hpp"
#include "gauss_dist.hpp"
#include "gauss_fused.hpp"

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

inline GfShape gf_shape(const GenLayout& L) {
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

// one net's layers 2 and 3, the biases, log_std and exp(-log_std) into LDS (zero padded): everything of the net but W1
__device__ __forceinline__ void gf_stage_upper(const GfLds& m, const GfShape& sh, const float* __restrict__ params, int net, int tid) {
    const int out = net == 0 ? 1 : sh.A;
    const float* W2 = params + sh.off[net][2];
    const float* W3 = params + sh.off[net][4];
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

// one net's weights into LDS (zero padded), log_std and exp(-log_std); every thread of the workgroup calls it; the caller's next barrier publishes it
__device__ __forceinline__ void gf_stage_weights(const GfLds& m, const GfShape& sh, const float* __restrict__ params, int net, int tid) {
    const int obs = sh.obs, obsP = m.obsP;
    const float* W1 = params + sh.off[net][0];
    for (int i = tid; i < 64 * obsP; i += GF_THREADS) {
        const int u = i / obsP, k = i - u * obsP;
        m.w1[i] = k < obs ? W1[u * obs + k] : 0.0f;
    }
    gf_stage_upper(m, sh, params, net, tid);
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

// the output layer: H2 (post-tanh, complete behind the caller's barrier) -> OUT rows 0 .. out - 1; wave w owns units w, w + 4, ... (< out <= 32)
__device__ __forceinline__ void gf_output_layer(const GfLds& m, int out, int s, int w) {
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

// layers 2 and 3 of the forward pass: H1 (post-tanh, complete behind the caller's barrier) -> H2 -> OUT rows 0 .. out - 1; a barrier behind each layer
__device__ __forceinline__ void gf_forward_upper(const GfLds& m, int out, int s, int w) {
    gf_hidden_layer(m.w2, m.b2, m.h1, m.h2, 64, s, w);
    __syncthreads();
    gf_output_layer(m, out, s, w);
    __syncthreads();
}

// THE forward pass of the resident kernels: the tile in m.x through obs -> 64 -> 64 -> out; leaves H1, H2 (post-tanh) and OUT rows 0 .. out - 1.
// Every thread of the workgroup calls it; barriers: one at entry (m.x and the weights are complete), one behind every layer.
__device__ __forceinline__ void gf_forward_tile(const GfLds& m, int out, int tid) {
    const int s = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    __syncthreads();
    gf_hidden_layer(m.w1, m.b1, m.x, m.h1, m.obsP, s, w);
    __syncthreads();
    gf_forward_upper(m, out, s, w);
}

// rows row0 .. row0 + 63 of a dense batch of n
__device__ __forceinline__ void gf_dense_rows(const GfLds& m, int64_t row0, int64_t n, int tid) {
    if (tid < 64) m.ridx[tid] = row0 + tid < n ? (int)(row0 + tid) : -1;
    __syncthreads();
}

// ---- layer 1 in chunks of GW_K observation columns (kernels_fused_wide.hip, kernels_fused_matrix.hip): the tile's X image one chunk at a time; a thread owns
// 16 elements of a chunk (element tid + 256 j: column 64 c + (tid & 63) of sample (tid >> 6) + 4 j -- a wave reads 64 consecutive floats of a row) ----
constexpr int GW_K = FUSED_WIDE_CHUNK;
__device__ __forceinline__ int gw_chunks(int O) { return (O + GW_K - 1) / GW_K; }
// chunk c of the tile's observations: rows ridx[s] of obs [., O]; zeros for a sample without a row (ridx < 0) and behind column O
__device__ __forceinline__ void gw_fetch_x(const float* __restrict__ obs, int O, const int* ridx, int c, int tid, float (&r)[16]) {
    const int k = GW_K * c + (tid & 63), s0 = tid >> 6;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int row = ridx[s0 + 4 * j];
        r[j] = (k < O && row >= 0) ? obs[(int64_t)row * O + k] : 0.0f;
    }
}
// ... as the [k][sample] image of the chunk
__device__ __forceinline__ void gw_store_x(float* __restrict__ x, int tid, const float (&r)[16]) {
    const int k = tid & 63, s0 = tid >> 6;
#pragma unroll
    for (int j = 0; j < 16; j++) x[k * GF_S + s0 + 4 * j] = r[j];
}

// columns of chunk c that take part in a product: 64, or what is left of O rounded up to 4 (the padding columns hold zeros on both sides)
__device__ __forceinline__ int gw_chunk_cols(int O, int c) {
    const int left = gf_pad4(O - GW_K * c);
    return left < GW_K ? left : GW_K;
}

// ---------------------------------------------------------------------------------------------------------
// The act kernels' work behind the forward (the mean / the logits of the tile are in OUT): wave 0, lane = row, does the heads; waves 1 .. 3 the step's
// other stores.  The caller's next barrier frees OUT, the H1 columns and the row list.
// ---------------------------------------------------------------------------------------------------------
struct GfStepStores { const int32_t* done_prev; float* obs_t; float* act_t; float* lp_t; float* dones_t; };

// gauss_heads_kernel's sample / log-prob / entropy (the same device functions, gauss_dist.hpp) + the rollout stores of the step (gauss_store_step_kernel's;
// st.obs_t == nullptr: the stand-alone policy, none)
template <bool GREEDY>
__device__ __forceinline__ void gauss_act_rows(const GfLds& m, int D, int O, const float* __restrict__ obs, const float* __restrict__ forced, int64_t row0, int64_t n,
                                               int64_t seed, int64_t row_offset, int64_t step_index, float* action, float* logprob, float* entropy,
                                               const GfStepStores& st, int tid) {
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
}

struct CfStepStores { const int32_t* done_prev; float* obs_t; uint8_t* mask_t; int32_t* act_t; float* lp_t; float* dones_t; };

// what heads_kernel (kernels_generic.hip) does with a row of logits, on the same device functions (categorical_head, sample_head, the same Philox keying), so
// equal logits give equal action, log-prob and entropy bits.  The row's logits stay where they are: z is the lane's column of OUT (log-probs in place), p the
// lane's column of the H1 image, which nobody reads behind the forward's last barrier -- run-time head offsets index LDS, no per-lane array exists.  Waves
// 1 .. 3 do the step's other stores meanwhile (store_step_kernel's: OBS[t], MASKS[t] -- all ones without a mask -- and DONES[t] from the previous done flags).
template <int DIST, bool GREEDY>
__device__ __forceinline__ void cat_act_rows(const GfLds& m, const GfShape& sh, const float* __restrict__ obs, const uint8_t* __restrict__ mask,
                                             const int64_t* __restrict__ forced, int64_t row0, int64_t n, int64_t seed, int64_t row_offset, int64_t step_index,
                                             int64_t* action, float* logprob, float* entropy, const CfStepStores& st, int tid) {
    const int A = sh.A, O = sh.obs, H = sh.n_heads;
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
}

// ---------------------------------------------------------------------------------------------------------
// The device envs' one-launch rollouts and evaluations (kernels_gauss_fused.hip; kernels_env_matrix.hip under PPO_KERNEL_ENV_MATRIX): the kernels' arguments,
// wave 0's per-lane functions, the dispatchers and what the launchers of either file fill.
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

struct GfEvalArgs {
    GfShape sh;
    const float* params;
    int64_t n_episodes, seed;
    int max_episode_steps, greedy;
    float* ep_return;
    int32_t* ep_length;
    int32_t* ep_trunc;
};

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

// the kernels' argument structs from the launchers' (GfRolloutArgs / CfRolloutArgs: the same fields, the family's action types)
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
static GfEvalArgs eval_kernel_args(const GenLayout& L, const FusedEvalArgs& e) {
    GfEvalArgs a{};
    a.sh = gf_shape(L);
    a.params = e.params;
    a.n_episodes = e.n_episodes; a.seed = e.seed;
    a.max_episode_steps = e.max_episode_steps; a.greedy = e.greedy != 0;
    a.ep_return = e.ep_return; a.ep_length = e.ep_length; a.ep_trunc = e.ep_trunc;
    return a;
}

// ---------------------------------------------------------------------------------------------------------
// The update kernels: one minibatch step of one net per workgroup column (blockIdx.y = net): gather through the index list, forward, PPO loss
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

// what an update workgroup carries across its tiles besides the weight gradients: the (global) minibatch's advantage statistics, the log_std gradient of the
// lanes of wave 0 and the five loss sums
struct GfLossState {
    float mean_f, inv_std;
    float dls[AM];
    double sums[5];
};

// mean and 1 / (Bessel std + 1e-8) of the (global) minibatch's advantages from the PPO_ADV_PARTS partial sums: gauss_loss_kernel's arithmetic
__device__ __forceinline__ void gf_loss_begin(const GfUpdArgs& a, int net, int w, GfLossState& ls) {
#pragma unroll
    for (int k = 0; k < AM; k++) ls.dls[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 5; k++) ls.sums[k] = 0.0;
    float mean_f = 0.0f, std_f = 0.0f;
    if (a.adv_stat && net == 1 && w == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int i = 0; i < PPO_ADV_PARTS; i++) { t1 += a.adv_stat[i].s1; t2 += a.adv_stat[i].s2; }
        const double mean_a = t1 / a.global_M;
        const double var = (t2 - t1 * mean_a) / (a.global_M - 1.0);
        mean_f = (float)mean_a;
        std_f = (float)sqrt(var < 0.0 ? 0.0 : var);
    }
    ls.mean_f = mean_f;
    ls.inv_std = 1.0f / (std_f + 1e-8f);
}

// The loss lanes: wave 0, lane s = sample s of the tile whose forward has just left OUT; d(loss)/d(output) replaces the output in OUT (zero for a sample
// without a row and for rows out .. outP - 1).  DIST: PPO_DIST_GAUSSIAN or PPO_DIST_CATEGORICAL / PPO_DIST_MASKED: only the actor's lane depends on it.
template <int DIST>
__device__ __forceinline__ void gf_loss_lanes(const GfUpdArgs& a, const GfLds& m, int net, int out, int outP, int s, GfLossState& ls) {
    constexpr bool GAUSS = DIST == PPO_DIST_GAUSSIAN;
    const int D = a.sh.D;
    const LossParams hp = a.hp;
    const float invM = a.invM, mean_f = ls.mean_f, inv_std = ls.inv_std;
    const float clip = hp.clip_coef, lo = 1 - clip, hi_c = 1 + clip;
    float (&dls)[AM] = ls.dls;
    double (&sums)[5] = ls.sums;
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

// The backward of a tile above layer 1, behind the loss lanes (the caller's barrier published dOUT): dW3, db3, dW2, db2 into the running sums, H2 <- dZ2,
// H1 <- dZ1.  Ends with the barrier that publishes dZ1; the X image is not touched.
__device__ __forceinline__ void gf_backward_upper(const GfLds& m, int out, int outP, int s, int w, int ub, int kb, float* gW2, float* gb2, float* gW3, float* gb3) {
    if (4 * ub < outP) gf_dw_tile(m.o, m.h2, ub, kb, gW3, gb3);     // dW3 = dOUT H2^T, db3
    __syncthreads();                                                // ... has read H2
    gf_dz_tile(m.o, out, m.w3, m.h2, s, w);                         // H2 <- dZ2
    __syncthreads();
    gf_dw_tile(m.h2, m.h1, ub, kb, gW2, gb2);                       // dW2 = dZ2 H1^T, db2
    __syncthreads();                                                // ... has read H1
    gf_dz_tile(m.h2, 64, m.w2, m.h1, s, w);                         // H1 <- dZ1
    __syncthreads();
}

// log_std's gradient (a Gaussian actor: behind the net's layers in the slab) and the workgroup's loss partials: wave 0, the loss lanes' state
template <int DIST>
__device__ __forceinline__ void gf_store_loss(const GfUpdArgs& a, float* slab, int net, int b, int s, int w, GfLossState& ls) {
    constexpr bool GAUSS = DIST == PPO_DIST_GAUSSIAN;
    const int base = a.sh.off[net][0], nb = a.nb, D = a.sh.D;
    if (w == 0) {
        if (GAUSS && net == 1) {
#pragma unroll
            for (int k = 0; k < AM; k++) {
                if (k < D) {
                    const float t = wave_sum(ls.dls[k]);
                    if (s == 0) slab[a.sh.logstd_off - base + k] = t;
                }
            }
        }
        // loss partials in gen_loss_sums's layout: the actor's workgroup b writes columns 0 .. 3 (and the padding 5 .. 7), the critic's column 4, of row b;
        // together the nb workgroups of a net write ALL GEN_LOSS_BLOCKS rows, the rows without a workgroup as zeros
        double t[5];
#pragma unroll
        for (int k = 0; k < 5; k++) t[k] = wave_sum_d_dpp(ls.sums[k]);
        if (s < 8 && (net == 1 ? s != 4 : s == 4)) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 5; k++) v = s == k ? t[k] : v;
            for (int row = b; row < GEN_LOSS_BLOCKS; row += nb) a.loss_part[row * 8 + s] = row == b ? v : 0.0;
        }
    }
}

// The workgroup's partial slab above W1, in the net's own parameter order: b1 W2 b2 W3 b3 (actor: then log_std, which sits behind it in the flat vector),
// and its loss partials.  The caller stores dW1 at slab + 0.
template <int DIST>
__device__ __forceinline__ void gf_store_upper(const GfUpdArgs& a, float* slab, int net, int b, int out, int s, int w, int ub, int kb, const float* gW2,
                                               const float* gW3, const float* gb1, const float* gb2, const float* gb3, GfLossState& ls) {
    const int base = a.sh.off[net][0];
    {
        float* dW2 = slab + (a.sh.off[net][2] - base);
        float* dW3 = slab + (a.sh.off[net][4] - base);
#pragma unroll
        for (int i = 0; i < 4; i++) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int u = 4 * ub + i, k = 4 * kb + j;
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
    gf_store_loss<DIST>(a, slab, net, b, s, w, ls);
}

// what an update launcher fills of the kernel's arguments from its own (gauss_fused_fwd_bwd's / cat_fused_fwd_bwd's, either kernel file)
inline GfUpdArgs gf_upd_args(const GenLayout& L, const LossParams& hp, const float* params, const float* obs, const float* actions, const uint8_t* masks,
                             const float* oldlp, const float* adv, const float* ret, const float* oldv, const int32_t* idx, int64_t M, double inv_global_M,
                             double global_M, const AdvStat* adv_stat, float* slab, double* loss_part) {
    GfUpdArgs a{};
    a.sh = gf_shape(L);
    a.hp = hp;
    a.params = params; a.obs = obs; a.actions = actions; a.oldlp = oldlp; a.adv = adv; a.ret = ret; a.oldv = oldv; a.idx = idx;
    a.masks = masks;
    a.M = (int)M;
    a.invM = (float)inv_global_M;
    a.adv_stat = (adv_stat && hp.norm_adv) ? adv_stat : nullptr;
    a.global_M = global_M;
    a.slab = slab;
    a.slab_stride = (int)gauss_fused_slab_stride(L);
    a.nb = (int)std::min<int64_t>((M + 63) / 64, GAUSS_FUSED_MAX_BLOCKS);
    a.loss_part = loss_part;
    return a;
}

// grads[i] = the slabs' elements in workgroup order (gauss_slab_reduce_kernel, kernels_gauss_fused.hip): the second launch of every update step
hipError_t gauss_fused_slab_reduce(const GenLayout& L, const float* slab, int slab_stride, int nb, float* grads, hipStream_t s);

// the row list and the waves' totals of gauss_dev_fold_kernel and its wide twin, behind the carve in the dynamic allocation
constexpr int GF_DEV_FOLD_LIST_INTS = DEV_FOLD_THREADS + 8;

template <typename K>
hipError_t gf_allow(std::atomic<unsigned long long>& done, K kernel, int bytes) {
    return bytes > 64 * 1024 ? allow_dynamic_lds(done, reinterpret_cast<const void*>(kernel)) : hipSuccess;
}
