// ppo-libtorch_amd/csrc/kernels_gauss.hip -- diagonal-Gaussian policies (PPO_DIST_GAUSSIAN) on the generic engine, f32 storage.
//
// The actor's output layer is the mean mu [n, D]; log_std [D] is a state-independent parameter, the last tensor of the flat parameter vector.  With
// z = (a - mu) exp(-log_std):  log-prob = sum_d (-z_d^2 / 2 - log_std_d - log(2 pi) / 2),  entropy = sum_d (1 / 2 + log(2 pi) / 2 + log_std_d).
// The reference has no continuous policy: the formulas are torch.distributions.Normal's, summed over the D dimensions.  z is formed in f32 from the f32
// inputs (one subtraction, one product with expf(-log_std)); the per-dimension terms and their sum over d are carried in f64 and rounded once: a D = 32
// log-prob is of magnitude 40 and an f32 running sum would lose bits that the probability ratio exp(new - old) needs.
// Everything else of a Gaussian context -- layer products, the backward pass with d(loss)/d(mu) in the place of d(loss)/d(logits), slab sums, gradient
// norm, clip, AdamW -- is the generic engine's own (kernels_generic.hip, kernels_gemm.hip).
#include "generic.hpp"
#include "gauss_dist.hpp"   // gauss_z / gauss_logp / gauss_entropy, the draw (gauss_eps4, gauss_sample): shared with kernels_gauss_fused.hip

namespace {

// One thread per row, D a run-time bound <= PPO_MAX_ACT, no per-row array: dimensions are walked four at a time (one Philox block gives two Box-Muller
// pairs).  The draw of dimension d of row r at step s is a function of (seed, row_offset + r, s, d) alone: counter (row, s mod 2^32, d / 4 | (s >> 32) << 8,
// 0x20) -- word 3 = 0x20 is used by no other draw of the library (categorical heads 0, resets 1, permutations 2, the synthetic env 0x10 .. 0x12) -- with
// u1 = (x >> 8) + 1 over 2^24 in (0, 1], u2 = (y >> 8) over 2^24 in [0, 1): eps = sqrt(-2 log u1) {cos, sin}(2 pi u2), and the same from (z, w).
// The returned action is the raw sample mu + sigma eps (no clipping); its log-prob is evaluated AT the rounded action, as a later update evaluates it.
// GREEDY: action = mu (bit for bit), no random number; forced != nullptr: that action's log-prob.
template <bool GREEDY>
__global__ __launch_bounds__(128) void gauss_heads_kernel(int D, const float* __restrict__ mean, const float* __restrict__ log_std,
                                                          const float* __restrict__ forced, int64_t n, int64_t seed, int64_t row_offset, int64_t step_index,
                                                          float* action, float* logprob, float* entropy) {
    const int64_t r = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (r >= n) return;
    double lp = 0.0, en = 0.0;
    for (int k4 = 0; k4 < D; k4 += 4) {
        float eps[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        if (!GREEDY && !forced) gauss_eps4(seed, row_offset + r, step_index, k4, eps);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = k4 + j;
            if (k < D) {
                const float mu = mean[r * D + k], ls = log_std[k];
                float a;
                if (GREEDY) a = mu;
                else if (forced) a = forced[r * D + k];
                else a = gauss_sample(mu, ls, eps[j]);
                if (action) action[r * D + k] = a;
                lp += gauss_logp(gauss_z(a, mu, expf(-ls)), ls);
                en += gauss_entropy(ls);
            }
        }
    }
    if (logprob) logprob[r] = (float)lp;
    if (entropy) entropy[r] = (float)en;
}

// PPO loss of a Gaussian policy and its gradient w.r.t. mean / value / log_std, one thread per row: loss_kernel's ratio, clip, tie splitting and value
// loss (kernels_generic.hip; PPO_Discrete.cpp:585-631) with the Gaussian log-prob in the place of the categorical one, the log-ratio formed in f64 from
// the f64 sum, and no entropy clamp.
//   d loss / d mu_d      = g_nlp z_d exp(-log_std_d)                      -> dmean [M, D]  (the backward pass reads it as it reads d(logits))
//   d loss / d log_std_d = sum over rows of g_nlp (z_d^2 - 1) + g_ent     (g_ent = -ent_coef / M_global: d entropy / d log_std_d = 1 on every row)
// The per-row arrays (z, the thread's column sums) have the compile-time bound AM and are indexed by unrolled loops under the wave-uniform predicate
// k < D only, so they live in registers (loss_reg_kernel's note on run-time indexed arrays and scratch).  The column sums leave the block by fixed writers
// (ls_part[block][D]: lanes in wave_sum's order, then the four waves in order) and gauss_logstd_grad_kernel adds the blocks in block order: no atomics,
// the same inputs give the same bits.
template <int AM>
__global__ __launch_bounds__(256) void gauss_loss_kernel(int D, LossParams hp, const float* __restrict__ mean, const float* __restrict__ val,
                                                         const float* __restrict__ row_act, const float* __restrict__ log_std,
                                                         const float* __restrict__ oldlp, const float* __restrict__ advs, const float* __restrict__ rets,
                                                         const float* __restrict__ oldv, int64_t M, float invM, const AdvStat* __restrict__ adv_stat,
                                                         double global_M, float* dmean, float* dval, double* loss_part, float* ls_part) {
    __shared__ double red[5][4];
    __shared__ float sdl[4][AM];
    __shared__ float s_ls[AM], s_inv[AM];
    if (threadIdx.x < AM) {
        const float ls = (int)threadIdx.x < D ? log_std[threadIdx.x] : 0.0f;
        s_ls[threadIdx.x] = ls;
        s_inv[threadIdx.x] = expf(-ls);
    }
    __syncthreads();
    double ent_d = 0.0;   // the same on every row
#pragma unroll
    for (int k = 0; k < AM; k++) if (k < D) ent_d += gauss_entropy(s_ls[k]);
    const float ent = (float)ent_d;
    float dls[AM];
#pragma unroll
    for (int k = 0; k < AM; k++) dls[k] = 0.0f;
    double s[5] = { 0, 0, 0, 0, 0 };
    // mean and 1 / (Bessel std + 1e-8) of the (global) minibatch's advantages from the PPO_ADV_PARTS partial sums: adv_finish_kernel's arithmetic
    float mean_f = 0.0f, std_f = 0.0f;
    if (adv_stat) {
        double t1 = 0.0, t2 = 0.0;
        for (int i = 0; i < PPO_ADV_PARTS; i++) { t1 += adv_stat[i].s1; t2 += adv_stat[i].s2; }
        const double mean_a = t1 / global_M;
        const double var = (t2 - t1 * mean_a) / (global_M - 1.0);
        mean_f = (float)mean_a;
        std_f = (float)sqrt(var < 0.0 ? 0.0 : var);
    }
    const float inv_std = 1.0f / (std_f + 1e-8f);
    const float clip = hp.clip_coef, lo = 1 - clip, hi_c = 1 + clip;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < M; r += (int64_t)gridDim.x * 256) {
        float z[AM];
        double nlp_d = 0.0;
#pragma unroll
        for (int k = 0; k < AM; k++) {
            z[k] = 0.0f;
            if (k < D) {
                z[k] = gauss_z(row_act[r * D + k], mean[r * D + k], s_inv[k]);
                nlp_d += gauss_logp(z[k], s_ls[k]);
            }
        }
        const float logratio = (float)(nlp_d - (double)oldlp[r]);
        const float ratio = expf(logratio);
        float adv = advs[r];
        if (hp.norm_adv) adv = (adv - mean_f) * inv_std;
        const float rc = ratio < lo ? lo : (ratio > hi_c ? hi_c : ratio);
        const float l1 = -adv * ratio, l2 = -adv * rc;
        const bool inside = (ratio >= lo && ratio <= hi_c);
        float d_ratio;
        if (l1 > l2) d_ratio = -adv;
        else if (l1 < l2) d_ratio = inside ? -adv : 0.0f;
        else d_ratio = 0.5f * -adv + (inside ? 0.5f * -adv : 0.0f);   // torch::max splits ties half/half
        const float g_nlp = invM * d_ratio * ratio;
        const float g_ent = -hp.ent_coef * invM;
#pragma unroll
        for (int k = 0; k < AM; k++) {
            if (k < D) {
                dmean[r * D + k] = g_nlp * z[k] * s_inv[k];
                dls[k] += g_nlp * (z[k] * z[k] - 1.0f) + g_ent;
            }
        }
        s[0] += (double)(l1 > l2 ? l1 : l2);
        s[1] += (double)ent;
        s[2] += (double)((ratio - 1.0f) - logratio);
        s[3] += (fabsf(ratio - 1.0f) > clip) ? 1.0 : 0.0;
        // value loss (:603-625)
        const float v = val[r], R = rets[r], vold = oldv[r];
        const float un = (v - R) * (v - R);
        float g_v, lossv;
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
        dval[r] = g_v;
        s[4] += (double)lossv;
    }
#pragma unroll
    for (int k = 0; k < AM; k++) {
        if (k < D) {
            const float t = wave_sum(dls[k]);
            if ((threadIdx.x & 63) == 0) sdl[threadIdx.x >> 6][k] = t;
        }
    }
    for (int k = 0; k < 5; k++) {
        const double t = wave_sum_d_dpp(s[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if (threadIdx.x < 5) loss_part[blockIdx.x * 8 + threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
    if ((int)threadIdx.x < D) ls_part[blockIdx.x * D + threadIdx.x] = ((sdl[0][threadIdx.x] + sdl[1][threadIdx.x]) + sdl[2][threadIdx.x]) + sdl[3][threadIdx.x];
}

// grad[d] = the blocks' column sums in block order (one thread per dimension)
__global__ __launch_bounds__(64) void gauss_logstd_grad_kernel(int D, const float* __restrict__ ls_part, int blocks, float* __restrict__ grad) {
    const int k = threadIdx.x;
    if (k >= D) return;
    float acc = 0.0f;
    for (int b = 0; b < blocks; b++) acc += ls_part[b * D + k];
    grad[k] = acc;
}

// rollout stores of one step: obs, the f32 actions, log-probs, the PREVIOUS step's done flags (store_step_kernel without masks)
__global__ __launch_bounds__(256) void gauss_store_step_kernel(int N, int O, int D, const float* __restrict__ obs, const float* __restrict__ actf,
                                                               const float* __restrict__ lp, const int32_t* __restrict__ done_prev, float* obs_t, float* act_t,
                                                               float* lp_t, float* dones_t) {
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = i0; i < (int64_t)N * O; i += stride) obs_t[i] = obs[i];
    for (int64_t i = i0; i < (int64_t)N * D; i += stride) act_t[i] = actf[i];
    for (int64_t i = i0; i < N; i += stride) { lp_t[i] = lp[i]; dones_t[i] = (float)done_prev[i]; }
}

}  // namespace

hipError_t gen_gauss_heads(int D, const float* mean, const float* log_std, const float* forced, int64_t n, int64_t seed, int64_t row_offset, int64_t step_index,
                           float* action, float* logprob, float* entropy, hipStream_t s, bool greedy) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 127) / 128)), block(128);
    if (greedy) hipLaunchKernelGGL(gauss_heads_kernel<true>, grid, block, 0, s, D, mean, log_std, nullptr, n, seed, row_offset, step_index, action, logprob, entropy);
    else hipLaunchKernelGGL(gauss_heads_kernel<false>, grid, block, 0, s, D, mean, log_std, forced, n, seed, row_offset, step_index, action, logprob, entropy);
    return hipGetLastError();
}

hipError_t gen_gauss_loss(const GenLayout& L, const LossParams& hp, const GenericCtx& g, const float* log_std, int64_t M, double inv_global_M, double global_M,
                          const AdvStat* adv_stat, float* grad_logstd, hipStream_t s) {
    if (g.bf16 || !L.gauss || L.gauss > PPO_MAX_ACT || !g.ls_part) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gauss_loss_kernel<PPO_MAX_ACT>, dim3(GEN_LOSS_BLOCKS), dim3(256), 0, s, L.gauss, hp, g.logits, g.val, reinterpret_cast<const float*>(g.row_act),
                       log_std, g.row_f[0], g.row_f[1], g.row_f[2], g.row_f[3], M, (float)inv_global_M, (adv_stat && hp.norm_adv) ? adv_stat : nullptr, global_M,
                       g.dlogits, g.dval, g.loss_part, g.ls_part);
    hipLaunchKernelGGL(gauss_logstd_grad_kernel, dim3(1), dim3(64), 0, s, L.gauss, g.ls_part, GEN_LOSS_BLOCKS, grad_logstd);
    return hipGetLastError();
}

hipError_t gen_gauss_store_step(const GenLayout& L, int N, const float* obs, const float* actf, const float* lp, const int32_t* done_prev, float* obs_t,
                                float* act_t, float* lp_t, float* dones_t, hipStream_t s) {
    const int64_t most = (int64_t)N * (L.obs > L.gauss ? L.obs : L.gauss);
    int64_t blocks = (most + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    hipLaunchKernelGGL(gauss_store_step_kernel, dim3((unsigned)blocks), dim3(256), 0, s, N, L.obs, L.gauss, obs, actf, lp, done_prev, obs_t, act_t, lp_t, dones_t);
    return hipGetLastError();
}
