// kernels_rewnorm.hip -- reward normalisation of caller-stepped envs by the running statistics of the discounted return (include/ppo_hip.h:
// ppo_reward_norm_*; the semantics of gym's NormalizeReward / the reward half of SB3's VecNormalize, which the reference never needed: CartPole and
// MountainCar pay rewards of unit scale).
//
// A batch is one env step: r[N] f32 and done[N] i32.  The state is f64: the per-env discounted-return accumulator ret[N] and stats = mean | var
// (population variance) of every return seen so far; the row count lives on the host and comes in as an argument (it grows by N per update).
//
// rewnorm_update_apply_kernel: ONE launch, ONE workgroup.  The batch is N scalars, so one workgroup of W = RN_THREADS reduces it, and a second one
// would need a grid-wide step between the passes.  Thread w takes rows w, w + W, w + 2 W, ... in ascending order, in f64; the W partial sums are added
// through LDS in slot order 0 .. W - 1 by every thread (rn_block_sum; lane w writes the 8 bytes at part + 8 w, every lane reads the same word per
// iteration: a broadcast, no bank conflict) -- no floating-point atomics, the same feed gives the same bits.  Three passes: R = ret * gamma + r and its
// sum (R parked in ret), M2 about the batch mean, then Chan's merge, the apply and the done reset of ret.  A row is only ever touched by its own
// thread, so the passes need no fence beyond the barriers of the two sums.  Correct for any N >= 1: a thread whose first row is past N adds 0.
// All f64 arithmetic is plain C++ (IEEE / and sqrt; the file is built without fast-math and without contraction).
#include "ppo_internal.hpp"

namespace {

constexpr int RN_THREADS = 256;
constexpr int RN_SCAN_AHEAD = 8;   // rewnorm_scan_kernel: steps whose rewards and dones are loaded in front of their chain

__device__ __forceinline__ float rn_apply(float r, double var, double eps, double clip) {
    double y = (double)r / sqrt(var + eps);
    y = y < -clip ? -clip : (y > clip ? clip : y);
    return (float)y;
}

// the W partials in LDS, added in slot order by every thread (all of them get the same bits)
__device__ __forceinline__ double rn_block_sum(double* part, double mine, int w) {
    __syncthreads();   // the previous round's reads are done
    part[w] = mine;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < RN_THREADS; k++) s += part[k];
    return s;
}

__global__ __launch_bounds__(RN_THREADS) void rewnorm_update_apply_kernel(const float* __restrict__ rew, const int32_t* __restrict__ done,
                                                                          float* __restrict__ out, int64_t N, double* __restrict__ ret,
                                                                          double* __restrict__ stats, double count, double gamma, double eps, double clip) {
    __shared__ double part[RN_THREADS];
    const int w = threadIdx.x;
    const double mean0 = stats[0], var0 = stats[1];
    const double n = (double)N;

    double s = 0.0;
    for (int64_t row = w; row < N; row += RN_THREADS) {
        const double R = ret[row] * gamma + (double)rew[row];
        ret[row] = R;
        s += R;
    }
    const double bm = rn_block_sum(part, s, w) / n;

    double q = 0.0;
    for (int64_t row = w; row < N; row += RN_THREADS) {
        const double d = ret[row] - bm;
        q += d * d;
    }
    const double bm2 = rn_block_sum(part, q, w);

    // Chan's merge of (count, mean0, var0) with (N, bm, bm2)
    const double tot = count + n;
    const double delta = bm - mean0;
    const double mean = mean0 + delta * n / tot;
    const double m2 = var0 * count + bm2 + delta * delta * count * n / tot;
    const double var = m2 / tot;
    if (w == 0) { stats[0] = mean; stats[1] = var; }   // every thread read the old pair in front of the sums' barriers
    for (int64_t row = w; row < N; row += RN_THREADS) {
        out[row] = rn_apply(rew[row], var, eps, clip);
        if (done[row] != 0) ret[row] = 0.0;
    }
}

// apply only (mode 2: frozen statistics).  One thread per row.
__global__ __launch_bounds__(RN_THREADS) void rewnorm_apply_kernel(const float* __restrict__ rew, float* __restrict__ out, int64_t N,
                                                                   const double* __restrict__ stats, double eps, double clip) {
    const int64_t i = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x;
    if (i >= N) return;
    out[i] = rn_apply(rew[i], stats[1], eps, clip);
}

// ---- a whole rollout of a fused device env (PPO_KERNEL_ENV_REWARD_NORM; api.hip: fused_env_rollout).  The rollout is one launch for all T steps, so there
// is no step to put rewnorm_update_apply_kernel in front of -- and no need: rewards never feed back into a rollout, so the T updates are a post-process of
// rew [T, N] (raw, overwritten with y) and fin_len [T, N] (done = fin_len != 0).  Three launches whatever T is, ordered by their launch boundaries alone,
// which leave the bits T launches of rewnorm_update_apply_kernel on rows 0 .. T - 1 would leave:
//   rewnorm_scan_kernel      one thread per env walks t = 0 .. T - 1: R = ret * gamma + r into the f64 workspace Rw [T, N], ret = done ? 0 : R; the only
//                            chain over t that touches N values, and it is N-wide parallel.
//   rewnorm_moments_kernel   one workgroup per step t: bm[t] = (sum R) / N and bm2[t] = sum (R - bm[t])^2 with the per-step kernel's sums -- slot w takes
//                            rows w, w + W, ... ascending, the W slots are added in slot order (rn_block_sum).  Workgroup 0 also parks the statistics the
//                            rollout started from in st0, so that the next launch may overwrite stats while others of its workgroups still start from them.
//   rewnorm_merge_apply_kernel   workgroup (t, j): Chan's merge is a chain of scalars, count0 + k N -> count0 + (k + 1) N for k = 0 .. t; every thread runs
//                            it from st0 over bm / bm2 (staged through LDS, RN_THREADS steps at a time; each thread reads the same word: a broadcast) and
//                            holds var[t]; then rew[t, :] = rn_apply(rew[t, :], var[t]) over the workgroup's share of the row.  Workgroup (T - 1, 0)
//                            writes the final pair.  The count advances by + N per step as the host's does (api.hip: rn_batch), so a count that
//                            ppo_reward_norm_set_h made fractional takes the same roundings.
// No floating-point atomics, no hand-over between workgroups of a launch.  Correct for any N >= 1 and T >= 1: a slot with no row adds 0.
__global__ __launch_bounds__(RN_THREADS) void rewnorm_scan_kernel(const float* __restrict__ rew, const int32_t* __restrict__ fin_len, int64_t N, int T,
                                                                  double* __restrict__ ret, double* __restrict__ Rw, double gamma) {
    const int64_t n = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x;
    if (n >= N) return;
    double acc = ret[n];
    // RN_SCAN_AHEAD steps' loads are issued in front of their chain: the loads do not depend on it, and one at a time they are the kernel's whole time
    // (43 us of latency at 4096 x 128)
    for (int t0 = 0; t0 < T; t0 += RN_SCAN_AHEAD) {
        float r[RN_SCAN_AHEAD];
        int32_t f[RN_SCAN_AHEAD];
#pragma unroll
        for (int k = 0; k < RN_SCAN_AHEAD; k++) {
            const bool in = t0 + k < T;
            const int64_t i = (int64_t)(in ? t0 + k : t0) * N + n;
            r[k] = rew[i];
            f[k] = fin_len[i];
        }
#pragma unroll
        for (int k = 0; k < RN_SCAN_AHEAD; k++) {
            if (t0 + k < T) {
                const double R = acc * gamma + (double)r[k];
                Rw[(int64_t)(t0 + k) * N + n] = R;
                acc = f[k] != 0 ? 0.0 : R;
            }
        }
    }
    ret[n] = acc;
}

__global__ __launch_bounds__(RN_THREADS) void rewnorm_moments_kernel(const double* __restrict__ Rw, int64_t N, const double* __restrict__ stats,
                                                                     double* __restrict__ bm_out, double* __restrict__ bm2_out, double* __restrict__ st0) {
    __shared__ double part[RN_THREADS];
    const int w = threadIdx.x;
    const int t = blockIdx.x;
    const double* R = Rw + (int64_t)t * N;
    const double n = (double)N;

    double s = 0.0;
    for (int64_t row = w; row < N; row += RN_THREADS) s += R[row];
    const double bm = rn_block_sum(part, s, w) / n;

    double q = 0.0;
    for (int64_t row = w; row < N; row += RN_THREADS) {
        const double d = R[row] - bm;
        q += d * d;
    }
    const double bm2 = rn_block_sum(part, q, w);
    if (w == 0) { bm_out[t] = bm; bm2_out[t] = bm2; }
    if (t == 0 && w < 2) st0[w] = stats[w];
}

__global__ __launch_bounds__(RN_THREADS) void rewnorm_merge_apply_kernel(float* rew, int64_t N, const double* __restrict__ bm_in,
                                                                         const double* __restrict__ bm2_in, const double* __restrict__ st0,
                                                                         double* __restrict__ stats, double count, double eps, double clip) {
    __shared__ double sbm[RN_THREADS], sbm2[RN_THREADS];
    const int w = threadIdx.x;
    const int t = blockIdx.x;
    const double n = (double)N;
    double mean = st0[0], var = st0[1];
    for (int base = 0; base <= t; base += RN_THREADS) {
        const int len = min(RN_THREADS, t + 1 - base);
        __syncthreads();   // the previous chunk's reads are done
        if (w < len) { sbm[w] = bm_in[base + w]; sbm2[w] = bm2_in[base + w]; }
        __syncthreads();
        for (int k = 0; k < len; k++) {
            // Chan's merge of (count, mean, var) with (N, bm[k], bm2[k]): rewnorm_update_apply_kernel's expressions, term for term
            const double tot = count + n;
            const double delta = sbm[k] - mean;
            const double m2 = var * count + sbm2[k] + delta * delta * count * n / tot;
            mean = mean + delta * n / tot;
            var = m2 / tot;
            count = tot;
        }
    }
    if (t == (int)gridDim.x - 1 && blockIdx.y == 0 && w == 0) { stats[0] = mean; stats[1] = var; }
    float* row_t = rew + (int64_t)t * N;
    for (int64_t row = (int64_t)blockIdx.y * RN_THREADS + w; row < N; row += (int64_t)gridDim.y * RN_THREADS) row_t[row] = rn_apply(row_t[row], var, eps, clip);
}

// mode 2 over a whole rollout: the frozen variance on all T N rewards, in place.  One thread per reward.
__global__ __launch_bounds__(RN_THREADS) void rewnorm_apply_inplace_kernel(float* rew, int64_t n, const double* __restrict__ stats, double eps, double clip) {
    const int64_t i = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x;
    if (i >= n) return;
    rew[i] = rn_apply(rew[i], stats[1], eps, clip);
}

}  // namespace

size_t rewnorm_rollout_workspace(int64_t N, int T) { return (size_t)T * (size_t)N + 2 * (size_t)T + 2; }

hipError_t launch_rewnorm_rollout(int mode, float* rew, const int32_t* fin_len, int64_t N, int T, double* ret, double* stats, double* ws, double count,
                                  float gamma, float eps, float clip, hipStream_t s) {
    if (N < 1 || T < 1 || (mode != 1 && mode != 2)) return hipErrorInvalidValue;
    const int64_t env_blocks = (N + RN_THREADS - 1) / RN_THREADS;
    const int64_t all_blocks = ((int64_t)T * N + RN_THREADS - 1) / RN_THREADS;
    if (env_blocks > 0x7fffffff || all_blocks > 0x7fffffff) return hipErrorInvalidValue;
    if (mode == 2) {
        hipLaunchKernelGGL(rewnorm_apply_inplace_kernel, dim3((unsigned)all_blocks), dim3(RN_THREADS), 0, s, rew, (int64_t)T * N, stats, (double)eps, (double)clip);
        return hipGetLastError();
    }
    double* Rw = ws;
    double* bm = ws + (size_t)T * (size_t)N;
    double* bm2 = bm + T;
    double* st0 = bm2 + T;
    hipLaunchKernelGGL(rewnorm_scan_kernel, dim3((unsigned)env_blocks), dim3(RN_THREADS), 0, s, rew, fin_len, N, T, ret, Rw, (double)gamma);
    hipLaunchKernelGGL(rewnorm_moments_kernel, dim3((unsigned)T), dim3(RN_THREADS), 0, s, Rw, N, stats, bm, bm2, st0);
    // a row's share per workgroup: 4 rewards a thread, at most 64 workgroups a row (each of them runs the chain to t)
    const unsigned per_row = (unsigned)std::min<int64_t>(64, (N + 4 * RN_THREADS - 1) / (4 * RN_THREADS));
    hipLaunchKernelGGL(rewnorm_merge_apply_kernel, dim3((unsigned)T, per_row), dim3(RN_THREADS), 0, s, rew, N, bm, bm2, st0, stats, count, (double)eps,
                       (double)clip);
    return hipGetLastError();
}

hipError_t launch_rewnorm_update_apply(const float* rew, const int32_t* done, float* out, int64_t N, double* ret, double* stats, double count, float gamma,
                                       float eps, float clip, hipStream_t s) {
    if (N < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rewnorm_update_apply_kernel, dim3(1), dim3(RN_THREADS), 0, s, rew, done, out, N, ret, stats, count, (double)gamma, (double)eps,
                       (double)clip);
    return hipGetLastError();
}

hipError_t launch_rewnorm_apply(const float* rew, float* out, int64_t N, const double* stats, float eps, float clip, hipStream_t s) {
    if (N < 1) return hipErrorInvalidValue;
    const int64_t blocks = (N + RN_THREADS - 1) / RN_THREADS;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rewnorm_apply_kernel, dim3((unsigned)blocks), dim3(RN_THREADS), 0, s, rew, out, N, stats, (double)eps, (double)clip);
    return hipGetLastError();
}
