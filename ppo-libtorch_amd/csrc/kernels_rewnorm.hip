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

}  // namespace

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
