// kernels_obsnorm.hip -- running mean / variance normalisation of the observations of caller-stepped envs (include/ppo_hip.h: ppo_obs_norm_*;
// the semantics of gym's NormalizeObservation / SB3's VecNormalize, which the reference never needed: CartPole and MountainCar are of unit scale).
//
// A batch is [N, O] f32, O contiguous.  The statistics are f64: mean[O], var[O] (population variance); the row count lives on the host and comes in as
// an argument (it grows by N per update, so the host knows it exactly, and no workgroup reads a word another one writes).
//
// obsnorm_update_apply_kernel: ONE launch per batch does the update and the apply.  Columns are independent, so there is no grid-wide step: a workgroup
// owns cw columns (cw = 2^k <= 16), reduces them over all N rows, merges with Chan's formulas, writes its columns' statistics and normalises its own
// columns.  Lanes run along the columns of a row (adjacent lanes read adjacent floats), the rows are split over the workgroup's R = 256 / cw row slots:
// thread (r, j) takes rows r, r + R, r + 2 R, ... of column j.  The reduction tree is fixed: a thread adds its rows in ascending order, the R partial
// sums of a column are added through LDS in slot order 0 .. R - 1 -- no floating-point atomics, the same bits on every run.  Two passes over the batch
// (mean, then M2 about that mean) and a third that writes y; the batch is small and stays in L2.
// All f64 arithmetic is plain C++ (IEEE / and sqrt; the file is built without fast-math and without contraction).
#include "ppo_internal.hpp"

namespace {

constexpr int ON_THREADS = 256;

__device__ __forceinline__ float on_apply(float x, double mean, double var, double eps, double clip) {
    double y = ((double)x - mean) / sqrt(var + eps);
    y = y < -clip ? -clip : (y > clip ? clip : y);
    return (float)y;
}

// the R partials of every column in LDS, added in slot order by every thread of the column (all of them get the same bits)
__device__ __forceinline__ double on_column_sum(double* part, double mine, int r, int j, int cw, int R) {
    __syncthreads();   // the previous round's reads are done
    part[r * cw + j] = mine;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < R; k++) s += part[k * cw + j];
    return s;
}

__global__ __launch_bounds__(ON_THREADS) void obsnorm_update_apply_kernel(const float* src, float* dst, int64_t N, int O, int cw,
                                                                          double* stats, double count, double eps, double clip) {
    __shared__ double part[ON_THREADS];
    const int tid = threadIdx.x;
    const int j = tid & (cw - 1), r = tid / cw, R = ON_THREADS / cw;
    const int col = blockIdx.x * cw + j;
    const bool live = col < O;
    const double mean0 = live ? stats[col] : 0.0, var0 = live ? stats[O + col] : 1.0;
    const double n = (double)N;

    double s = 0.0;
    if (live)
        for (int64_t row = r; row < N; row += R) s += (double)src[row * O + col];
    const double bm = on_column_sum(part, s, r, j, cw, R) / n;

    double q = 0.0;
    if (live)
        for (int64_t row = r; row < N; row += R) {
            const double d = (double)src[row * O + col] - bm;
            q += d * d;
        }
    const double bm2 = on_column_sum(part, q, r, j, cw, R);

    // Chan's merge of (count, mean0, var0) with (N, bm, bm2)
    const double tot = count + n;
    const double delta = bm - mean0;
    const double mean = mean0 + delta * n / tot;
    const double m2 = var0 * count + bm2 + delta * delta * count * n / tot;
    const double var = m2 / tot;
    if (live && r == 0) { stats[col] = mean; stats[O + col] = var; }
    if (live)
        for (int64_t row = r; row < N; row += R) dst[row * O + col] = on_apply(src[row * O + col], mean, var, eps, clip);   // dst may be src: same thread, same element
}

// apply only: the frozen statistics (mode 2), ppo_obs_norm_apply and the final observations of truncated episodes.  One thread per element.
// truncated / done (both or neither): only rows where both are non-zero are read and written.
__global__ __launch_bounds__(ON_THREADS) void obsnorm_apply_kernel(const float* src, float* dst, int64_t N, int O, const double* __restrict__ stats,
                                                                   double eps, double clip, const int32_t* __restrict__ truncated,
                                                                   const int32_t* __restrict__ done) {
    const int64_t i = (int64_t)blockIdx.x * ON_THREADS + threadIdx.x;
    if (i >= N * O) return;
    const int64_t row = i / O;
    const int col = (int)(i - row * O);
    if (truncated && (truncated[row] == 0 || done[row] == 0)) return;
    dst[i] = on_apply(src[i], stats[col], stats[O + col], eps, clip);
}

}  // namespace

hipError_t launch_obsnorm_update_apply(const float* src, float* dst, int64_t N, int O, double* stats, double count, float eps, float clip, hipStream_t s) {
    if (N < 1 || O < 1) return hipErrorInvalidValue;
    int cw = 1;
    while (cw < 16 && cw < O) cw *= 2;
    const int blocks = (O + cw - 1) / cw;
    hipLaunchKernelGGL(obsnorm_update_apply_kernel, dim3(blocks), dim3(ON_THREADS), 0, s, src, dst, N, O, cw, stats, count, (double)eps, (double)clip);
    return hipGetLastError();
}

hipError_t launch_obsnorm_apply(const float* src, float* dst, int64_t N, int O, const double* stats, float eps, float clip, const int32_t* truncated,
                                const int32_t* done, hipStream_t s) {
    if (N < 1 || O < 1) return hipErrorInvalidValue;
    const int64_t blocks = (N * O + ON_THREADS - 1) / ON_THREADS;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(obsnorm_apply_kernel, dim3((unsigned)blocks), dim3(ON_THREADS), 0, s, src, dst, N, O, stats, (double)eps, (double)clip, truncated, done);
    return hipGetLastError();
}
