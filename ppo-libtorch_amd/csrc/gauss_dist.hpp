// ppo-libtorch_amd/csrc/gauss_dist.hpp -- the diagonal Gaussian's device functions: ONE definition for gauss_heads_kernel / gauss_loss_kernel
// (kernels_gauss.hip, the generic engine) and the fused 2 x 64 kernels (kernels_gauss_fused.hip), so that a mean gets the same draw, log-prob and entropy
// from either, bit for bit.  The library is compiled with -ffp-contract=off: mu + sigma * eps is a product and a sum, rounded separately, in both.
#pragma once
#include "ppo_internal.hpp"

#ifdef __HIPCC__
constexpr double GAUSS_HALF_LOG_2PI = 0.91893853320467274178;

// the standardised action and its log-density; inv_sigma = expf(-log_std)
__device__ __forceinline__ float gauss_z(float a, float mu, float inv_sigma) { return (a - mu) * inv_sigma; }
__device__ __forceinline__ double gauss_logp(float z, float log_std) { return (-0.5 * (double)z * (double)z - (double)log_std) - GAUSS_HALF_LOG_2PI; }
__device__ __forceinline__ double gauss_entropy(float log_std) { return (0.5 + GAUSS_HALF_LOG_2PI) + (double)log_std; }

// Standard-normal draws of dimensions k4 .. k4 + 3 (k4 a multiple of 4) of one row at one step: one Philox block, two Box-Muller pairs.  Counter (row,
// step mod 2^32, k4 / 4 | (step >> 32) << 8, 0x20) -- word 3 = 0x20 is used by no other draw of the library (categorical heads 0, resets 1, permutations 2,
// the synthetic env 0x10 .. 0x12) -- with u1 = (x >> 8) + 1 over 2^24 in (0, 1], u2 = (y >> 8) over 2^24 in [0, 1): eps = sqrt(-2 log u1) {cos, sin}(2 pi u2),
// and the same from (z, w).
__device__ __forceinline__ void gauss_eps4(int64_t seed, int64_t row, int64_t step_index, int k4, float* eps) {
    const uint4 w = philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)row, (uint32_t)step_index,
                                  (uint32_t)(k4 >> 2) | ((uint32_t)((uint64_t)step_index >> 32) << 8), 0x20u);
    const float ra = sqrtf(-2.0f * logf((float)((w.x >> 8) + 1u) * 0x1p-24f)), rb = sqrtf(-2.0f * logf((float)((w.z >> 8) + 1u) * 0x1p-24f));
    float sa, ca, sb, cb;
    sincospif((float)(w.y >> 8) * 0x1p-23f, &sa, &ca);
    sincospif((float)(w.w >> 8) * 0x1p-23f, &sb, &cb);
    eps[0] = ra * ca; eps[1] = ra * sa; eps[2] = rb * cb; eps[3] = rb * sb;
}
// the raw sample (no clipping)
__device__ __forceinline__ float gauss_sample(float mu, float log_std, float eps) { return mu + expf(log_std) * eps; }
#endif
