// ppo-libtorch_amd/csrc/fused_matrix_dev.hpp -- the device functions of the f32 matrix-core forward (v_mfma_f32_16x16x4_f32) that kernels_fused_matrix.hip
// (PPO_KERNEL_FUSED_MATRIX: caller-stepped envs) and kernels_env_matrix.hip (PPO_KERNEL_ENV_MATRIX: the device envs' one-launch rollouts) share: the lane
// map, the carve, the operand fetches and the products.  The lane map and the reasons for it are at the head of kernels_fused_matrix.hip.  One function,
// gm_forward_regs, holds a tile's products: both files' forwards end in it, so an observation gets the same bits from every kernel of either file.
#pragma once
#include "gauss_fused_dev.hpp"

static_assert(GW_K == 64 && GF_THREADS == 256, "four waves own 16 units each of a 64-wide layer; a chunk is one 64-deep product");

typedef float gm_f4 __attribute__((ext_vector_type(4)));

// the k of step t in k-slot kg (the head of kernels_fused_matrix.hip)
__device__ __forceinline__ int gm_k(int t, int kg) { return 16 * (t >> 2) + 4 * kg + (t & 3); }

// nx: the X chunk buffers (two where layer 1 is pipelined over chunks, one where the observation is a single resident chunk)
__host__ __device__ inline int gm_lds_floats(int outP, int nx = 2) {
    return 4096 + 64 * outP + 64 + 64 + 32 + 32 + 32 + 64 + nx * GW_K * GF_S + 64 * GF_S + 64 * GF_S + outP * GF_S;
}

// the family's images without a W1 image; m.x names buffer 0 of the nx X chunk buffers, m.obsP is the chunk width
__device__ __forceinline__ GfLds gm_carve(float* base, int outP, int nx = 2) {
    GfLds m;
    m.obsP = GW_K; m.outP = outP;
    float* p = base;
    m.w1 = nullptr;
    m.w2 = p; p += 4096;
    m.w3 = p; p += 64 * outP;
    m.b1 = p; p += 64;
    m.b2 = p; p += 64;
    m.b3 = p; p += 32;
    m.ls = p; p += 32;
    m.inv = p; p += 32;
    m.ridx = reinterpret_cast<int*>(p); p += 64;
    m.x = p; p += nx * GW_K * GF_S;
    m.h1 = p; p += 64 * GF_S;
    m.h2 = p; p += 64 * GF_S;
    m.o = p;
    return m;
}
__device__ __forceinline__ float* gm_x(const GfLds& m, int b) { return m.x + b * (GW_K * GF_S); }

// the A operand of a 64-deep product out of a row-major matrix W [64, ld] in global memory: row u, columns k0 + gm_k(t, kg), zero behind column K
__device__ __forceinline__ void gm_fetch_a(const float* __restrict__ W, int ld, int K, int k0, int u, int kg, float (&a)[16]) {
    const float* row = W + u * ld + k0;
#pragma unroll
    for (int t = 0; t < 16; t++) a[t] = k0 + gm_k(t, kg) < K ? row[gm_k(t, kg)] : 0.0f;
}

// acc[j] += A B_j over quarters 0 .. nq - 1 (16 k each): B_j [k][16 j + e] out of an image [k][sample]
__device__ __forceinline__ void gm_mma_k(const float (&a)[16], const float* __restrict__ img, int nq, int e, int kg, gm_f4 (&acc)[4]) {
#pragma unroll
    for (int t = 0; t < 16; t++) {
        if ((t >> 2) < nq) {   // uniform
            const float* row = img + gm_k(t, kg) * GF_S + e;
#pragma unroll
            for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], row[16 * j], acc[j], 0, 0, 0);
        }
    }
}

// acc[j][r] = b[16 w + 4 kg + r]: a hidden layer's accumulators start at the bias
__device__ __forceinline__ void gm_bias(const float* __restrict__ b, int w, int kg, gm_f4 (&acc)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(&b[16 * w + 4 * kg]);
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = gm_f4{ v.x, v.y, v.z, v.w };
}
// out[16 w + 4 kg + r][16 j + e] = tanh(acc[j][r])
__device__ __forceinline__ void gm_store_tanh(float* __restrict__ out, int w, int e, int kg, const gm_f4 (&acc)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) out[(16 * w + 4 * kg + r) * GF_S + 16 * j + e] = tanh_fast(acc[j][r]);
}

// The products of a tile's forward on given operand registers: a1 is the wave's slice of the last (or only) W1 chunk, x that chunk's image [k][sample] with
// nq quarters of 16 k that hold something, acc the layer-1 accumulators (the bias, plus the earlier chunks' products), a2 the wave's slice of W2.  The
// caller's barrier has published x.  Leaves H1, H2 (post-tanh) and OUT rows 0 .. out - 1, a barrier behind each layer; every thread of the workgroup calls it.
__device__ __forceinline__ void gm_forward_regs(const GfLds& m, const float (&a1)[16], const float* __restrict__ x, int nq, gm_f4 (&acc)[4], const float (&a2)[16],
                                                int out, int tid) {
    const int s = tid & 63, e = tid & 15, kg = (tid >> 4) & 3, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    gm_mma_k(a1, x, nq, e, kg, acc);
    gm_store_tanh(m.h1, w, e, kg, acc);
    __syncthreads();
    gm_bias(m.b2, w, kg, acc);
    gm_mma_k(a2, m.h1, 4, e, kg, acc);
    gm_store_tanh(m.h2, w, e, kg, acc);
    __syncthreads();
    gf_output_layer(m, out, s, w);
    __syncthreads();
}

// the wave's slice of one net's W2, the A operand of layer 2
__device__ __forceinline__ void gm_fetch_w2(const GfShape& sh, const float* __restrict__ params, int net, int tid, float (&a2)[16]) {
    gm_fetch_a(params + sh.off[net][2], 64, 64, 0, 16 * (tid >> 6) + (tid & 15), (tid >> 4) & 3, a2);
}
