// ppo-libtorch_amd/csrc/kernels_fused_matrix_h128.hip -- PPO_KERNEL_FUSED_MATRIX at hidden = 128, n_hidden = 2: the fused families (PPO_KERNEL_GAUSS_FUSED,
// PPO_KERNEL_CAT_FUSED) on a 2 x 128 f32 network, every 64- and 128-deep product on the f32 matrix cores (v_mfma_f32_16x16x4_f32, plain f32 operands, f32
// accumulation).  A kernel set of its own beside kernels_fused_matrix.hip: the same tile (64 samples per workgroup pass, images [unit][sample] of stride
// GF_S), the same chunk pipeline of layer 1 (nc = ceil(obs / 64) = 1 .. 6), the family's heads, draws, loss lanes, step stores, slab layout and
// gauss_slab_reduce_kernel -- and a different split of the work, because at this width nothing of W2 fits beside the images.
//
// The wave split: 4 waves, each owning 32 units.  lane = 16 kg + e.  Wave w owns units 32 w .. 32 w + 31 of all 64 samples as two row tiles i = 0, 1 by four
// column tiles j = 0 .. 3: element r of accumulator [i][j] in lane (e, kg) is unit 32 w + 16 i + 4 kg + r of sample 16 j + e; 32 accumulator registers.  The k
// order of a 64-deep product is gm_k (fused_matrix_dev.hpp), a 128-deep product is two of them.  Every B value read from an image feeds two instructions (one
// per row tile): half the LDS reads per product of the 64-wide kernels.  The alternative, 8 waves of 16 units at 256 registers each, would keep the per-wave
// budgets of kernels_fused_matrix.hip, but every function of the family that is not a product (the X chunk fetch, the heads, the loss lanes, the step stores,
// the fold's compaction, dW3's thread grid) is written for a workgroup of 256 and serves here unchanged.  Measured (-Rpass-analysis=kernel-resource-usage): the
// act, critic and fold kernels take 226 .. 247 VGPRs + 64 AGPRs with the W2 slice resident; the update kernels 256 + 245 (Gaussian), 256 + 218 (masked),
// 256 + 210 (categorical); scratch 0 bytes per lane in all eleven, no VGPR spill counted in any.  None of them fits a 256-register wave.
//
// Where the weights live.  W2 is 65 536 bytes: with it the carve would be 196 KB.  It goes the way W1 goes: from L2 straight into operand registers, each
// element into exactly one lane.  The forward's A operand is the wave's 32 x 128 slice, 64 registers: the act, critic and fold kernels fetch it once per
// kernel; the update kernel fetches it in front of every tile's forward, because beside the loss lanes' state it does not fit (with it resident, and the dW2
// accumulators too, the three update kernels spilled 76 .. 172 bytes per lane).  The backward's A operand for dZ1 = (W2^T dZ2)(1 - H1^2) is the transposed
// slice, W2[o][32 w + 16 i + e]: lanes e read 64 consecutive bytes; it is fetched per tile, one 64-deep half (32 registers) at a time.  W3 (at most 32 x 128),
// the biases and log_std are staged in LDS.
//
//   layer 1: kernels_fused_matrix.hip's pipeline: chunk c + 1's W1 slice (32 registers) and X elements (16) are loaded in front of chunk c's products.
//   layer 2: two 64-deep products on H1 rows 0 .. 63 and 64 .. 127.
//   layer 3, dW3 / db3, dZ2: out <= 32, on vector functions (hm_output_layer, gf_dw_tile on a 8 x 32 thread grid, hm_dz_tile): the family's, over K = 128.
//   dW2 = dZ2 H1^T: K = the tile's 64 samples; A = the wave's 32 rows of dZ2, B = the 128 rows of H1: 2 x 8 accumulators, 64 registers.
//   dW1 = dZ1 X^T: the chunks walk downward as in the 64-wide kernel, 32 accumulators per chunk.
//   Neither dW2's nor a dW1 chunk's accumulators outlive the product: they are summed from zero and go to the workgroup's own slab at once -- stored by the
//            workgroup's first tile, added to what the same thread stored by a later one (plain loads and stores of elements no other thread touches; no
//            atomics; the order is the tile order, so equal inputs give equal bits).  A minibatch of at most 64 x GAUSS_FUSED_MAX_BLOCKS rows gives every
//            workgroup one tile and no read.  Kept in registers they would be 64 + 32 nc, 256 at nc = 6.  So the kernel is ONE instantiation per policy
//            kind for every nc, and the observation limit stays FUSED_WIDE_MAX_OBS = 384: no instantiation forced a lower one.
// One forward function (hm_forward_tile) serves all kernels of the file: an observation gets the same mean / logits and the same value from every entry point,
// bit for bit.
//
// LDS (floats; outP = the output width rounded up to 4; the update kernel carves for the wider net, the actor):
//   W3 128 outP | b1 128 | b2 128 | b3 32 | log_std 32 | exp(-log_std) 32 | row index 64 | X 2 x 64 68 | H1 128 68 | H2 128 68 | OUT outP 68
//   32 outputs: 4096 + 416 + 8704 + 8704 + 8704 + 2176 = 32 800 floats = 131 200 bytes; 1 output: 512 + 416 + 26 112 + 272 = 27 312 floats = 109 248 bytes
//   (the fold adds its list, 1 056).  One workgroup per CU.  The size does not depend on obs_size.
// Every kernel is __launch_bounds__(256): one wave per SIMD, 512 registers; LDS is all dynamic, the sizes above.
#include "fused_matrix_dev.hpp"

namespace {

constexpr int HM_H = 128;   // the hidden width this file is written for

__host__ __device__ inline int hm_lds_floats(int outP) {
    return HM_H * outP + HM_H + HM_H + 32 + 32 + 32 + 64 + 2 * GW_K * GF_S + HM_H * GF_S + HM_H * GF_S + outP * GF_S;
}

// the family's images at 128 units: no W1 and no W2 image; m.x names buffer 0 of the two X chunk buffers (gm_x), m.obsP is the chunk width
__device__ __forceinline__ GfLds hm_carve(float* base, int outP) {
    GfLds m;
    m.obsP = GW_K; m.outP = outP;
    float* p = base;
    m.w1 = nullptr; m.w2 = nullptr;
    m.w3 = p; p += HM_H * outP;
    m.b1 = p; p += HM_H;
    m.b2 = p; p += HM_H;
    m.b3 = p; p += 32;
    m.ls = p; p += 32;
    m.inv = p; p += 32;
    m.ridx = reinterpret_cast<int*>(p); p += 64;
    m.x = p; p += 2 * GW_K * GF_S;
    m.h1 = p; p += HM_H * GF_S;
    m.h2 = p; p += HM_H * GF_S;
    m.o = p;
    return m;
}

// one net's layer 3, the biases, log_std and exp(-log_std) into LDS (zero padded); the caller's next barrier publishes it
__device__ __forceinline__ void hm_stage_upper(const GfLds& m, const GfShape& sh, const float* __restrict__ params, int net, int tid) {
    const int out = net == 0 ? 1 : sh.A;
    const float* W3 = params + sh.off[net][4];
    for (int i = tid; i < HM_H * m.outP; i += GF_THREADS) m.w3[i] = (i >> 7) < out ? W3[i] : 0.0f;
    if (tid < HM_H) { m.b1[tid] = params[sh.off[net][1] + tid]; m.b2[tid] = params[sh.off[net][3] + tid]; }
    if (tid < 32) {
        m.b3[tid] = tid < out ? params[sh.off[net][5] + tid] : 0.0f;
        const float ls = tid < sh.D ? params[sh.logstd_off + tid] : 0.0f;
        m.ls[tid] = ls;
        m.inv[tid] = expf(-ls);
    }
}

// acc[i][j] += A_i B_j over quarters 0 .. nq - 1 (16 k each): A_i the lane's operand of row tile i, B_j [k][16 j + e] out of an image [k][sample]
__device__ __forceinline__ void hm_mma_k(const float (&a)[2][16], const float* __restrict__ img, int nq, int e, int kg, gm_f4 (&acc)[2][4]) {
#pragma unroll
    for (int t = 0; t < 16; t++) {
        if ((t >> 2) < nq) {   // uniform
            const float* row = img + gm_k(t, kg) * GF_S + e;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float b = row[16 * j];
                acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][t], b, acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][t], b, acc[1][j], 0, 0, 0);
            }
        }
    }
}

// acc[i][j][r] = b[32 w + 16 i + 4 kg + r]: a hidden layer's accumulators start at the bias
__device__ __forceinline__ void hm_bias(const float* __restrict__ b, int w, int kg, gm_f4 (&acc)[2][4]) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const float4 v = *reinterpret_cast<const float4*>(&b[32 * w + 16 * i + 4 * kg]);
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = gm_f4{ v.x, v.y, v.z, v.w };
    }
}
// out[32 w + 16 i + 4 kg + r][16 j + e] = tanh(acc[i][j][r])
__device__ __forceinline__ void hm_store_tanh(float* __restrict__ out, int w, int e, int kg, const gm_f4 (&acc)[2][4]) {
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) out[(32 * w + 16 * i + 4 * kg + r) * GF_S + 16 * j + e] = tanh_fast(acc[i][j][r]);
}

// the wave's slice of one net's W2, the A operand of layer 2: a2[h][i] = rows 32 w + 16 i + e, columns 64 h + gm_k(t, kg)
__device__ __forceinline__ void hm_fetch_w2(const GfShape& sh, const float* __restrict__ params, int net, int tid, float (&a2)[2][2][16]) {
    const int e = tid & 15, kg = (tid >> 4) & 3, w = tid >> 6;
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int i = 0; i < 2; i++) gm_fetch_a(params + sh.off[net][2], HM_H, HM_H, 64 * h, 32 * w + 16 * i + e, kg, a2[h][i]);
}

// the output layer: H2 (post-tanh, complete behind the caller's barrier) -> OUT rows 0 .. out - 1; wave w owns units w, w + 4, ... (< out <= 32); lane = sample
__device__ __forceinline__ void hm_output_layer(const GfLds& m, int out, int s, int w) {
    const int nu = (out - w + 3) >> 2;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = m.b3[(4 * i + w) & 31];
    for (int k = 0; k < HM_H; k += 4) {
        const float x0 = m.h2[(k + 0) * GF_S + s], x1 = m.h2[(k + 1) * GF_S + s], x2 = m.h2[(k + 2) * GF_S + s], x3 = m.h2[(k + 3) * GF_S + s];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (i < nu) {
                const float4 wv = *reinterpret_cast<const float4*>(&m.w3[(4 * i + w) * HM_H + k]);
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

// THE forward pass of every kernel in this file: the tile whose row indices are in m.ridx (published by the caller's barrier, as are the staged upper layers)
// through obs -> 128 -> 128 -> out, layer 1 over nc = ceil(O / 64) chunks.  a2 is the wave's slice of W2 (hm_fetch_w2, once per kernel).  Leaves H1, H2
// (post-tanh), OUT rows 0 .. out - 1, chunk nc - 1 of X in buffer (nc - 1) & 1 and chunk nc - 2 in the other.  Every thread of the workgroup calls it; the
// caller's barrier behind the previous tile has freed every image.
__device__ __forceinline__ void hm_forward_tile(const GfLds& m, const GfShape& sh, const float* __restrict__ params, int net, const float* __restrict__ obs, int nc,
                                                int out, int tid, const float (&a2)[2][2][16]) {
    const int s = tid & 63, e = tid & 15, kg = (tid >> 4) & 3, w = __builtin_amdgcn_readfirstlane(tid >> 6), O = sh.obs;
    const float* W1 = params + sh.off[net][0];
    float ra[2][16], rn[2][16], rx[16];
    gm_f4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; i++) gm_fetch_a(W1, O, O, 0, 32 * w + 16 * i + e, kg, ra[i]);
    gw_fetch_x(obs, O, m.ridx, 0, tid, rx);
    hm_bias(m.b1, w, kg, acc);
    gw_store_x(gm_x(m, 0), tid, rx);
    __syncthreads();
    for (int c = 0; c + 1 < nc; c++) {
#pragma unroll
        for (int i = 0; i < 2; i++) gm_fetch_a(W1, O, O, GW_K * (c + 1), 32 * w + 16 * i + e, kg, rn[i]);
        gw_fetch_x(obs, O, m.ridx, c + 1, tid, rx);
        hm_mma_k(ra, gm_x(m, c & 1), (gw_chunk_cols(O, c) + 15) >> 4, e, kg, acc);
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int t = 0; t < 16; t++) ra[i][t] = rn[i][t];
        gw_store_x(gm_x(m, (c + 1) & 1), tid, rx);
        __syncthreads();
    }
    hm_mma_k(ra, gm_x(m, (nc - 1) & 1), (gw_chunk_cols(O, nc - 1) + 15) >> 4, e, kg, acc);
    hm_store_tanh(m.h1, w, e, kg, acc);
    __syncthreads();
    hm_bias(m.b2, w, kg, acc);
    hm_mma_k(a2[0], m.h1, 4, e, kg, acc);
    hm_mma_k(a2[1], m.h1 + 64 * GF_S, 4, e, kg, acc);
    hm_store_tanh(m.h2, w, e, kg, acc);
    __syncthreads();
    hm_output_layer(m, out, s, w);
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------
// The act kernels, the critic and the fold: kernels_fused_matrix.hip's, line for line, behind this file's forward.
// ---------------------------------------------------------------------------------------------------------
template <bool GREEDY>
__global__ __launch_bounds__(GF_THREADS) void hm_gauss_act_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs,
                                                                  const float* __restrict__ forced, int64_t n, int64_t seed, int64_t row_offset, int64_t step_index,
                                                                  float* action, float* logprob, float* entropy, GfStepStores st) {
    extern __shared__ __attribute__((aligned(16))) float hm_lds[];
    const int tid = threadIdx.x, D = sh.D, O = sh.obs, nc = gw_chunks(O);
    const GfLds m = hm_carve(hm_lds, gf_pad4(D));
    hm_stage_upper(m, sh, params, 1, tid);
    float a2[2][2][16];
    hm_fetch_w2(sh, params, 1, tid, a2);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(m, row0, n, tid);
        hm_forward_tile(m, sh, params, 1, obs, nc, D, tid, a2);
        gauss_act_rows<GREEDY>(m, D, O, obs, forced, row0, n, seed, row_offset, step_index, action, logprob, entropy, st, tid);
        __syncthreads();   // OUT and the row list are read: the next tile may overwrite them
    }
}

template <int DIST, bool GREEDY>
__global__ __launch_bounds__(GF_THREADS) void hm_cat_act_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs,
                                                                const uint8_t* __restrict__ mask, const int64_t* __restrict__ forced, int64_t n, int64_t seed,
                                                                int64_t row_offset, int64_t step_index, int64_t* action, float* logprob, float* entropy,
                                                                CfStepStores st) {
    extern __shared__ __attribute__((aligned(16))) float hm_lds[];
    const int tid = threadIdx.x, A = sh.A, nc = gw_chunks(sh.obs);
    const GfLds m = hm_carve(hm_lds, gf_pad4(A));
    hm_stage_upper(m, sh, params, 1, tid);
    float a2[2][2][16];
    hm_fetch_w2(sh, params, 1, tid, a2);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(m, row0, n, tid);
        hm_forward_tile(m, sh, params, 1, obs, nc, A, tid, a2);
        cat_act_rows<DIST, GREEDY>(m, sh, obs, mask, forced, row0, n, seed, row_offset, step_index, action, logprob, entropy, st, tid);
        __syncthreads();   // OUT, the H1 columns and the row list are read: the next tile may overwrite them
    }
}

// the critic over n rows
__global__ __launch_bounds__(GF_THREADS) void hm_values_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs, int64_t n,
                                                               float* __restrict__ value) {
    extern __shared__ __attribute__((aligned(16))) float hm_lds[];
    const int tid = threadIdx.x, nc = gw_chunks(sh.obs);
    const GfLds m = hm_carve(hm_lds, 4);
    hm_stage_upper(m, sh, params, 0, tid);
    float a2[2][2][16];
    hm_fetch_w2(sh, params, 0, tid, a2);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(m, row0, n, tid);
        hm_forward_tile(m, sh, params, 0, obs, nc, 1, tid, a2);
        if (tid < 64 && row0 + tid < n) value[row0 + tid] = m.o[tid];
        __syncthreads();
    }
}

// ppo_dev_observe with truncation flags: gm_dev_fold_kernel's front end (one compaction per 256 env rows, a workgroup without a flagged row returns before it
// loads a weight), then hm_values_kernel's forward on the listed rows of final_obs: v is that kernel's value of the row, bit for bit.  LDS: all dynamic, the
// row list [256] and the waves' totals [8] behind the carve.
__global__ __launch_bounds__(DEV_FOLD_THREADS) void hm_dev_fold_kernel(GfShape sh, const float* __restrict__ params, DevFoldArgs a) {
    static_assert(DEV_FOLD_THREADS == GF_THREADS, "fold_compact and hm_forward_tile are written for the same workgroup");
    extern __shared__ __attribute__((aligned(16))) float hm_lds[];
    const int tid = threadIdx.x, nc = gw_chunks(sh.obs);
    int* list = reinterpret_cast<int*>(hm_lds + hm_lds_floats(4));
    int* wtot = list + DEV_FOLD_THREADS;
    const int cnt = dev_fold_compact(a, list, wtot);
    if (cnt == 0) return;
    const int base = wtot[4];
    const GfLds m = hm_carve(hm_lds, 4);
    hm_stage_upper(m, sh, params, 0, tid);
    float a2[2][2][16];
    hm_fetch_w2(sh, params, 0, tid, a2);
    for (int k0 = 0; k0 < cnt; k0 += 64) {
        const int k = k0 + tid;   // tid < 64: this lane's place in the list
        if (tid < 64) m.ridx[tid] = k < cnt ? list[k] : -1;
        __syncthreads();
        hm_forward_tile(m, sh, params, 0, a.final_obs, nc, 1, tid, a2);
        if (tid < 64 && k < cnt) dev_fold_store(a, base, k, list[k], m.o[tid]);
        __syncthreads();   // OUT and the row indices are read: the next tile may overwrite them
    }
}

// ---------------------------------------------------------------------------------------------------------
// hm_fwd_bwd_kernel<DIST>: one minibatch step of one net per workgroup column (blockIdx.y = net), every nc in one instantiation.
// ---------------------------------------------------------------------------------------------------------
// the A operand of a product over the tile's samples: row u of an image [unit][sample], sample gm_k(t, kg) at step t (four 16-byte reads)
__device__ __forceinline__ void hm_load_a_s(const float* __restrict__ img, int u, int kg, float (&a)[16]) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float4 v = *reinterpret_cast<const float4*>(&img[u * GF_S + 16 * q + 4 * kg]);
        a[4 * q + 0] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
    }
}
// acc[i][j] += A_i B_j^T over the 64 samples, j < nj <= NJ: B_j = rows 16 j + e of an image [row][sample]
template <int NJ>
__device__ __forceinline__ void hm_mma_s(const float (&a)[2][16], const float* __restrict__ img, int nj, int e, int kg, gm_f4 (&acc)[2][NJ]) {
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        if (j < nj) {   // uniform
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 v = *reinterpret_cast<const float4*>(&img[(16 * j + e) * GF_S + 16 * q + 4 * kg]);
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][4 * q + 0], v.x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][4 * q + 1], v.y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][4 * q + 2], v.z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][4 * q + 3], v.w, acc[i][j], 0, 0, 0);
                }
            }
        }
    }
}
// the sum of a row of the image over its 64 samples out of the operand hm_load_a_s left: the lane's 16 in step order, then the four k-slots (every lane of the
// unit ends with the same bits)
__device__ __forceinline__ float hm_row_sum(const float (&a)[16]) {
    float v = a[0];
#pragma unroll
    for (int t = 1; t < 16; t++) v += a[t];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// h[k][s] <- (sum_o W[o][k] dout[o][s]) (1 - h[k][s]^2), o ascending below n_out: dZ2 in H2's place (gf_dz_tile over 128 units: W is the staged W3
// [o][128]).  lane = sample, wave w owns k = 32 w .. 32 w + 31; a thread reads and writes only its own elements of h
__device__ __forceinline__ void hm_dz_tile(const float* __restrict__ dout, int n_out, const float* __restrict__ W, float* h, int s, int w) {
    float acc[32];
#pragma unroll
    for (int i = 0; i < 32; i++) acc[i] = 0.0f;
    for (int o = 0; o < n_out; o++) {
        const float d = dout[o * GF_S + s];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const float4 wv = *reinterpret_cast<const float4*>(&W[o * HM_H + 32 * w + 4 * q]);
            acc[4 * q + 0] = __builtin_fmaf(wv.x, d, acc[4 * q + 0]);
            acc[4 * q + 1] = __builtin_fmaf(wv.y, d, acc[4 * q + 1]);
            acc[4 * q + 2] = __builtin_fmaf(wv.z, d, acc[4 * q + 2]);
            acc[4 * q + 3] = __builtin_fmaf(wv.w, d, acc[4 * q + 3]);
        }
    }
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const float a = h[(32 * w + i) * GF_S + s];
        h[(32 * w + i) * GF_S + s] = acc[i] * (1.0f - a * a);
    }
}

// What a wave carries across its tiles: gb1 / gb2 [i] = the bias gradient of unit 32 w + 16 i + e (the same bits in its four k-slots); gW3 / gb3 on the thread
// grid ub = tid >> 5 (output units 4 ub ..), kb = tid & 31 (columns 4 kb ..); the loss lanes' state.  dW1 and dW2 live in the workgroup's slab between the
// tiles (the head of the file): element r of product tile [i][j] is row 32 w + 16 i + 4 kg + r, column 16 j + e (dW1: of the chunk).
template <int DIST>
__global__ __launch_bounds__(GF_THREADS) void hm_fwd_bwd_kernel(GfUpdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float hm_lds[];
    const int tid = threadIdx.x, O = a.sh.obs, nc = gw_chunks(O);
    const int net = blockIdx.y, b = blockIdx.x, nb = a.nb;
    const int out = net == 0 ? 1 : a.sh.A, outP = gf_pad4(out);
    const GfLds m = hm_carve(hm_lds, gf_pad4(a.sh.A));
    hm_stage_upper(m, a.sh, a.params, net, tid);
    const int s = tid & 63, e = tid & 15, kg = (tid >> 4) & 3, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ub = tid >> 5, kb = tid & 31;
    const float* W2 = a.params + a.sh.off[net][2];
    float* slab = a.slab + ((size_t)net * nb + b) * a.slab_stride;

    float gW3[16], gb3[4], gb1[2] = { 0.0f, 0.0f }, gb2[2] = { 0.0f, 0.0f };
    const gm_f4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
    for (int i = 0; i < 16; i++) gW3[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) gb3[i] = 0.0f;
    GfLossState ls;
    gf_loss_begin(a, net, w, ls);

    const int tiles = (a.M + 63) / 64;
    for (int tile = b; tile < tiles; tile += nb) {
        const bool first = tile == b;   // of this workgroup: its slab elements are stored, not added to
        if (tid < 64) m.ridx[tid] = tile * 64 + tid < a.M ? a.idx[tile * 64 + tid] : -1;
        __syncthreads();
        {
            float a2[2][2][16];
            hm_fetch_w2(a.sh, a.params, net, tid, a2);
            hm_forward_tile(m, a.sh, a.params, net, a.obs, nc, out, tid, a2);
        }
        if (w == 0) gf_loss_lanes<DIST>(a, m, net, out, outP, s, ls);
        __syncthreads();
        if (4 * ub < outP) gf_dw_tile(m.o, m.h2, ub, kb, gW3, gb3);     // dW3 = dOUT H2^T, db3
        __syncthreads();                                                // ... has read H2
        hm_dz_tile(m.o, out, m.w3, m.h2, s, w);                         // H2 <- dZ2
        __syncthreads();
        float dz[2][16];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            hm_load_a_s(m.h2, 32 * w + 16 * i + e, kg, dz[i]);
            gb2[i] += hm_row_sum(dz[i]);                                // db2
        }
        {
            gm_f4 gW2[2][8];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 8; j++) gW2[i][j] = zero;
            hm_mma_s<8>(dz, m.h1, 8, e, kg, gW2);                       // dW2 = dZ2 H1^T
            float* dW2 = slab + (a.sh.off[net][2] - a.sh.off[net][0]);
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 8; j++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        float* p = &dW2[(32 * w + 16 * i + 4 * kg + r) * HM_H + 16 * j + e];
                        *p = first ? gW2[i][j][r] : *p + gW2[i][j][r];
                    }
        }
        __syncthreads();                                                // ... has read H1
        {   // H1 <- dZ1 = (W2^T dZ2)(1 - H1^2): A[unit u][o] = W2[o][u], u = 32 w + 16 i + e, one 64-deep half of o at a time
            gm_f4 d[2][4] = { { zero, zero, zero, zero }, { zero, zero, zero, zero } };
#pragma unroll
            for (int h = 0; h < 2; h++) {
                float wt[2][16];
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int t = 0; t < 16; t++) wt[i][t] = W2[(64 * h + gm_k(t, kg)) * HM_H + 32 * w + 16 * i + e];
                hm_mma_k(wt, m.h2 + 64 * h * GF_S, 4, e, kg, d);
            }
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        float* hp = &m.h1[(32 * w + 16 * i + 4 * kg + r) * GF_S + 16 * j + e];
                        const float v = *hp;
                        *hp = d[i][j][r] * (1.0f - v * v);
                    }
        }
        __syncthreads();
        // dW1 = dZ1 X^T, db1: chunk c out of buffer c & 1 (chunks nc - 1 and nc - 2 are the forward's; chunk c - 2 arrives behind chunk c's barrier); the
        // chunk's sum from zero goes to the slab: stored by the workgroup's first tile, added by a later one
#pragma unroll
        for (int i = 0; i < 2; i++) {
            hm_load_a_s(m.h1, 32 * w + 16 * i + e, kg, dz[i]);
            gb1[i] += hm_row_sum(dz[i]);
        }
        float rx[16];
        for (int c = nc - 1; c >= 0; c--) {
            if (c >= 2) gw_fetch_x(a.obs, O, m.ridx, c - 2, tid, rx);
            gm_f4 g[2][4] = { { zero, zero, zero, zero }, { zero, zero, zero, zero } };
            hm_mma_s<4>(dz, gm_x(m, c & 1), (gw_chunk_cols(O, c) + 15) >> 4, e, kg, g);
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int k = GW_K * c + 16 * j + e;
                    if (k < O) {
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            float* p = &slab[(32 * w + 16 * i + 4 * kg + r) * O + k];
                            *p = first ? g[i][j][r] : *p + g[i][j][r];
                        }
                    }
                }
            __syncthreads();                                 // ... has read the buffer; behind chunk 0: the images are free for the next tile
            if (c >= 2) gw_store_x(gm_x(m, c & 1), tid, rx);
        }
    }

    const int base = a.sh.off[net][0];
    float* dW3 = slab + (a.sh.off[net][4] - base);
#pragma unroll
    for (int i = 0; i < 2; i++) {
        if (kg == 0) {
            slab[a.sh.off[net][1] - base + 32 * w + 16 * i + e] = gb1[i];
            slab[a.sh.off[net][3] - base + 32 * w + 16 * i + e] = gb2[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int u = 4 * ub + i;
#pragma unroll
        for (int j = 0; j < 4; j++) if (u < out) dW3[u * HM_H + 4 * kb + j] = gW3[i * 4 + j];
        if (kb == 0 && u < out) slab[a.sh.off[net][5] - base + u] = gb3[i];
    }
    gf_store_loss<DIST>(a, slab, net, b, s, w, ls);
}

template <int DIST>
hipError_t hm_upd_launch(const GfUpdArgs& a, int bytes, hipStream_t s) {
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, hm_fwd_bwd_kernel<DIST>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((hm_fwd_bwd_kernel<DIST>), dim3(a.nb, 2), dim3(GF_THREADS), bytes, s, a);
    return hipGetLastError();
}

template <int DIST, bool GREEDY>
hipError_t hm_cat_act_launch(const GfShape& sh, int bytes, dim3 grid, const float* params, const float* obs, const uint8_t* mask, const int64_t* forced, int64_t n,
                             int64_t seed, int64_t row_offset, int64_t step_index, int64_t* action, float* logprob, float* entropy, const CfStepStores& ss, hipStream_t s) {
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, hm_cat_act_kernel<DIST, GREEDY>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((hm_cat_act_kernel<DIST, GREEDY>), grid, dim3(GF_THREADS), bytes, s, sh, params, obs, mask, forced, n, seed, row_offset, step_index, action,
                       logprob, entropy, ss);
    return hipGetLastError();
}

// the shapes this file's kernels are launched for: 2 x 128, one to six chunks
bool hm_shape_ok(const GenLayout& L) {
    return L.fused_matrix && L.hidden == HM_H && L.n_hidden == 2 && L.obs >= 1 && L.obs <= FUSED_WIDE_MAX_OBS && L.act >= 1 && L.act <= PPO_MAX_ACT;
}

}  // namespace

hipError_t fused_matrix_h128_gauss_act(const GenLayout& L, const float* params, const float* obs, const float* forced, int64_t n, int64_t seed, int64_t row_offset,
                                       int64_t step_index, bool greedy, float* action, float* logprob, float* entropy, const GaussStepStores* st, hipStream_t s) {
    if (!hm_shape_ok(L) || !L.gauss) return hipErrorInvalidValue;
    const GfShape sh = gf_shape(L);
    const int bytes = hm_lds_floats(gf_pad4(L.gauss)) * 4;
    const dim3 grid((unsigned)std::min<int64_t>((n + 63) / 64, 1024)), block(GF_THREADS);
    GfStepStores ss{};
    if (st) ss = GfStepStores{ st->done_prev, st->obs_t, st->act_t, st->lp_t, st->dones_t };
    static std::atomic<unsigned long long> done_g{ 0 }, done_s{ 0 };
    if (greedy) {
        const hipError_t e = gf_allow(done_g, hm_gauss_act_kernel<true>, bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(hm_gauss_act_kernel<true>, grid, block, bytes, s, sh, params, obs, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss);
    } else {
        const hipError_t e = gf_allow(done_s, hm_gauss_act_kernel<false>, bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(hm_gauss_act_kernel<false>, grid, block, bytes, s, sh, params, obs, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss);
    }
    return hipGetLastError();
}

hipError_t fused_matrix_h128_cat_act(const GenLayout& L, int dist_kind, const float* params, const float* obs, const uint8_t* mask, const int64_t* forced, int64_t n,
                                     int64_t seed, int64_t row_offset, int64_t step_index, bool greedy, int64_t* action, float* logprob, float* entropy,
                                     const CatStepStores* st, hipStream_t s) {
    if (!hm_shape_ok(L) || L.gauss) return hipErrorInvalidValue;
    const GfShape sh = gf_shape(L);
    const int bytes = hm_lds_floats(gf_pad4(L.act)) * 4;
    const dim3 grid((unsigned)std::min<int64_t>((n + 63) / 64, 1024));
    CfStepStores ss{};
    if (st) ss = CfStepStores{ st->done_prev, st->obs_t, st->mask_t, st->act_t, st->lp_t, st->dones_t };
    const bool masked = dist_kind == PPO_DIST_MASKED;
    if (greedy)
        return masked ? hm_cat_act_launch<PPO_DIST_MASKED, true>(sh, bytes, grid, params, obs, mask, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss, s)
                      : hm_cat_act_launch<PPO_DIST_CATEGORICAL, true>(sh, bytes, grid, params, obs, mask, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss, s);
    return masked ? hm_cat_act_launch<PPO_DIST_MASKED, false>(sh, bytes, grid, params, obs, mask, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss, s)
                  : hm_cat_act_launch<PPO_DIST_CATEGORICAL, false>(sh, bytes, grid, params, obs, mask, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss, s);
}

hipError_t fused_matrix_h128_values(const GenLayout& L, const float* params, const float* obs, int64_t n, float* value, hipStream_t s) {
    if (!hm_shape_ok(L)) return hipErrorInvalidValue;
    const GfShape sh = gf_shape(L);
    const int bytes = hm_lds_floats(4) * 4;
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, hm_values_kernel, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hm_values_kernel, dim3((unsigned)std::min<int64_t>((n + 63) / 64, 1024)), dim3(GF_THREADS), bytes, s, sh, params, obs, n, value);
    return hipGetLastError();
}

hipError_t fused_matrix_h128_dev_fold(const GenLayout& L, const float* params, const DevFoldArgs& a, hipStream_t s) {
    if (!hm_shape_ok(L)) return hipErrorInvalidValue;
    const GfShape sh = gf_shape(L);
    // the row list and the waves' totals are part of the dynamic allocation: the attribute is decided on every byte of LDS the kernel uses
    const int bytes = hm_lds_floats(4) * 4 + GF_DEV_FOLD_LIST_INTS * (int)sizeof(int);
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, hm_dev_fold_kernel, bytes);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)(((int64_t)a.N + DEV_FOLD_THREADS - 1) / DEV_FOLD_THREADS);
    hipLaunchKernelGGL(hm_dev_fold_kernel, dim3(grid), dim3(DEV_FOLD_THREADS), bytes, s, sh, params, a);
    return hipGetLastError();
}

hipError_t fused_matrix_h128_fwd_bwd(const GenLayout& L, const GfUpdArgs& a, float* grads, hipStream_t s) {
    if (!hm_shape_ok(L)) return hipErrorInvalidValue;
    const int bytes = hm_lds_floats(gf_pad4(L.act)) * 4;
    hipError_t e;
    if (L.gauss) e = hm_upd_launch<PPO_DIST_GAUSSIAN>(a, bytes, s);
    else if (a.hp.dist_kind == PPO_DIST_MASKED) e = hm_upd_launch<PPO_DIST_MASKED>(a, bytes, s);
    else e = hm_upd_launch<PPO_DIST_CATEGORICAL>(a, bytes, s);
    if (e != hipSuccess) return e;
    return gauss_fused_slab_reduce(L, a.slab, a.slab_stride, a.nb, grads, s);
}
