// ppo-libtorch_amd/csrc/kernels_fused_matrix.hip -- PPO_KERNEL_FUSED_MATRIX: the fused 2 x 64 families (PPO_KERNEL_GAUSS_FUSED, PPO_KERNEL_CAT_FUSED) with their
// four 64-wide products on the f32 matrix cores (v_mfma_f32_16x16x4_f32: D[i][j] += sum_k A[i][k] B[k][j], 4 k per instruction, plain f32 operands and f32
// accumulation -- no split terms, no operand range, no fall-back launch).  ONE kernel set for every observation width a flagged context accepts:
// kernels_fused_wide.hip's chunk structure with nc = ceil(obs / 64) = 1 .. 6, nc = 1 being the resident case.  Everything that is not such a product is the
// family's (gauss_fused_dev.hpp): one workgroup = 4 waves = one 64-sample tile at a time, H1 / H2 / OUT / X as [unit][sample] images of stride GF_S, the heads,
// draws, loss lanes, stores, slab layout and gauss_slab_reduce_kernel, and layer 3 with its backward (out <= 32), which stay on the vector functions.
//
// The lane map.  lane = 16 kg + e.  Wave w owns units 16 w .. 16 w + 15 of all 64 samples, as gf_hidden_layer does: four 16 x 16 accumulator tiles j = 0 .. 3
// (samples 16 j + e), 16 VGPRs; element r of tile j in lane (e, kg) is unit 16 w + 4 kg + r of sample 16 j + e.  An instruction takes one A value (row e,
// k-slot kg) and one B value (column e, k-slot kg) per lane.  Step t = 0 .. 15 of a 64-deep product uses k = gm_k(t, kg) = 16 (t >> 2) + 4 kg + (t & 3) -- any
// bijection serves as long as both operands use it; this one makes
//   * a B read of an image [k][sample] hit rows 4 kg + const: 272 kg floats apart, 16 kg banks apart -- the four k-slots of a step share no bank;
//   * an operand whose k runs ALONG an image row (the backward's sums over samples) one 16-byte LDS read per four steps;
//   * a lane's 16 W1 values of a chunk four runs of four consecutive floats, the four k-slots of a unit together 64 consecutive bytes.
// Steps are issued in quarters of four (16 k each); quarters behind a ragged chunk's last column are skipped (both operands hold zeros there).
//
//   layer 1, chunk by chunk: A = the wave's 16 x 64 slice of the W1 chunk, B = the X chunk image [k][sample]; the 16 accumulators start at the bias and live
//            across all chunks; one tanh_fast and one store into H1 behind the last chunk.
//            W1 does NOT pass through LDS: a wave needs only its own slice, 16 VGPRs per lane, and every element of it is used by exactly one lane -- an LDS
//            round trip would add a store, a barrier dependency and a read of 16 rows at one k (stride 64: one bank) to move each value once.  The slice goes
//            from global / L2 straight into the fragment registers; the wide kernels' two 16 KB W1 chunk buffers are gone from the carve.
//            The wide kernel's software pipeline stands: chunk c + 1's W1 slice and X elements are loaded (32 registers) in front of chunk c's products, the X
//            elements go into buffer (c + 1) & 1 behind them, one barrier per chunk.
//   layer 2: the same product, A = the wave's slice of W2 held in 16 registers for the whole kernel (loaded once per workgroup), B = H1.
//   dZ1 = (W2^T dZ2)(1 - H1^2): A = W2^T out of the resident LDS copy (lanes e consecutive: no conflict within a k-slot), B = the dZ2 image.
//   dW2 = dZ2 H1^T, dW1 = dZ1 X^T: K is the tile's 64 samples; A = the wave's 16 rows of dZ (four float4 LDS reads, kept across the dW1 chunks), B = rows of H1 /
//            of the X chunk.  dW1 goes into 16 accumulator VGPRs per chunk (96 at NC = 6); the chunks walk downward, so the forward's last two X chunks are
//            reused.  db2 / db1 come from the same pass: the lane's 16 A values summed, then the four k-slots by two lane exchanges.  A sample without a row has
//            dOUT = 0, hence dZ2 = dZ1 = +-0 and X = 0: exact zeros on both operands.
// One forward function (gm_forward_tile) serves all five kernels: an observation gets the same mean / logits and the same value from every entry point, bit for
// bit.  No float atomics anywhere: equal inputs give equal bits on every run.  The summation order is the instruction's, so the bits differ from the vector
// kernels'.
//
// LDS (floats; outP = the output width rounded up to 4; the update kernel carves for the wider net, the actor):
//   W2 4096 | W3 64 outP | b1 64 | b2 64 | b3 32 | log_std 32 | exp(-log_std) 32 | row index 64 | X 2 x 64 68 | H1 64 68 | H2 64 68 | OUT outP 68
//   32 outputs: 4096 + 2048 + 288 + 8704 + 4352 + 4352 + 2176 = 26 016 floats = 104 064 bytes; 1 output: 4096 + 256 + 288 + 8704 + 8704 + 272 = 22 320 floats
//   = 89 280 bytes (the fold adds its list, 1 056).  One workgroup per CU.  The size does not depend on obs_size.
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; __launch_bounds__(256): one wave per SIMD, 512 registers; scratch 0 bytes/lane in every
// kernel of this file; LDS is all dynamic, the sizes above):
//   gm_fwd_bwd_kernel<GAUSSIAN, 6>: 256 VGPRs + 205 AGPRs, LDS 104 064 bytes at D = 32 (D = 17: 97 728), scratch 0
//   gm_fwd_bwd_kernel<MASKED, 6>:   256 VGPRs + 250 AGPRs, scratch 0; <CATEGORICAL, 6>: 256 + 209, scratch 0
//   gm_fwd_bwd_kernel<GAUSSIAN, 1>: 222 VGPRs + 48 AGPRs, scratch 0
//   gm_gauss_act_kernel / gm_cat_act_kernel: 128 .. 132 VGPRs + 28 AGPRs; gm_values_kernel: 114 + 28; gm_dev_fold_kernel: 116 + 28; scratch 0
//   "Must not spill" is met in the sense that nothing goes to memory.  Where the 256 architectural VGPRs run out the compiler parks values in AGPRs (its
//   "VGPRs Spill" count; v_accvgpr moves, register to register): 54 in <MASKED, 6>, 38 / 19 / 2 in <MASKED, 5 / 4 / 3>, 16 in <CATEGORICAL, 6>, 0 in every
//   other instantiation, the Gaussian ones included.
#include "fused_matrix_dev.hpp"

namespace {

// the A operand of a product over the tile's samples: row u of an image [unit][sample], sample gm_k(t, kg) at step t (four 16-byte reads)
__device__ __forceinline__ void gm_load_a_s(const float* __restrict__ img, int u, int kg, float (&a)[16]) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float4 v = *reinterpret_cast<const float4*>(&img[u * GF_S + 16 * q + 4 * kg]);
        a[4 * q + 0] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
    }
}
// acc[j] += A B_j^T over the 64 samples, j < nj: B_j = rows 16 j + e of an image [row][sample]
__device__ __forceinline__ void gm_mma_s(const float (&a)[16], const float* __restrict__ img, int nj, int e, int kg, gm_f4 (&acc)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (j < nj) {   // uniform
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 v = *reinterpret_cast<const float4*>(&img[(16 * j + e) * GF_S + 16 * q + 4 * kg]);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 0], v.x, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 1], v.y, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 2], v.z, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 3], v.w, acc[j], 0, 0, 0);
            }
        }
    }
}
// the sum of row u of the image over its 64 samples out of the operand gm_load_a_s left: the lane's 16 in step order, then the four k-slots (every lane of the
// unit ends with the same bits)
__device__ __forceinline__ float gm_row_sum(const float (&a)[16]) {
    float v = a[0];
#pragma unroll
    for (int t = 1; t < 16; t++) v += a[t];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// THE forward pass of every kernel in this file: the tile whose row indices are in m.ridx (published by the caller's barrier, as are the staged upper layers)
// through obs -> 64 -> 64 -> out, layer 1 over nc = ceil(O / 64) chunks.  a2 is the wave's slice of W2 (gm_fetch_a, once per kernel).  Leaves H1, H2
// (post-tanh), OUT rows 0 .. out - 1, chunk nc - 1 of X in buffer (nc - 1) & 1 and chunk nc - 2 in the other.  Every thread of the workgroup calls it; the
// caller's barrier behind the previous tile has freed every image.
__device__ __forceinline__ void gm_forward_tile(const GfLds& m, const GfShape& sh, const float* __restrict__ params, int net, const float* __restrict__ obs, int nc,
                                                int out, int tid, const float (&a2)[16]) {
    const int e = tid & 15, kg = (tid >> 4) & 3, w = __builtin_amdgcn_readfirstlane(tid >> 6), O = sh.obs;
    const float* W1 = params + sh.off[net][0];
    float ra[16], rn[16], rx[16];
    gm_f4 acc[4];
    // the fetch: every chunk's operands, and the products of the chunks in front of the last
    gm_fetch_a(W1, O, O, 0, 16 * w + e, kg, ra);
    gw_fetch_x(obs, O, m.ridx, 0, tid, rx);
    gm_bias(m.b1, w, kg, acc);
    gw_store_x(gm_x(m, 0), tid, rx);
    __syncthreads();
    for (int c = 0; c + 1 < nc; c++) {
        gm_fetch_a(W1, O, O, GW_K * (c + 1), 16 * w + e, kg, rn);
        gw_fetch_x(obs, O, m.ridx, c + 1, tid, rx);
        gm_mma_k(ra, gm_x(m, c & 1), (gw_chunk_cols(O, c) + 15) >> 4, e, kg, acc);
#pragma unroll
        for (int t = 0; t < 16; t++) ra[t] = rn[t];
        gw_store_x(gm_x(m, (c + 1) & 1), tid, rx);
        __syncthreads();
    }
    // the products on the operand registers (fused_matrix_dev.hpp), shared with the device envs' rollouts
    gm_forward_regs(m, ra, gm_x(m, (nc - 1) & 1), (gw_chunk_cols(O, nc - 1) + 15) >> 4, acc, a2, out, tid);
}

// ---------------------------------------------------------------------------------------------------------
// The act kernels, the critic and the fold: kernels_fused_wide.hip's, line for line, behind this file's forward.
// ---------------------------------------------------------------------------------------------------------
template <bool GREEDY>
__global__ __launch_bounds__(GF_THREADS) void gm_gauss_act_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs,
                                                                  const float* __restrict__ forced, int64_t n, int64_t seed, int64_t row_offset, int64_t step_index,
                                                                  float* action, float* logprob, float* entropy, GfStepStores st) {
    extern __shared__ __attribute__((aligned(16))) float gm_lds[];
    const int tid = threadIdx.x, D = sh.D, O = sh.obs, nc = gw_chunks(O);
    const GfLds m = gm_carve(gm_lds, gf_pad4(D));
    gf_stage_upper(m, sh, params, 1, tid);
    float a2[16];
    gm_fetch_w2(sh, params, 1, tid, a2);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(m, row0, n, tid);
        gm_forward_tile(m, sh, params, 1, obs, nc, D, tid, a2);
        gauss_act_rows<GREEDY>(m, D, O, obs, forced, row0, n, seed, row_offset, step_index, action, logprob, entropy, st, tid);
        __syncthreads();   // OUT and the row list are read: the next tile may overwrite them
    }
}

template <int DIST, bool GREEDY>
__global__ __launch_bounds__(GF_THREADS) void gm_cat_act_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs,
                                                                const uint8_t* __restrict__ mask, const int64_t* __restrict__ forced, int64_t n, int64_t seed,
                                                                int64_t row_offset, int64_t step_index, int64_t* action, float* logprob, float* entropy,
                                                                CfStepStores st) {
    extern __shared__ __attribute__((aligned(16))) float gm_lds[];
    const int tid = threadIdx.x, A = sh.A, nc = gw_chunks(sh.obs);
    const GfLds m = gm_carve(gm_lds, gf_pad4(A));
    gf_stage_upper(m, sh, params, 1, tid);
    float a2[16];
    gm_fetch_w2(sh, params, 1, tid, a2);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(m, row0, n, tid);
        gm_forward_tile(m, sh, params, 1, obs, nc, A, tid, a2);
        cat_act_rows<DIST, GREEDY>(m, sh, obs, mask, forced, row0, n, seed, row_offset, step_index, action, logprob, entropy, st, tid);
        __syncthreads();   // OUT, the H1 columns and the row list are read: the next tile may overwrite them
    }
}

// the critic over n rows
__global__ __launch_bounds__(GF_THREADS) void gm_values_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs, int64_t n,
                                                               float* __restrict__ value) {
    extern __shared__ __attribute__((aligned(16))) float gm_lds[];
    const int tid = threadIdx.x, nc = gw_chunks(sh.obs);
    const GfLds m = gm_carve(gm_lds, 4);
    gf_stage_upper(m, sh, params, 0, tid);
    float a2[16];
    gm_fetch_w2(sh, params, 0, tid, a2);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(m, row0, n, tid);
        gm_forward_tile(m, sh, params, 0, obs, nc, 1, tid, a2);
        if (tid < 64 && row0 + tid < n) value[row0 + tid] = m.o[tid];
        __syncthreads();
    }
}

// ppo_dev_observe with truncation flags: gw_dev_fold_kernel's front end (one compaction per 256 env rows, a workgroup without a flagged row returns before it
// loads a weight), then gm_values_kernel's forward on the listed rows of final_obs: v is that kernel's value of the row, bit for bit.  LDS: all dynamic, the
// row list [256] and the waves' totals [8] behind the carve.
__global__ __launch_bounds__(DEV_FOLD_THREADS) void gm_dev_fold_kernel(GfShape sh, const float* __restrict__ params, DevFoldArgs a) {
    static_assert(DEV_FOLD_THREADS == GF_THREADS, "fold_compact and gm_forward_tile are written for the same workgroup");
    extern __shared__ __attribute__((aligned(16))) float gm_lds[];
    const int tid = threadIdx.x, nc = gw_chunks(sh.obs);
    int* list = reinterpret_cast<int*>(gm_lds + gm_lds_floats(4));
    int* wtot = list + DEV_FOLD_THREADS;
    const int cnt = dev_fold_compact(a, list, wtot);
    if (cnt == 0) return;
    const int base = wtot[4];
    const GfLds m = gm_carve(gm_lds, 4);
    gf_stage_upper(m, sh, params, 0, tid);
    float a2[16];
    gm_fetch_w2(sh, params, 0, tid, a2);
    for (int k0 = 0; k0 < cnt; k0 += 64) {
        const int k = k0 + tid;   // tid < 64: this lane's place in the list
        if (tid < 64) m.ridx[tid] = k < cnt ? list[k] : -1;
        __syncthreads();
        gm_forward_tile(m, sh, params, 0, a.final_obs, nc, 1, tid, a2);
        if (tid < 64 && k < cnt) dev_fold_store(a, base, k, list[k], m.o[tid]);
        __syncthreads();   // OUT and the row indices are read: the next tile may overwrite them
    }
}

// ---------------------------------------------------------------------------------------------------------
// gm_fwd_bwd_kernel<DIST, NC>: gw_fwd_bwd_kernel's plan for NC = 1 .. 6 chunks with the products of the head of the file.  dW3 / db3 and dZ2 (out <= 32) are
// the family's vector tile functions; dW2, dZ1 and dW1 run on the matrix cores.  A wave's gradient accumulators: gW1[c][j][r] = dW1[16 w + 4 kg + r][64 c +
// 16 j + e], gW2[j][r] = dW2[16 w + 4 kg + r][16 j + e], gb1 / gb2 = the bias gradient of unit 16 w + e (the same bits in its four k-slots).  The slab layout,
// the loss partials and the second launch (gauss_slab_reduce_kernel) are the family's.
// ---------------------------------------------------------------------------------------------------------
template <int DIST, int NC>
__global__ __launch_bounds__(GF_THREADS) void gm_fwd_bwd_kernel(GfUpdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gm_lds[];
    const int tid = threadIdx.x, O = a.sh.obs;
    const int net = blockIdx.y, b = blockIdx.x, nb = a.nb;
    const int out = net == 0 ? 1 : a.sh.A, outP = gf_pad4(out);
    const GfLds m = gm_carve(gm_lds, gf_pad4(a.sh.A));
    gf_stage_upper(m, a.sh, a.params, net, tid);
    const int s = tid & 63, e = tid & 15, kg = (tid >> 4) & 3, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ub = tid >> 4, kb = tid & 15;
    float a2[16];
    gm_fetch_w2(a.sh, a.params, net, tid, a2);

    gm_f4 gW1[NC][4], gW2[4];
    float gW3[16], gb3[4], gb1 = 0.0f, gb2 = 0.0f;
    const gm_f4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int j = 0; j < 4; j++) gW1[c][j] = zero;
#pragma unroll
    for (int j = 0; j < 4; j++) gW2[j] = zero;
#pragma unroll
    for (int i = 0; i < 16; i++) gW3[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) gb3[i] = 0.0f;
    GfLossState ls;
    gf_loss_begin(a, net, w, ls);

    const int tiles = (a.M + 63) / 64;
    for (int tile = b; tile < tiles; tile += nb) {
        if (tid < 64) m.ridx[tid] = tile * 64 + tid < a.M ? a.idx[tile * 64 + tid] : -1;
        __syncthreads();
        gm_forward_tile(m, a.sh, a.params, net, a.obs, NC, out, tid, a2);
        if (w == 0) gf_loss_lanes<DIST>(a, m, net, out, outP, s, ls);
        __syncthreads();
        if (4 * ub < outP) gf_dw_tile(m.o, m.h2, ub, kb, gW3, gb3);     // dW3 = dOUT H2^T, db3
        __syncthreads();                                                // ... has read H2
        gf_dz_tile(m.o, out, m.w3, m.h2, s, w);                         // H2 <- dZ2
        __syncthreads();
        float dz[16];
        gm_load_a_s(m.h2, 16 * w + e, kg, dz);
        gb2 += gm_row_sum(dz);                                          // db2
        gm_mma_s(dz, m.h1, 4, e, kg, gW2);                              // dW2 = dZ2 H1^T
        __syncthreads();                                                // ... has read H1
        {   // H1 <- dZ1 = (W2^T dZ2)(1 - H1^2): A[unit 16 w + e][o] = W2[o][16 w + e]
            float wt[16];
#pragma unroll
            for (int t = 0; t < 16; t++) wt[t] = m.w2[gm_k(t, kg) * 64 + 16 * w + e];
            gm_f4 d[4] = { zero, zero, zero, zero };
            gm_mma_k(wt, m.h2, 4, e, kg, d);
#pragma unroll
            for (int j = 0; j < 4; j++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float* h = &m.h1[(16 * w + 4 * kg + r) * GF_S + 16 * j + e];
                    const float v = *h;
                    *h = d[j][r] * (1.0f - v * v);
                }
            }
        }
        __syncthreads();
        // dW1 = dZ1 X^T, db1: chunk c out of buffer c & 1 (chunks NC - 1 and NC - 2 are the forward's; chunk c - 2 arrives behind chunk c's barrier)
        gm_load_a_s(m.h1, 16 * w + e, kg, dz);
        gb1 += gm_row_sum(dz);
        float rx[16];
#pragma unroll
        for (int c = NC - 1; c >= 0; c--) {
            if (c >= 2) gw_fetch_x(a.obs, O, m.ridx, c - 2, tid, rx);
            gm_mma_s(dz, gm_x(m, c & 1), (gw_chunk_cols(O, c) + 15) >> 4, e, kg, gW1[c]);
            __syncthreads();                                 // ... has read the buffer; behind chunk 0: the images are free for the next tile
            if (c >= 2) gw_store_x(gm_x(m, c & 1), tid, rx);
        }
    }

    float* slab = a.slab + ((size_t)net * nb + b) * a.slab_stride;
    const int base = a.sh.off[net][0];
    float* dW2 = slab + (a.sh.off[net][2] - base);
    float* dW3 = slab + (a.sh.off[net][4] - base);
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int u = 16 * w + 4 * kg + r;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const int k = GW_K * c + 16 * j + e;
                if (k < O) slab[u * O + k] = gW1[c][j][r];
            }
            dW2[u * 64 + 16 * j + e] = gW2[j][r];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int u = 4 * ub + i;
#pragma unroll
        for (int j = 0; j < 4; j++) if (u < out) dW3[u * 64 + 4 * kb + j] = gW3[i * 4 + j];
        if (kb == 0 && u < out) slab[a.sh.off[net][5] - base + u] = gb3[i];
    }
    if (kg == 0) {
        slab[a.sh.off[net][1] - base + 16 * w + e] = gb1;
        slab[a.sh.off[net][3] - base + 16 * w + e] = gb2;
    }
    gf_store_loss<DIST>(a, slab, net, b, s, w, ls);
}

template <int DIST, int NC>
hipError_t gm_upd_launch(const GfUpdArgs& a, int bytes, hipStream_t s) {
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, gm_fwd_bwd_kernel<DIST, NC>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((gm_fwd_bwd_kernel<DIST, NC>), dim3(a.nb, 2), dim3(GF_THREADS), bytes, s, a);
    return hipGetLastError();
}
template <int DIST>
hipError_t gm_upd_chunks(int nc, const GfUpdArgs& a, int bytes, hipStream_t s) {
    switch (nc) {
        case 1: return gm_upd_launch<DIST, 1>(a, bytes, s);
        case 2: return gm_upd_launch<DIST, 2>(a, bytes, s);
        case 3: return gm_upd_launch<DIST, 3>(a, bytes, s);
        case 4: return gm_upd_launch<DIST, 4>(a, bytes, s);
        case 5: return gm_upd_launch<DIST, 5>(a, bytes, s);
        case 6: return gm_upd_launch<DIST, 6>(a, bytes, s);
    }
    return hipErrorInvalidValue;
}

template <int DIST, bool GREEDY>
hipError_t gm_cat_act_launch(const GfShape& sh, int bytes, dim3 grid, const float* params, const float* obs, const uint8_t* mask, const int64_t* forced, int64_t n,
                             int64_t seed, int64_t row_offset, int64_t step_index, int64_t* action, float* logprob, float* entropy, const CfStepStores& ss, hipStream_t s) {
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, gm_cat_act_kernel<DIST, GREEDY>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((gm_cat_act_kernel<DIST, GREEDY>), grid, dim3(GF_THREADS), bytes, s, sh, params, obs, mask, forced, n, seed, row_offset, step_index, action,
                       logprob, entropy, ss);
    return hipGetLastError();
}

// the shapes this file's kernels are launched for: 2 x 64, one to six chunks
bool gm_shape_ok(const GenLayout& L) { return L.fused_matrix && L.hidden == 64 && L.obs >= 1 && L.obs <= FUSED_WIDE_MAX_OBS && L.act >= 1 && L.act <= PPO_MAX_ACT; }

}  // namespace

hipError_t fused_matrix_gauss_act(const GenLayout& L, const float* params, const float* obs, const float* forced, int64_t n, int64_t seed, int64_t row_offset,
                                  int64_t step_index, bool greedy, float* action, float* logprob, float* entropy, const GaussStepStores* st, hipStream_t s) {
    if (!gm_shape_ok(L) || !L.gauss) return hipErrorInvalidValue;
    const GfShape sh = gf_shape(L);
    const int bytes = gm_lds_floats(gf_pad4(L.gauss)) * 4;
    const dim3 grid((unsigned)std::min<int64_t>((n + 63) / 64, 1024)), block(GF_THREADS);
    GfStepStores ss{};
    if (st) ss = GfStepStores{ st->done_prev, st->obs_t, st->act_t, st->lp_t, st->dones_t };
    static std::atomic<unsigned long long> done_g{ 0 }, done_s{ 0 };
    if (greedy) {
        const hipError_t e = gf_allow(done_g, gm_gauss_act_kernel<true>, bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(gm_gauss_act_kernel<true>, grid, block, bytes, s, sh, params, obs, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss);
    } else {
        const hipError_t e = gf_allow(done_s, gm_gauss_act_kernel<false>, bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(gm_gauss_act_kernel<false>, grid, block, bytes, s, sh, params, obs, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss);
    }
    return hipGetLastError();
}

hipError_t fused_matrix_cat_act(const GenLayout& L, int dist_kind, const float* params, const float* obs, const uint8_t* mask, const int64_t* forced, int64_t n,
                                int64_t seed, int64_t row_offset, int64_t step_index, bool greedy, int64_t* action, float* logprob, float* entropy,
                                const CatStepStores* st, hipStream_t s) {
    if (!gm_shape_ok(L) || L.gauss) return hipErrorInvalidValue;
    const GfShape sh = gf_shape(L);
    const int bytes = gm_lds_floats(gf_pad4(L.act)) * 4;
    const dim3 grid((unsigned)std::min<int64_t>((n + 63) / 64, 1024));
    CfStepStores ss{};
    if (st) ss = CfStepStores{ st->done_prev, st->obs_t, st->mask_t, st->act_t, st->lp_t, st->dones_t };
    const bool masked = dist_kind == PPO_DIST_MASKED;
    if (greedy)
        return masked ? gm_cat_act_launch<PPO_DIST_MASKED, true>(sh, bytes, grid, params, obs, mask, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss, s)
                      : gm_cat_act_launch<PPO_DIST_CATEGORICAL, true>(sh, bytes, grid, params, obs, mask, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss, s);
    return masked ? gm_cat_act_launch<PPO_DIST_MASKED, false>(sh, bytes, grid, params, obs, mask, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss, s)
                  : gm_cat_act_launch<PPO_DIST_CATEGORICAL, false>(sh, bytes, grid, params, obs, mask, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss, s);
}

hipError_t fused_matrix_values(const GenLayout& L, const float* params, const float* obs, int64_t n, float* value, hipStream_t s) {
    if (!gm_shape_ok(L)) return hipErrorInvalidValue;
    const GfShape sh = gf_shape(L);
    const int bytes = gm_lds_floats(4) * 4;
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, gm_values_kernel, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gm_values_kernel, dim3((unsigned)std::min<int64_t>((n + 63) / 64, 1024)), dim3(GF_THREADS), bytes, s, sh, params, obs, n, value);
    return hipGetLastError();
}

hipError_t fused_matrix_dev_fold(const GenLayout& L, const float* params, const DevFoldArgs& a, hipStream_t s) {
    if (!gm_shape_ok(L)) return hipErrorInvalidValue;
    const GfShape sh = gf_shape(L);
    // the row list and the waves' totals are part of the dynamic allocation: the attribute is decided on every byte of LDS the kernel uses
    const int bytes = gm_lds_floats(4) * 4 + GF_DEV_FOLD_LIST_INTS * (int)sizeof(int);
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, gm_dev_fold_kernel, bytes);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)(((int64_t)a.N + DEV_FOLD_THREADS - 1) / DEV_FOLD_THREADS);
    hipLaunchKernelGGL(gm_dev_fold_kernel, dim3(grid), dim3(DEV_FOLD_THREADS), bytes, s, sh, params, a);
    return hipGetLastError();
}

hipError_t fused_matrix_fwd_bwd(const GenLayout& L, const GfUpdArgs& a, float* grads, hipStream_t s) {
    if (!gm_shape_ok(L)) return hipErrorInvalidValue;
    const int nc = (L.obs + GW_K - 1) / GW_K;
    const int bytes = gm_lds_floats(gf_pad4(L.act)) * 4;
    hipError_t e;
    if (L.gauss) e = gm_upd_chunks<PPO_DIST_GAUSSIAN>(nc, a, bytes, s);
    else if (a.hp.dist_kind == PPO_DIST_MASKED) e = gm_upd_chunks<PPO_DIST_MASKED>(nc, a, bytes, s);
    else e = gm_upd_chunks<PPO_DIST_CATEGORICAL>(nc, a, bytes, s);
    if (e != hipSuccess) return e;
    return gauss_fused_slab_reduce(L, a.slab, a.slab_stride, a.nb, grads, s);
}
