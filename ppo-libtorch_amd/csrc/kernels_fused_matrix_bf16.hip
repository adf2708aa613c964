// ppo-libtorch_amd/csrc/kernels_fused_matrix_bf16.hip -- PPO_KERNEL_FUSED_MATRIX at compute_dtype = PPO_DTYPE_BF16: the fused families (PPO_KERNEL_GAUSS_FUSED,
// PPO_KERNEL_CAT_FUSED) on a 2 x 64 or 2 x 128 network with every 64- and 128-deep product on v_mfma_f32_16x16x32_bf16: bf16 operands (round to nearest
// even, v_cvt_pk_bf16_f32), f32 accumulation, f32 parameters, gradients and optimizer.  A kernel set of its own beside kernels_fused_matrix.hip and
// kernels_fused_matrix_h128.hip, one template over the width H: the same tile (64 samples per workgroup pass), workgroup (256 threads), chunk pipeline of
// layer 1 (nc = ceil(obs / 64) = 1 .. 6), heads, draws, loss lanes, step stores, slab layout and gauss_slab_reduce_kernel; the products and the way the data
// moves through LDS are new, because the instruction wants its operands k-contiguous.
//
// The arithmetic (DESIGN.md has it in full).  x^ = bf16(x); z1 = bf16(W1) x^ + b1; h1 = bf16(tanh(z1)); z2 = bf16(W2) h1 + b2; h2 = bf16(tanh(z2));
// out = W3 h2 + b3 in f32 on the vector ALU.  dW3, db3, dz2 = (W3^T dOut)(1 - h2^2) in f32; db2 = sum dz2 (unrounded); dW2 = bf16(dz2) h1^T;
// dz1 = (bf16(W2)^T bf16(dz2))(1 - h1^2); db1 = sum dz1 (unrounded); dW1 = bf16(dz1) x^^T.  Weights are converted in registers at every fetch from the f32
// parameters: there are no prepared planes, so an optimizer step leaves nothing stale.  No float atomics: equal inputs give equal bits.
//
// The lane map.  lane = 16 kg + e (e = 0 .. 15, kg = 0 .. 3).  One v_mfma_f32_16x16x32_bf16 is D[16][16] += A[16][32] B[32][16]: the lane holds, in 4 VGPRs
// per operand, the 8 consecutive k = 8 kg .. 8 kg + 7 of A's row e and of B's column e; element r of the accumulator is row 4 kg + r, column e.  A 64-deep
// product is 2 instructions per accumulator (step t covers k = 32 t ..), a 128-deep one 4.  Wave w owns units U0 = (H / 4) w .. U0 + H / 4 - 1 of all 64
// samples as NI = H / 64 row tiles by four column tiles: element r of accumulator [i][j] is unit U0 + 16 i + 4 kg + r of sample 16 j + e.
//
// The images are bf16 and k-contiguous.  A forward B operand is [sample][unit] with a padded row stride (H + 8 elements; the X chunk buffers 72: 16 rows of
// a 16-byte read fall on 16 different bank quads), read with ONE 16-byte LDS read per instruction; the accumulator layout gives a lane 4 consecutive units of
// one sample, so H1 / H2 are stored as one 8-byte write of 4 bf16.  The products whose K is the sample (dW2, dW1) want the other orientation of dz2, H1, dz1
// and x^.  gfx950 has a transposing LDS read; it was not tried: LDS is not short here (below) and plain 16-byte reads of a second image need no new lane
// arithmetic, so the update kernel keeps SECOND images [unit][sample] of stride 72 (H1T, the two X chunk buffers XT, and DZT:
// dz2, then dz1 in its place), written with 2-byte stores beside the first.  The act, critic and fold kernels carry none of them.
//
// Where the weights live.  W1 chunk slices go from L2 into operand registers as in the f32 kernels, converted pairwise: 8 NI registers per chunk.  The wave's
// W2 slice (rows U0 + 16 i + e, the A operand of layer 2) is 32 registers at H = 128 (8 at 64) and is resident for the whole kernel in ALL kernels, the
// update kernels too; so is the transposed slice W2[o][U0 + 16 i + e] for dz1, another 32 (8).  W3, the biases, log_std and exp(-log_std) are staged in LDS
// in f32.  dW2 and the dW1 chunks are summed from zero per tile and go to the workgroup's slab at once (stored by its first tile, added by a later one), as
// in kernels_fused_matrix_h128.hip: one instantiation per policy kind for every nc.
//
// LDS (bytes; outP = the output width rounded up to 4; S = H + 8):
//   f32:  W3 H outP | b1 H | b2 H | b3 32 | log_std 32 | exp(-log_std) 32 | row index 64 | OUT outP 68 | the heads' scratch outP 68
//   bf16: X 2 x 64 x 72 | H1 64 S | H2 64 S          update only: XT 2 x 64 x 72 | H1T H 72 | DZT H 72
//   H = 128: act, 32 outputs 88 704; critic 59 136 (two workgroups per CU); update, 32 outputs 144 000 (one).  The fold adds its list, 1 056.
//   H =  64: act, 32 outputs 63 616 (two per CU); critic 41 216 (three); update 63 616 + 36 864 = 100 480 (one).
//   The sizes do not depend on obs_size.  Two workgroups per CU are taken wherever the bytes above allow: the act, critic and fold kernels stay at or under
//   256 registers in all (below), so nothing else stands in the way.
//
// Compiler output (-Rpass-analysis=kernel-resource-usage, gfx950), scratch 0 bytes per lane in every kernel (VGPRs + AGPRs):
//   H = 128: Gaussian act 155 + 56 (greedy) / 160 + 56, categorical act 155 .. 160 + 56, critic 141 + 56, fold 144 + 56: two waves per SIMD;
//            update 256 + 146 (Gaussian), 256 + 182 (masked), 256 + 148 (categorical): one wave per SIMD, both W2 slices resident.
//   H =  64: act 96 .. 100 + 28, critic 82 + 28, fold 84 + 28: four waves per SIMD; update 232 + 28 (Gaussian), 256 + 43 (masked), 256 + 29 (categorical).
// Every kernel is __launch_bounds__(256); LDS is all dynamic, the sizes above.
#include "fused_matrix_dev.hpp"

namespace {

typedef __bf16 bq_bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 bq_bf2 __attribute__((ext_vector_type(2)));
typedef uint32_t bq_u4 __attribute__((ext_vector_type(4)));   // an operand: 8 bf16
typedef uint32_t bq_u2 __attribute__((ext_vector_type(2)));

constexpr int BQ_XS = 72;   // the row stride (elements) of every 64-wide bf16 image

__device__ __forceinline__ uint32_t bq_pack(float x0, float x1) { const bq_bf2 v = { (__bf16)x0, (__bf16)x1 }; return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint16_t bq_bits(float x) { const __bf16 b = (__bf16)x; return __builtin_bit_cast(uint16_t, b); }
__device__ __forceinline__ float bq_lo(uint32_t v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float bq_hi(uint32_t v) { return __uint_as_float(v & 0xffff0000u); }
__device__ __forceinline__ gm_f4 bq_mfma(bq_u4 a, bq_u4 b, gm_f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bq_bf8, a), __builtin_bit_cast(bq_bf8, b), c, 0, 0, 0);
}

struct BqLds {
    GfLds f;                 // w3 b1 b2 b3 ls inv ridx o as the family's functions know them; f.h1 is the heads' f32 scratch [outP][GF_S]
    uint16_t *x, *h1, *h2;   // [sample][k]: two X chunk buffers of stride BQ_XS; H1, H2 of stride H + 8
    uint16_t *xt, *h1t, *dzt;   // the update kernel's second images [k][sample] of stride BQ_XS
};

template <int H>
__host__ __device__ inline int bq_lds_bytes(int outP, bool bwd) {
    const int f32 = H * outP + H + H + 32 + 32 + 32 + 64 + 2 * outP * GF_S;
    const int b16 = 2 * 64 * BQ_XS + 2 * 64 * (H + 8) + (bwd ? 2 * 64 * BQ_XS + 2 * H * BQ_XS : 0);
    return 4 * f32 + 2 * b16;
}

template <int H>
__device__ __forceinline__ BqLds bq_carve(float* base, int outP, bool bwd) {
    BqLds m;
    m.f.obsP = GW_K; m.f.outP = outP;
    float* p = base;
    m.f.w1 = nullptr; m.f.w2 = nullptr; m.f.x = nullptr; m.f.h2 = nullptr;
    m.f.w3 = p; p += H * outP;
    m.f.b1 = p; p += H;
    m.f.b2 = p; p += H;
    m.f.b3 = p; p += 32;
    m.f.ls = p; p += 32;
    m.f.inv = p; p += 32;
    m.f.ridx = reinterpret_cast<int*>(p); p += 64;
    m.f.o = p; p += outP * GF_S;
    m.f.h1 = p; p += outP * GF_S;
    uint16_t* q = reinterpret_cast<uint16_t*>(p);   // 16-byte aligned: every size above is a multiple of 4 floats
    m.x = q; q += 2 * 64 * BQ_XS;
    m.h1 = q; q += 64 * (H + 8);
    m.h2 = q; q += 64 * (H + 8);
    m.xt = q; q += bwd ? 2 * 64 * BQ_XS : 0;
    m.h1t = q; q += bwd ? H * BQ_XS : 0;
    m.dzt = q;
    return m;
}

// one net's layer 3, the biases, log_std and exp(-log_std) into LDS (zero padded); the caller's next barrier publishes it
template <int H>
__device__ __forceinline__ void bq_stage_upper(const GfLds& m, const GfShape& sh, const float* __restrict__ params, int net, int tid) {
    const int out = net == 0 ? 1 : sh.A;
    const float* W3 = params + sh.off[net][4];
    for (int i = tid; i < H * m.outP; i += GF_THREADS) m.w3[i] = (i / H) < out ? W3[i] : 0.0f;
    if (tid < H) { m.b1[tid] = params[sh.off[net][1] + tid]; m.b2[tid] = params[sh.off[net][3] + tid]; }
    if (tid < 32) {
        m.b3[tid] = tid < out ? params[sh.off[net][5] + tid] : 0.0f;
        const float ls = tid < sh.D ? params[sh.logstd_off + tid] : 0.0f;
        m.ls[tid] = ls;
        m.inv[tid] = expf(-ls);
    }
}

// an operand out of f32 memory: p[0], p[stride], .. p[7 stride] as bf16, zero where k0 + q >= K
__device__ __forceinline__ bq_u4 bq_fetch8(const float* __restrict__ p, int stride, int k0, int K) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; q++) v[q] = k0 + q < K ? p[q * stride] : 0.0f;
    return bq_u4{ bq_pack(v[0], v[1]), bq_pack(v[2], v[3]), bq_pack(v[4], v[5]), bq_pack(v[6], v[7]) };
}

// the A operand of a 64-deep product out of a row-major matrix W [., K] in global memory: rows U0 + 16 i + e, columns k0 + 32 t + 8 kg + q, zero behind K
template <int NI>
__device__ __forceinline__ void bq_fetch_a64(const float* __restrict__ W, int K, int k0, int u0, int e, int kg, bq_u4 (&a)[NI][2]) {
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int k = k0 + 32 * t + 8 * kg;
            a[i][t] = bq_fetch8(W + (size_t)(u0 + 16 * i + e) * K + k, 1, k, K);
        }
}

// the wave's slices of one net's W2: a2 [i][t] = rows U0 + 16 i + e, columns 32 t + 8 kg + q (layer 2's A operand); TRANSPOSED: the element W2[o][u] with
// u = U0 + 16 i + e and o = 32 t + 8 kg + q (dz1's A operand)
template <int H, bool TRANSPOSED>
__device__ __forceinline__ void bq_fetch_w2(const GfShape& sh, const float* __restrict__ params, int net, int tid, bq_u4 (&a)[H / 64][H / 32]) {
    const int e = tid & 15, kg = (tid >> 4) & 3, u0 = (H / 4) * (tid >> 6);
    const float* W2 = params + sh.off[net][2];
#pragma unroll
    for (int i = 0; i < H / 64; i++)
#pragma unroll
        for (int t = 0; t < H / 32; t++) {
            const int u = u0 + 16 * i + e, k = 32 * t + 8 * kg;
            a[i][t] = TRANSPOSED ? bq_fetch8(W2 + k * H + u, H, 0, 8) : bq_fetch8(W2 + u * H + k, 1, 0, 8);
        }
}

// acc[i][j] += A_i B_j over steps t < nt (32 k each): B_j = the 8 k of sample (or row) 16 j + e out of an image [row][k] of stride S: one 16-byte read
template <int NI, int NT>
__device__ __forceinline__ void bq_mma(const bq_u4 (&a)[NI][NT], const uint16_t* __restrict__ img, int S, int nt, int e, int kg, gm_f4 (&acc)[NI][4]) {
#pragma unroll
    for (int t = 0; t < NT; t++) {
        if (t < nt) {   // uniform
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bq_u4 b = *reinterpret_cast<const bq_u4*>(&img[(16 * j + e) * S + 32 * t + 8 * kg]);
#pragma unroll
                for (int i = 0; i < NI; i++) acc[i][j] = bq_mfma(a[i][t], b, acc[i][j]);
            }
        }
    }
}

// acc[i][j][r] = b[U0 + 16 i + 4 kg + r]: a hidden layer's accumulators start at the f32 bias
template <int NI>
__device__ __forceinline__ void bq_bias(const float* __restrict__ b, int u0, int kg, gm_f4 (&acc)[NI][4]) {
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const float4 v = *reinterpret_cast<const float4*>(&b[u0 + 16 * i + 4 * kg]);
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = gm_f4{ v.x, v.y, v.z, v.w };
    }
}

// img[16 j + e][U0 + 16 i + 4 kg + r] = bf16(tanh(acc[i][j][r])): one 8-byte write per accumulator; T: also the [unit][sample] image imgT
template <int NI, bool T>
__device__ __forceinline__ void bq_store_tanh(uint16_t* __restrict__ img, int S, uint16_t* __restrict__ imgT, int u0, int e, int kg, const gm_f4 (&acc)[NI][4]) {
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int u = u0 + 16 * i + 4 * kg, s = 16 * j + e;
            const bq_u2 v = { bq_pack(tanh_fast(acc[i][j][0]), tanh_fast(acc[i][j][1])), bq_pack(tanh_fast(acc[i][j][2]), tanh_fast(acc[i][j][3])) };
            *reinterpret_cast<bq_u2*>(&img[s * S + u]) = v;
            if (T) {
                imgT[(u + 0) * BQ_XS + s] = (uint16_t)v.x; imgT[(u + 1) * BQ_XS + s] = (uint16_t)(v.x >> 16);
                imgT[(u + 2) * BQ_XS + s] = (uint16_t)v.y; imgT[(u + 3) * BQ_XS + s] = (uint16_t)(v.y >> 16);
            }
        }
}

// a chunk of x^ out of gw_fetch_x's registers (column tid & 63 of samples (tid >> 6) + 4 j): the [sample][column] image and / or the [column][sample] one
template <bool PLAIN, bool T>
__device__ __forceinline__ void bq_store_x(uint16_t* __restrict__ x, uint16_t* __restrict__ xt, int tid, const float (&r)[16]) {
    const int k = tid & 63, s0 = tid >> 6;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint16_t v = bq_bits(r[j]);
        if (PLAIN) x[(s0 + 4 * j) * BQ_XS + k] = v;
        if (T) xt[k * BQ_XS + s0 + 4 * j] = v;
    }
}

// the output layer in f32: H2 (bf16, complete behind the caller's barrier) -> OUT rows 0 .. out - 1; wave w owns units w, w + 4, ... (< out <= 32);
// lane = sample: one 16-byte read of 8 activations against two 16-byte broadcast reads of W3
template <int H>
__device__ __forceinline__ void bq_output_layer(const BqLds& m, int out, int s, int w) {
    const int nu = (out - w + 3) >> 2;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = m.f.b3[(4 * i + w) & 31];
    for (int k = 0; k < H; k += 8) {
        const bq_u4 v = *reinterpret_cast<const bq_u4*>(&m.h2[s * (H + 8) + k]);
        const float x[8] = { bq_lo(v.x), bq_hi(v.x), bq_lo(v.y), bq_hi(v.y), bq_lo(v.z), bq_hi(v.z), bq_lo(v.w), bq_hi(v.w) };
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (i < nu) {
                const float4 w0 = *reinterpret_cast<const float4*>(&m.f.w3[(4 * i + w) * H + k]);
                const float4 w1 = *reinterpret_cast<const float4*>(&m.f.w3[(4 * i + w) * H + k + 4]);
                acc[i] = __builtin_fmaf(w0.x, x[0], acc[i]);
                acc[i] = __builtin_fmaf(w0.y, x[1], acc[i]);
                acc[i] = __builtin_fmaf(w0.z, x[2], acc[i]);
                acc[i] = __builtin_fmaf(w0.w, x[3], acc[i]);
                acc[i] = __builtin_fmaf(w1.x, x[4], acc[i]);
                acc[i] = __builtin_fmaf(w1.y, x[5], acc[i]);
                acc[i] = __builtin_fmaf(w1.z, x[6], acc[i]);
                acc[i] = __builtin_fmaf(w1.w, x[7], acc[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) if (i < nu) m.f.o[(4 * i + w) * GF_S + s] = acc[i];
}

// THE forward pass of every kernel in this file: the tile whose row indices are in m.f.ridx (published by the caller's barrier, as are the staged upper
// layers) through obs -> H -> H -> out, layer 1 over nc chunks.  a2 is the wave's slice of W2 (bq_fetch_w2, once per kernel).  Leaves H1, H2 (bf16 of the
// tanh), OUT rows 0 .. out - 1 and chunks nc - 1, nc - 2 of x^ in buffers (nc - 1) & 1 and the other; BWD: H1T and the chunks' XT as well.  Every thread of
// the workgroup calls it; the caller's barrier behind the previous tile has freed every image.
template <int H, bool BWD>
__device__ __forceinline__ void bq_forward_tile(const BqLds& m, const GfShape& sh, const float* __restrict__ params, int net, const float* __restrict__ obs, int nc,
                                                int out, int tid, const bq_u4 (&a2)[H / 64][H / 32]) {
    constexpr int NI = H / 64, S = H + 8;
    const int s = tid & 63, e = tid & 15, kg = (tid >> 4) & 3, w = __builtin_amdgcn_readfirstlane(tid >> 6), O = sh.obs, u0 = (H / 4) * w;
    const float* W1 = params + sh.off[net][0];
    bq_u4 ra[NI][2], rn[NI][2];
    float rx[16];
    gm_f4 acc[NI][4];
    bq_fetch_a64<NI>(W1, O, 0, u0, e, kg, ra);
    gw_fetch_x(obs, O, m.f.ridx, 0, tid, rx);
    bq_bias<NI>(m.f.b1, u0, kg, acc);
    bq_store_x<true, BWD>(m.x, m.xt, tid, rx);
    __syncthreads();
    for (int c = 0; c + 1 < nc; c++) {
        bq_fetch_a64<NI>(W1, O, GW_K * (c + 1), u0, e, kg, rn);
        gw_fetch_x(obs, O, m.f.ridx, c + 1, tid, rx);
        bq_mma<NI, 2>(ra, m.x + (c & 1) * 64 * BQ_XS, BQ_XS, 2, e, kg, acc);
#pragma unroll
        for (int i = 0; i < NI; i++) { ra[i][0] = rn[i][0]; ra[i][1] = rn[i][1]; }
        bq_store_x<true, BWD>(m.x + ((c + 1) & 1) * 64 * BQ_XS, m.xt + ((c + 1) & 1) * 64 * BQ_XS, tid, rx);
        __syncthreads();
    }
    bq_mma<NI, 2>(ra, m.x + ((nc - 1) & 1) * 64 * BQ_XS, BQ_XS, (gw_chunk_cols(O, nc - 1) + 31) >> 5, e, kg, acc);
    bq_store_tanh<NI, BWD>(m.h1, S, m.h1t, u0, e, kg, acc);
    __syncthreads();
    bq_bias<NI>(m.f.b2, u0, kg, acc);
    bq_mma<NI, H / 32>(a2, m.h1, S, H / 32, e, kg, acc);
    bq_store_tanh<NI, false>(m.h2, S, nullptr, u0, e, kg, acc);
    __syncthreads();
    bq_output_layer<H>(m, out, s, w);
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------
// The act kernels, the critic and the fold: the family's, behind this file's forward.
// ---------------------------------------------------------------------------------------------------------
template <int H, bool GREEDY>
__global__ __launch_bounds__(GF_THREADS) void bq_gauss_act_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs,
                                                                  const float* __restrict__ forced, int64_t n, int64_t seed, int64_t row_offset, int64_t step_index,
                                                                  float* action, float* logprob, float* entropy, GfStepStores st) {
    extern __shared__ __attribute__((aligned(16))) float bq_lds[];
    const int tid = threadIdx.x, D = sh.D, O = sh.obs, nc = gw_chunks(O);
    const BqLds m = bq_carve<H>(bq_lds, gf_pad4(D), false);
    bq_stage_upper<H>(m.f, sh, params, 1, tid);
    bq_u4 a2[H / 64][H / 32];
    bq_fetch_w2<H, false>(sh, params, 1, tid, a2);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(m.f, row0, n, tid);
        bq_forward_tile<H, false>(m, sh, params, 1, obs, nc, D, tid, a2);
        gauss_act_rows<GREEDY>(m.f, D, O, obs, forced, row0, n, seed, row_offset, step_index, action, logprob, entropy, st, tid);
        __syncthreads();   // OUT and the row list are read: the next tile may overwrite them
    }
}

template <int H, int DIST, bool GREEDY>
__global__ __launch_bounds__(GF_THREADS) void bq_cat_act_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs,
                                                                const uint8_t* __restrict__ mask, const int64_t* __restrict__ forced, int64_t n, int64_t seed,
                                                                int64_t row_offset, int64_t step_index, int64_t* action, float* logprob, float* entropy,
                                                                CfStepStores st) {
    extern __shared__ __attribute__((aligned(16))) float bq_lds[];
    const int tid = threadIdx.x, A = sh.A, nc = gw_chunks(sh.obs);
    const BqLds m = bq_carve<H>(bq_lds, gf_pad4(A), false);
    bq_stage_upper<H>(m.f, sh, params, 1, tid);
    bq_u4 a2[H / 64][H / 32];
    bq_fetch_w2<H, false>(sh, params, 1, tid, a2);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(m.f, row0, n, tid);
        bq_forward_tile<H, false>(m, sh, params, 1, obs, nc, A, tid, a2);
        cat_act_rows<DIST, GREEDY>(m.f, sh, obs, mask, forced, row0, n, seed, row_offset, step_index, action, logprob, entropy, st, tid);
        __syncthreads();   // OUT, the heads' scratch and the row list are read: the next tile may overwrite them
    }
}

// the critic over n rows
template <int H>
__global__ __launch_bounds__(GF_THREADS) void bq_values_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs, int64_t n,
                                                               float* __restrict__ value) {
    extern __shared__ __attribute__((aligned(16))) float bq_lds[];
    const int tid = threadIdx.x, nc = gw_chunks(sh.obs);
    const BqLds m = bq_carve<H>(bq_lds, 4, false);
    bq_stage_upper<H>(m.f, sh, params, 0, tid);
    bq_u4 a2[H / 64][H / 32];
    bq_fetch_w2<H, false>(sh, params, 0, tid, a2);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(m.f, row0, n, tid);
        bq_forward_tile<H, false>(m, sh, params, 0, obs, nc, 1, tid, a2);
        if (tid < 64 && row0 + tid < n) value[row0 + tid] = m.f.o[tid];
        __syncthreads();
    }
}

// ppo_dev_observe with truncation flags: gm_dev_fold_kernel's front end (one compaction per 256 env rows, a workgroup without a flagged row returns before it
// loads a weight), then bq_values_kernel's forward on the listed rows of final_obs: v is that kernel's value of the row, bit for bit.  LDS: all dynamic, the
// row list [256] and the waves' totals [8] behind the carve.
template <int H>
__global__ __launch_bounds__(DEV_FOLD_THREADS) void bq_dev_fold_kernel(GfShape sh, const float* __restrict__ params, DevFoldArgs a) {
    static_assert(DEV_FOLD_THREADS == GF_THREADS, "fold_compact and bq_forward_tile are written for the same workgroup");
    extern __shared__ __attribute__((aligned(16))) float bq_lds[];
    const int tid = threadIdx.x, nc = gw_chunks(sh.obs);
    int* list = reinterpret_cast<int*>(bq_lds + bq_lds_bytes<H>(4, false) / 4);
    int* wtot = list + DEV_FOLD_THREADS;
    const int cnt = dev_fold_compact(a, list, wtot);
    if (cnt == 0) return;
    const int base = wtot[4];
    const BqLds m = bq_carve<H>(bq_lds, 4, false);
    bq_stage_upper<H>(m.f, sh, params, 0, tid);
    bq_u4 a2[H / 64][H / 32];
    bq_fetch_w2<H, false>(sh, params, 0, tid, a2);
    for (int k0 = 0; k0 < cnt; k0 += 64) {
        const int k = k0 + tid;   // tid < 64: this lane's place in the list
        if (tid < 64) m.f.ridx[tid] = k < cnt ? list[k] : -1;
        __syncthreads();
        bq_forward_tile<H, false>(m, sh, params, 0, a.final_obs, nc, 1, tid, a2);
        if (tid < 64 && k < cnt) dev_fold_store(a, base, k, list[k], m.f.o[tid]);
        __syncthreads();   // OUT and the row indices are read: the next tile may overwrite them
    }
}

// ---------------------------------------------------------------------------------------------------------
// bq_fwd_bwd_kernel<H, DIST>: one minibatch step of one net per workgroup column (blockIdx.y = net), every nc in one instantiation.
// ---------------------------------------------------------------------------------------------------------
// the A operand of a product over the tile's 64 samples: rows U0 + 16 i + e of an image [unit][sample], samples 32 t + 8 kg ..
template <int NI>
__device__ __forceinline__ void bq_load_a_s(const uint16_t* __restrict__ imgT, int u0, int e, int kg, bq_u4 (&a)[NI][2]) {
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
        for (int t = 0; t < 2; t++) a[i][t] = *reinterpret_cast<const bq_u4*>(&imgT[(u0 + 16 * i + e) * BQ_XS + 32 * t + 8 * kg]);
}

// dW3 = dOUT H2^T and db3 in f32 on the thread grid ub = tid / (H / 4) (output units 4 ub ..), kb = tid % (H / 4) (columns 4 kb ..): the tile's sum from zero
// in ascending s, then added to the running sum (gf_dw_tile reading the bf16 image [sample][unit])
template <int H>
__device__ __forceinline__ void bq_dw3_tile(const float* __restrict__ dout, const uint16_t* __restrict__ h2, int ub, int kb, float* acc, float* accb) {
    float t[16], tb[4];
#pragma unroll
    for (int i = 0; i < 16; i++) t[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) tb[i] = 0.0f;
    for (int s4 = 0; s4 < 64; s4 += 4) {
        float d[4][4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float4 v = *reinterpret_cast<const float4*>(&dout[(4 * ub + i) * GF_S + s4]);
            d[i][0] = v.x; d[i][1] = v.y; d[i][2] = v.z; d[i][3] = v.w;
        }
#pragma unroll
        for (int ss = 0; ss < 4; ss++) {
            const bq_u2 hv = *reinterpret_cast<const bq_u2*>(&h2[(s4 + ss) * (H + 8) + 4 * kb]);
            const float h[4] = { bq_lo(hv.x), bq_hi(hv.x), bq_lo(hv.y), bq_hi(hv.y) };
#pragma unroll
            for (int i = 0; i < 4; i++) {
#pragma unroll
                for (int j = 0; j < 4; j++) t[i * 4 + j] = __builtin_fmaf(d[i][ss], h[j], t[i * 4 + j]);
                tb[i] += d[i][ss];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] += t[i];
#pragma unroll
    for (int i = 0; i < 4; i++) accb[i] += tb[i];
}

// dz2 = (W3^T dOUT)(1 - H2^2) in f32: lane = sample s, wave w owns units U0 .. U0 + H / 4 - 1 (W is the staged W3 [o][H], o ascending below n_out).  bf16(dz2)
// replaces H2 in the [sample][unit] image (a thread reads and writes only its own elements) and goes to DZT [unit][sample]; the unrounded values are summed
// over the wave's 64 samples (wave_sum: a fixed order) into gb2: lane l keeps unit U0 + l % (H / 4)
template <int H>
__device__ __forceinline__ void bq_dz2_tile(const BqLds& m, int n_out, int s, int w, int lane, float& gb2) {
    constexpr int NU = H / 4, S = H + 8;
    const int u0 = NU * w;
    float acc[NU];
#pragma unroll
    for (int i = 0; i < NU; i++) acc[i] = 0.0f;
    for (int o = 0; o < n_out; o++) {
        const float d = m.f.o[o * GF_S + s];
#pragma unroll
        for (int q = 0; q < NU / 4; q++) {
            const float4 wv = *reinterpret_cast<const float4*>(&m.f.w3[o * H + u0 + 4 * q]);
            acc[4 * q + 0] = __builtin_fmaf(wv.x, d, acc[4 * q + 0]);
            acc[4 * q + 1] = __builtin_fmaf(wv.y, d, acc[4 * q + 1]);
            acc[4 * q + 2] = __builtin_fmaf(wv.z, d, acc[4 * q + 2]);
            acc[4 * q + 3] = __builtin_fmaf(wv.w, d, acc[4 * q + 3]);
        }
    }
#pragma unroll
    for (int g = 0; g < NU / 8; g++) {
        bq_u4* hp = reinterpret_cast<bq_u4*>(&m.h2[s * S + u0 + 8 * g]);
        const bq_u4 hv = *hp;
        const float h[8] = { bq_lo(hv.x), bq_hi(hv.x), bq_lo(hv.y), bq_hi(hv.y), bq_lo(hv.z), bq_hi(hv.z), bq_lo(hv.w), bq_hi(hv.w) };
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            v[q] = acc[8 * g + q] * (1.0f - h[q] * h[q]);
            const float t = wave_sum(v[q]);
            gb2 += (lane & (NU - 1)) == 8 * g + q ? t : 0.0f;
            m.dzt[(u0 + 8 * g + q) * BQ_XS + s] = bq_bits(v[q]);
        }
        *hp = bq_u4{ bq_pack(v[0], v[1]), bq_pack(v[2], v[3]), bq_pack(v[4], v[5]), bq_pack(v[6], v[7]) };
    }
}

// What a wave carries across its tiles: its W2 slice and the transposed one; gb2 (above); gb1[i] = the bias gradient of unit U0 + 16 i + 4 kg + (e & 3); gW3 /
// gb3 on bq_dw3_tile's thread grid; the loss lanes' state.  dW1 and dW2 live in the workgroup's slab between the tiles (the head of the file): element r of
// product tile [i][j] is row U0 + 16 i + 4 kg + r, column 16 j + e (dW1: of the chunk).
template <int H, int DIST>
__global__ __launch_bounds__(GF_THREADS) void bq_fwd_bwd_kernel(GfUpdArgs a) {
    constexpr int NI = H / 64, NT = H / 32, S = H + 8;
    extern __shared__ __attribute__((aligned(16))) float bq_lds[];
    const int tid = threadIdx.x, O = a.sh.obs, nc = gw_chunks(O);
    const int net = blockIdx.y, b = blockIdx.x, nb = a.nb;
    const int out = net == 0 ? 1 : a.sh.A, outP = gf_pad4(out);
    const BqLds m = bq_carve<H>(bq_lds, gf_pad4(a.sh.A), true);
    bq_stage_upper<H>(m.f, a.sh, a.params, net, tid);
    const int s = tid & 63, e = tid & 15, kg = (tid >> 4) & 3, w = __builtin_amdgcn_readfirstlane(tid >> 6), u0 = (H / 4) * w;
    const int ub = tid / (H / 4), kb = tid % (H / 4);
    float* slab = a.slab + ((size_t)net * nb + b) * a.slab_stride;
    bq_u4 a2[NI][NT], w2t[NI][NT];
    bq_fetch_w2<H, false>(a.sh, a.params, net, tid, a2);
    bq_fetch_w2<H, true>(a.sh, a.params, net, tid, w2t);

    float gW3[16], gb3[4], gb1[NI], gb2 = 0.0f;
    const gm_f4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
    for (int i = 0; i < 16; i++) gW3[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) gb3[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < NI; i++) gb1[i] = 0.0f;
    GfLossState ls;
    gf_loss_begin(a, net, w, ls);

    const int tiles = (a.M + 63) / 64;
    for (int tile = b; tile < tiles; tile += nb) {
        const bool first = tile == b;   // of this workgroup: its slab elements are stored, not added to
        if (tid < 64) m.f.ridx[tid] = tile * 64 + tid < a.M ? a.idx[tile * 64 + tid] : -1;
        __syncthreads();
        bq_forward_tile<H, true>(m, a.sh, a.params, net, a.obs, nc, out, tid, a2);
        if (w == 0) gf_loss_lanes<DIST>(a, m.f, net, out, outP, s, ls);
        __syncthreads();
        if (4 * ub < outP) bq_dw3_tile<H>(m.f.o, m.h2, ub, kb, gW3, gb3);   // dW3 = dOUT H2^T, db3
        __syncthreads();                                                    // ... has read H2
        bq_dz2_tile<H>(m, out, s, w, s, gb2);                               // H2 <- bf16(dZ2), DZT likewise; db2
        __syncthreads();
        {   // dW2 = bf16(dZ2) H1^T: K = the tile's 64 samples; four column tiles of H1's units at a time
            bq_u4 dz[NI][2];
            bq_load_a_s<NI>(m.dzt, u0, e, kg, dz);
            float* dW2 = slab + (a.sh.off[net][2] - a.sh.off[net][0]);
#pragma unroll
            for (int jg = 0; jg < H / 64; jg++) {
                gm_f4 g[NI][4];
#pragma unroll
                for (int i = 0; i < NI; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) g[i][j] = zero;
                bq_mma<NI, 2>(dz, m.h1t + 64 * jg * BQ_XS, BQ_XS, 2, e, kg, g);
#pragma unroll
                for (int i = 0; i < NI; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            float* p = &dW2[(u0 + 16 * i + 4 * kg + r) * H + 64 * jg + 16 * j + e];
                            *p = first ? g[i][j][r] : *p + g[i][j][r];
                        }
            }
        }
        __syncthreads();                                                    // ... has read DZT (dZ2)
        {   // dZ1 = (bf16(W2)^T bf16(dZ2))(1 - H1^2): A = the resident transposed slice, B = dZ2 in H2's place; bf16(dZ1) -> DZT, db1 from the unrounded values
            gm_f4 d[NI][4];
#pragma unroll
            for (int i = 0; i < NI; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) d[i][j] = zero;
            bq_mma<NI, NT>(w2t, m.h2, S, NT, e, kg, d);
#pragma unroll
            for (int i = 0; i < NI; i++) {
                float sum[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int u = u0 + 16 * i + 4 * kg, sj = 16 * j + e;
                    const bq_u2 hv = *reinterpret_cast<const bq_u2*>(&m.h1[sj * S + u]);
                    const float h[4] = { bq_lo(hv.x), bq_hi(hv.x), bq_lo(hv.y), bq_hi(hv.y) };
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float v = d[i][j][r] * (1.0f - h[r] * h[r]);
                        sum[r] += v;
                        m.dzt[(u + r) * BQ_XS + sj] = bq_bits(v);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float v = sum[r];
                    v += __shfl_xor(v, 1, 64);
                    v += __shfl_xor(v, 2, 64);
                    v += __shfl_xor(v, 4, 64);
                    v += __shfl_xor(v, 8, 64);
                    gb1[i] += (e & 3) == r ? v : 0.0f;
                }
            }
        }
        __syncthreads();
        // dW1 = bf16(dZ1) x^^T: chunk c out of XT buffer c & 1 (chunks nc - 1 and nc - 2 are the forward's; chunk c - 2 arrives behind chunk c's barrier); the
        // chunk's sum from zero goes to the slab: stored by the workgroup's first tile, added by a later one
        bq_u4 dz[NI][2];
        bq_load_a_s<NI>(m.dzt, u0, e, kg, dz);
        float rx[16];
        for (int c = nc - 1; c >= 0; c--) {
            if (c >= 2) gw_fetch_x(a.obs, O, m.f.ridx, c - 2, tid, rx);
            gm_f4 g[NI][4];
#pragma unroll
            for (int i = 0; i < NI; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) g[i][j] = zero;
            bq_mma<NI, 2>(dz, m.xt + (c & 1) * 64 * BQ_XS, BQ_XS, 2, e, kg, g);
#pragma unroll
            for (int i = 0; i < NI; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int k = GW_K * c + 16 * j + e;
                    if (k < O) {
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            float* p = &slab[(size_t)(u0 + 16 * i + 4 * kg + r) * O + k];
                            *p = first ? g[i][j][r] : *p + g[i][j][r];
                        }
                    }
                }
            __syncthreads();                                 // ... has read the buffer; behind chunk 0: the images are free for the next tile
            if (c >= 2) bq_store_x<false, true>(nullptr, m.xt + (c & 1) * 64 * BQ_XS, tid, rx);
        }
    }

    const int base = a.sh.off[net][0];
    float* dW3 = slab + (a.sh.off[net][4] - base);
#pragma unroll
    for (int i = 0; i < NI; i++)
        if (e < 4) slab[a.sh.off[net][1] - base + u0 + 16 * i + 4 * kg + e] = gb1[i];
    if (s < H / 4) slab[a.sh.off[net][3] - base + u0 + s] = gb2;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int u = 4 * ub + i;
#pragma unroll
        for (int j = 0; j < 4; j++) if (u < out) dW3[u * H + 4 * kb + j] = gW3[i * 4 + j];
        if (kb == 0 && u < out) slab[a.sh.off[net][5] - base + u] = gb3[i];
    }
    gf_store_loss<DIST>(a, slab, net, b, s, w, ls);
}

template <int H, int DIST>
hipError_t bq_upd_launch(const GfUpdArgs& a, int bytes, hipStream_t s) {
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, bq_fwd_bwd_kernel<H, DIST>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((bq_fwd_bwd_kernel<H, DIST>), dim3(a.nb, 2), dim3(GF_THREADS), bytes, s, a);
    return hipGetLastError();
}

template <int H, bool GREEDY>
hipError_t bq_gauss_act_launch(const GfShape& sh, int bytes, dim3 grid, const float* params, const float* obs, const float* forced, int64_t n, int64_t seed,
                               int64_t row_offset, int64_t step_index, float* action, float* logprob, float* entropy, const GfStepStores& ss, hipStream_t s) {
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, bq_gauss_act_kernel<H, GREEDY>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((bq_gauss_act_kernel<H, GREEDY>), grid, dim3(GF_THREADS), bytes, s, sh, params, obs, forced, n, seed, row_offset, step_index, action, logprob,
                       entropy, ss);
    return hipGetLastError();
}

template <int H, int DIST, bool GREEDY>
hipError_t bq_cat_act_launch(const GfShape& sh, int bytes, dim3 grid, const float* params, const float* obs, const uint8_t* mask, const int64_t* forced, int64_t n,
                             int64_t seed, int64_t row_offset, int64_t step_index, int64_t* action, float* logprob, float* entropy, const CfStepStores& ss, hipStream_t s) {
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, bq_cat_act_kernel<H, DIST, GREEDY>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((bq_cat_act_kernel<H, DIST, GREEDY>), grid, dim3(GF_THREADS), bytes, s, sh, params, obs, mask, forced, n, seed, row_offset, step_index, action,
                       logprob, entropy, ss);
    return hipGetLastError();
}

template <int H>
hipError_t bq_gauss_act(const GenLayout& L, const float* params, const float* obs, const float* forced, int64_t n, int64_t seed, int64_t row_offset, int64_t step_index,
                        bool greedy, float* action, float* logprob, float* entropy, const GaussStepStores* st, hipStream_t s) {
    const GfShape sh = gf_shape(L);
    const int bytes = bq_lds_bytes<H>(gf_pad4(L.gauss), false);
    const dim3 grid((unsigned)std::min<int64_t>((n + 63) / 64, 1024));
    GfStepStores ss{};
    if (st) ss = GfStepStores{ st->done_prev, st->obs_t, st->act_t, st->lp_t, st->dones_t };
    return greedy ? bq_gauss_act_launch<H, true>(sh, bytes, grid, params, obs, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss, s)
                  : bq_gauss_act_launch<H, false>(sh, bytes, grid, params, obs, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss, s);
}

template <int H>
hipError_t bq_cat_act(const GenLayout& L, int dist_kind, const float* params, const float* obs, const uint8_t* mask, const int64_t* forced, int64_t n, int64_t seed,
                      int64_t row_offset, int64_t step_index, bool greedy, int64_t* action, float* logprob, float* entropy, const CatStepStores* st, hipStream_t s) {
    const GfShape sh = gf_shape(L);
    const int bytes = bq_lds_bytes<H>(gf_pad4(L.act), false);
    const dim3 grid((unsigned)std::min<int64_t>((n + 63) / 64, 1024));
    CfStepStores ss{};
    if (st) ss = CfStepStores{ st->done_prev, st->obs_t, st->mask_t, st->act_t, st->lp_t, st->dones_t };
    const bool masked = dist_kind == PPO_DIST_MASKED;
    if (greedy)
        return masked ? bq_cat_act_launch<H, PPO_DIST_MASKED, true>(sh, bytes, grid, params, obs, mask, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss, s)
                      : bq_cat_act_launch<H, PPO_DIST_CATEGORICAL, true>(sh, bytes, grid, params, obs, mask, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss, s);
    return masked ? bq_cat_act_launch<H, PPO_DIST_MASKED, false>(sh, bytes, grid, params, obs, mask, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss, s)
                  : bq_cat_act_launch<H, PPO_DIST_CATEGORICAL, false>(sh, bytes, grid, params, obs, mask, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss, s);
}

template <int H>
hipError_t bq_values(const GenLayout& L, const float* params, const float* obs, int64_t n, float* value, hipStream_t s) {
    const GfShape sh = gf_shape(L);
    const int bytes = bq_lds_bytes<H>(4, false);
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, bq_values_kernel<H>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bq_values_kernel<H>, dim3((unsigned)std::min<int64_t>((n + 63) / 64, 1024)), dim3(GF_THREADS), bytes, s, sh, params, obs, n, value);
    return hipGetLastError();
}

template <int H>
hipError_t bq_dev_fold(const GenLayout& L, const float* params, const DevFoldArgs& a, hipStream_t s) {
    const GfShape sh = gf_shape(L);
    // the row list and the waves' totals are part of the dynamic allocation: the attribute is decided on every byte of LDS the kernel uses
    const int bytes = bq_lds_bytes<H>(4, false) + GF_DEV_FOLD_LIST_INTS * (int)sizeof(int);
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, bq_dev_fold_kernel<H>, bytes);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)(((int64_t)a.N + DEV_FOLD_THREADS - 1) / DEV_FOLD_THREADS);
    hipLaunchKernelGGL(bq_dev_fold_kernel<H>, dim3(grid), dim3(DEV_FOLD_THREADS), bytes, s, sh, params, a);
    return hipGetLastError();
}

template <int H>
hipError_t bq_fwd_bwd(const GenLayout& L, const GfUpdArgs& a, float* grads, hipStream_t s) {
    const int bytes = bq_lds_bytes<H>(gf_pad4(L.act), true);
    hipError_t e;
    if (L.gauss) e = bq_upd_launch<H, PPO_DIST_GAUSSIAN>(a, bytes, s);
    else if (a.hp.dist_kind == PPO_DIST_MASKED) e = bq_upd_launch<H, PPO_DIST_MASKED>(a, bytes, s);
    else e = bq_upd_launch<H, PPO_DIST_CATEGORICAL>(a, bytes, s);
    if (e != hipSuccess) return e;
    return gauss_fused_slab_reduce(L, a.slab, a.slab_stride, a.nb, grads, s);
}

// the shapes this file's kernels are launched for: 2 x 64 or 2 x 128 at bf16, one to six chunks
bool bq_shape_ok(const GenLayout& L) {
    return L.fused_matrix && L.fused_bf16 && (L.hidden == 64 || L.hidden == 128) && L.n_hidden == 2 && L.obs >= 1 && L.obs <= FUSED_WIDE_MAX_OBS && L.act >= 1 &&
           L.act <= PPO_MAX_ACT;
}

}  // namespace

hipError_t fused_matrix_bf16_gauss_act(const GenLayout& L, const float* params, const float* obs, const float* forced, int64_t n, int64_t seed, int64_t row_offset,
                                       int64_t step_index, bool greedy, float* action, float* logprob, float* entropy, const GaussStepStores* st, hipStream_t s) {
    if (!bq_shape_ok(L) || !L.gauss) return hipErrorInvalidValue;
    return L.hidden == 64 ? bq_gauss_act<64>(L, params, obs, forced, n, seed, row_offset, step_index, greedy, action, logprob, entropy, st, s)
                          : bq_gauss_act<128>(L, params, obs, forced, n, seed, row_offset, step_index, greedy, action, logprob, entropy, st, s);
}

hipError_t fused_matrix_bf16_cat_act(const GenLayout& L, int dist_kind, const float* params, const float* obs, const uint8_t* mask, const int64_t* forced, int64_t n,
                                     int64_t seed, int64_t row_offset, int64_t step_index, bool greedy, int64_t* action, float* logprob, float* entropy,
                                     const CatStepStores* st, hipStream_t s) {
    if (!bq_shape_ok(L) || L.gauss) return hipErrorInvalidValue;
    return L.hidden == 64 ? bq_cat_act<64>(L, dist_kind, params, obs, mask, forced, n, seed, row_offset, step_index, greedy, action, logprob, entropy, st, s)
                          : bq_cat_act<128>(L, dist_kind, params, obs, mask, forced, n, seed, row_offset, step_index, greedy, action, logprob, entropy, st, s);
}

hipError_t fused_matrix_bf16_values(const GenLayout& L, const float* params, const float* obs, int64_t n, float* value, hipStream_t s) {
    if (!bq_shape_ok(L)) return hipErrorInvalidValue;
    return L.hidden == 64 ? bq_values<64>(L, params, obs, n, value, s) : bq_values<128>(L, params, obs, n, value, s);
}

hipError_t fused_matrix_bf16_dev_fold(const GenLayout& L, const float* params, const DevFoldArgs& a, hipStream_t s) {
    if (!bq_shape_ok(L)) return hipErrorInvalidValue;
    return L.hidden == 64 ? bq_dev_fold<64>(L, params, a, s) : bq_dev_fold<128>(L, params, a, s);
}

hipError_t fused_matrix_bf16_fwd_bwd(const GenLayout& L, const GfUpdArgs& a, float* grads, hipStream_t s) {
    if (!bq_shape_ok(L)) return hipErrorInvalidValue;
    return L.hidden == 64 ? bq_fwd_bwd<64>(L, a, grads, s) : bq_fwd_bwd<128>(L, a, grads, s);
}
