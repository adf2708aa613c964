// ppo-libtorch_amd/csrc/kernels_fused_wide.hip -- PPO_KERNEL_FUSED_WIDE_OBS: the fused 2 x 64 families (PPO_KERNEL_GAUSS_FUSED, PPO_KERNEL_CAT_FUSED) at
// observations of 65 .. 384 columns.  kernels_gauss_fused.hip keeps all of W1 (64 x obsP) and the tile's whole X image (obsP x 68) in LDS: 528 bytes per
// observation column, 103 040 bytes at obs 64.  Here layer 1 is STREAMED: it runs over K-chunks of 64 observation columns (the last one ragged, zero padded),
// and only two chunks of W1 (64 units x 64 columns each) and two chunks of X (64 columns x 64 samples each) are in LDS at a time.  Everything else is the
// family's: one workgroup = 4 waves = one 64-sample tile at a time, W2, W3, the biases and log_std resident, H1 / H2 / OUT as [unit][sample] images of stride
// PPO_LDS_STRIDE, layers 2 and 3, the heads, the loss lanes and the backward's tile functions from gauss_fused_dev.hpp.
//
// The chunk pipeline (gw_forward_tile, the ONE forward of every kernel here, so an observation gets the same mean / logits and the same value from every entry
// point, bit for bit).  A thread owns 16 elements of a W1 chunk and 16 of an X chunk (element tid + 256 j: column 64 c + (tid & 63) of unit / sample
// (tid >> 6) + 4 j -- a wave reads 64 consecutive floats of a row).  Per chunk c:
//     global loads of chunk c + 1 (W1 from global / L2, X through the tile's row indices) into 32 registers      <- issued first, in flight during ...
//     the products of chunk c out of buffer c & 1: acc[i] = fmaf(W1[16 w + i][k], x[k][s], acc[i]), k ascending    <- ... 64 x 16 fmas per lane
//     the registers into buffer (c + 1) & 1, one barrier
// The 16 accumulators of a lane (lane = sample, wave w owns units 16 w .. 16 w + 15, as in gf_hidden_layer) start at the bias and live in registers across all
// chunks: the chain is the unchunked ascending-k chain, product for product, so a wide context whose columns 64 .. are zero gives the 64-column kernel's bits
// (fmaf(w, 0, acc) = acc).  One tanh_fast and one store into H1 follow the last chunk.  One barrier per chunk suffices because the buffer written behind
// chunk c's products is the one chunk c - 1 was read from, and chunk c - 1's barrier lies between.
//
// The update's dW1 = dZ1 X^T runs chunk by chunk too, gf_dw_tile's thread map (ub, kb, a 4 x 4 block) into a per-chunk set of 16 register accumulators; the
// chunk count NC = 2 .. 6 is a template parameter, so the sets are compile-time indexed (96 floats at NC = 6).  It walks the chunks DOWNWARD: the forward left
// chunks NC - 1 and NC - 2 in the two X buffers, so only chunks NC - 3 .. 0 are fetched again -- chunk c - 2 into the registers in front of chunk c's products,
// into buffer c & 1 behind that chunk's barrier.
//
// LDS (floats; outP = the output width rounded up to 4; the update kernel carves for the wider net, the actor):
//   W1 2 x 4096 | W2 4096 | W3 64 outP | b1 64 | b2 64 | b3 32 | log_std 32 | exp(-log_std) 32 | row index 64 | X 2 x 64 68 | H1 64 68 | H2 64 68 | OUT outP 68
//   32 outputs (the largest shape served, any obs): 8192 + 4096 + 2048 + 288 + 8704 + 4352 + 4352 + 2176 = 34 208 floats = 136 832 bytes of 163 840.
//   1 output (the critic kernel, the fold): 8192 + 4096 + 256 + 288 + 8704 + 8704 + 272 = 30 512 floats = 122 048 bytes; the fold adds its list, 1 056 bytes.
//   Always above 64 KB (the attribute is asked for) and ONE workgroup per CU -- arithmetic, not a measurement.  The size does not depend on obs_size.
// Known cost: W1 is re-streamed from global / L2 once per tile (64 x obs floats, up to 96 KB); two tiles per chunk would halve it (not built).
#include "gauss_fused_dev.hpp"

namespace {

static_assert(GW_K == 64 && GF_THREADS == 256, "a thread owns elements tid + 256 j, j < 16, of a 64 x 64 chunk; tid & 63 is its column");

struct GwLds {
    GfLds m;            // the family's images; m.w1 / m.x name buffer 0 of the two chunk buffers each has, m.obsP is the chunk width
};
// buffer b (0 / 1) of the W1 chunks and of the X chunks: arithmetic on the base, so a run-time b indexes no array of pointers
__device__ __forceinline__ float* gw_w1(const GwLds& g, int b) { return g.m.w1 + b * (64 * GW_K); }
__device__ __forceinline__ float* gw_x(const GwLds& g, int b) { return g.m.x + b * (GW_K * GF_S); }

__host__ __device__ inline int gw_lds_floats(int outP) { return 2 * 64 * GW_K + 4096 + 64 * outP + 64 + 64 + 32 + 32 + 32 + 64 + 2 * GW_K * GF_S + 64 * GF_S + 64 * GF_S + outP * GF_S; }

__device__ __forceinline__ GwLds gw_carve(float* base, int outP) {
    GwLds g;
    GfLds& m = g.m;
    m.obsP = GW_K; m.outP = outP;
    float* p = base;
    m.w1 = p; p += 2 * 64 * GW_K;
    m.w2 = p; p += 4096;
    m.w3 = p; p += 64 * outP;
    m.b1 = p; p += 64;
    m.b2 = p; p += 64;
    m.b3 = p; p += 32;
    m.ls = p; p += 32;
    m.inv = p; p += 32;
    m.ridx = reinterpret_cast<int*>(p); p += 64;
    m.x = p; p += 2 * GW_K * GF_S;
    m.h1 = p; p += 64 * GF_S;
    m.h2 = p; p += 64 * GF_S;
    m.o = p;
    return g;
}

// chunk c of W1 [64, O]: this thread's 16 elements, zero behind column O
__device__ __forceinline__ void gw_fetch_w(const float* __restrict__ W1, int O, int c, int tid, float (&r)[16]) {
    const int k = GW_K * c + (tid & 63), u0 = tid >> 6;
#pragma unroll
    for (int j = 0; j < 16; j++) r[j] = k < O ? W1[(u0 + 4 * j) * O + k] : 0.0f;
}
__device__ __forceinline__ void gw_store_w(float* __restrict__ w1, int tid, const float (&r)[16]) {
    const int k = tid & 63, u0 = tid >> 6;
#pragma unroll
    for (int j = 0; j < 16; j++) w1[(u0 + 4 * j) * GW_K + k] = r[j];
}
// one chunk of layer 1 onto the lane's accumulators: gf_hidden_layer's loop between the bias and the tanh
__device__ __forceinline__ void gw_l1_chunk(const float* __restrict__ W, const float* __restrict__ in, int K, int s, int w, float (&acc)[16]) {
    for (int k = 0; k < K; k += 4) {
        const float x0 = in[(k + 0) * GF_S + s], x1 = in[(k + 1) * GF_S + s], x2 = in[(k + 2) * GF_S + s], x3 = in[(k + 3) * GF_S + s];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const float4 wv = *reinterpret_cast<const float4*>(&W[(16 * w + i) * GW_K + k]);
            acc[i] = __builtin_fmaf(wv.x, x0, acc[i]);
            acc[i] = __builtin_fmaf(wv.y, x1, acc[i]);
            acc[i] = __builtin_fmaf(wv.z, x2, acc[i]);
            acc[i] = __builtin_fmaf(wv.w, x3, acc[i]);
        }
    }
}

// THE forward pass of every kernel in this file: the tile whose row indices are in m.ridx (published by the caller's barrier, as are the staged upper layers)
// through obs -> 64 -> 64 -> out, layer 1 over nc = ceil(O / 64) chunks as described at the head of the file.  Leaves H1, H2 (post-tanh), OUT rows
// 0 .. out - 1, chunk nc - 1 of X in buffer (nc - 1) & 1 and chunk nc - 2 in the other.  Every thread of the workgroup calls it; the caller's barrier behind
// the previous tile has freed every image.
__device__ __forceinline__ void gw_forward_tile(const GwLds& g, const GfShape& sh, const float* __restrict__ params, int net, const float* __restrict__ obs, int nc,
                                                int out, int tid) {
    const GfLds& m = g.m;
    const int s = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), O = sh.obs;
    const float* W1 = params + sh.off[net][0];
    float rw[16], rx[16], acc[16];
    gw_fetch_w(W1, O, 0, tid, rw);
    gw_fetch_x(obs, O, m.ridx, 0, tid, rx);
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = m.b1[16 * w + i];
    gw_store_w(gw_w1(g, 0), tid, rw);
    gw_store_x(gw_x(g, 0), tid, rx);
    __syncthreads();
    for (int c = 0; c < nc; c++) {
        const bool more = c + 1 < nc;   // uniform
        if (more) {
            gw_fetch_w(W1, O, c + 1, tid, rw);
            gw_fetch_x(obs, O, m.ridx, c + 1, tid, rx);
        }
        gw_l1_chunk(gw_w1(g, c & 1), gw_x(g, c & 1), gw_chunk_cols(O, c), s, w, acc);
        if (more) {
            gw_store_w(gw_w1(g, (c + 1) & 1), tid, rw);
            gw_store_x(gw_x(g, (c + 1) & 1), tid, rx);
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) m.h1[(16 * w + i) * GF_S + s] = tanh_fast(acc[i]);
    __syncthreads();
    gf_forward_upper(m, out, s, w);
}

// ---------------------------------------------------------------------------------------------------------
// The act kernels: gauss_act_kernel's / cat_act_kernel's plan (wave 0 the heads, waves 1 .. 3 the step's stores: gauss_act_rows / cat_act_rows) behind the
// wide forward.  Every pointer names the first of the launch's n rows (an env group's slice: row_offset carries its origin).
// ---------------------------------------------------------------------------------------------------------
template <bool GREEDY>
__global__ __launch_bounds__(GF_THREADS) void gw_gauss_act_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs,
                                                                  const float* __restrict__ forced, int64_t n, int64_t seed, int64_t row_offset, int64_t step_index,
                                                                  float* action, float* logprob, float* entropy, GfStepStores st) {
    extern __shared__ __attribute__((aligned(16))) float gw_lds[];
    const int tid = threadIdx.x, D = sh.D, O = sh.obs, nc = gw_chunks(O);
    const GwLds g = gw_carve(gw_lds, gf_pad4(D));
    gf_stage_upper(g.m, sh, params, 1, tid);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(g.m, row0, n, tid);
        gw_forward_tile(g, sh, params, 1, obs, nc, D, tid);
        gauss_act_rows<GREEDY>(g.m, D, O, obs, forced, row0, n, seed, row_offset, step_index, action, logprob, entropy, st, tid);
        __syncthreads();   // OUT and the row list are read: the next tile may overwrite them
    }
}

template <int DIST, bool GREEDY>
__global__ __launch_bounds__(GF_THREADS) void gw_cat_act_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs,
                                                                const uint8_t* __restrict__ mask, const int64_t* __restrict__ forced, int64_t n, int64_t seed,
                                                                int64_t row_offset, int64_t step_index, int64_t* action, float* logprob, float* entropy,
                                                                CfStepStores st) {
    extern __shared__ __attribute__((aligned(16))) float gw_lds[];
    const int tid = threadIdx.x, A = sh.A, nc = gw_chunks(sh.obs);
    const GwLds g = gw_carve(gw_lds, gf_pad4(A));
    gf_stage_upper(g.m, sh, params, 1, tid);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(g.m, row0, n, tid);
        gw_forward_tile(g, sh, params, 1, obs, nc, A, tid);
        cat_act_rows<DIST, GREEDY>(g.m, sh, obs, mask, forced, row0, n, seed, row_offset, step_index, action, logprob, entropy, st, tid);
        __syncthreads();   // OUT, the H1 columns and the row list are read: the next tile may overwrite them
    }
}

// the critic over n rows
__global__ __launch_bounds__(GF_THREADS) void gw_values_kernel(GfShape sh, const float* __restrict__ params, const float* __restrict__ obs, int64_t n,
                                                               float* __restrict__ value) {
    extern __shared__ __attribute__((aligned(16))) float gw_lds[];
    const int tid = threadIdx.x, nc = gw_chunks(sh.obs);
    const GwLds g = gw_carve(gw_lds, 4);
    gf_stage_upper(g.m, sh, params, 0, tid);
    const int64_t tiles = (n + 63) / 64;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64;
        gf_dense_rows(g.m, row0, n, tid);
        gw_forward_tile(g, sh, params, 0, obs, nc, 1, tid);
        if (tid < 64 && row0 + tid < n) value[row0 + tid] = g.m.o[tid];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------
// gw_dev_fold_kernel (ppo_dev_observe with truncation flags): gauss_dev_fold_kernel's front end -- a 256-thread workgroup owns env rows [256 b, 256 b + 256),
// ONE compaction, and a workgroup without a flagged row returns before it loads a weight (the count is the same in every thread, so the return is uniform).
// Otherwise the critic's upper layers are staged on gw_values_kernel's carve and the workgroup walks its list (ascending, up to 256 rows) in tiles of 64: the
// list's row numbers, or -1, are the tile's row indices, the forward reads those rows of final_obs [N, O] and no other, and it is gw_values_kernel's forward, so
// v is that kernel's value of the row, bit for bit.  Lane k of wave 0 folds row k of the tile (dev_fold_store).  LDS: all dynamic, the row list [256] and the
// waves' totals [8] behind the carve.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DEV_FOLD_THREADS) void gw_dev_fold_kernel(GfShape sh, const float* __restrict__ params, DevFoldArgs a) {
    static_assert(DEV_FOLD_THREADS == GF_THREADS, "fold_compact and gw_forward_tile are written for the same workgroup");
    extern __shared__ __attribute__((aligned(16))) float gw_lds[];
    const int tid = threadIdx.x, nc = gw_chunks(sh.obs);
    int* list = reinterpret_cast<int*>(gw_lds + gw_lds_floats(4));
    int* wtot = list + DEV_FOLD_THREADS;
    const int cnt = dev_fold_compact(a, list, wtot);
    if (cnt == 0) return;
    const int base = wtot[4];
    const GwLds g = gw_carve(gw_lds, 4);
    gf_stage_upper(g.m, sh, params, 0, tid);
    for (int k0 = 0; k0 < cnt; k0 += 64) {
        const int k = k0 + tid;   // tid < 64: this lane's place in the list
        if (tid < 64) g.m.ridx[tid] = k < cnt ? list[k] : -1;
        __syncthreads();
        gw_forward_tile(g, sh, params, 0, a.final_obs, nc, 1, tid);
        if (tid < 64 && k < cnt) dev_fold_store(a, base, k, list[k], g.m.o[tid]);
        __syncthreads();   // OUT and the row indices are read: the next tile may overwrite them
    }
}

// ---------------------------------------------------------------------------------------------------------
// gw_fwd_bwd_kernel<DIST, NC>: gf_fwd_bwd_body's plan (kernels_gauss_fused.hip) for NC chunks of observation columns: the wide forward, the family's loss lanes
// and upper backward, then dW1 chunk by chunk, downward (the head of the file).  The slab layout, the loss partials and the second launch
// (gauss_slab_reduce_kernel) are the family's.
// ---------------------------------------------------------------------------------------------------------
template <int DIST, int NC>
__global__ __launch_bounds__(GF_THREADS) void gw_fwd_bwd_kernel(GfUpdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gw_lds[];
    const int tid = threadIdx.x, O = a.sh.obs;
    const int net = blockIdx.y, b = blockIdx.x, nb = a.nb;
    const int out = net == 0 ? 1 : a.sh.A, outP = gf_pad4(out);
    const GwLds g = gw_carve(gw_lds, gf_pad4(a.sh.A));
    const GfLds& m = g.m;
    gf_stage_upper(m, a.sh, a.params, net, tid);
    const int s = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ub = tid >> 4, kb = tid & 15;

    float gW1[NC][16], gW2[16], gW3[16], gb1[4], gb2[4], gb3[4];
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int i = 0; i < 16; i++) gW1[c][i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; i++) gW2[i] = gW3[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) gb1[i] = gb2[i] = gb3[i] = 0.0f;
    GfLossState ls;
    gf_loss_begin(a, net, w, ls);

    const int tiles = (a.M + 63) / 64;
    for (int tile = b; tile < tiles; tile += nb) {
        if (tid < 64) m.ridx[tid] = tile * 64 + tid < a.M ? a.idx[tile * 64 + tid] : -1;
        __syncthreads();
        gw_forward_tile(g, a.sh, a.params, net, a.obs, NC, out, tid);
        if (w == 0) gf_loss_lanes<DIST>(a, m, net, out, outP, s, ls);
        __syncthreads();
        gf_backward_upper(m, out, outP, s, w, ub, kb, gW2, gb2, gW3, gb3);
        // dW1 = dZ1 X^T, db1: chunk c out of buffer c & 1 (chunks NC - 1 and NC - 2 are the forward's; chunk c - 2 arrives behind chunk c's barrier)
        float rx[16];
#pragma unroll
        for (int c = NC - 1; c >= 0; c--) {
            if (c >= 2) gw_fetch_x(a.obs, O, m.ridx, c - 2, tid, rx);
            float no_bias[4] = { 0.0f, 0.0f, 0.0f, 0.0f };   // db1 is summed once, with chunk 0 (whole: every thread runs it)
            if (4 * kb < gw_chunk_cols(O, c)) gf_dw_tile(m.h1, gw_x(g, c & 1), ub, kb, gW1[c], c == 0 ? gb1 : no_bias);
            __syncthreads();                                 // ... has read the buffer; behind chunk 0: the images are free for the next tile
            if (c >= 2) gw_store_x(gw_x(g, c & 1), tid, rx);
        }
    }

    float* slab = a.slab + ((size_t)net * nb + b) * a.slab_stride;
#pragma unroll
    for (int c = 0; c < NC; c++) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int u = 4 * ub + i, k = GW_K * c + 4 * kb + j;
                if (k < O) slab[u * O + k] = gW1[c][i * 4 + j];
            }
        }
    }
    gf_store_upper<DIST>(a, slab, net, b, out, s, w, ub, kb, gW2, gW3, gb1, gb2, gb3, ls);
}

template <int DIST, int NC>
hipError_t gw_upd_launch(const GfUpdArgs& a, int bytes, hipStream_t s) {
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, gw_fwd_bwd_kernel<DIST, NC>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((gw_fwd_bwd_kernel<DIST, NC>), dim3(a.nb, 2), dim3(GF_THREADS), bytes, s, a);
    return hipGetLastError();
}
template <int DIST>
hipError_t gw_upd_chunks(int nc, const GfUpdArgs& a, int bytes, hipStream_t s) {
    switch (nc) {
        case 2: return gw_upd_launch<DIST, 2>(a, bytes, s);
        case 3: return gw_upd_launch<DIST, 3>(a, bytes, s);
        case 4: return gw_upd_launch<DIST, 4>(a, bytes, s);
        case 5: return gw_upd_launch<DIST, 5>(a, bytes, s);
        case 6: return gw_upd_launch<DIST, 6>(a, bytes, s);
    }
    return hipErrorInvalidValue;
}

template <int DIST, bool GREEDY>
hipError_t gw_cat_act_launch(const GfShape& sh, int bytes, dim3 grid, const float* params, const float* obs, const uint8_t* mask, const int64_t* forced, int64_t n,
                             int64_t seed, int64_t row_offset, int64_t step_index, int64_t* action, float* logprob, float* entropy, const CfStepStores& ss, hipStream_t s) {
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, gw_cat_act_kernel<DIST, GREEDY>, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((gw_cat_act_kernel<DIST, GREEDY>), grid, dim3(GF_THREADS), bytes, s, sh, params, obs, mask, forced, n, seed, row_offset, step_index, action,
                       logprob, entropy, ss);
    return hipGetLastError();
}

// the shapes this file's kernels are launched for: the chunk count is 2 .. 6
bool gw_shape_ok(const GenLayout& L) { return L.obs > GAUSS_FUSED_MAX_OBS && L.obs <= FUSED_WIDE_MAX_OBS && L.act >= 1 && L.act <= PPO_MAX_ACT; }

}  // namespace

bool fused_wide_serves_obs(int obs) { return obs >= 1 && obs <= FUSED_WIDE_MAX_OBS; }

hipError_t fused_wide_gauss_act(const GenLayout& L, const float* params, const float* obs, const float* forced, int64_t n, int64_t seed, int64_t row_offset,
                                int64_t step_index, bool greedy, float* action, float* logprob, float* entropy, const GaussStepStores* st, hipStream_t s) {
    if (!gw_shape_ok(L) || !L.gauss) return hipErrorInvalidValue;
    const GfShape sh = gf_shape(L);
    const int bytes = gw_lds_floats(gf_pad4(L.gauss)) * 4;
    const dim3 grid((unsigned)std::min<int64_t>((n + 63) / 64, 1024)), block(GF_THREADS);
    GfStepStores ss{};
    if (st) ss = GfStepStores{ st->done_prev, st->obs_t, st->act_t, st->lp_t, st->dones_t };
    static std::atomic<unsigned long long> done_g{ 0 }, done_s{ 0 };
    if (greedy) {
        const hipError_t e = gf_allow(done_g, gw_gauss_act_kernel<true>, bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(gw_gauss_act_kernel<true>, grid, block, bytes, s, sh, params, obs, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss);
    } else {
        const hipError_t e = gf_allow(done_s, gw_gauss_act_kernel<false>, bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(gw_gauss_act_kernel<false>, grid, block, bytes, s, sh, params, obs, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss);
    }
    return hipGetLastError();
}

hipError_t fused_wide_cat_act(const GenLayout& L, int dist_kind, const float* params, const float* obs, const uint8_t* mask, const int64_t* forced, int64_t n,
                              int64_t seed, int64_t row_offset, int64_t step_index, bool greedy, int64_t* action, float* logprob, float* entropy,
                              const CatStepStores* st, hipStream_t s) {
    if (!gw_shape_ok(L) || L.gauss) return hipErrorInvalidValue;
    const GfShape sh = gf_shape(L);
    const int bytes = gw_lds_floats(gf_pad4(L.act)) * 4;
    const dim3 grid((unsigned)std::min<int64_t>((n + 63) / 64, 1024));
    CfStepStores ss{};
    if (st) ss = CfStepStores{ st->done_prev, st->obs_t, st->mask_t, st->act_t, st->lp_t, st->dones_t };
    const bool masked = dist_kind == PPO_DIST_MASKED;
    if (greedy)
        return masked ? gw_cat_act_launch<PPO_DIST_MASKED, true>(sh, bytes, grid, params, obs, mask, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss, s)
                      : gw_cat_act_launch<PPO_DIST_CATEGORICAL, true>(sh, bytes, grid, params, obs, mask, nullptr, n, seed, row_offset, step_index, action, logprob, entropy, ss, s);
    return masked ? gw_cat_act_launch<PPO_DIST_MASKED, false>(sh, bytes, grid, params, obs, mask, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss, s)
                  : gw_cat_act_launch<PPO_DIST_CATEGORICAL, false>(sh, bytes, grid, params, obs, mask, forced, n, seed, row_offset, step_index, action, logprob, entropy, ss, s);
}

hipError_t fused_wide_values(const GenLayout& L, const float* params, const float* obs, int64_t n, float* value, hipStream_t s) {
    if (!gw_shape_ok(L)) return hipErrorInvalidValue;
    const GfShape sh = gf_shape(L);
    const int bytes = gw_lds_floats(4) * 4;
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, gw_values_kernel, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gw_values_kernel, dim3((unsigned)std::min<int64_t>((n + 63) / 64, 1024)), dim3(GF_THREADS), bytes, s, sh, params, obs, n, value);
    return hipGetLastError();
}

hipError_t fused_wide_dev_fold(const GenLayout& L, const float* params, const DevFoldArgs& a, hipStream_t s) {
    if (!gw_shape_ok(L)) return hipErrorInvalidValue;
    const GfShape sh = gf_shape(L);
    // the row list and the waves' totals are part of the dynamic allocation: the attribute is decided on every byte of LDS the kernel uses
    const int bytes = gw_lds_floats(4) * 4 + GF_DEV_FOLD_LIST_INTS * (int)sizeof(int);
    static std::atomic<unsigned long long> done{ 0 };
    const hipError_t e = gf_allow(done, gw_dev_fold_kernel, bytes);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)(((int64_t)a.N + DEV_FOLD_THREADS - 1) / DEV_FOLD_THREADS);
    hipLaunchKernelGGL(gw_dev_fold_kernel, dim3(grid), dim3(DEV_FOLD_THREADS), bytes, s, sh, params, a);
    return hipGetLastError();
}

hipError_t fused_wide_fwd_bwd(const GenLayout& L, const GfUpdArgs& a, float* grads, hipStream_t s) {
    if (!gw_shape_ok(L)) return hipErrorInvalidValue;
    const int nc = (L.obs + GW_K - 1) / GW_K;
    const int bytes = gw_lds_floats(gf_pad4(L.act)) * 4;
    hipError_t e;
    if (L.gauss) e = gw_upd_chunks<PPO_DIST_GAUSSIAN>(nc, a, bytes, s);
    else if (a.hp.dist_kind == PPO_DIST_MASKED) e = gw_upd_chunks<PPO_DIST_MASKED>(nc, a, bytes, s);
    else e = gw_upd_chunks<PPO_DIST_CATEGORICAL>(nc, a, bytes, s);
    if (e != hipSuccess) return e;
    return gauss_fused_slab_reduce(L, a.slab, a.slab_stride, a.nb, grads, s);
}
