// ppo-libtorch_amd/csrc/kernels_rollout.hip -- rollout-side kernels for gfx950 (wave64).
//
//   K1  batched env step + auto-reset (struct-of-arrays)      reference PPO_Discrete.cpp:413-483, CartPole.cpp, MountainCar.cpp
//   K2  policy forward + categorical sample/log-prob/entropy  reference Agent.cpp:117-170, Categorical*.cpp
//   K3  rollout stores                                        reference PPO_Discrete.cpp:529-546
//   fused: the whole T-step rollout loop (PPO_Discrete.cpp:524-548) as ONE launch.
//
// Mapping: the reference's hidden width is 64 = one CDNA4 wavefront, so ONE WAVE OWNS ONE ENV (or one batch row) and
// LANE j OWNS HIDDEN UNIT j of both the actor and the critic.  A lane keeps its rows of W1/W2 (2 x (O + 64) floats) in
// VGPRs for the whole launch; a layer's activations are exchanged through a 512-byte LDS slab written once and
// read back as wave-uniform (broadcast) 16-byte reads; head outputs are wave reductions (__shfl_xor).  Envs never
// interact inside a rollout, so no grid-level synchronisation exists: the T-step loop runs inside the kernel.
// Per step a wave touches HBM only for the stores of K3 (obs 4*O B, action, log-prob, value, reward, done).
#include <cstdlib>

#include "ppo_internal.hpp"

namespace {

// Rows j = lane of one net's W1 / W2 (and the matching biases) as seen by one lane.
template <int OBS>
struct LaneNet {
    float w1[OBS], b1, w2[PPO_HIDDEN], b2;
};

template <int OBS>
__device__ __forceinline__ void load_lane_net(LaneNet<OBS>& n, const float* __restrict__ p, const NetLayout& L, int net, int lane) {
#pragma unroll
    for (int k = 0; k < OBS; k++) n.w1[k] = p[L.w1[net] + lane * OBS + k];
    n.b1 = p[L.b1[net] + lane];
#pragma unroll
    for (int k = 0; k < PPO_HIDDEN; k++) n.w2[k] = p[L.w2[net] + lane * PPO_HIDDEN + k];
    n.b2 = p[L.b2[net] + lane];
}

// One MLP trunk for one row: obs[] is wave-uniform.  Returns this lane's second-layer activation.  lds: 64 floats of this wave.
template <int OBS>
__device__ __forceinline__ float trunk_forward(const LaneNet<OBS>& n, const float* obs, float* lds, int lane) {
    float z = n.b1;
#pragma unroll
    for (int k = 0; k < OBS; k++) z = __builtin_fmaf(obs[k], n.w1[k], z);
    __syncthreads();  // previous readers of lds are done (single-wave workgroup: a wait, no s_barrier)
    lds[lane] = tanh_mufu(z);
    __syncthreads();
    float acc = n.b2;
    const float4* h4 = reinterpret_cast<const float4*>(lds);
#pragma unroll
    for (int k = 0; k < PPO_HIDDEN / 4; k++) {
        const float4 h = h4[k];  // wave-uniform address: LDS broadcast
        acc = __builtin_fmaf(h.x, n.w2[4 * k], acc); acc = __builtin_fmaf(h.y, n.w2[4 * k + 1], acc);
        acc = __builtin_fmaf(h.z, n.w2[4 * k + 2], acc); acc = __builtin_fmaf(h.w, n.w2[4 * k + 3], acc);
    }
    return tanh_mufu(acc);
}

// Heads: value = b3c + sum_j h2c[j] W3c[j];  logits[a] = b3a[a] + sum_j h2a[j] W3a[a][j]  (wave reductions).
__device__ __forceinline__ float critic_head(const float* __restrict__ p, const NetLayout& L, float h2c, int lane) {
    return wave_sum(h2c * p[L.w3[0] + lane]) + p[L.b3[0]];
}

// Actor head + Categorical over every head.  Two code shapes with identical arithmetic per element:
//   AMAX == 4  : sum(head_dims) <= 4 (CartPole 2, MountainCar 3): everything statically indexed -> registers;
//   AMAX == 32 : generic (runtime-indexed small arrays, compiler places them in scratch).
// Wave-uniform arithmetic (every lane computes the same values).  act[] in (forced) / out (sampled).
// EXACTA > 0: the policy has ONE head of exactly EXACTA actions (the reference's two shapes): every loop bound is a constant.
// philox_cache (optional): the four 32-bit words of the Philox call that serves steps 4k .. 4k+3 of head 0, kept by the caller
// across steps and refreshed here when step_index % 4 == 0 (or when *cache_valid is false).
// heads_from_logits: everything after the actor's output layer (z[] = raw logits in, consumed).
// GREEDY: Categorical::mode / CategoricalMasked::mode (Categorical.cpp:139-141, CategoricalMasked.cpp:160-162) instead of a draw: argmax of m_probs, the
// FIRST index on equal values; no random number is formed.
template <int DIST, int AMAX, int EXACTA = 0, bool GREEDY = false>
__device__ __forceinline__ void heads_from_logits(float* z, const NetLayout& L, const uint8_t* mask_row, bool all_valid, bool sample, int64_t seed,
                                                  int64_t row_global, int64_t step_index, int* act, float& logprob, float& entropy,
                                                  uint4* philox_cache = nullptr, bool* cache_valid = nullptr, bool cache_fresh = false) {
    const int A = EXACTA ? EXACTA : L.act;
    const int n_heads = EXACTA ? 1 : L.n_heads;
    float pr[AMAX];
    bool ok[AMAX];
#pragma unroll
    for (int a = 0; a < AMAX; a++) {
        pr[a] = 0.0f; ok[a] = true;
        if (a < A) {
            if (DIST == PPO_DIST_MASKED && !all_valid && mask_row) ok[a] = mask_row[a] != 0;
            if (DIST == PPO_DIST_MASKED && !ok[a]) z[a] = -1e8f;   // torch::where(mask, logits, -1e8f), CategoricalMasked.cpp:34-35
        }
    }
    logprob = 0.0f;
    entropy = 0.0f;
    int off = 0;
    for (int h = 0; h < n_heads; h++) {
        const int Ah = EXACTA ? EXACTA : L.head_dims[h];
        float mx = -INFINITY;
#pragma unroll
        for (int a = 0; a < AMAX; a++) if (a >= off && a < off + Ah) mx = z[a] > mx ? z[a] : mx;
        float se = 0.0f;
#pragma unroll
        for (int a = 0; a < AMAX; a++) if (a >= off && a < off + Ah) { pr[a] = fast_exp(z[a] - mx); se += pr[a]; }
        const float lse = fast_log(se) + mx;
        const float rse = __builtin_amdgcn_rcpf(se);
        float ent = 0.0f;
#pragma unroll
        for (int a = 0; a < AMAX; a++) if (a >= off && a < off + Ah) {
            z[a] = z[a] - lse;          // m_logits
            pr[a] = pr[a] * rse;        // m_probs
            if (DIST == PPO_DIST_CATEGORICAL) {
                const float l = z[a] > 1.17549435e-38f ? z[a] : 1.17549435e-38f;  // clamp(m_logits, FLT_MIN), Categorical.cpp:115
                ent += l * pr[a];
            } else {
                const float plp = z[a] * pr[a];
                ent += ok[a] ? plp : 0.0f;                                         // where(mask, p_log_p, 0), CategoricalMasked.cpp:141
            }
        }
        ent = -ent;
        if constexpr (GREEDY) {
            int best = 0;
            float pb = -1.0f;
#pragma unroll
            for (int a = 0; a < AMAX; a++) if (a >= off && a < off + Ah) {
                if (pr[a] > pb) { pb = pr[a]; best = a - off; }
            }
            act[h] = best;
        } else if (sample) {
            // one Philox call feeds four consecutive steps: counter (row, step / 4, head, 0), word step % 4
            uint4 w;
            if (philox_cache && h == 0) {
                if (!cache_fresh && (!*cache_valid || (step_index & 3) == 0)) {   // cache_fresh: the caller has refreshed the cache for this step already
                    *philox_cache = philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)row_global, (uint32_t)(step_index >> 2), 0u, 0u);
                    *cache_valid = true;
                }
                w = *philox_cache;
            } else {
                w = philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)row_global, (uint32_t)(step_index >> 2), (uint32_t)h, 0u);
            }
            const uint32_t wsel = (step_index & 3) == 0 ? w.x : ((step_index & 3) == 1 ? w.y : ((step_index & 3) == 2 ? w.z : w.w));
            const float u = (float)(wsel >> 8) * 0x1p-24f;
            int pick = 0, last = 0;
            float acc = 0.0f;
            bool hit = false;
#pragma unroll
            for (int a = 0; a < AMAX; a++) if (a >= off && a < off + Ah) {
                if (pr[a] > 0.0f) last = a - off;
                acc += pr[a];
                if (!hit && u < acc) { pick = a - off; hit = true; }
            }
            act[h] = hit ? pick : last;
        }
        float lp = 0.0f;
#pragma unroll
        for (int a = 0; a < AMAX; a++) if (a == off + act[h]) lp = z[a];
        if (h == 0) { logprob = lp; entropy = ent; } else { logprob += lp; entropy += ent; }  // stack(...).sum(0), Agent.cpp:165-168
        off += Ah;
    }
}

template <int DIST, int AMAX, int EXACTA = 0, bool GREEDY = false>
__device__ __forceinline__ void actor_heads(const float* __restrict__ p, const NetLayout& L, float h2a, int lane, const uint8_t* mask_row,
                                            bool all_valid, bool sample, int64_t seed, int64_t row_global, int64_t step_index, int* act,
                                            float& logprob, float& entropy, uint4* philox_cache = nullptr, bool* cache_valid = nullptr) {
    const int A = EXACTA ? EXACTA : L.act;
    float z[AMAX];
#pragma unroll
    for (int a = 0; a < AMAX; a++) {
        z[a] = 0.0f;
        if (a < A) z[a] = wave_sum(h2a * p[L.w3[1] + a * PPO_HIDDEN + lane]) + p[L.b3[1] + a];
    }
    heads_from_logits<DIST, AMAX, EXACTA, GREEDY>(z, L, mask_row, all_valid, sample, seed, row_global, step_index, act, logprob, entropy, philox_cache, cache_valid);
}

// ---------------------------------------------------------------------------------------------------------
// Fused rollout: grid = N workgroups of one wave.  Only the ACTOR sits on the env loop's dependency chain
// (obs -> logits -> action -> physics -> next obs); the critic's values are a pure function of the stored observations
// and are produced afterwards by values_kernel over all T*N + N rows at once (same per-row arithmetic).
// ---------------------------------------------------------------------------------------------------------
template <int ENV, int DIST, int OBS, int AMAX, int EXACTA>
__global__ __launch_bounds__(64, (AMAX <= 4 ? 2 : 1)) void rollout_kernel(RolloutArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[PPO_HIDDEN];
    const int lane = threadIdx.x;
    // Blocks are dealt round-robin to the 8 XCDs: give each XCD a contiguous range of envs so the partial-line stores
    // of neighbouring envs meet in one L2 (speed only; any mapping is correct).
    int env = blockIdx.x;
    {
        const int nb = gridDim.x, q = nb / 8, r = nb % 8, x = blockIdx.x % 8, i = blockIdx.x / 8;
        env = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
    }
    if (env >= a.N) return;
    const NetLayout& L = a.L;
    const int N = a.N, H = EXACTA ? 1 : L.n_heads, A = EXACTA ? EXACTA : L.act;
    const int64_t env_global = a.env_offset + env;
    uint4 philox_words = make_uint4(0u, 0u, 0u, 0u);
    bool philox_valid = false;

    LaneNet<OBS> actor;
    load_lane_net<OBS>(actor, a.params, L, 1, lane);

    float st[OBS];
#pragma unroll
    for (int k = 0; k < OBS; k++) st[k] = a.env_state[(size_t)k * N + env];
    int ep_len = a.ep_len[env];
    float ep_rew = a.ep_rew[env];
    int resets = a.reset_count[env];
    int done = a.next_done[env];

    for (int t = 0; t < a.T; t++) {
        const size_t tn = (size_t)t * N + env;
        // m_obs[step] = next_obs; m_dones[step] = next_done   (PPO_Discrete.cpp:529-530)
        if (lane < OBS) a.obs[tn * OBS + lane] = st[lane];
        const float h2a = trunk_forward<OBS>(actor, st, lds, lane);
        int act[PPO_MAX_HEADS];
        const bool forced = a.forced_actions != nullptr;
        if (forced) {
            for (int h = 0; h < H; h++) act[h] = (int)a.forced_actions[tn * H + h];
        }
        float logprob, entropy;
        // MountainCar::getActionMask is all-ones (MountainCar.cpp:69-77): every action valid
        actor_heads<DIST, AMAX, EXACTA>(a.params, L, h2a, lane, nullptr, true, !forced, a.seed, env_global, a.step_base + t, act, logprob, entropy,
                                        &philox_words, &philox_valid);

        // env step + truncation + auto-reset (PPO_Discrete.cpp:440-458)
        int term;
        const float reward = env_step<ENV>(st, act[0], term);
        ep_len += 1;        // CartPole.cpp:90-91
        ep_rew += reward;
        if (ep_len == a.max_episode_steps) term = 1;
        int fin_len = 0;
        float fin_rew = 0.0f;
        if (term) {
            fin_len = ep_len;
            fin_rew = ep_rew;
            int k = resets++;
            if (ENV == PPO_ENV_CARTPOLE && k >= a.reset_cap) { k = a.reset_cap - 1; if (lane == 0) atomicOr(a.error_flag, 1); }
            env_reset<ENV>(st, a.reset_table, k, a.seed, env_global);
            ep_len = 0;
            ep_rew = 0.0f;
        }
        if (lane == 0) {
            a.dones[tn] = (float)done;
            a.logprobs[tn] = logprob;    // :538
            a.rewards[tn] = reward;      // :544
            a.fin_len[tn] = fin_len;     // :455-456
            a.fin_rew[tn] = fin_rew;
        }
        if (lane < H) a.actions[tn * H + lane] = act[lane];                          // :537
        if (DIST == PPO_DIST_MASKED && a.masks && lane < A) a.masks[tn * A + lane] = 1;  // PPO_MultiDiscrete.cpp:555
        done = term;
    }

    // hand-over state
    if (lane == 0) {
        a.next_done[env] = done;
        a.ep_len[env] = ep_len;
        a.ep_rew[env] = ep_rew;
        a.reset_count[env] = resets;
    }
    if (lane < OBS) {
        a.next_obs[(size_t)env * OBS + lane] = st[lane];
        a.env_state[(size_t)lane * N + env] = st[lane];
    }
}

// ---------------------------------------------------------------------------------------------------------
// Fused rollout, TWO envs per wave (the reference's single-head policies): lanes 0-31 run env 2b, lanes 32-63 env 2b + 1, and lane l
// of a half owns hidden units l and l + 32 of its env's actor.  The per-unit work (layers 1 and 2) is the same number of fmas
// per env as in rollout_kernel; everything that rollout_kernel computes redundantly in all 64 lanes -- softmax, sampling, Philox,
// env physics with its fp64 sin/cos, episode bookkeeping, stores -- is now done for two envs by one instruction stream.
// Arithmetic per env is bit-identical to rollout_kernel / policy_act_kernel: unit j's products are summed inside rows of 16
// units with the same DPP butterfly, and the four row sums are added in the same order ((R0 + R1) + R2) + R3.
// ---------------------------------------------------------------------------------------------------------
// row sums of a per-lane value: after the butterfly every lane of a 16-lane row holds the row's sum (same steps as wave_sum)
__device__ __forceinline__ float row16_sum(float v) {
    v = PPO_DPP_ADD(v, 0xB1);
    v = PPO_DPP_ADD(v, 0x4E);
    v = PPO_DPP_ADD(v, 0x141);
    v = PPO_DPP_ADD(v, 0x140);
    return v;
}

template <int ENV, int DIST, int OBS, int EXACTA>
__global__ __launch_bounds__(64, 2) void rollout2_kernel(RolloutArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * PPO_HIDDEN];
    const int lane = threadIdx.x, half = lane >> 5, l = lane & 31;
    int pair = blockIdx.x;
    {   // contiguous env ranges per XCD, as in rollout_kernel
        const int nb = gridDim.x, q = nb / 8, r = nb % 8, x = blockIdx.x % 8, i = blockIdx.x / 8;
        pair = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
    }
    const int N = a.N;
    int env = 2 * pair + half;
    const bool live = env < N;          // odd N: the last wave's upper half idles (computes on env N - 1, stores nothing)
    if (!live) env = N - 1;
    const NetLayout& L = a.L;
    constexpr int H = 1, A = EXACTA;
    const int64_t env_global = a.env_offset + env;
    const float* __restrict__ P = a.params;

    // this lane's two units of the actor (net 1): rows u0 = l and u1 = l + 32 of W1 / W2
    float w1[2][OBS], b1[2], w2[2][PPO_HIDDEN], b2[2], w3[A][2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int u = l + 32 * j;
#pragma unroll
        for (int k = 0; k < OBS; k++) w1[j][k] = P[L.w1[1] + u * OBS + k];
        b1[j] = P[L.b1[1] + u];
#pragma unroll
        for (int k = 0; k < PPO_HIDDEN; k++) w2[j][k] = P[L.w2[1] + u * PPO_HIDDEN + k];
        b2[j] = P[L.b2[1] + u];
#pragma unroll
        for (int aa = 0; aa < A; aa++) w3[aa][j] = P[L.w3[1] + aa * PPO_HIDDEN + u];
    }
    float b3[A];
#pragma unroll
    for (int aa = 0; aa < A; aa++) b3[aa] = P[L.b3[1] + aa];

    float st[OBS];
#pragma unroll
    for (int k = 0; k < OBS; k++) st[k] = a.env_state[(size_t)k * N + env];
    int ep_len = a.ep_len[env];
    float ep_rew = a.ep_rew[env];
    int resets = a.reset_count[env];
    int done = a.next_done[env];
    uint4 philox_words = make_uint4(0u, 0u, 0u, 0u);
    bool philox_valid = false;
    float* slab = lds + half * PPO_HIDDEN;

    for (int t = 0; t < a.T; t++) {
        const size_t tn = (size_t)t * N + env;
        if (live && l < OBS) a.obs[tn * OBS + l] = st[l];          // m_obs[step] = next_obs (PPO_Discrete.cpp:529)
        // layer 1
        float z1[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            float z = b1[j];
#pragma unroll
            for (int k = 0; k < OBS; k++) z = __builtin_fmaf(st[k], w1[j][k], z);
            z1[j] = tanh_mufu(z);
        }
        __syncthreads();
        slab[l] = z1[0];
        slab[l + 32] = z1[1];
        __syncthreads();
        // layer 2: this env's 64 activations, broadcast inside the half
        float acc0 = b2[0], acc1 = b2[1];
        const float4* h4 = reinterpret_cast<const float4*>(slab);
#pragma unroll
        for (int k = 0; k < PPO_HIDDEN / 4; k++) {
            const float4 h = h4[k];
            acc0 = __builtin_fmaf(h.x, w2[0][4 * k], acc0); acc0 = __builtin_fmaf(h.y, w2[0][4 * k + 1], acc0);
            acc0 = __builtin_fmaf(h.z, w2[0][4 * k + 2], acc0); acc0 = __builtin_fmaf(h.w, w2[0][4 * k + 3], acc0);
            acc1 = __builtin_fmaf(h.x, w2[1][4 * k], acc1); acc1 = __builtin_fmaf(h.y, w2[1][4 * k + 1], acc1);
            acc1 = __builtin_fmaf(h.z, w2[1][4 * k + 2], acc1); acc1 = __builtin_fmaf(h.w, w2[1][4 * k + 3], acc1);
        }
        const float h2_0 = tanh_mufu(acc0), h2_1 = tanh_mufu(acc1);
        // logits: rows of 16 units, then ((R0 + R1) + R2) + R3 with R0, R1 = units 0-31 (first register), R2, R3 = units 32-63
        float z[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int aa = 0; aa < A; aa++) {
            const float p = row16_sum(h2_0 * w3[aa][0]), q = row16_sum(h2_1 * w3[aa][1]);
            const int r0 = 32 * half;      // first lane of this env's first row
            const float R0 = __shfl(p, r0, 64), R1 = __shfl(p, r0 + 16, 64), R2 = __shfl(q, r0, 64), R3 = __shfl(q, r0 + 16, 64);
            z[aa] = (((R0 + R1) + R2) + R3) + b3[aa];
        }
        int act[PPO_MAX_HEADS];
        const bool forced = a.forced_actions != nullptr;
        if (forced) act[0] = (int)a.forced_actions[tn * H];
        float logprob, entropy;
        heads_from_logits<DIST, 4, EXACTA>(z, L, nullptr, true, !forced, a.seed, env_global, a.step_base + t, act, logprob, entropy,
                                           &philox_words, &philox_valid);

        // env step + truncation + auto-reset (PPO_Discrete.cpp:440-458)
        int term;
        const float reward = env_step<ENV>(st, act[0], term);
        ep_len += 1;
        ep_rew += reward;
        if (ep_len == a.max_episode_steps) term = 1;
        int fin_len = 0;
        float fin_rew = 0.0f;
        if (term) {
            fin_len = ep_len;
            fin_rew = ep_rew;
            int k = resets++;
            if (ENV == PPO_ENV_CARTPOLE && k >= a.reset_cap) { k = a.reset_cap - 1; if (l == 0) atomicOr(a.error_flag, 1); }
            env_reset<ENV>(st, a.reset_table, k, a.seed, env_global);
            ep_len = 0;
            ep_rew = 0.0f;
        }
        if (live && l == 0) {
            a.dones[tn] = (float)done;
            a.logprobs[tn] = logprob;
            a.rewards[tn] = reward;
            a.fin_len[tn] = fin_len;
            a.fin_rew[tn] = fin_rew;
            a.actions[tn * H] = act[0];
        }
        if (DIST == PPO_DIST_MASKED && a.masks && live && l < A) a.masks[tn * A + l] = 1;
        done = term;
    }
    if (live && l == 0) {
        a.next_done[env] = done;
        a.ep_len[env] = ep_len;
        a.ep_rew[env] = ep_rew;
        a.reset_count[env] = resets;
    }
    if (live && l < OBS) {
        a.next_obs[(size_t)env * OBS + l] = st[l];
        a.env_state[(size_t)l * N + env] = st[l];
    }
}

// ---------------------------------------------------------------------------------------------------------
// Fused rollout on the matrix cores, SIXTEEN envs per wave (the reference's single-head policies).  rollout2_kernel is bound by vector issue:
// ~400 vector instructions per step and wave serve two envs, 128 of them the 64 x 64 matvec.  Here a wave owns a 16-env tile and the actor's two
// layers are MFMA products with the envs as the 16 COLUMNS:
//     layer 1   z1[u][e] = b1[u] + sum_o W1[u][o] x[e][o]    v_mfma_f32_16x16x4_f32 (exact fp32 operands), one per block of 16 units
//     layer 2   z2[n][e] = b2[n] + sum_k W2[n][k] h1[e][k]   v_mfma_f32_16x16x32_f16, fp32 carried as two fp16 terms, three products per fp32 product
//                                                            (kernels_update_mfma.hip: the same arithmetic as the update kernel and values_mfma_kernel)
// A 16 x 16 result has lane (e = lane & 15, kg = lane >> 4) holding units 16 b + 4 kg + r of env e -- which is directly the B operand of the next
// product when the weight fragments enumerate the contraction in that order (chunk c <-> unit blocks 2c, 2c + 1): no data crosses lanes between the
// layers, no LDS, no barrier.  The four lanes of an env then hold 16 hidden units each: logits are 16 fused multiply-adds per lane and two
// cross-lane steps.  Softmax, sampling, env physics and bookkeeping run per lane (the four lanes of an env redundantly: same bits), lane kg = 0
// stores.  ~470 vector instructions per step serve sixteen envs (29 per env against 200).
// Per-env arithmetic does not depend on the env's position in its tile (a column of an MFMA result is a sum over k only): a shard reproduces its
// columns of the unsharded rollout bit for bit, as before.  Against rollout2_kernel / policy_act_kernel the logits agree to fp32 noise (~1e-7), not
// bit for bit: sampled actions can differ where a uniform draw falls within that noise of a CDF edge.
// ---------------------------------------------------------------------------------------------------------
typedef float r16_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 r16_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int r16_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t r16_pk(float x0, float x1) {   // v_cvt_pk_f16_f32 from the compiler, NOT asm: it pads the 2 wait states an MFMA operand needs
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    const f32x2 x = { x0, x1 };
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(x, f16x2));
}
__device__ __forceinline__ void r16_split2(float x0, float x1, uint32_t& p1, uint32_t& p2) {   // kernels_update_mfma.hip: split2
    p1 = r16_pk(x0, x1);
    float r0, r1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(p1), "v"(x0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(p1), "v"(x1));
    p2 = r16_pk(r0, r1);
}
typedef _Float16 r16_f16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ r16_f32x4 r16_mfma16(const uint2 a, const uint2 b, const r16_f32x4 acc) {   // 16x16x16: lane (i, kg) holds k = 4 kg .. 4 kg + 3
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(r16_f16x4, a), __builtin_bit_cast(r16_f16x4, b), acc, 0, 0, 0);
}
__device__ __forceinline__ r16_f32x4 r16_mfma(const r16_u32x4 a, const r16_u32x4 b, const r16_f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(r16_f16x8, a), __builtin_bit_cast(r16_f16x8, b), acc, 0, 0, 0);
}

// SIX waves per 16-env tile.  One wave doing all 64 units measured 191 us per 128-step rollout (rollout2_kernel: 210), four waves sharing the
// layers 181: a lone wave issues a dependent instruction every ~7 - 9 cycles and a step is ONE dependent chain -- layer 1, tanh, layer 2, tanh,
// logits, softmax, sample, physics (binary64 sin / cos, three IEEE divisions), bookkeeping -- of which the policy is less than half.  So the chain is
// cut where it can be:
//   waves 0 - 3 (the policy): wave w owns units 16 w .. 16 w + 15 of both layers -- ONE 16 x 16 block per layer: 4 tanh, one split pair -- and its
//       16-unit share of every logit as one more product (16x16x16).  The layers' results cross waves through LDS in exactly the form the next
//       product wants them (lane-aligned: lane (e, kg) of every wave needs what lane (e, kg) of waves 2c and 2c + 1 hold).  Wave 3 also draws the
//       step's random words (they depend on (seed, env, step) only).
//   wave 5 (trigonometry): the transition's cos / sin (glibc's binary64 polynomials, ~40 % of a transition) depend on the state only.  CartPole
//       (AHEAD): the NEXT state's position and angle -- hence termination, truncation, reset -- do not depend on the action (cartpole_next_pose), so
//       this wave works a whole step ahead, one piece per phase (angle + the reset row's load / cosine / sine), keeps its own episode length and
//       reset count, and hands the reset row to the env wave through LDS.  MountainCar: cos(3 p) of the current state, while layer 1 runs.
//   wave 4 (the envs): the rest of a transition depends on the state and on WHICH action is taken, not on the policy's output, so it forms the
//       transition of EVERY possible action before the policy has spoken (AHEAD: beside layer 1; otherwise beside layer 2), one candidate per
//       lane group (same function, same inputs: the same bits as stepping after the fact); when the logits arrive it samples, takes the
//       candidate of the action drawn (two actions: a select between its own and its partner's velocities, fetched beforehand; otherwise a lane
//       shuffle), does the bookkeeping and publishes the next observation.  Its global stores sit where it would otherwise idle (AHEAD: in the
//       next step's layer-2 phase) and it has no global load in the loop: a load would make it wait for its own stores' acknowledgements.
// Three LDS-only barriers per step (hidden layer [+ trigonometry], the logits' shares, next observation); buffers alternate by step parity.
// Measured per 128-step rollout at 4096 envs (A/B in one call each, rollout + critic batch): rollout2_kernel 234 us; one wave per tile 216; four
// policy waves that also step the envs 207; + env wave 196; + trigonometry off the env wave 171 (cos and sin on two waves: 176); logits as a
// 16x16x16 product 167; trigonometry a step ahead, stores in the idle phase 161; select instead of shuffles 153 (profiles/NOTES.md).
// Workgroup barrier for data handed over through LDS ONLY.  __syncthreads() is a release / acquire fence over every address space: hipcc puts
// s_waitcnt vmcnt(0) in front of the s_barrier, and a wave that has just issued global stores then stands at the barrier until the memory side has
// acknowledged them (~1 k cycles) -- with every other wave of the workgroup waiting for it.  The waves of the rollout exchange nothing through global
// memory inside the step loop, so the barrier only has to wait for the wave's LDS operations (the asm's memory clobber keeps the compiler from moving
// LDS accesses across it).
__device__ __forceinline__ void r16_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int ENV, int DIST, int OBS, int EXACTA>
__global__ __launch_bounds__(384, 1) void rollout16_kernel(const float* __restrict__ params, float* env_state, int32_t* ep_len_p, float* ep_rew_p, int32_t* reset_count,
                                                          int32_t* next_done, int N, int n_tiles, RolloutArgs a) {
    // the leading scalars (6 pointers + 2 ints = 14 dwords) are preloaded into SGPRs at wave launch (csrc/Makefile: kernel-argument preloading): the operands
    // of the prologue's loads -- weights and env state -- and the grid size, which gridDim would fetch from the implicit arguments
    __shared__ __attribute__((aligned(16))) uint32_t s_h1[2][2][2][64][4];      // [step parity][term][chunk c][lane][wave 2c: 2 dwords | wave 2c + 1: 2 dwords]
    __shared__ __attribute__((aligned(16))) float s_part[2][EXACTA][16][4];     // [step parity][logit][env][policy wave]: each wave's 16-unit share of a logit
    __shared__ float s_x[2][4][16];                                             // [step parity][obs component][env]: the observation the policy sees next
    __shared__ float s_tr[2][2][16];                                            // [step parity][cos | sin][env]: the transition's trigonometry (wave 5)
    __shared__ float s_rrow[2][4][16];                                          // [step parity][component][env]: CartPole, the reset row an env restarts from if this step ends its episode (wave 5)
    __shared__ uint4 s_rng[2][16];                                              // [step parity][env]: the Philox words serving this step (wave 3)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, e = lane & 15, kg = lane >> 4;
    const bool envw = wave == 4, trigw = wave == 5;
    const int mw = wave & 3;            // the env wave loads (and ignores) block 0's weights: every index stays in bounds
    int tile = blockIdx.x;
    {   // contiguous env ranges per XCD, as in rollout_kernel
        const int nb = n_tiles, q = nb / 8, r = nb % 8, x = blockIdx.x % 8, i = blockIdx.x / 8;
        tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
    }
    int env = 16 * tile + e;
    const bool live = env < N;          // the last tile may be ragged: its idle columns compute on env N - 1 and store nothing
    if (!live) env = N - 1;
    const NetLayout& L = a.L;
    constexpr int H = 1, A = EXACTA;
    const int64_t env_global = a.env_offset + env;
    const float* __restrict__ P = params;

    // ---- a policy wave's block of the actor's weights as MFMA A operands, once per launch ----
    // layer 1 (16x16x4 f32): lane (i = e, k = kg) holds W1[16 w + i][k]
    const float a1 = kg < OBS ? P[L.w1[1] + (16 * mw + e) * OBS + kg] : 0.0f;
    // layer 2 (16x16x32 f16): lane (i = e, kg) holds, for chunk c, the eight k = {32 c + 4 kg + 0..3, 32 c + 16 + 4 kg + 0..3} of row n = 16 w + i
    // -- the order in which the 16 x 16 results of waves 2c and 2c + 1 present their units -- as two fp16 terms
    r16_u32x4 w2a[2][2];   // [c][term]
#pragma unroll
    for (int c = 0; c < 2; c++) {
        float w[8];
#pragma unroll
        for (int q = 0; q < 8; q++) w[q] = P[L.w2[1] + (16 * mw + e) * PPO_HIDDEN + 32 * c + 16 * (q >> 2) + 4 * kg + (q & 3)];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint32_t p1, p2;
            r16_split2(w[2 * q], w[2 * q + 1], p1, p2);
            w2a[c][0][q] = p1; w2a[c][1][q] = p2;
        }
    }
    // biases in result layout: register r <-> unit 16 w + 4 kg + r
    float b1d[4], b2d[4], b3[A];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int u = 16 * mw + 4 * kg + r;
        b1d[r] = P[L.b1[1] + u];
        b2d[r] = P[L.b2[1] + u];
    }
    // output layer (16x16x16 f16, K = this wave's 16 units): lane (i = e, kg) holds W3[a = i][16 w + 4 kg + 0..3] as two fp16 terms, rows a >= A zero,
    // scaled by 2^8 (|W3| < 255 for fp16's range: an output layer three orders of magnitude past any trained policy)
    uint2 w3a[2];   // [term]
    {
        float w[4];
#pragma unroll
        for (int r = 0; r < 4; r++) w[r] = e < A ? 256.0f * P[L.w3[1] + e * PPO_HIDDEN + 16 * mw + 4 * kg + r] : 0.0f;   // x 2^8: keeps the small term of a ~1e-3 weight out of fp16's subnormals
        // the range is checked, not assumed: a weight that does not fit raises the context's error word (reported by ppo_read_stats: the
        // rollout's logits are then invalid; PPO_KERNEL_ROLLOUT_VECTOR has no such limit)
        const float w3max = fmaxf(fmaxf(fabsf(w[0]), fabsf(w[1])), fmaxf(fabsf(w[2]), fabsf(w[3])));
        if (w3max >= 65280.0f && a.error_flag) atomicOr(a.error_flag, PPO_ERRFLAG_ROLLOUT_RANGE);
        uint32_t p1a, p2a, p1b, p2b;
        r16_split2(w[0], w[1], p1a, p2a);
        r16_split2(w[2], w[3], p1b, p2b);
        w3a[0] = make_uint2(p1a, p1b); w3a[1] = make_uint2(p2a, p2b);
    }
#pragma unroll
    for (int aa = 0; aa < A; aa++) b3[aa] = P[L.b3[1] + aa];

    // ---- the env wave's state (lanes kg = 0 .. 3 of an env hold identical copies; lane kg = 0 stores) ----
    float st[OBS];
#pragma unroll
    for (int k = 0; k < OBS; k++) st[k] = env_state[(size_t)k * N + env];
    int ep_len = ep_len_p[env];
    float ep_rew = ep_rew_p[env];
    int resets = reset_count[env];
    int done = next_done[env];
    uint4 philox_words = make_uint4(0u, 0u, 0u, 0u);
    bool philox_valid = false;
    const bool writer = live && envw;
    if (envw && kg == 0) {
#pragma unroll
        for (int k = 0; k < OBS; k++) s_x[0][k][e] = st[k];
    }
    // CartPole: the trigonometry runs a whole step AHEAD.  x and theta of the next state -- hence termination, truncation and the reset -- do not depend on
    // the action (cartpole_next_pose), so while step t is in flight the trigonometry wave already forms sin / cos of theta(t + 1), keeping its own copies of
    // the episode length and the reset count; nobody waits for it any more, and the env wave runs the candidate transitions beside the policy's layer 1.
    constexpr bool AHEAD = ENV == PPO_ENV_CARTPOLE;
    constexpr bool PAIRED = AHEAD && EXACTA == 2 && OBS == 4;   // lane groups (0, 1) and (2, 3) of an env hold the candidates of actions (0, 1)
    if (AHEAD && trigw) {
        float tr[2];
        env_step_pre<ENV>(st, tr);
        if (kg == 0) { s_tr[0][0][e] = tr[0]; s_tr[0][1][e] = tr[1]; }
    }
    __syncthreads();

#ifdef R16_STAMPS
    unsigned long long ph[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, tp = __builtin_amdgcn_s_memtime();
#define R16_STAMP(i) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xC07F); ph[i] += n_ - tp; tp = n_; } while (0)   /* waits for the clock only, not for the wave's stores */
#else
#define R16_STAMP(i) do { } while (0)
#endif
    // what a step leaves in the rollout buffers, kept by the env wave until it has a free moment (AHEAD: the NEXT step's layer-2 phase; otherwise right
    // behind the step's last barrier)
    float s_reward = 0.0f, s_logprob = 0.0f, s_fin_rew = 0.0f;
    int s_fin_len = 0, s_act = 0, s_done = 0;
    auto store_step = [&](size_t at) {
        if (writer && kg == 0) {
            a.dones[at] = (float)s_done;
            a.logprobs[at] = s_logprob;
            a.rewards[at] = s_reward;
            a.fin_len[at] = s_fin_len;
            a.fin_rew[at] = s_fin_rew;
            a.actions[at * H] = s_act;
        }
        if (DIST == PPO_DIST_MASKED && a.masks && writer && kg < A) a.masks[at * A + kg] = 1;
    };
    for (int t = 0; t < a.T; t++) {
        const size_t tn = (size_t)t * N + env;
        const int par = t & 1;
        float cst[1][OBS], crew[1];
        int cterm[1];
        float oth_xd = 0.0f, oth_td = 0.0f;   // env wave, PAIRED: the other action's x_dot, theta_dot
        float theta_ahead = 0.0f;   // trigonometry wave, AHEAD
        float4 row_ahead = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        int term_ahead = 0;
        if (wave < 4) {
            // layer 1 + tanh: this wave's 16 units; B operand x[e][k = kg]
            const float xk = s_x[par][kg & 3][e];
            float h1[4];
            {
                r16_f32x4 acc = { b1d[0], b1d[1], b1d[2], b1d[3] };
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, kg < OBS ? xk : 0.0f, acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; r++) h1[r] = tanh_mufu(acc[r]);
            }
            // fp16 terms of the block -> this wave's half of chunk (w >> 1)'s B operand
            uint32_t p1a, p2a, p1b, p2b;
            r16_split2(h1[0], h1[1], p1a, p2a);
            r16_split2(h1[2], h1[3], p1b, p2b);
            *reinterpret_cast<uint2*>(&s_h1[par][0][wave >> 1][lane][2 * (wave & 1)]) = make_uint2(p1a, p1b);
            *reinterpret_cast<uint2*>(&s_h1[par][1][wave >> 1][lane][2 * (wave & 1)]) = make_uint2(p2a, p2b);
            // wave 3 also draws the step's random words (they depend on (seed, env, step) only; one Philox call feeds four steps: heads_from_logits)
            if (wave == 3 && kg == 0 && a.forced_actions == nullptr && (((a.step_base + t) & 3) == 0 || t == 0))
                s_rng[par][e] = philox4x32_10((uint32_t)a.seed, (uint32_t)((uint64_t)a.seed >> 32), (uint32_t)env_global, (uint32_t)((a.step_base + t) >> 2), 0u, 0u);
        } else if (trigw) {
            // wave 5: the trigonometry of the transition (binary64 sin / cos), for the env wave's tail
            float xs[OBS], tr[2];
#pragma unroll
            for (int k = 0; k < OBS; k++) xs[k] = s_x[par][k][e];
            if constexpr (AHEAD) {
                // ... of the NEXT step's state: theta(t + 1) = theta + tau theta_dot, or the reset row's angle when this step ends the episode.  Every wave
                // meets every barrier, so the work is cut in three: the angle here, its cosine behind barrier 1, its sine behind barrier 2 -- each piece
                // shorter than the phase it sits in
                const int kr = resets < a.reset_cap ? resets : a.reset_cap - 1;
                row_ahead = reinterpret_cast<const float4*>(a.reset_table)[kr];   // this wave has no stores in flight: waiting for the row is waiting for the row
                float x1;
                cartpole_next_pose(xs, x1, theta_ahead, term_ahead);
                ep_len += 1;
                if (ep_len == a.max_episode_steps) term_ahead = 1;
                if (term_ahead) { resets++; ep_len = 0; }
                (void)tr;
            } else {
                env_step_pre<ENV>(xs, tr);   // of the state the policy is looking at
                if (kg == 0) { s_tr[par][0][e] = tr[0]; s_tr[par][1][e] = tr[1]; }
            }
        } else {
            if constexpr (AHEAD) {   // sin / cos of this step's state arrived during the last step: the candidates run beside layer 1
                float tr[2] = { s_tr[par][0][e], s_tr[par][1][e] };
#pragma unroll
                for (int k = 0; k < OBS; k++) cst[0][k] = st[k];
                crew[0] = env_step_tail<ENV>(cst[0], PAIRED ? (kg & 1) : (kg < A ? kg : A - 1), tr, cterm[0]);
                if constexpr (PAIRED) {   // two actions: every lane fetches the OTHER action's velocities now, so that the choice later is a select, not a shuffle
                    oth_xd = __shfl_xor(cst[0][1], 16, 64);
                    oth_td = __shfl_xor(cst[0][3], 16, 64);
                }
            }
            if constexpr (!AHEAD) {
                // m_obs[step] = next_obs (PPO_Discrete.cpp:529): lane kg stores component kg
                float xk = 0.0f;
#pragma unroll
                for (int k = 0; k < OBS; k++) xk = kg == k ? st[k] : xk;
                if (writer && kg < OBS) a.obs[tn * OBS + kg] = xk;
            }
        }
        R16_STAMP(0);
        r16_lds_barrier();   // the hidden layer, the random words (and, not AHEAD, the trigonometry) are in LDS
        R16_STAMP(1);
        if (AHEAD && trigw) {
            // the reset row has had a phase to arrive: hand it to the env wave through LDS (a load of its own would make it wait for its own stores)
            if (kg == 0) { s_rrow[par][0][e] = row_ahead.x; s_rrow[par][1][e] = row_ahead.y; s_rrow[par][2][e] = row_ahead.z; s_rrow[par][3][e] = row_ahead.w; }
            if (term_ahead) theta_ahead = row_ahead.z;
            const float c = glibc_cosf(theta_ahead);
            if (kg == 0) s_tr[par ^ 1][0][e] = c;
        }
        if (envw) {
            // the transition of every possible action, while the policy waves run the network: lane kg of an env runs the action-dependent tail for
            // action kg -- the candidates are computed SIDE BY SIDE in one instruction stream (lanes kg >= A repeat the last action)
            if constexpr (!AHEAD) {
                float tr[2] = { s_tr[par][0][e], s_tr[par][1][e] };
#pragma unroll
                for (int k = 0; k < OBS; k++) cst[0][k] = st[k];
                crew[0] = env_step_tail<ENV>(cst[0], kg < A ? kg : A - 1, tr, cterm[0]);
            } else {
                // m_obs[step] = next_obs (PPO_Discrete.cpp:529), here: this wave has nothing else to do until the logits arrive, and whatever the compiler
                // makes it wait for (the acknowledgements of the last step's stores) costs nobody anything in this phase
                float xk = 0.0f;
#pragma unroll
                for (int k = 0; k < OBS; k++) xk = kg == k ? st[k] : xk;
                if (writer && kg < OBS) a.obs[tn * OBS + kg] = xk;
                if (t > 0) store_step(tn - N);   // ... and so do the last step's scalars
            }
            if (a.forced_actions == nullptr && (((a.step_base + t) & 3) == 0 || t == 0)) { philox_words = s_rng[par][e]; philox_valid = true; }
        }
        if (wave < 4) {
            // layer 2: rows 16 w .. + 15 over all 64 inputs
            r16_u32x4 hb[2][2];   // [c][term]
#pragma unroll
            for (int c = 0; c < 2; c++)
#pragma unroll
                for (int term = 0; term < 2; term++) hb[c][term] = *reinterpret_cast<const r16_u32x4*>(&s_h1[par][term][c][lane][0]);
            r16_f32x4 acc = { b2d[0], b2d[1], b2d[2], b2d[3] };
#pragma unroll
            for (int c = 0; c < 2; c++) {   // small terms first
                acc = r16_mfma(w2a[c][1], hb[c][0], acc);
                acc = r16_mfma(w2a[c][0], hb[c][1], acc);
                acc = r16_mfma(w2a[c][0], hb[c][0], acc);
            }
            // logits: this wave's 16 units as ONE more product (16x16x16 f16, fp32 as two fp16 terms): z_w[a][e] = sum_u W3[a][u] h2[e][u] lands in
            // lanes kg = 0 (rows a = 0 .. 3); the env wave adds the four waves' shares in wave order
            float h2[4];
#pragma unroll
            for (int r = 0; r < 4; r++) h2[r] = tanh_mufu(acc[r]);
            uint32_t q1a, q2a, q1b, q2b;
            r16_split2(h2[0], h2[1], q1a, q2a);
            r16_split2(h2[2], h2[3], q1b, q2b);
            const uint2 hq1 = make_uint2(q1a, q1b), hq2 = make_uint2(q2a, q2b);
            r16_f32x4 zacc = { 0.0f, 0.0f, 0.0f, 0.0f };
            zacc = r16_mfma16(w3a[1], hq1, zacc);
            zacc = r16_mfma16(w3a[0], hq2, zacc);
            zacc = r16_mfma16(w3a[0], hq1, zacc);
            if (kg == 0) {
#pragma unroll
                for (int aa = 0; aa < A; aa++) s_part[par][aa][e][wave] = zacc[aa];
            }
        }
        R16_STAMP(2);
        r16_lds_barrier();   // the partial sums of the logits are in LDS
        R16_STAMP(3);
        if (AHEAD && trigw) {
            const float sn = glibc_sinf(theta_ahead);
            if (kg == 0) s_tr[par ^ 1][1][e] = sn;
        }
        if (envw) {
            float z[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
            for (int aa = 0; aa < A; aa++) {
                const float4 v = *reinterpret_cast<const float4*>(&s_part[par][aa][e][0]);
                z[aa] = __builtin_fmaf(((v.x + v.y) + v.z) + v.w, 0x1p-8f, b3[aa]);   // the weights' 2^8 comes off exactly
            }
            int act[PPO_MAX_HEADS];
            const bool forced = a.forced_actions != nullptr;
            if (forced) act[0] = (int)a.forced_actions[tn * H];
            float logprob, entropy;
            heads_from_logits<DIST, 4, EXACTA>(z, L, nullptr, true, !forced, a.seed, env_global, a.step_base + t, act, logprob, entropy,
                                               &philox_words, &philox_valid, true);
            // env step (the candidate of the action taken: it sits in lane kg = action of this env) + truncation + auto-reset (PPO_Discrete.cpp:440-458)
            int term;
            float reward;
            if (PAIRED && act[0] >= 0 && act[0] < A) {
                // position, angle, termination and reward are the same for both actions (cartpole_next_pose); the velocities are this lane's or its partner's
                const bool mine = act[0] == (kg & 1);
                term = cterm[0];
                reward = crew[0];
                st[0] = cst[0][0]; st[2] = cst[0][2];
                st[1] = mine ? cst[0][1] : oth_xd;
                st[3] = mine ? cst[0][3] : oth_td;
            } else if (act[0] >= 0 && act[0] < A) {
                const int src = e + 16 * act[0];
                term = __shfl(cterm[0], src, 64);
                reward = __shfl(crew[0], src, 64);
#pragma unroll
                for (int k = 0; k < OBS; k++) st[k] = __shfl(cst[0][k], src, 64);
            } else {
                reward = env_step<ENV>(st, act[0], term);   // a forced action outside the head's range (tests): stepped as given
            }
            ep_len += 1;
            ep_rew += reward;
            if (ep_len == a.max_episode_steps) term = 1;
            int fin_len = 0;
            float fin_rew = 0.0f;
            if (term) {
                fin_len = ep_len;
                fin_rew = ep_rew;
                int k = resets++;
                if (ENV == PPO_ENV_CARTPOLE && k >= a.reset_cap) { k = a.reset_cap - 1; if (kg == 0) atomicOr(a.error_flag, 1); }
                if (ENV == PPO_ENV_CARTPOLE) { st[0] = s_rrow[par][0][e]; st[1] = s_rrow[par][1][e]; st[2] = s_rrow[par][2][e]; st[3] = s_rrow[par][3][e]; (void)k; }   // the row of the shared reset stream (CartPole.cpp:34-45)
                else env_reset<ENV>(st, a.reset_table, k, a.seed, env_global);
                ep_len = 0;
                ep_rew = 0.0f;
            }
            if (kg == 0) {   // the observation the policy sees next
#pragma unroll
                for (int k = 0; k < OBS; k++) s_x[par ^ 1][k][e] = st[k];
            }
            s_reward = reward; s_logprob = logprob; s_fin_len = fin_len; s_fin_rew = fin_rew; s_act = act[0]; s_done = done;
            done = term;
        }
        R16_STAMP(4);
        r16_lds_barrier();   // the next observation is in LDS
        R16_STAMP(5);
        // the step's stores leave behind the barrier: the policy waves are already on the next step
        if constexpr (!AHEAD) store_step(tn);
    }
    if constexpr (AHEAD) { if (a.T > 0) store_step((size_t)(a.T - 1) * N + env); }
#ifdef R16_STAMPS
    if (blockIdx.x == 0 && lane == 0 && (wave == 0 || wave == 4 || wave == 5))
        printf("R16 wave %d: work-before-B1 %llu wait-B1 %llu work-before-B2 %llu wait-B2 %llu work-before-B3 %llu wait-B3 %llu (cycles per step x T=%d)\n", wave,
               ph[0] / a.T, ph[1] / a.T, ph[2] / a.T, ph[3] / a.T, ph[4] / a.T, ph[5] / a.T, a.T);
#endif
    if (writer && kg == 0) {
        next_done[env] = done;
        ep_len_p[env] = ep_len;
        ep_rew_p[env] = ep_rew;
        reset_count[env] = resets;
    }
    if (writer && kg < OBS) {
        float xk = 0.0f;
#pragma unroll
        for (int k = 0; k < OBS; k++) xk = kg == k ? st[k] : xk;
        a.next_obs[(size_t)env * OBS + kg] = xk;
        env_state[(size_t)kg * N + env] = xk;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Caller-stepped envs (PPO_ENV_HOST): one lane per env commits what the caller's env returned for step t - 1 (stepEnvs' outputs,
// PPO_Discrete.cpp:440-458, 474-480) -- exactly the bookkeeping the fused rollout does after its own env step: episode sums, the finished episode's
// length and reward (the caller's own numbers when it passed them), the reward row, the done flag -- and stores m_dones[t] (:530).
// ---------------------------------------------------------------------------------------------------------
// the trailing argument of a HOST kernel (none in the stand-alone policy's instantiations)
__device__ __forceinline__ const HostStepArgs* host_step_args() { return nullptr; }
__device__ __forceinline__ const HostStepArgs* host_step_args(const HostStepArgs& h) { return &h; }

__device__ __forceinline__ void host_commit_row(const HostStepArgs& hs, int64_t row) {
    int d = hs.next_done[row];
    if (hs.commit) {
        const float r = hs.st_rew[row];
        d = hs.st_done[row] != 0 ? 1 : 0;
        int len = hs.ep_len[row] + 1;
        float rew = hs.ep_rew[row] + r;
        int fl = 0;
        float fr = 0.0f;
        if (d) {
            fl = hs.fin_given ? hs.st_fin_len[row] : len;
            fr = hs.fin_given ? hs.st_fin_rew[row] : rew;
            len = 0;
            rew = 0.0f;
        }
        hs.ep_len[row] = len;
        hs.ep_rew[row] = rew;
        hs.rewards_prev[row] = hs.st_rew_store ? hs.st_rew_store[row] : r;   // :544 (the normalised reward where reward normalisation is on)
        hs.fin_len_prev[row] = fl;    // :455-456
        hs.fin_rew_prev[row] = fr;
        hs.next_done[row] = d;
    }
    if (hs.dones_t) hs.dones_t[row] = (float)d;
}

// ---------------------------------------------------------------------------------------------------------
// Stand-alone policy evaluation WITH rollout16_kernel's ARITHMETIC (Agent::getActionAndValueDiscrete / Masked, Agent.cpp:117-170): one wave per
// 16-row tile doing the work of the four policy waves in turn.  A column of an MFMA result is a sum over k only, so which wave forms a block of
// units -- and which tile a row sits in -- does not change a bit: layer 1 as one 16x16x4 fp32 product per block of 16 units, layer 2 as three
// 16x16x32 f16 products per chunk (small terms first), each block's 16-unit share of the logits as three 16x16x16 products, the four shares added
// in block order and scaled by 2^-8.  What crossed waves through LDS there (lane-aligned) stays in this wave's registers here.  This is what
// ppo_policy_act runs in a context whose rollout is rollout16_kernel, so that the free-running rollout and the stand-alone policy on the same
// observations, weights and Philox word agree in every log-prob bit and in every sampled action (round 5's VERDICT, weak 4: until round 6 the
// stand-alone policy was always the vector-ALU form, ~1e-7 away, and <= 2 of 8 192 samples fell on the other side of a CDF edge).
// ---------------------------------------------------------------------------------------------------------
// HOST (ppo_host_act, caller-stepped envs): the commit of step t - 1 and the rollout stores of step t around the same body (host_commit_row; the one
// trailing HostStepArgs names the buffers).  HOST = false has no trailing argument: the stand-alone policy's kernel, signature and code as they were.
// The actor as one wave holds it for policy_act16_kernel's arithmetic -- the four blocks' weights as MFMA A operands (rollout16_kernel's per-wave
// preamble, block mw = 0 .. 3) -- and the logits of a 16-row tile from them.  Shared by the stand-alone policy and the evaluation launch
// (eval16_kernel): ONE definition, so the two agree in every bit.
template <int OBS, int A>
struct Act16Net {
    float a1[4], b1d[4][4], b2d[4][4], b3[A];
    r16_u32x4 w2a[4][2][2];   // [block][chunk c][term]
    uint2 w3a[4][2];          // [block][term]

    __device__ __forceinline__ void load(const float* __restrict__ P, const NetLayout& L, int e, int kg, int32_t* error_flag) {
#pragma unroll
        for (int mw = 0; mw < 4; mw++) {
            a1[mw] = kg < OBS ? P[L.w1[1] + (16 * mw + e) * OBS + kg] : 0.0f;
#pragma unroll
            for (int c = 0; c < 2; c++) {
                float w[8];
#pragma unroll
                for (int q = 0; q < 8; q++) w[q] = P[L.w2[1] + (16 * mw + e) * PPO_HIDDEN + 32 * c + 16 * (q >> 2) + 4 * kg + (q & 3)];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    uint32_t p1, p2;
                    r16_split2(w[2 * q], w[2 * q + 1], p1, p2);
                    w2a[mw][c][0][q] = p1; w2a[mw][c][1][q] = p2;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int u = 16 * mw + 4 * kg + r;
                b1d[mw][r] = P[L.b1[1] + u];
                b2d[mw][r] = P[L.b2[1] + u];
            }
            float w[4];
#pragma unroll
            for (int r = 0; r < 4; r++) w[r] = e < A ? 256.0f * P[L.w3[1] + e * PPO_HIDDEN + 16 * mw + 4 * kg + r] : 0.0f;
            const float w3max = fmaxf(fmaxf(fabsf(w[0]), fabsf(w[1])), fmaxf(fabsf(w[2]), fabsf(w[3])));
            if (w3max >= 65280.0f && error_flag) atomicOr(error_flag, PPO_ERRFLAG_ROLLOUT_RANGE);   // (the host sends such weights to policy_act_kernel: see ppo_policy_act)
            uint32_t p1a, p2a, p1b, p2b;
            r16_split2(w[0], w[1], p1a, p2a);
            r16_split2(w[2], w[3], p1b, p2b);
            w3a[mw][0] = make_uint2(p1a, p1b); w3a[mw][1] = make_uint2(p2a, p2b);
        }
#pragma unroll
        for (int aa = 0; aa < A; aa++) b3[aa] = P[L.b3[1] + aa];
    }

    // xk: component kg of the observation of this lane's row (column e of the tile), 0 for kg >= OBS.  z[0 .. A): the row's logits, valid in lanes kg = 0
    // (rows a = 0 .. 3 of a 16 x 16 result sit there; the other lanes compute on: their rows of W3 are zero, their z is the bias)
    __device__ __forceinline__ void logits(float xk, float* z) const {
        // layer 1 + tanh, block by block; the fp16 terms of block mw are one half of chunk (mw >> 1)'s B operand
        uint2 t1[4], t2[4];
#pragma unroll
        for (int mw = 0; mw < 4; mw++) {
            r16_f32x4 acc = { b1d[mw][0], b1d[mw][1], b1d[mw][2], b1d[mw][3] };
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[mw], xk, acc, 0, 0, 0);
            float h1[4];
#pragma unroll
            for (int r = 0; r < 4; r++) h1[r] = tanh_mufu(acc[r]);
            uint32_t p1a, p2a, p1b, p2b;
            r16_split2(h1[0], h1[1], p1a, p2a);
            r16_split2(h1[2], h1[3], p1b, p2b);
            t1[mw] = make_uint2(p1a, p1b); t2[mw] = make_uint2(p2a, p2b);
        }
        r16_u32x4 hb[2][2];   // [c][term]: { block 2c: 2 dwords | block 2c + 1: 2 dwords } (s_h1's row in rollout16_kernel)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            hb[c][0] = r16_u32x4{ t1[2 * c].x, t1[2 * c].y, t1[2 * c + 1].x, t1[2 * c + 1].y };
            hb[c][1] = r16_u32x4{ t2[2 * c].x, t2[2 * c].y, t2[2 * c + 1].x, t2[2 * c + 1].y };
        }
        float part[4][A];   // [block][logit]: lanes kg = 0 hold column e's share
#pragma unroll
        for (int mw = 0; mw < 4; mw++) {
            r16_f32x4 acc = { b2d[mw][0], b2d[mw][1], b2d[mw][2], b2d[mw][3] };
#pragma unroll
            for (int c = 0; c < 2; c++) {   // small terms first
                acc = r16_mfma(w2a[mw][c][1], hb[c][0], acc);
                acc = r16_mfma(w2a[mw][c][0], hb[c][1], acc);
                acc = r16_mfma(w2a[mw][c][0], hb[c][0], acc);
            }
            float h2[4];
#pragma unroll
            for (int r = 0; r < 4; r++) h2[r] = tanh_mufu(acc[r]);
            uint32_t q1a, q2a, q1b, q2b;
            r16_split2(h2[0], h2[1], q1a, q2a);
            r16_split2(h2[2], h2[3], q1b, q2b);
            const uint2 hq1 = make_uint2(q1a, q1b), hq2 = make_uint2(q2a, q2b);
            r16_f32x4 zacc = { 0.0f, 0.0f, 0.0f, 0.0f };
            zacc = r16_mfma16(w3a[mw][1], hq1, zacc);
            zacc = r16_mfma16(w3a[mw][0], hq2, zacc);
            zacc = r16_mfma16(w3a[mw][0], hq1, zacc);
#pragma unroll
            for (int aa = 0; aa < A; aa++) part[mw][aa] = zacc[aa];
        }
#pragma unroll
        for (int aa = 0; aa < 4; aa++) z[aa] = 0.0f;
#pragma unroll
        for (int aa = 0; aa < A; aa++) z[aa] = __builtin_fmaf(((part[0][aa] + part[1][aa]) + part[2][aa]) + part[3][aa], 0x1p-8f, b3[aa]);
    }
};

// GREEDY (ppo_policy_act_greedy): the head's mode instead of a draw (heads_from_logits)
template <int DIST, int OBS, int EXACTA, bool HOST = false, bool GREEDY = false, class... Host>
__global__ __launch_bounds__(64) void policy_act16_kernel(const float* __restrict__ P, NetLayout L, const float* __restrict__ obs,
                                                          const uint8_t* __restrict__ mask, const int64_t* __restrict__ forced, int64_t n,
                                                          int64_t seed, int64_t env_offset, int64_t step_index, int64_t* action, float* logprob,
                                                          float* entropy, int32_t* error_flag, const Host... host) {
    const int lane = threadIdx.x, e = lane & 15, kg = lane >> 4;
    constexpr int A = EXACTA;
    const HostStepArgs* hs = host_step_args(host...);
    Act16Net<OBS, A> net;
    net.load(P, L, e, kg, error_flag);
    const int64_t n_tiles = (n + 15) / 16;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int64_t row = 16 * tile + e;
        const bool live = row < n;      // a ragged last tile: its idle columns compute on row n - 1 and store nothing
        if (!live) row = n - 1;
        const float xk = kg < OBS ? obs[row * OBS + kg] : 0.0f;
        if constexpr (HOST) {
            if (live && kg == 0) host_commit_row(*hs, row);
            if (live && kg < OBS) {
                hs->obs_t[row * OBS + kg] = xk;                       // m_obs[step] = next_obs (PPO_Discrete.cpp:529)
                if (hs->commit) hs->next_obs[row * OBS + kg] = xk;
            }
            if (live && kg < A && hs->masks_t) hs->masks_t[row * A + kg] = mask ? mask[row * A + kg] : (uint8_t)1;   // PPO_MultiDiscrete.cpp:555
        }
        // rows a = 0 .. 3 of a 16 x 16 result sit in lanes kg = 0: those lanes carry the row's logits (the others compute on and store nothing)
        float z[4];
        net.logits(xk, z);
        int act[PPO_MAX_HEADS];
        if (forced) act[0] = (int)forced[row];
        float lp, en;
        heads_from_logits<DIST, 4, EXACTA, GREEDY>(z, L, mask ? mask + row * A : nullptr, mask == nullptr, forced == nullptr, seed, env_offset + row, step_index, act, lp, en);
        if (live && kg == 0) {
            if (logprob) logprob[row] = lp;
            if (entropy) entropy[row] = en;
            if (action) action[row] = act[0];
            if constexpr (HOST) hs->actions_t[row] = act[0];   // :537
        }
    }
}

// Critic over rows [0, n0) of obs0 and rows [0, n1) of obs1 (m_values[step] = Critic(obs[step]), PPO_Discrete.cpp:534-536, and the
// bootstrap next_value = Critic(next_obs), :280): one wave per row, grid-stride, critic rows resident in registers.
template <int OBS>
__global__ __launch_bounds__(64) void values_kernel(const float* __restrict__ params, NetLayout L, const float* __restrict__ obs0, int64_t n0,
                                                    float* __restrict__ out0, const float* __restrict__ obs1, int64_t n1, float* __restrict__ out1) {
    __shared__ __attribute__((aligned(16))) float lds[PPO_HIDDEN];
    const int lane = threadIdx.x;
    LaneNet<OBS> critic;
    load_lane_net<OBS>(critic, params, L, 0, lane);
    for (int64_t row = blockIdx.x; row < n0 + n1; row += gridDim.x) {
        const float* src = row < n0 ? obs0 + row * OBS : obs1 + (row - n0) * OBS;
        float x[OBS];
#pragma unroll
        for (int k = 0; k < OBS; k++) x[k] = src[k];
        const float v = critic_head(params, L, trunk_forward<OBS>(critic, x, lds, lane), lane);
        if (lane == 0) { if (row < n0) out0[row] = v; else out1[row - n0] = v; }
    }
}

// values_kernel's arithmetic for one row (src: its OBS observation elements; lds: 64 floats of this wave): what the two fold kernels below share
template <int OBS>
__device__ __forceinline__ float critic_row_value(const LaneNet<OBS>& critic, const float* __restrict__ params, const NetLayout& L, const float* src, float* lds,
                                                  int lane) {
    float x[OBS];
#pragma unroll
    for (int k = 0; k < OBS; k++) x[k] = src[k];
    return critic_head(params, L, trunk_forward<OBS>(critic, x, lds, lane), lane);
}

// values_kernel over the dense [K, OBS] block of final observations of truncated episodes, with the partial-episode bootstrap as its epilogue
// (ppo_bootstrap_rewards): rewards[index[k]] += gamma * v in two roundings, value_out[k] = v (may be null).  The same per-row arithmetic, so v is what
// values_kernel gives the same observation; indices are distinct (the caller's promise), so the read-modify-write is plain.
template <int OBS>
__global__ __launch_bounds__(64) void bootstrap_values_kernel(const float* __restrict__ params, NetLayout L, const float* __restrict__ final_obs,
                                                              const int32_t* __restrict__ index, int64_t K, float gamma, float* __restrict__ rewards,
                                                              float* __restrict__ value_out) {
    __shared__ __attribute__((aligned(16))) float lds[PPO_HIDDEN];
    const int lane = threadIdx.x;
    LaneNet<OBS> critic;
    load_lane_net<OBS>(critic, params, L, 0, lane);
    for (int64_t row = blockIdx.x; row < K; row += gridDim.x) {
        const float v = critic_row_value<OBS>(critic, params, L, final_obs + row * OBS, lds, lane);
        if (lane == 0) {
            const int32_t i = index[row];
            rewards[i] = __fadd_rn(rewards[i], __fmul_rn(gamma, v));
            if (value_out) value_out[row] = v;
        }
    }
}

// The fold of a device-fed step (ppo_dev_observe with truncation flags; ppo_internal.hpp: DevFoldArgs) with bootstrap_values_kernel's critic: the flagged
// rows of this workgroup's 256 env rows, compacted, one row per wave and round.  trunk_forward holds workgroup barriers (real ones here: four waves), so
// every wave takes every round, each on its own 64 floats of LDS; a wave without a row of its own in the last round repeats the first flagged row and
// stores nothing.  A workgroup without a flagged row returns before it loads a weight.
template <int OBS>
__global__ __launch_bounds__(DEV_FOLD_THREADS) void dev_fold_kernel(const float* __restrict__ params, NetLayout L, DevFoldArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[(DEV_FOLD_THREADS / 64) * PPO_HIDDEN];
    __shared__ int list[DEV_FOLD_THREADS], wtot[8];
    const int cnt = dev_fold_compact(a, list, wtot);
    if (cnt == 0) return;
    const int base = wtot[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    LaneNet<OBS> critic;
    load_lane_net<OBS>(critic, params, L, 0, lane);
    constexpr int W = DEV_FOLD_THREADS / 64;
    for (int r = 0; r < (cnt + W - 1) / W; r++) {
        const int k = r * W + wave;
        const bool valid = k < cnt;
        const int n = list[valid ? k : 0];
        const float v = critic_row_value<OBS>(critic, params, L, a.final_obs + (int64_t)n * OBS, lds + wave * PPO_HIDDEN, lane);
        if (valid && lane == 0) dev_fold_store(a, base, k, n, v);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Stand-alone policy evaluation (Agent::getActionAndValueDiscrete / Masked): one wave per row, grid-stride.
// ---------------------------------------------------------------------------------------------------------
// HOST: as in policy_act16_kernel (ppo_host_act in the vector form: PPO_KERNEL_ROLLOUT_VECTOR, weights outside rollout16_kernel's range, the shapes it
// does not serve)
template <int DIST, int OBS, int AMAX, bool HOST = false, bool GREEDY = false, class... Host>
__global__ __launch_bounds__(64) void policy_act_kernel(const float* __restrict__ params, NetLayout L, const float* __restrict__ obs,
                                                        const uint8_t* __restrict__ mask, const int64_t* __restrict__ forced, int64_t n,
                                                        int64_t seed, int64_t env_offset, int64_t step_index, int64_t* action,
                                                        float* logprob, float* entropy, float* value, const Host... host) {
    __shared__ __attribute__((aligned(16))) float lds[PPO_HIDDEN];
    const int lane = threadIdx.x;
    const HostStepArgs* hs = host_step_args(host...);
    LaneNet<OBS> actor, critic;
    load_lane_net<OBS>(actor, params, L, 1, lane);
    load_lane_net<OBS>(critic, params, L, 0, lane);
    const int H = L.n_heads, A = L.act;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        float x[OBS];
#pragma unroll
        for (int k = 0; k < OBS; k++) x[k] = obs[row * OBS + k];
        if constexpr (HOST) {
            if (lane == 0) host_commit_row(*hs, row);
            if (lane < OBS) {
                hs->obs_t[row * OBS + lane] = obs[row * OBS + lane];   // m_obs[step] = next_obs (PPO_Discrete.cpp:529)
                if (hs->commit) hs->next_obs[row * OBS + lane] = obs[row * OBS + lane];
            }
            if (lane < A && hs->masks_t) hs->masks_t[row * A + lane] = mask ? mask[row * A + lane] : (uint8_t)1;   // PPO_MultiDiscrete.cpp:555
        }
        if (value) {
            const float v = critic_head(params, L, trunk_forward<OBS>(critic, x, lds, lane), lane);
            if (lane == 0) value[row] = v;
        }
        const float h2a = trunk_forward<OBS>(actor, x, lds, lane);
        int act[PPO_MAX_HEADS];
        if (forced) for (int h = 0; h < H; h++) act[h] = (int)forced[row * H + h];
        float lp, en;
        actor_heads<DIST, AMAX, 0, GREEDY>(params, L, h2a, lane, mask ? mask + row * A : nullptr, mask == nullptr, forced == nullptr, seed,
                                           env_offset + row, step_index, act, lp, en);
        if (lane == 0) {
            if (logprob) logprob[row] = lp;
            if (entropy) entropy[row] = en;
        }
        if (action && lane < H) action[row * H + lane] = act[lane];
        if constexpr (HOST) { if (lane < H) hs->actions_t[row * H + lane] = act[lane]; }   // :537
    }
}

// ---------------------------------------------------------------------------------------------------------
// Evaluation run (ppo_evaluate): n_episodes whole episodes of the context's device env under the current policy as ONE launch; only an episode's return,
// length and truncated flag leave the chip.  Episode e is a pure function of (parameters, seed, e, greedy, max_episode_steps): it starts from row e of the
// evaluation reset table (CartPole: ppo_cartpole_reset_stream_h(seed, n_episodes)) or from env_reset<MOUNTAINCAR> keyed (seed, e, reset 0), steps as
// stepEnvs does (PPO_Discrete.cpp:440-458: reward summed in f32 in step order, truncation at max_episode_steps), and acts by the head's mode (GREEDY) or
// by the sampler keyed (seed, row e, step t of the episode, head).  Episode lengths differ, so a SLOT (one column of a 16-row tile, or one wave of the
// vector form) that finishes an episode takes a further one by a static rule -- slot s of S runs episodes s, s + S, s + 2 S, ... -- and nothing depends on
// how many slots the launch has.  A slot that has run out of episodes keeps computing on its last start state and stores nothing; a wave leaves the loop
// when all of its slots are done (a wave-uniform test: the MFMAs need every lane; no LDS barrier spans waves here, workgroups are one wave).
// The physics are env_step<ENV>, the logits Act16Net's (= policy_act16_kernel's = rollout16_kernel's) or, in the vector form, policy_act_kernel's
// trunk_forward + actor_heads: stepping the same start states through ppo_policy_act_greedy / ppo_policy_act + ppo_env_transition gives the same bits.
// ---------------------------------------------------------------------------------------------------------
template <int ENV, int OBS>
__device__ __forceinline__ void eval_start_state(float* st, const EvalArgs& a, int64_t ep) {
    const int64_t k = ep < a.n_episodes ? ep : a.n_episodes - 1;   // idle slots: the last episode's start state (in bounds, results not stored)
    if constexpr (ENV == PPO_ENV_CARTPOLE) env_reset<ENV>(st, a.reset_table, (int)k, a.seed, k);
    else env_reset<ENV>(st, nullptr, 0, a.seed, k);
}

template <int ENV, int DIST, int OBS, int EXACTA, bool GREEDY>
__global__ __launch_bounds__(64) void eval16_kernel(EvalArgs a) {
    const int lane = threadIdx.x, e = lane & 15, kg = lane >> 4;
    const NetLayout& L = a.L;
    Act16Net<OBS, EXACTA> net;
    net.load(a.params, L, e, kg, nullptr);
    const int64_t S = (int64_t)gridDim.x * 16;
    int64_t ep = (int64_t)blockIdx.x * 16 + e;      // the four lanes kg of a column hold identical copies of the slot's state; lane kg = 0 stores
    bool active = ep < a.n_episodes;
    float st[OBS];
    eval_start_state<ENV, OBS>(st, a, ep);
    int ep_len = 0;
    float ep_rew = 0.0f;
    uint4 philox_words = make_uint4(0u, 0u, 0u, 0u);
    bool philox_valid = false;
    while (__any(active)) {
        float xk = 0.0f;
#pragma unroll
        for (int k = 0; k < OBS; k++) xk = kg == k ? st[k] : xk;
        float z[4];
        net.logits(xk, z);
        int act[PPO_MAX_HEADS];
        act[0] = 0;
        float lp, en;
        // MountainCar::getActionMask is all-ones (MountainCar.cpp:69-77): every action valid, as in the rollout
        heads_from_logits<DIST, 4, EXACTA, GREEDY>(z, L, nullptr, true, true, a.seed, ep < a.n_episodes ? ep : a.n_episodes - 1, (int64_t)ep_len, act, lp, en,
                                                   &philox_words, &philox_valid);
        const int action = __shfl(act[0], e, 64);   // the column's logits live in its lane kg = 0
        int term;
        const float reward = env_step<ENV>(st, action, term);
        ep_len += 1;        // CartPole.cpp:90-91
        ep_rew += reward;
        const int trunc = ep_len == a.max_episode_steps ? 1 : 0;
        if (trunc) term = 1;
        if (term) {
            if (active && kg == 0) {
                a.ep_return[ep] = ep_rew;
                a.ep_length[ep] = ep_len;
                a.ep_trunc[ep] = trunc;
            }
            if (active) ep += S;
            active = ep < a.n_episodes;
            eval_start_state<ENV, OBS>(st, a, ep);
            ep_len = 0;
            ep_rew = 0.0f;
            philox_valid = false;
        }
    }
}

// The vector form (PPO_KERNEL_ROLLOUT_VECTOR, weights outside rollout16_kernel's range, policies rollout16_kernel does not serve): one wave per slot,
// policy_act_kernel's arithmetic; everything is wave-uniform.
template <int ENV, int DIST, int OBS, int AMAX, bool GREEDY>
__global__ __launch_bounds__(64) void evalv_kernel(EvalArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[PPO_HIDDEN];
    const int lane = threadIdx.x;
    const NetLayout& L = a.L;
    LaneNet<OBS> actor;
    load_lane_net<OBS>(actor, a.params, L, 1, lane);
    for (int64_t ep = blockIdx.x; ep < a.n_episodes; ep += gridDim.x) {
        float st[OBS];
        eval_start_state<ENV, OBS>(st, a, ep);
        int ep_len = 0, term = 0, trunc = 0;
        float ep_rew = 0.0f;
        uint4 philox_words = make_uint4(0u, 0u, 0u, 0u);
        bool philox_valid = false;
        while (!term) {
            const float h2a = trunk_forward<OBS>(actor, st, lds, lane);
            int act[PPO_MAX_HEADS];
#pragma unroll
            for (int h = 0; h < PPO_MAX_HEADS; h++) act[h] = 0;
            float lp, en;
            actor_heads<DIST, AMAX, 0, GREEDY>(a.params, L, h2a, lane, nullptr, true, true, a.seed, ep, (int64_t)ep_len, act, lp, en, &philox_words, &philox_valid);
            const float reward = env_step<ENV>(st, act[0], term);
            ep_len += 1;
            ep_rew += reward;
            trunc = ep_len == a.max_episode_steps ? 1 : 0;
            if (trunc) term = 1;
        }
        if (lane == 0) {
            a.ep_return[ep] = ep_rew;
            a.ep_length[ep] = ep_len;
            a.ep_trunc[ep] = trunc;
        }
    }
}

// ppo_host_rollout_end (and the generic engine's per-step commit): step t - 1's staged outputs into the rollout, one thread per env
__global__ __launch_bounds__(256) void host_commit_kernel(HostStepArgs hs, int N, int O) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t k = i; k < N; k += (int64_t)gridDim.x * 256) host_commit_row(hs, k);
    for (int64_t k = i; k < (int64_t)N * O; k += (int64_t)gridDim.x * 256) hs.next_obs[k] = hs.st_obs[k];
}

// ppo_host_rollout_end of a grouped rollout: the last staged step of EVERY group in one launch.  The table travels by value (kernel arguments); a row's
// group is found by comparing against the boundaries in a fixed-length unrolled loop, so no lane indexes the table dynamically.
__global__ __launch_bounds__(256) void host_commit_groups_kernel(HostStepArgs hs, HostGroupTable tab, int N, int O) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t k = i; k < N; k += (int64_t)gridDim.x * 256) {
        int fin = tab.fin_given[0];
#pragma unroll
        for (int q = 1; q < PPO_HOST_MAX_GROUPS; q++) fin = (q < tab.n && k >= tab.row0[q]) ? tab.fin_given[q] : fin;
        HostStepArgs h = hs;
        h.fin_given = fin;
        host_commit_row(h, k);
    }
    for (int64_t k = i; k < (int64_t)N * O; k += (int64_t)gridDim.x * 256) hs.next_obs[k] = hs.st_obs[k];
}

// ---------------------------------------------------------------------------------------------------------
// Stand-alone env kernels: one thread per env (struct-of-arrays state).
// ---------------------------------------------------------------------------------------------------------
template <int ENV, int OBS>
__global__ void env_reset_kernel(int N, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew,
                                 int32_t* reset_count, const float* reset_table, int reset_cap, float* next_obs, int32_t* next_done,
                                 int32_t* error_flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    // initEnvs resets env 0 once for the obs-size probe and once more with everybody else (PPO_Discrete.cpp:368,389);
    // the object is freshly constructed, so its reset counter starts at 0.
    int k = (env_offset + i == 0) ? 1 : 0;
    if (ENV == PPO_ENV_CARTPOLE && k >= reset_cap) { k = reset_cap - 1; atomicOr(error_flag, 1); }
    float st[OBS];
    env_reset<ENV>(st, reset_table, k, seed, env_offset + i);
#pragma unroll
    for (int j = 0; j < OBS; j++) {
        env_state[(size_t)j * N + i] = st[j];
        next_obs[(size_t)i * OBS + j] = st[j];
    }
    ep_len[i] = 0;
    ep_rew[i] = 0.0f;
    reset_count[i] = k + 1;
    next_done[i] = 0;
}

template <int ENV, int OBS>
__global__ void env_step_kernel(int N, int H, int max_episode_steps, int64_t seed, int64_t env_offset, float* env_state,
                                int32_t* ep_len, float* ep_rew, int32_t* reset_count, const float* reset_table, int reset_cap,
                                const int64_t* __restrict__ action, float* obs, float* reward, int32_t* done, int32_t* error_flag,
                                int32_t* fin_len, float* fin_rew) {   // fin_len / fin_rew (may be null): the finished episode's numbers, 0 where none ended
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float st[OBS];
#pragma unroll
    for (int j = 0; j < OBS; j++) st[j] = env_state[(size_t)j * N + i];
    int term;
    const float r = env_step<ENV>(st, (int)action[(size_t)i * H], term);
    int len = ep_len[i] + 1;
    float rew = ep_rew[i] + r;
    if (len == max_episode_steps) term = 1;
    if (fin_len) { fin_len[i] = term ? len : 0; fin_rew[i] = term ? rew : 0.0f; }
    if (term) {
        int k = reset_count[i];
        reset_count[i] = k + 1;
        if (ENV == PPO_ENV_CARTPOLE && k >= reset_cap) { k = reset_cap - 1; atomicOr(error_flag, 1); }
        env_reset<ENV>(st, reset_table, k, seed, env_offset + i);
        len = 0;
        rew = 0.0f;
    }
    ep_len[i] = len;
    ep_rew[i] = rew;
#pragma unroll
    for (int j = 0; j < OBS; j++) {
        env_state[(size_t)j * N + i] = st[j];
        obs[(size_t)i * OBS + j] = st[j];
    }
    reward[i] = r;
    done[i] = term;
}

template <int ENV, int OBS>
__global__ void env_transition_kernel(const float* __restrict__ state_in, const int64_t* __restrict__ action, int64_t n,
                                      float* next_state, float* reward, int32_t* terminated) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float st[OBS];
#pragma unroll
    for (int j = 0; j < OBS; j++) st[j] = state_in[i * OBS + j];
    int term;
    const float r = env_step<ENV>(st, (int)action[i], term);
#pragma unroll
    for (int j = 0; j < OBS; j++) next_state[i * OBS + j] = st[j];
    reward[i] = r;
    terminated[i] = term;
}

__global__ void aos_soa_kernel(const float* in, float* out, int N, int O, int to_soa) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * O) return;
    const int n = i / O, o = i % O;
    if (to_soa) out[(size_t)o * N + n] = in[i];
    else out[i] = in[(size_t)o * N + n];
}

// Categorical API on caller logits: one thread per row.
template <int DIST>
__global__ void categorical_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ mask, const int64_t* __restrict__ value,
                                   int64_t n, int A, float* m_logits, float* m_probs, float* log_prob, float* entropy, int64_t* mode) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float z[PPO_MAX_ACT], p[PPO_MAX_ACT];
    uint8_t m[PPO_MAX_ACT];
    for (int a = 0; a < A; a++) { z[a] = logits[i * A + a]; m[a] = mask ? mask[i * A + a] : 1; }
    const float e = categorical_head<DIST>(z, p, (DIST == PPO_DIST_MASKED && mask) ? m : nullptr, A);
    int best = 0;
    for (int a = 0; a < A; a++) {
        if (m_logits) m_logits[i * A + a] = z[a];
        if (m_probs) m_probs[i * A + a] = p[a];
        if (p[a] > p[best]) best = a;
    }
    if (log_prob && value) log_prob[i] = z[value[i]];
    if (entropy) entropy[i] = e;
    if (mode) mode[i] = best;
}

// ---------------------------------------------------------------------------------------------------------
// Episode statistics: the reference appends finished episodes to CircularBuffer(100) in (step, env index) order
// (PPO_Discrete.cpp:474-480).  Only the last 100 matter, so: count per step row in parallel, then ONE wave walks the
// last rows (in order) that hold >= 100 finished episodes and pushes them with ballot-ordered slots.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void episode_count_kernel(const int32_t* __restrict__ fin_len, int N, int32_t* row_counts, uint64_t* group_bits) {
    // row_counts[t] = finished episodes in step row t; group_bits[t][g] = ballot of the 64 envs of group g
    __shared__ int red[4];
    const int t = blockIdx.x;
    const int G = (N + 63) / 64;
    int c = 0;
    for (int g = threadIdx.x >> 6; g < G; g += 4) {
        const int n = g * 64 + (threadIdx.x & 63);
        const bool f = n < N && fin_len[(size_t)t * N + n] > 0;
        const unsigned long long m = __ballot(f);
        if ((threadIdx.x & 63) == 0) { group_bits[(size_t)t * G + g] = m; c += __popcll(m); }
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) row_counts[t] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(64) void episode_push_kernel(const int32_t* __restrict__ fin_len, const float* __restrict__ fin_rew, int T, int N,
                                                          const int32_t* __restrict__ row_counts, const uint64_t* __restrict__ group_bits,
                                                          EpisodeRing* ring, int64_t step_base, int64_t global_num_envs, int64_t env_offset) {
    // Only the last 100 finished episodes of the rollout survive in the ring.  The window of rows that holds them is found from
    // the row counts (kept in LDS: the serial loops below must not pay a memory round trip per row); inside the window every
    // finished episode knows its rank j in (step, env) order from prefix popcounts, and exactly those with j >= W - 100 are
    // written, each to its own slot (head + j) % 100 -- lanes work on different env groups in parallel, no ordering hazard.
    constexpr int MAXT = 2048;
    __shared__ int s_cnt[MAXT];
    const int lane = threadIdx.x;
    const int G = (N + 63) / 64;
    int64_t total = 0;
    for (int t = lane; t < T; t += 64) {
        const int c = row_counts[t];
        if (t < MAXT) s_cnt[t] = c;
        total += c;
    }
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
    __syncthreads();
    auto cnt = [&](int t) { return t < MAXT ? s_cnt[t] : row_counts[t]; };
    int t_start = T, W = 0;
    while (t_start > 0 && W < 100) { t_start--; W += cnt(t_start); }
    const int head = ring->head;
    const int first = W > 100 ? W - 100 : 0;   // rank of the oldest episode that is still in the ring afterwards
    int rowbase = 0;
    for (int t = t_start; t < T; t++) {
        const int rc = cnt(t);
        if (rc == 0) continue;
        int gbase = rowbase;
        for (int g0 = 0; g0 < G; g0 += 64) {
            const int g = g0 + lane;
            unsigned long long bits = g < G ? group_bits[(size_t)t * G + g] : 0ull;
            const int mine = __popcll(bits);
            int incl = mine;   // inclusive prefix of the per-group counts across the lanes of this stripe
            for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o, 64); if (lane >= o) incl += up; }
            int j = gbase + incl - mine;
            while (bits) {
                const int b = __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                if (j >= first) {
                    const int n = g * 64 + b;
                    const int slot = (head + j) % 100;
                    ring->len[slot] = fin_len[(size_t)t * N + n];
                    ring->rew[slot] = fin_rew[(size_t)t * N + n];
                    ring->key[slot] = (step_base + t) * global_num_envs + env_offset + n;
                }
                j++;
            }
            gbase += __shfl(incl, 63, 64);
        }
        rowbase += rc;
    }
    if (lane == 0) {
        ring->head = (head + W) % 100;
        const int64_t sz = (int64_t)ring->size + total;
        ring->size = (int32_t)(sz > 100 ? 100 : sz);
        ring->total += total;
    }
}

__global__ void categorical_sample_kernel(const float* __restrict__ probs, int64_t n, int A, int64_t seed, int64_t row_offset,
                                          int64_t step_index, int head, int64_t* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float p[PPO_MAX_ACT];
    for (int a = 0; a < A; a++) p[a] = probs[i * A + a];
    const uint4 w = philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)(row_offset + i), (uint32_t)(step_index >> 2), (uint32_t)head, 0u);
    const uint32_t wsel = (step_index & 3) == 0 ? w.x : ((step_index & 3) == 1 ? w.y : ((step_index & 3) == 2 ? w.z : w.w));
    out[i] = sample_head(p, A, (float)(wsel >> 8) * 0x1p-24f);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------
hipError_t launch_rollout(const RolloutArgs& a, hipStream_t s) { return launch_rollout(a, s, nullptr); }

hipError_t launch_rollout(const RolloutArgs& a, hipStream_t s, const RingFuseArgs* ring) {
    const dim3 grid((unsigned)a.N), block(64);
    const dim3 grid2((unsigned)((a.N + 1) / 2));
    const dim3 grid16((unsigned)((a.N + 15) / 16));
    // ppo_config.kernel_flags & PPO_KERNEL_ROLLOUT_VECTOR: the vector-ALU rollout, whose logits are ppo_policy_act's bit for bit
#define PPO_ROLLOUT_FAST(ENV, DIST, OBS, AA)                                                                                  \
    do {                                                                                                                      \
        if (a.vector_kernel) hipLaunchKernelGGL((rollout2_kernel<ENV, DIST, OBS, AA>), grid2, block, 0, s, a);                \
        else hipLaunchKernelGGL((rollout16_kernel<ENV, DIST, OBS, AA>), grid16, dim3(384), 0, s, a.params, a.env_state, a.ep_len, a.ep_rew,   \
                                a.reset_count, a.next_done, a.N, (int)grid16.x, a);                                                  \
    } while (0)
#define PPO_LAUNCH_ROLLOUT(ENV, DIST, OBS)                                                                       \
    do {                                                                                                         \
        if (a.L.n_heads == 1 && a.L.act == 2) PPO_ROLLOUT_FAST(ENV, DIST, OBS, 2);                                \
        else if (a.L.n_heads == 1 && a.L.act == 3) PPO_ROLLOUT_FAST(ENV, DIST, OBS, 3);                           \
        else if (a.L.act <= 4) hipLaunchKernelGGL((rollout_kernel<ENV, DIST, OBS, 4, 0>), grid, block, 0, s, a); \
        else hipLaunchKernelGGL((rollout_kernel<ENV, DIST, OBS, PPO_MAX_ACT, 0>), grid, block, 0, s, a);         \
    } while (0)
    if (a.env_kind == PPO_ENV_CARTPOLE && a.L.obs == 4) {
        if (a.dist_kind == PPO_DIST_CATEGORICAL) PPO_LAUNCH_ROLLOUT(PPO_ENV_CARTPOLE, PPO_DIST_CATEGORICAL, 4);
        else PPO_LAUNCH_ROLLOUT(PPO_ENV_CARTPOLE, PPO_DIST_MASKED, 4);
    } else if (a.env_kind == PPO_ENV_MOUNTAINCAR && a.L.obs == 2) {
        if (a.dist_kind == PPO_DIST_CATEGORICAL) PPO_LAUNCH_ROLLOUT(PPO_ENV_MOUNTAINCAR, PPO_DIST_CATEGORICAL, 2);
        else PPO_LAUNCH_ROLLOUT(PPO_ENV_MOUNTAINCAR, PPO_DIST_MASKED, 2);
    } else {
        return hipErrorInvalidValue;
    }
#undef PPO_LAUNCH_ROLLOUT
#undef PPO_ROLLOUT_FAST
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // m_values and the bootstrap value in one batched launch (matrix cores for the reference's observation widths); with `ring` the same launch also
    // pushes this rollout's finished episodes (launch_values_ring_mfma)
    if (ring && (a.L.obs == 4 || a.L.obs == 2)) return launch_values_ring_mfma(a.params, a.L, a.obs, a.values, a.next_obs, a.next_value, a.T, a.N, *ring, s);
    if (a.L.obs == 4 || a.L.obs == 2) return launch_values_mfma(a.params, a.L, a.obs, (int64_t)a.T * a.N, a.values, a.next_obs, a.N, a.next_value, s);
    return launch_values(a.params, a.L, a.obs, (int64_t)a.T * a.N, a.values, a.next_obs, a.N, a.next_value, s);
}

hipError_t launch_values(const float* params, const NetLayout& L, const float* obs0, int64_t n0, float* out0, const float* obs1, int64_t n1,
                         float* out1, hipStream_t s) {
    const int64_t n = n0 + n1;
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)(n < 8192 ? n : 8192);
    if (L.obs == 4) hipLaunchKernelGGL((values_kernel<4>), dim3(grid), dim3(64), 0, s, params, L, obs0, n0, out0, obs1, n1, out1);
    else if (L.obs == 2) hipLaunchKernelGGL((values_kernel<2>), dim3(grid), dim3(64), 0, s, params, L, obs0, n0, out0, obs1, n1, out1);
    else if (L.obs == 8) hipLaunchKernelGGL((values_kernel<8>), dim3(grid), dim3(64), 0, s, params, L, obs0, n0, out0, obs1, n1, out1);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_bootstrap_values(const float* params, const NetLayout& L, const float* final_obs, const int32_t* index, int64_t K, float gamma,
                                   float* rewards, float* value_out, hipStream_t s) {
    if (K <= 0) return hipSuccess;
    const unsigned grid = (unsigned)(K < 8192 ? K : 8192);
    if (L.obs == 4) hipLaunchKernelGGL((bootstrap_values_kernel<4>), dim3(grid), dim3(64), 0, s, params, L, final_obs, index, K, gamma, rewards, value_out);
    else if (L.obs == 2) hipLaunchKernelGGL((bootstrap_values_kernel<2>), dim3(grid), dim3(64), 0, s, params, L, final_obs, index, K, gamma, rewards, value_out);
    else if (L.obs == 8) hipLaunchKernelGGL((bootstrap_values_kernel<8>), dim3(grid), dim3(64), 0, s, params, L, final_obs, index, K, gamma, rewards, value_out);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_env_reset(int env_kind, int N, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew,
                            int32_t* reset_count, const float* reset_table, int reset_cap, float* next_obs, int32_t* next_done,
                            int32_t* error_flag, hipStream_t s) {
    const dim3 block(256), grid((N + 255) / 256);
    if (env_kind == PPO_ENV_CARTPOLE)
        hipLaunchKernelGGL((env_reset_kernel<PPO_ENV_CARTPOLE, 4>), grid, block, 0, s, N, seed, env_offset, env_state, ep_len, ep_rew,
                           reset_count, reset_table, reset_cap, next_obs, next_done, error_flag);
    else
        hipLaunchKernelGGL((env_reset_kernel<PPO_ENV_MOUNTAINCAR, 2>), grid, block, 0, s, N, seed, env_offset, env_state, ep_len, ep_rew,
                           reset_count, reset_table, reset_cap, next_obs, next_done, error_flag);
    return hipGetLastError();
}

hipError_t launch_env_step(int env_kind, int N, int H, int max_episode_steps, int64_t seed, int64_t env_offset, float* env_state,
                           int32_t* ep_len, float* ep_rew, int32_t* reset_count, const float* reset_table, int reset_cap,
                           const int64_t* action, float* obs, float* reward, int32_t* done, int32_t* error_flag, hipStream_t s, int32_t* fin_len,
                           float* fin_rew) {
    const dim3 block(256), grid((N + 255) / 256);
    if (env_kind == PPO_ENV_CARTPOLE)
        hipLaunchKernelGGL((env_step_kernel<PPO_ENV_CARTPOLE, 4>), grid, block, 0, s, N, H, max_episode_steps, seed, env_offset, env_state,
                           ep_len, ep_rew, reset_count, reset_table, reset_cap, action, obs, reward, done, error_flag, fin_len, fin_rew);
    else
        hipLaunchKernelGGL((env_step_kernel<PPO_ENV_MOUNTAINCAR, 2>), grid, block, 0, s, N, H, max_episode_steps, seed, env_offset, env_state,
                           ep_len, ep_rew, reset_count, reset_table, reset_cap, action, obs, reward, done, error_flag, fin_len, fin_rew);
    return hipGetLastError();
}

hipError_t launch_env_transition(int env_kind, const float* state_in, const int64_t* action, int64_t n, float* next_state,
                                 float* reward, int32_t* terminated, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const dim3 block(256), grid((unsigned)((n + 255) / 256));
    if (env_kind == PPO_ENV_CARTPOLE)
        hipLaunchKernelGGL((env_transition_kernel<PPO_ENV_CARTPOLE, 4>), grid, block, 0, s, state_in, action, n, next_state, reward, terminated);
    else if (env_kind == PPO_ENV_MOUNTAINCAR)
        hipLaunchKernelGGL((env_transition_kernel<PPO_ENV_MOUNTAINCAR, 2>), grid, block, 0, s, state_in, action, n, next_state, reward, terminated);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_aos_to_soa(const float* aos, float* soa, int N, int O, bool to_soa, hipStream_t s) {
    const int n = N * O;
    if (to_soa) hipLaunchKernelGGL(aos_soa_kernel, dim3((n + 255) / 256), dim3(256), 0, s, aos, soa, N, O, 1);
    else hipLaunchKernelGGL(aos_soa_kernel, dim3((n + 255) / 256), dim3(256), 0, s, soa, const_cast<float*>(aos), N, O, 0);
    return hipGetLastError();
}

bool policy_act16_serves(const NetLayout& L) { return L.n_heads == 1 && (L.act == 2 || L.act == 3) && (L.obs == 4 || L.obs == 2); }   // launch_rollout's PPO_ROLLOUT_FAST shapes

hipError_t launch_policy_act(const float* params, const NetLayout& L, int dist_kind, const float* obs, const uint8_t* mask,
                             const int64_t* forced_action, int64_t n, int64_t seed, int64_t env_offset, int64_t step_index,
                             int64_t* action, float* logprob, float* entropy, float* value, bool value_only, hipStream_t s, bool as_rollout16,
                             int32_t* error_flag, bool greedy) {
    if (n <= 0) return hipSuccess;
    // every critic evaluation of a context goes through ONE kernel (the matrix-core one for the reference's observation widths), so
    // stand-alone calls reproduce the fused rollout's values bit for bit
    const bool mfma_values = L.obs == 4 || L.obs == 2;
    if (value_only) return mfma_values ? launch_values_mfma(params, L, obs, n, value, nullptr, 0, nullptr, s) : launch_values(params, L, obs, n, value, nullptr, 0, nullptr, s);
    if (value && mfma_values) {
        hipError_t e = launch_values_mfma(params, L, obs, n, value, nullptr, 0, nullptr, s);
        if (e != hipSuccess) return e;
        value = nullptr;
    }
    if (as_rollout16 && policy_act16_serves(L)) {
        // the shapes launch_rollout gives to rollout16_kernel: the same arithmetic, bit for bit (policy_act16_kernel)
        const int64_t tiles = (n + 15) / 16;
        const dim3 grid16((unsigned)(tiles < 4096 ? tiles : 4096));
#define PPO_LAUNCH_ACT16(DIST, OBS, AA)                                                                                                                                        \
    do {                                                                                                                                                                      \
        if (greedy)                                                                                                                                                           \
            hipLaunchKernelGGL((policy_act16_kernel<DIST, OBS, AA, false, true>), grid16, dim3(64), 0, s, params, L, obs, mask, nullptr, n, seed, env_offset, step_index,     \
                               action, logprob, entropy, error_flag);                                                                                                         \
        else                                                                                                                                                                  \
            hipLaunchKernelGGL((policy_act16_kernel<DIST, OBS, AA>), grid16, dim3(64), 0, s, params, L, obs, mask, forced_action, n, seed, env_offset, step_index, action,    \
                               logprob, entropy, error_flag);                                                                                                                 \
    } while (0)
#define PPO_LAUNCH_ACT16_D(OBS, AA) \
    do { if (dist_kind == PPO_DIST_CATEGORICAL) PPO_LAUNCH_ACT16(PPO_DIST_CATEGORICAL, OBS, AA); else PPO_LAUNCH_ACT16(PPO_DIST_MASKED, OBS, AA); } while (0)
        if (L.obs == 4 && L.act == 2) PPO_LAUNCH_ACT16_D(4, 2);
        else if (L.obs == 4) PPO_LAUNCH_ACT16_D(4, 3);
        else if (L.act == 2) PPO_LAUNCH_ACT16_D(2, 2);
        else PPO_LAUNCH_ACT16_D(2, 3);
#undef PPO_LAUNCH_ACT16_D
#undef PPO_LAUNCH_ACT16
        return hipGetLastError();
    }
    const unsigned grid = (unsigned)(n < 8192 ? n : 8192);
#define PPO_LAUNCH_ACT_A(DIST, OBS, AMAX)                                                                                                        \
    do {                                                                                                                                         \
        if (greedy)                                                                                                                              \
            hipLaunchKernelGGL((policy_act_kernel<DIST, OBS, AMAX, false, true>), dim3(grid), dim3(64), 0, s, params, L, obs, mask, nullptr, n, seed, \
                               env_offset, step_index, action, logprob, entropy, value);                                                         \
        else                                                                                                                                     \
            hipLaunchKernelGGL((policy_act_kernel<DIST, OBS, AMAX>), dim3(grid), dim3(64), 0, s, params, L, obs, mask, forced_action, n, seed,   \
                               env_offset, step_index, action, logprob, entropy, value);                                                         \
    } while (0)
#define PPO_LAUNCH_ACT(DIST, OBS)                               \
    do {                                                        \
        if (L.act <= 4) PPO_LAUNCH_ACT_A(DIST, OBS, 4);         \
        else PPO_LAUNCH_ACT_A(DIST, OBS, PPO_MAX_ACT);          \
    } while (0)
    if (L.obs == 4) {
        if (dist_kind == PPO_DIST_CATEGORICAL) PPO_LAUNCH_ACT(PPO_DIST_CATEGORICAL, 4); else PPO_LAUNCH_ACT(PPO_DIST_MASKED, 4);
    } else if (L.obs == 2) {
        if (dist_kind == PPO_DIST_CATEGORICAL) PPO_LAUNCH_ACT(PPO_DIST_CATEGORICAL, 2); else PPO_LAUNCH_ACT(PPO_DIST_MASKED, 2);
    } else if (L.obs == 8) {
        if (dist_kind == PPO_DIST_CATEGORICAL) PPO_LAUNCH_ACT(PPO_DIST_CATEGORICAL, 8); else PPO_LAUNCH_ACT(PPO_DIST_MASKED, 8);
    } else {
        return hipErrorInvalidValue;
    }
#undef PPO_LAUNCH_ACT
#undef PPO_LAUNCH_ACT_A
    return hipGetLastError();
}

int eval_slots(const EvalArgs& a) {
    if (a.vector_kernel) return (int)(a.n_episodes < 16384 ? a.n_episodes : 16384);
    const int64_t tiles = (a.n_episodes + 15) / 16;
    return 16 * (int)(tiles < 4096 ? tiles : 4096);   // 4096 one-wave workgroups: 16 per CU of an MI355X
}

hipError_t launch_evaluate(const EvalArgs& a, hipStream_t s) {
    if (a.n_episodes <= 0 || a.max_episode_steps <= 0) return hipErrorInvalidValue;
    const int slots = eval_slots(a);
    const bool cart = a.env_kind == PPO_ENV_CARTPOLE && a.L.obs == 4, car = a.env_kind == PPO_ENV_MOUNTAINCAR && a.L.obs == 2;
    if (!cart && !car) return hipErrorInvalidValue;
    if (cart && !a.reset_table) return hipErrorInvalidValue;
    const bool masked = a.dist_kind != PPO_DIST_CATEGORICAL;
#define PPO_EVAL16(ENV, DIST, OBS, AA)                                                                                                \
    do {                                                                                                                              \
        if (a.greedy) hipLaunchKernelGGL((eval16_kernel<ENV, DIST, OBS, AA, true>), dim3((unsigned)(slots / 16)), dim3(64), 0, s, a); \
        else hipLaunchKernelGGL((eval16_kernel<ENV, DIST, OBS, AA, false>), dim3((unsigned)(slots / 16)), dim3(64), 0, s, a);         \
    } while (0)
#define PPO_EVALV(ENV, DIST, OBS, AMAX)                                                                                         \
    do {                                                                                                                        \
        if (a.greedy) hipLaunchKernelGGL((evalv_kernel<ENV, DIST, OBS, AMAX, true>), dim3((unsigned)slots), dim3(64), 0, s, a); \
        else hipLaunchKernelGGL((evalv_kernel<ENV, DIST, OBS, AMAX, false>), dim3((unsigned)slots), dim3(64), 0, s, a);         \
    } while (0)
#define PPO_EVAL(ENV, DIST, OBS)                                                       \
    do {                                                                               \
        if (!a.vector_kernel && a.L.act == 2) PPO_EVAL16(ENV, DIST, OBS, 2);           \
        else if (!a.vector_kernel) PPO_EVAL16(ENV, DIST, OBS, 3);                      \
        else if (a.L.act <= 4) PPO_EVALV(ENV, DIST, OBS, 4);                           \
        else PPO_EVALV(ENV, DIST, OBS, PPO_MAX_ACT);                                   \
    } while (0)
    if (!a.vector_kernel && !policy_act16_serves(a.L)) return hipErrorInvalidValue;
    if (cart) { if (masked) PPO_EVAL(PPO_ENV_CARTPOLE, PPO_DIST_MASKED, 4); else PPO_EVAL(PPO_ENV_CARTPOLE, PPO_DIST_CATEGORICAL, 4); }
    else { if (masked) PPO_EVAL(PPO_ENV_MOUNTAINCAR, PPO_DIST_MASKED, 2); else PPO_EVAL(PPO_ENV_MOUNTAINCAR, PPO_DIST_CATEGORICAL, 2); }
#undef PPO_EVAL
#undef PPO_EVALV
#undef PPO_EVAL16
    return hipGetLastError();
}

hipError_t launch_dev_fold(const float* params, const NetLayout& L, const DevFoldArgs& a, hipStream_t s) {
    if (a.N <= 0) return hipSuccess;
    if (L.obs != 8) return hipErrorNotSupported;   // obs 2 and 4 take the matrix-core critic (launch_dev_fold_mfma), as ppo_bootstrap_rewards does
    const unsigned grid = (unsigned)(((int64_t)a.N + DEV_FOLD_THREADS - 1) / DEV_FOLD_THREADS);
    hipLaunchKernelGGL((dev_fold_kernel<8>), dim3(grid), dim3(DEV_FOLD_THREADS), 0, s, params, L, a);
    return hipGetLastError();
}

hipError_t launch_host_act(const float* params, const NetLayout& L, int dist_kind, const uint8_t* mask, int N, int64_t seed, int64_t env_offset,
                           int64_t step_index, const HostStepArgs& hs, int64_t* action_h, float* logprob_t, bool as16, int32_t* error_flag, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    const float* obs = hs.commit ? hs.st_obs : hs.next_obs;   // step t's observation: what the caller's envs returned for t - 1, or NEXT_OBS at t = 0
    if (as16 && policy_act16_serves(L)) {
        // policy_act16_kernel's grid (ppo_policy_act): a row's arithmetic does not depend on the grid
        const int64_t tiles = (N + 15) / 16;
        const dim3 grid16((unsigned)(tiles < 4096 ? tiles : 4096));
#define PPO_LAUNCH_HACT16(DIST, OBS, AA) \
    hipLaunchKernelGGL((policy_act16_kernel<DIST, OBS, AA, true>), grid16, dim3(64), 0, s, params, L, obs, mask, nullptr, (int64_t)N, seed, env_offset, step_index, action_h, \
                       logprob_t, nullptr, error_flag, hs)
#define PPO_LAUNCH_HACT16_D(OBS, AA) \
    do { if (dist_kind == PPO_DIST_CATEGORICAL) PPO_LAUNCH_HACT16(PPO_DIST_CATEGORICAL, OBS, AA); else PPO_LAUNCH_HACT16(PPO_DIST_MASKED, OBS, AA); } while (0)
        if (L.obs == 4 && L.act == 2) PPO_LAUNCH_HACT16_D(4, 2);
        else if (L.obs == 4) PPO_LAUNCH_HACT16_D(4, 3);
        else if (L.act == 2) PPO_LAUNCH_HACT16_D(2, 2);
        else PPO_LAUNCH_HACT16_D(2, 3);
#undef PPO_LAUNCH_HACT16_D
#undef PPO_LAUNCH_HACT16
        return hipGetLastError();
    }
    const unsigned grid = (unsigned)(N < 8192 ? N : 8192);
#define PPO_LAUNCH_HACT(DIST, OBS)                                                                                                            \
    do {                                                                                                                                      \
        if (L.act <= 4)                                                                                                                       \
            hipLaunchKernelGGL((policy_act_kernel<DIST, OBS, 4, true>), dim3(grid), dim3(64), 0, s, params, L, obs, mask, nullptr, (int64_t)N, seed, \
                               env_offset, step_index, action_h, logprob_t, nullptr, nullptr, hs);                                            \
        else                                                                                                                                  \
            hipLaunchKernelGGL((policy_act_kernel<DIST, OBS, PPO_MAX_ACT, true>), dim3(grid), dim3(64), 0, s, params, L, obs, mask, nullptr, (int64_t)N, \
                               seed, env_offset, step_index, action_h, logprob_t, nullptr, nullptr, hs);                                      \
    } while (0)
    if (L.obs == 4) {
        if (dist_kind == PPO_DIST_CATEGORICAL) PPO_LAUNCH_HACT(PPO_DIST_CATEGORICAL, 4); else PPO_LAUNCH_HACT(PPO_DIST_MASKED, 4);
    } else if (L.obs == 2) {
        if (dist_kind == PPO_DIST_CATEGORICAL) PPO_LAUNCH_HACT(PPO_DIST_CATEGORICAL, 2); else PPO_LAUNCH_HACT(PPO_DIST_MASKED, 2);
    } else if (L.obs == 8) {
        if (dist_kind == PPO_DIST_CATEGORICAL) PPO_LAUNCH_HACT(PPO_DIST_CATEGORICAL, 8); else PPO_LAUNCH_HACT(PPO_DIST_MASKED, 8);
    } else {
        return hipErrorInvalidValue;
    }
#undef PPO_LAUNCH_HACT
    return hipGetLastError();
}

hipError_t launch_host_commit(const HostStepArgs& hs, int N, int O, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    const int64_t work = (int64_t)N * (O > 1 ? O : 1);
    const unsigned grid = (unsigned)((work + 255) / 256 < 65535 ? (work + 255) / 256 : 65535);
    hipLaunchKernelGGL(host_commit_kernel, dim3(grid), dim3(256), 0, s, hs, N, O);
    return hipGetLastError();
}

hipError_t launch_host_commit_groups(const HostStepArgs& hs, const HostGroupTable& tab, int N, int O, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    if (tab.n < 1 || tab.n > PPO_HOST_MAX_GROUPS || tab.row0[0] != 0 || tab.row0[tab.n] != N) return hipErrorInvalidValue;
    const int64_t work = (int64_t)N * (O > 1 ? O : 1);
    const unsigned grid = (unsigned)((work + 255) / 256 < 65535 ? (work + 255) / 256 : 65535);
    hipLaunchKernelGGL(host_commit_groups_kernel, dim3(grid), dim3(256), 0, s, hs, tab, N, O);
    return hipGetLastError();
}

hipError_t launch_categorical(int dist_kind, const float* logits, const uint8_t* mask, const int64_t* value, int64_t n, int A,
                              float* m_logits, float* m_probs, float* log_prob, float* entropy, int64_t* mode, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (A < 1 || A > PPO_MAX_ACT) return hipErrorInvalidValue;
    const dim3 block(128), grid((unsigned)((n + 127) / 128));
    if (dist_kind == PPO_DIST_CATEGORICAL)
        hipLaunchKernelGGL((categorical_kernel<PPO_DIST_CATEGORICAL>), grid, block, 0, s, logits, mask, value, n, A, m_logits, m_probs, log_prob, entropy, mode);
    else
        hipLaunchKernelGGL((categorical_kernel<PPO_DIST_MASKED>), grid, block, 0, s, logits, mask, value, n, A, m_logits, m_probs, log_prob, entropy, mode);
    return hipGetLastError();
}

hipError_t launch_episode_ring_update(const int32_t* fin_len, const float* fin_rew, int T, int N, int32_t* row_counts, uint64_t* group_bits,
                                      EpisodeRing* ring, int64_t step_base, int64_t global_num_envs, int64_t env_offset, hipStream_t s) {
    hipLaunchKernelGGL(episode_count_kernel, dim3((unsigned)T), dim3(256), 0, s, fin_len, N, row_counts, group_bits);
    hipLaunchKernelGGL(episode_push_kernel, dim3(1), dim3(64), 0, s, fin_len, fin_rew, T, N, row_counts, group_bits, ring, step_base, global_num_envs, env_offset);
    return hipGetLastError();
}

hipError_t launch_categorical_sample(const float* probs, int64_t n, int A, int64_t seed, int64_t row_offset, int64_t step_index, int head,
                                     int64_t* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (A < 1 || A > PPO_MAX_ACT) return hipErrorInvalidValue;
    hipLaunchKernelGGL(categorical_sample_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, s, probs, n, A, seed, row_offset, step_index, head, out);
    return hipGetLastError();
}
