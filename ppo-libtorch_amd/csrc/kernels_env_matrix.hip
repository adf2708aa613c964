// ppo-libtorch_amd/csrc/kernels_env_matrix.hip -- PPO_KERNEL_ENV_MATRIX: the one-launch rollouts and evaluations of the seven fused device envs (gauss_rollout_kernel,
// cat_rollout_kernel, gauss_eval_kernel, cat_eval_kernel: kernels_gauss_fused.hip) with the policy's two 64-wide products on the f32 matrix cores
// (v_mfma_f32_16x16x4_f32) and the weights of both products RESIDENT IN REGISTERS for the whole launch.
//
// Why here.  A rollout workgroup owns one 64-env tile for all T steps, so the operands that do not change -- the wave's 16 x 64 slices of W1 and W2 -- are
// fetched once in front of the step loop (gm_fetch_a, one chunk: every device env has obs <= 64; gm_fetch_w2) and stay in 16 + 16 VGPRs per lane.  The vector
// kernels read a 64 x obs W1 image and the 64 x 64 W2 image out of LDS on every step; here LDS holds no W1 at all, and W2's copy is not read by the forward.
// Only the B operands move: the X image [k][sample] that wave 0 writes, and H1.
//
// The lane map is kernels_fused_matrix.hip's: lane = 16 kg + e; wave w owns units 16 w .. 16 w + 15 of all 64 envs in four 16 x 16 accumulator tiles; step t
// of a product uses k = gm_k(t, kg).  A step's arithmetic IS gm_forward_tile's: the accumulators start at the bias, layer 1 runs over NQ = (Env::OBS + 15) >> 4
// quarters of 16 k (compile time: 1 for Pendulum, MountainCarContinuous, Acrobot and FrozenLake 4x4, 2 for Taxi, 3 for Blackjack, 4 for FrozenLake 8x8; the
// quarters behind it are skipped), tanh_fast, layer 2 over four quarters, gf_output_layer for layer 3 -- one function, gm_forward_regs (fused_matrix_dev.hpp),
// which gm_forward_tile also ends in.  So a stepwise loop of ppo_policy_act + ppo_env_step on the same context (gm_gauss_act_kernel / gm_cat_act_kernel)
// reproduces every stored bit, and the critic (gm_values_kernel) and the update (gm_fwd_bwd_kernel<DIST, 1>) see the same forward.  A one-hot env's layer 1 is
// NOT a gather of W1 columns: the instruction's summation order is not one a gather reproduces.
//
// The rest of a step is the vector kernels', text for text: lanes 0 .. 63 of wave 0 own the env (state, episode sums, reset count, previous done flag) in
// registers, form the head with the family's lane functions (gauss_sample / gauss_logp; cat_lane_head on the lane's columns of OUT and H1, the mask bits riding
// in the row-index words), step with Env::step_episode and write the next observation into their column of X (a one-hot env moves its Env::HOT ones).  Waves
// 1 .. 3 store the step's observation, mask and done rows out of LDS meanwhile.
//
// Barriers per rollout step: FIVE, each run by every thread (a short tile masks its stores only).
//   1  in front of layer 1: wave 0's column writes of X and the done / mask words are published (the first step: the staged biases and W3 too);
//   2  behind layer 1: H1 is complete -- layer 2's B operand crosses waves (a wave reads all 64 units of H1, and wrote 16);
//   3  behind layer 2: H2 is complete, for the same reason; H1 is free for the heads' probability columns;
//   4  behind layer 3: OUT is complete -- wave 0's lanes read rows that waves 1 .. 3 wrote;
//   5  behind the heads and the stores: X, OUT, the H1 columns and the done words are read -- wave 0 may write the next step's.
// Barriers 2 .. 4 are gm_forward_regs' own.  An evaluation step has the same five; the fifth also hands the live count to the other waves.
//
// LDS (floats): gm_carve(outP, 1) -- the matrix family's images with ONE X buffer and no W1 image:
//   W2 4096 | W3 64 outP | b1 64 | b2 64 | b3 32 | log_std 32 | exp(-log_std) 32 | row index 64 | X 64 68 | H1 64 68 | H2 64 68 | OUT outP 68
//   outP = 4 (Pendulum, MountainCarContinuous, Acrobot, both FrozenLakes, Blackjack): 17 968 floats = 71 872 bytes; outP = 8 (Taxi): 18 496 floats = 73 984 bytes.
//   Two workgroups per CU (160 KB) on every env: FrozenLake 8x8 had one (88 256 bytes) and Blackjack one (79 808); Pendulum, MountainCarContinuous, Acrobot and
//   FrozenLake 4x4 had two and keep two.  The size does not depend on the observation width.  Rows 0 .. 16 NQ - 1 of X are the ones a product reads; wave 0
//   zeroes its column of them once, the rows behind are never read.
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; __launch_bounds__(256); scratch 0 bytes/lane in every kernel of this file; LDS is all
// dynamic, the sizes above):
//   gm_gauss_rollout_kernel<Pendulum>: 104 VGPRs + 16 AGPRs; <MountainCarContinuous>: 105 + 16
//   gm_cat_rollout_kernel<Acrobot>: 135 + 16; <Taxi, MASKED>: 130 + 16; <Taxi, CATEGORICAL>: 129 + 16; <FrozenLake 4x4>: 109 + 16; <FrozenLake 8x8>: 146 + 16;
//       <Blackjack>: 122 + 16
//   gm_gauss_eval_kernel<MountainCarContinuous>: 101 + 16
//   gm_cat_eval_kernel<Acrobot>: 105 + 16; <Taxi, MASKED>: 102 + 16; <Taxi, CATEGORICAL>: 102 + 16; <FrozenLake 4x4>: 91 + 16; <FrozenLake 8x8>: 108 + 16;
//       <Blackjack>: 108 + 16
//   The 16 AGPRs are the accumulator tiles; the register file allows 3 to 4 waves per SIMD in every kernel, more than the two workgroups LDS admits.  The
//   rollout kernels keep some scalars in VGPR lanes (the compiler's "SGPRs Spill": 2 .. 42, register to register); nothing goes to memory.
#include "fused_matrix_dev.hpp"

namespace {

// the operands that stay in registers for the whole launch: the wave's slices of the actor's W1 (one chunk, zero behind column OBS) and W2
template <int OBS>
__device__ __forceinline__ void gm_env_operands(const GfShape& sh, const float* __restrict__ params, int tid, float (&a1)[16], float (&a2)[16]) {
    static_assert(OBS >= 1 && OBS <= GW_K, "one chunk: every device env's observation is at most 64 wide");
    gm_fetch_a(params + sh.off[1][0], OBS, OBS, 0, 16 * (tid >> 6) + (tid & 15), (tid >> 4) & 3, a1);
    gm_fetch_w2(sh, params, 1, tid, a2);
}

// a step's forward: barrier 1, then gm_forward_tile's arithmetic on the resident operands (barriers 2 .. 4)
template <int NQ>
__device__ __forceinline__ void gm_env_forward(const GfLds& m, const float (&a1)[16], const float (&a2)[16], int out, int tid) {
    __syncthreads();
    gm_f4 acc[4];
    gm_bias(m.b1, __builtin_amdgcn_readfirstlane(tid >> 6), (tid >> 4) & 3, acc);
    gm_forward_regs(m, a1, m.x, NQ, acc, a2, out, tid);
}

// Lane `tid` of wave 0 and its column of the X image.  An env whose observation is dense keeps it in registers and writes it out per step; a one-hot env
// keeps the rows of its ones and moves them (cat_rollout_kernel's rule and its reason).  Rows OBS .. 16 NQ - 1 are the products' zero padding.
template <class Env, bool = Env::OBS_ONE_HOT>
struct GmHotRows { static constexpr int N = 1; };   // a GaussEnv* trait has no HOT
template <class Env>
struct GmHotRows<Env, true> { static constexpr int N = Env::HOT; };
template <class Env>
struct GmEnvColumn {
    static constexpr int OBS = Env::OBS, NQ = (OBS + 15) >> 4;
    static constexpr bool ONE_HOT = Env::OBS_ONE_HOT;
    float ob[ONE_HOT ? 1 : OBS];
    int hot[GmHotRows<Env>::N];

    // once: has = the lane has an env (its state is loaded; otherwise st is the all-zero state, whose rows are inside the image like any other's)
    __device__ __forceinline__ void init(const GfLds& m, const float* st, bool has, int tid) {
        if constexpr (ONE_HOT) {
#pragma unroll
            for (int k = 0; k < 16 * NQ; k++) m.x[k * GF_S + tid] = 0.0f;
            Env::hot(st, hot);
        } else {
#pragma unroll
            for (int k = 0; k < OBS; k++) ob[k] = 0.0f;
            if (has) Env::obs(st, ob);
#pragma unroll
            for (int k = OBS; k < 16 * NQ; k++) m.x[k * GF_S + tid] = 0.0f;
        }
    }
    // per step, in front of barrier 1: the observation of st into the column
    __device__ __forceinline__ void put(const GfLds& m, const float* st, int tid) {
        if constexpr (ONE_HOT) {
#pragma unroll
            for (int k = 0; k < Env::HOT; k++) m.x[hot[k] * GF_S + tid] = 0.0f;   // the previous step's ones (the first step: zeros over zeros)
            Env::hot(st, hot);
#pragma unroll
            for (int k = 0; k < Env::HOT; k++) m.x[hot[k] * GF_S + tid] = 1.0f;
        } else {
#pragma unroll
            for (int k = 0; k < OBS; k++) m.x[k * GF_S + tid] = ob[k];
        }
    }
    // behind the env's step
    __device__ __forceinline__ void stepped(const float* st) {
        if constexpr (!ONE_HOT) Env::obs(st, ob);
    }
    // behind the last step: the observation of st as a row of PPO_BUF_NEXT_OBS
    __device__ __forceinline__ void store(const float* st, float* __restrict__ row) const {
        if constexpr (ONE_HOT) {
            float fo[OBS];
            Env::obs(st, fo);
#pragma unroll
            for (int k = 0; k < OBS; k++) row[k] = fo[k];
        } else {
#pragma unroll
            for (int k = 0; k < OBS; k++) row[k] = ob[k];
        }
    }
};

// waves 1 .. 3: rows 0 .. rows - 1 of the step's observations out of the X image (obs_t: the tile's first row of PPO_BUF_OBS[t])
template <int OBS>
__device__ __forceinline__ void gm_store_obs_rows(const GfLds& m, float* __restrict__ obs_t, int rows, int tid) {
    for (int i = tid - 64; i < rows * OBS; i += GF_THREADS - 64) {
        const int s = i / OBS, k = i - OBS * s;
        obs_t[i] = m.x[k * GF_S + s];
    }
}

// ---------------------------------------------------------------------------------------------------------
// gm_gauss_rollout_kernel<Env> (PPO_ENV_PENDULUM, PPO_ENV_MOUNTAINCAR_CONTINUOUS): gauss_rollout_kernel's step behind the resident matrix forward.
// ---------------------------------------------------------------------------------------------------------
template <class Env>
__global__ __launch_bounds__(GF_THREADS) void gm_gauss_rollout_kernel(GfRolloutArgs a) {
    constexpr int OBS = Env::OBS, ST = Env::STATE, NQ = (OBS + 15) >> 4;
    extern __shared__ __attribute__((aligned(16))) float gm_lds[];
    const int tid = threadIdx.x, N = a.N;
    const GfLds m = gm_carve(gm_lds, 4, 1);
    gf_stage_upper(m, a.sh, a.params, 1, tid);
    float a1[16], a2[16];
    gm_env_operands<OBS>(a.sh, a.params, tid, a1, a2);
    const int row0 = blockIdx.x * 64;
    const int env = row0 + (tid & 63);
    const bool owner = tid < 64 && env < N;
    const int64_t env_global = a.env_offset + env;
    float st[ST], ep_rew = 0.0f;
#pragma unroll
    for (int k = 0; k < ST; k++) st[k] = 0.0f;
    int ep_len = 0, resets = 0, done = 0;
    if (owner) {
#pragma unroll
        for (int k = 0; k < ST; k++) st[k] = a.env_state[(size_t)k * N + env];
        ep_len = a.ep_len[env];
        ep_rew = a.ep_rew[env];
        resets = a.reset_count[env];
        done = a.next_done[env];
    }
    GmEnvColumn<Env> col;
    if (tid < 64) col.init(m, st, owner, tid);
    const int rows = N - row0 < 64 ? N - row0 : 64;
    for (int t = 0; t < a.T; t++) {
        const size_t tn = (size_t)t * N;
        if (tid < 64) {
            col.put(m, st, tid);
            m.ridx[tid] = done;
        }
        gm_env_forward<NQ>(m, a1, a2, 1, tid);
        if (tid < 64) {
            if (owner) {
                const float mu = m.o[tid], ls = m.ls[0];
                float eps[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                if (!a.forced) gauss_eps4(a.seed, env_global, a.step_base + t, 0, eps);
                const float act = a.forced ? a.forced[tn + env] : gauss_sample(mu, ls, eps[0]);
                double lp = 0.0;
                lp += gauss_logp(gauss_z(act, mu, expf(-ls)), ls);
                int fin_len;
                float fin_rew;
                const float r = Env::step_episode(st, act, a.max_episode_steps, a.seed, env_global, ep_len, ep_rew, resets, done, fin_len, fin_rew);
                col.stepped(st);
                a.actions[tn + env] = act;
                a.logprobs[tn + env] = (float)lp;
                a.rewards[tn + env] = r;
                a.fin_len[tn + env] = fin_len;
                a.fin_rew[tn + env] = fin_rew;
            }
        } else {   // waves 1 .. 3: the step's observation rows and done flags, out of LDS
            gm_store_obs_rows<OBS>(m, a.obs + (tn + row0) * OBS, rows, tid);
            if (tid < 128 && env < N) a.dones[tn + env] = (float)m.ridx[tid & 63];
        }
        __syncthreads();   // barrier 5: X, OUT and the done words are read
    }
    if (owner) {
        col.store(st, a.next_obs + (size_t)env * OBS);
        a.next_done[env] = done;
#pragma unroll
        for (int k = 0; k < ST; k++) a.env_state[(size_t)k * N + env] = st[k];
        a.ep_len[env] = ep_len;
        a.ep_rew[env] = ep_rew;
        a.reset_count[env] = resets;
    }
}

// ---------------------------------------------------------------------------------------------------------
// gm_cat_rollout_kernel<Env, DIST> (PPO_ENV_ACROBOT, PPO_ENV_TAXI, the two PPO_ENV_FROZENLAKE kinds, PPO_ENV_BLACKJACK): cat_rollout_kernel's step behind the
// resident matrix forward.  MASKED (Env::HAS_MASK under PPO_DIST_MASKED): the mask bits of the state the action is drawn in ride next to the done flag.
// ---------------------------------------------------------------------------------------------------------
template <class Env, int DIST>
__global__ __launch_bounds__(GF_THREADS) void gm_cat_rollout_kernel(CfRolloutArgs a) {
    constexpr int OBS = Env::OBS, ST = Env::STATE, A = Env::ACTIONS, OUTP = (A + 3) & ~3, NQ = (OBS + 15) >> 4;
    constexpr bool MASKED = Env::HAS_MASK && DIST == PPO_DIST_MASKED;
    static_assert(A <= 8, "the mask bits of a head of at most 8 logits ride in the row-index words");
    static_assert(DIST == PPO_DIST_CATEGORICAL || Env::HAS_MASK, "a masked policy needs an env that forms a mask");
    extern __shared__ __attribute__((aligned(16))) float gm_lds[];
    const int tid = threadIdx.x, N = a.N;
    const GfLds m = gm_carve(gm_lds, OUTP, 1);
    gf_stage_upper(m, a.sh, a.params, 1, tid);
    float a1[16], a2[16];
    gm_env_operands<OBS>(a.sh, a.params, tid, a1, a2);
    const int row0 = blockIdx.x * 64;
    const int env = row0 + (tid & 63);
    const bool owner = tid < 64 && env < N;
    const int64_t env_global = a.env_offset + env;
    float st[ST], ep_rew = 0.0f;
#pragma unroll
    for (int k = 0; k < ST; k++) st[k] = 0.0f;
    int ep_len = 0, resets = 0, done = 0;
    if (owner) {
#pragma unroll
        for (int k = 0; k < ST; k++) st[k] = a.env_state[(size_t)k * N + env];
        ep_len = a.ep_len[env];
        ep_rew = a.ep_rew[env];
        resets = a.reset_count[env];
        done = a.next_done[env];
    }
    GmEnvColumn<Env> col;
    if (tid < 64) col.init(m, st, owner, tid);
    const int rows = N - row0 < 64 ? N - row0 : 64;
    for (int t = 0; t < a.T; t++) {
        const size_t tn = (size_t)t * N;
        uint32_t allowed = 0xffu;
        if (tid < 64) {
            col.put(m, st, tid);
            if constexpr (MASKED) {
                allowed = Env::mask_bits(st);
                m.ridx[tid] = done | (int)(allowed << 1);
            } else {
                m.ridx[tid] = done;
            }
        }
        gm_env_forward<NQ>(m, a1, a2, A, tid);
        if (tid < 64) {
            if (owner) {
                const int64_t step_index = a.step_base + t;
                const uint32_t ws = a.forced ? 0u : cat_draw_word(a.seed, env_global, step_index);
                float lp;
                const int act = cat_lane_head<MASKED ? PPO_DIST_MASKED : PPO_DIST_CATEGORICAL, false>(m, tid, A, allowed, a.forced != nullptr,
                                                                                                      a.forced ? cat_action_int(a.forced[tn + env]) : 0, ws, lp);
                int fin_len;
                float fin_rew;
                const float r = Env::step_episode(st, act, a.max_episode_steps, a.seed, env_global, ep_len, ep_rew, resets, done, fin_len, fin_rew);
                col.stepped(st);
                a.actions[tn + env] = act;
                a.logprobs[tn + env] = lp;
                a.rewards[tn + env] = r;
                a.fin_len[tn + env] = fin_len;
                a.fin_rew[tn + env] = fin_rew;
            }
        } else {   // waves 1 .. 3: the step's observation rows, mask rows and done flags; X and the done words are not touched by wave 0's head work
            gm_store_obs_rows<OBS>(m, a.obs + (tn + row0) * OBS, rows, tid);
            uint8_t* mask_t = a.masks + (tn + row0) * A;
            if constexpr (MASKED) {
                for (int i = tid - 64; i < rows * A; i += GF_THREADS - 64) {
                    const int s = i / A, k = i - A * s;
                    mask_t[i] = (uint8_t)((m.ridx[s] >> (1 + k)) & 1);
                }
                if (tid < 128 && env < N) a.dones[tn + env] = (float)(m.ridx[tid & 63] & 1);
            } else {
                for (int i = tid - 64; i < rows * A; i += GF_THREADS - 64) mask_t[i] = (uint8_t)1;
                if (tid < 128 && env < N) a.dones[tn + env] = (float)m.ridx[tid & 63];
            }
        }
        __syncthreads();   // barrier 5: X, OUT, the H1 columns and the done words are read
    }
    if (owner) {
        col.store(st, a.next_obs + (size_t)env * OBS);
        a.next_done[env] = done;
#pragma unroll
        for (int k = 0; k < ST; k++) a.env_state[(size_t)k * N + env] = st[k];
        a.ep_len[env] = ep_len;
        a.ep_rew[env] = ep_rew;
        a.reset_count[env] = resets;
    }
}

// ---------------------------------------------------------------------------------------------------------
// gm_gauss_eval_kernel<Env> / gm_cat_eval_kernel<Env, DIST> (ppo_evaluate): the episode loops of gauss_eval_kernel and cat_eval_kernel behind the resident
// matrix forward.  A workgroup owns 64 episodes for their whole length; the loop's exit is uniform: wave 0 publishes its live count in the row-index words and
// barrier 5 hands it to the other waves (the next write of the count is behind the next forward's barriers).  At most max_episode_steps steps.
// ---------------------------------------------------------------------------------------------------------
template <class Env>
__global__ __launch_bounds__(GF_THREADS) void gm_gauss_eval_kernel(GfEvalArgs a) {
    constexpr int OBS = Env::OBS, ST = Env::STATE, NQ = (OBS + 15) >> 4;
    static_assert(Env::OBS_IS_STATE, "as gauss_eval_kernel");
    extern __shared__ __attribute__((aligned(16))) float gm_lds[];
    const int tid = threadIdx.x;
    const GfLds m = gm_carve(gm_lds, 4, 1);
    gf_stage_upper(m, a.sh, a.params, 1, tid);
    float a1[16], a2[16];
    gm_env_operands<OBS>(a.sh, a.params, tid, a1, a2);
    const int64_t ep = (int64_t)blockIdx.x * 64 + (tid & 63);
    bool alive = tid < 64 && ep < a.n_episodes;
    const bool owner = alive;
    float st[ST], ep_rew = 0.0f;
#pragma unroll
    for (int k = 0; k < ST; k++) st[k] = 0.0f;
    int ep_len = 0, trunc = 0;
    if (owner) Env::reset(st, 0, a.seed, ep);
    GmEnvColumn<Env> col;
    if (tid < 64) col.init(m, st, owner, tid);
    for (;;) {
        if (tid < 64) col.put(m, st, tid);
        gm_env_forward<NQ>(m, a1, a2, 1, tid);
        if (tid < 64) {
            if (alive) {
                const float mu = m.o[tid], ls = m.ls[0];
                float eps[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                if (!a.greedy) gauss_eps4(a.seed, ep, (int64_t)ep_len, 0, eps);
                const float act = a.greedy ? mu : gauss_sample(mu, ls, eps[0]);
                int term;
                const float r = Env::step(st, act, term);
                ep_len += 1;
                ep_rew += r;
                trunc = ep_len == a.max_episode_steps ? 1 : 0;
                if (term || trunc) alive = false;
                col.stepped(st);
            }
            const unsigned long long live = __ballot(alive);
            if (tid == 0) m.ridx[0] = __popcll(live);
        }
        __syncthreads();   // barrier 5: the live count is published; OUT is read
        if (m.ridx[0] == 0) break;
    }
    if (owner) {
        a.ep_return[ep] = ep_rew;
        a.ep_length[ep] = ep_len;
        a.ep_trunc[ep] = trunc;
    }
}

template <class Env, int DIST>
__global__ __launch_bounds__(GF_THREADS) void gm_cat_eval_kernel(GfEvalArgs a) {
    constexpr int OBS = Env::OBS, ST = Env::STATE, A = Env::ACTIONS, OUTP = (A + 3) & ~3, NQ = (OBS + 15) >> 4;
    constexpr bool MASKED = Env::HAS_MASK && DIST == PPO_DIST_MASKED;
    constexpr int HEAD = MASKED ? PPO_DIST_MASKED : PPO_DIST_CATEGORICAL;
    static_assert(A <= 8, "as gm_cat_rollout_kernel");
    static_assert(DIST == PPO_DIST_CATEGORICAL || Env::HAS_MASK, "a masked policy needs an env that forms a mask");
    extern __shared__ __attribute__((aligned(16))) float gm_lds[];
    const int tid = threadIdx.x;
    const GfLds m = gm_carve(gm_lds, OUTP, 1);
    gf_stage_upper(m, a.sh, a.params, 1, tid);
    float a1[16], a2[16];
    gm_env_operands<OBS>(a.sh, a.params, tid, a1, a2);
    const int64_t ep = (int64_t)blockIdx.x * 64 + (tid & 63);
    bool alive = tid < 64 && ep < a.n_episodes;
    const bool owner = alive;
    float st[ST], ep_rew = 0.0f;
#pragma unroll
    for (int k = 0; k < ST; k++) st[k] = 0.0f;
    int ep_len = 0, trunc = 0;
    if (owner) Env::reset(st, 0, a.seed, ep);
    GmEnvColumn<Env> col;
    if (tid < 64) col.init(m, st, owner, tid);
    for (;;) {
        if (tid < 64) col.put(m, st, tid);
        gm_env_forward<NQ>(m, a1, a2, A, tid);
        if (tid < 64) {
            if (alive) {
                uint32_t allowed = 0xffu;
                if constexpr (MASKED) allowed = Env::mask_bits(st);
                float lp;
                int act;
                if (a.greedy) act = cat_lane_head<HEAD, true>(m, tid, A, allowed, false, 0, 0u, lp);
                else act = cat_lane_head<HEAD, false>(m, tid, A, allowed, false, 0, cat_draw_word(a.seed, ep, (int64_t)ep_len), lp);
                int term;
                const float r = Env::step(st, act, term);
                ep_len += 1;
                ep_rew += r;
                trunc = ep_len == a.max_episode_steps ? 1 : 0;
                if (term || trunc) alive = false;
                col.stepped(st);
            }
            const unsigned long long live = __ballot(alive);
            if (tid == 0) m.ridx[0] = __popcll(live);
        }
        __syncthreads();   // barrier 5: the live count is published; OUT and the H1 columns are read
        if (m.ridx[0] == 0) break;
    }
    if (owner) {
        a.ep_return[ep] = ep_rew;
        a.ep_length[ep] = ep_len;
        a.ep_trunc[ep] = trunc;
    }
}

// every kernel of this file passes 64 KB: the attribute, once per instantiation
template <class K, class Args>
hipError_t gm_env_launch(std::atomic<unsigned long long>& done, K kernel, int outP, int64_t tiles, const Args& a, hipStream_t s) {
    const int bytes = gm_lds_floats(outP, 1) * 4;
    const hipError_t e = gf_allow(done, kernel, bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(GF_THREADS), bytes, s, a);
    return hipGetLastError();
}
template <class Env, int DIST>
hipError_t gm_cat_rollout_launch(const CfRolloutArgs& a, hipStream_t s) {
    static std::atomic<unsigned long long> done{ 0 };
    return gm_env_launch(done, gm_cat_rollout_kernel<Env, DIST>, gf_pad4(Env::ACTIONS), (a.N + 63) / 64, a, s);
}
template <class Env, int DIST>
hipError_t gm_cat_eval_launch(const GfEvalArgs& a, hipStream_t s) {
    static std::atomic<unsigned long long> done{ 0 };
    return gm_env_launch(done, gm_cat_eval_kernel<Env, DIST>, gf_pad4(Env::ACTIONS), (a.n_episodes + 63) / 64, a, s);
}

}  // namespace

// launch_fused_env_rollout's checks are done; r.cut is null (ppo_ctx_create refuses PPO_KERNEL_ENV_CUT_STATE beside the flag)
hipError_t env_matrix_rollout(int env_kind, int dist_kind, const GenLayout& L, const FusedRolloutArgs& r, hipStream_t s) {
    if (!L.env_matrix || r.cut) return hipErrorInvalidValue;
    return fused_env_dispatch(env_kind, [&](auto env) {
        using Env = decltype(env);
        if (!gauss_env_shape_ok<Env>(L)) return hipErrorInvalidValue;
        static std::atomic<unsigned long long> done{ 0 };
        return gm_env_launch(done, gm_gauss_rollout_kernel<Env>, 4, (r.N + 63) / 64, rollout_kernel_args<GfRolloutArgs>(L, r), s);
    }, [&](auto env) {
        using Env = decltype(env);
        if (!cat_env_shape_ok<Env>(L) || !cat_env_dist_ok<Env>(dist_kind)) return hipErrorInvalidValue;
        CfRolloutArgs a = rollout_kernel_args<CfRolloutArgs>(L, r);
        a.masks = r.masks;
        if constexpr (Env::HAS_MASK) {
            if (dist_kind == PPO_DIST_MASKED) return gm_cat_rollout_launch<Env, PPO_DIST_MASKED>(a, s);
        }
        return gm_cat_rollout_launch<Env, PPO_DIST_CATEGORICAL>(a, s);
    });
}

// fused_env_evaluate's checks are done; the Gaussian evaluation exists for the envs whose observation is their state, as without the flag
hipError_t env_matrix_evaluate(int env_kind, int dist_kind, const GenLayout& L, const FusedEvalArgs& e, hipStream_t s) {
    if (!L.env_matrix) return hipErrorInvalidValue;
    return fused_env_dispatch(env_kind, [&](auto env) {
        using Env = decltype(env);
        if constexpr (Env::OBS_IS_STATE) {
            if (!gauss_env_shape_ok<Env>(L)) return hipErrorInvalidValue;
            static std::atomic<unsigned long long> done{ 0 };
            return gm_env_launch(done, gm_gauss_eval_kernel<Env>, 4, (e.n_episodes + 63) / 64, eval_kernel_args(L, e), s);
        } else {
            return hipErrorInvalidValue;
        }
    }, [&](auto env) {
        using Env = decltype(env);
        if (!cat_env_shape_ok<Env>(L) || !cat_env_dist_ok<Env>(dist_kind)) return hipErrorInvalidValue;
        const GfEvalArgs a = eval_kernel_args(L, e);
        if constexpr (Env::HAS_MASK) {
            if (dist_kind == PPO_DIST_MASKED) return gm_cat_eval_launch<Env, PPO_DIST_MASKED>(a, s);
        }
        return gm_cat_eval_launch<Env, PPO_DIST_CATEGORICAL>(a, s);
    });
}
