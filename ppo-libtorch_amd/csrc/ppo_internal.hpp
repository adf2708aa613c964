// ppo-libtorch_amd/csrc/ppo_internal.hpp -- shared host/device definitions of libppo_hip.so (gfx950 only).
//
// Number model of the parity-critical paths (env step, reset mapping, GAE, AdamW element-wise): IEEE binary32 with
// separately rounded operations.  The whole library is compiled with -ffp-contract=off; every fused multiply-add in
// the MLP paths is an explicit __builtin_fmaf.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <cstdio>
#include <string>

#include "ppo_hip.h"

#define PPO_HIDDEN 64          // one hidden unit per lane of a 64-wide wavefront
#define PPO_MAX_OBS 8
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) acts on the CURRENT device's copy of a kernel: a call site remembers, per device ordinal, that it
// has been made (one bit each; `done` is the site's own static).  Thread-safe: the worst a race does is set the attribute twice.
#include <atomic>
inline hipError_t allow_dynamic_lds(std::atomic<unsigned long long>& done, const void* kernel, int bytes = 160 * 1024) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
    return e;
}

#define PPO_MAX_ACT 32         // sum of head widths
#define PPO_TILE 64            // samples per update tile
#define PPO_LDS_STRIDE 68      // padded row stride (floats) of [unit][sample] LDS tiles: 16-B aligned, bank-spreading

// ---------------------------------------------------------------------------------------------------------
// Flat parameter layout = Agent::parameters() order (reference PPO/Agent.cpp:65-66): critic {W1,b1,W2,b2,W3,b3}, actor {..}
// ---------------------------------------------------------------------------------------------------------
struct NetLayout {
    int obs, act, n_heads;
    int head_dims[PPO_MAX_HEADS];
    int w1[2], b1[2], w2[2], b2[2], w3[2], b3[2];  // offsets (floats) per net: 0 = critic, 1 = actor
    int net_off[2], net_size[2];
    int P;
    int n_tensors;
    int tensor_off[13];                             // 12 tensors + end
};

inline NetLayout make_layout(int obs, int n_heads, const int* head_dims) {
    NetLayout L{};
    L.obs = obs;
    L.n_heads = n_heads;
    L.act = 0;
    for (int h = 0; h < n_heads; h++) { L.head_dims[h] = head_dims[h]; L.act += head_dims[h]; }
    int o = 0, t = 0;
    for (int net = 0; net < 2; net++) {
        const int out = net == 0 ? 1 : L.act;
        L.net_off[net] = o;
        L.tensor_off[t++] = o; L.w1[net] = o; o += PPO_HIDDEN * obs;
        L.tensor_off[t++] = o; L.b1[net] = o; o += PPO_HIDDEN;
        L.tensor_off[t++] = o; L.w2[net] = o; o += PPO_HIDDEN * PPO_HIDDEN;
        L.tensor_off[t++] = o; L.b2[net] = o; o += PPO_HIDDEN;
        L.tensor_off[t++] = o; L.w3[net] = o; o += out * PPO_HIDDEN;
        L.tensor_off[t++] = o; L.b3[net] = o; o += out;
        L.net_size[net] = o - L.net_off[net];
    }
    L.tensor_off[t] = o;
    L.n_tensors = t;
    L.P = o;
    return L;
}

// Hyper-parameters as the kernels consume them.
struct LossParams {
    float clip_coef, ent_coef, vf_coef;
    int norm_adv, clip_vloss;
    int dist_kind;
};

// Per-minibatch advantage statistics (sum, sum of squares over the GLOBAL minibatch) and the scalars derived from them.
struct AdvStat { double s1, s2; };
#define PPO_ADV_PARTS 32  // partial sums per minibatch (one workgroup each), added in order by the consumer (A/B on one box, tools/ab.sh: 32 parts 56.7 us per update launch and 161.7 M env-steps/s, 8 parts 57.9 us and 158.5 M)
#define PPO_EV_BLOCKS 512 // partial rows of the explained-variance sums, added in order by the host
// Job-global statistics block of a sharded run (doubles; summed over ranks by the per-update all-reduce, every rank writes only its own slot, so the
// "sum" is a gather): the reference prints ONE table for the job (PPO_Discrete.cpp:474-480, 647-648, 700-774), so every rank must hold the same numbers.
//   [0..3]   explained-variance sums {sum y, sum y^2, sum d, sum d^2} of this rank's shard (added over ranks = the global sums)
//   [4..7]   reserved (zero)
//   rank r:  [8 + r * PPO_GSTAT_RANK + 0] finished episodes so far, [.. + 1] entries in this rank's ring, [.. + 4 + 3 i + {0, 1, 2}] = {key, length, reward}
//            of ring entry i; key = (absolute rollout step) * global_num_envs + global env index = the position of the episode in the reference's
//            push order, so the host rebuilds the job's CircularBuffer(100) exactly: the newest 100 keys of the union.
#define PPO_GSTAT_HEAD 8
#define PPO_GSTAT_RANK (4 + 3 * 100)
#define PPO_GSTAT_DOUBLES (PPO_GSTAT_HEAD + 8 * PPO_GSTAT_RANK)

// Device-side record of one optimizer step's scalars (doubles so the host reads them as-is).
struct StepStats {
    double pg_loss, v_loss, entropy_loss, approx_kl, clipfrac, loss, total_norm, pad;
};

// Host-computed AdamW scalars of one step (LibTorch optim/adamw.cpp narrows its double scalars to float this way).
struct AdamCoef { float decay, neg_step, sqrt_bc2, pad; };

#ifdef __HIPCC__
// ---------------------------------------------------------------------------------------------------------
// Philox4x32-10 (build's own counter-based generator; mirrored bit-for-bit by oracle/ppo_oracle.c:orc_philox4x32)
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// Keyed bijection of [0, 2^bits) (xor / odd multiply / xorshift are each invertible mod 2^bits), cycle-walked into [0, B) by its callers: the update's
// permutations (kernels_update.hip: permutation_kernel, perm_adv_stats_kernel; kernels_update_mfma.hip: pack_perm_stats_kernel).
__device__ __forceinline__ uint32_t mix_bits(uint32_t x, uint32_t mask, int bits, uint4 k) {
    const int sh = bits > 1 ? bits / 2 : 1;
    x ^= k.x & mask; x = (x * 0x9E3779B1u) & mask; x ^= x >> sh;
    x ^= k.y & mask; x = (x * 0x85EBCA77u) & mask; x ^= x >> sh;
    x ^= k.z & mask; x = (x * 0xC2B2AE3Du) & mask; x ^= x >> sh;
    x ^= k.w & mask; x = (x * 0x27D4EB2Fu) & mask; x ^= x >> sh;
    return x;
}

// libstdc++ uniform_real_distribution<float>(a,b) on one 32-bit word (reference Environments/CartPole.cpp:96-100).
__device__ __forceinline__ float canon_to_uniform(uint32_t u, float a, float b) {
    float r = (float)u / 4294967296.0f;
    if (r >= 1.0f) r = 0x1.fffffep-1f;
    return r * (b - a) + a;
}

// ---------------------------------------------------------------------------------------------------------
// glibc 2.35 sinf/cosf (x86-64 FMA ifunc variant), evaluated in binary64 with explicit fma -- what std::sin/std::cos
// on float resolve to in the reference (Environments/CartPole.cpp:59-60, MountainCar.cpp:34).  Valid for |x| < 120;
// the environments stay far inside.  Mirrors oracle/ppo_oracle.c:orc_sinf/orc_cosf, which is pinned exhaustively
// against the host libm.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sc_poly(double x, double x2, int n, bool neg) {
    const double C0 = 0x1p0, C1 = -0x1.ffffffd0c621cp-2, C2 = 0x1.55553e1068f19p-5, C3 = -0x1.6c087e89a359dp-10,
                 C4 = 0x1.99343027bf8c3p-16;
    const double S1 = -0x1.555545995a603p-3, S2 = 0x1.1107605230bc4p-7, S3 = -0x1.994eb3774cf24p-13;
    if ((n & 1) == 0) {
        const double x3 = x * x2;
        const double s1 = __builtin_fma(x2, S3, S2);
        const double x7 = x3 * x2;
        const double s = __builtin_fma(x3, S1, x);
        return (float)__builtin_fma(x7, s1, s);
    } else {
        const double sg = neg ? -1.0 : 1.0;
        const double x4 = x2 * x2;
        const double c2 = __builtin_fma(x2, sg * C4, sg * C3);
        const double c1 = __builtin_fma(x2, sg * C1, sg * C0);
        const double x6 = x4 * x2;
        const double c = __builtin_fma(x4, sg * C2, c1);
        return (float)__builtin_fma(x6, c2, c);
    }
}
__device__ __forceinline__ uint32_t abstop12(float x) { return (__float_as_uint(x) >> 20) & 0x7ffu; }
__device__ __forceinline__ double sc_reduce_fast(double x, int& n) {
    const double r = x * 0x1.45F306DC9C883p+23;
    n = ((int32_t)r + 0x800000) >> 24;
    return __builtin_fma(-(double)n, 0x1.921FB54442D18p0, x);
}
__device__ __forceinline__ float glibc_sinf(float y) {
    double x = y;
    if (abstop12(y) < abstop12(0x1.921FB6p-1f)) {
        if (abstop12(y) < abstop12(0x1p-12f)) return y;
        return sc_poly(x, x * x, 0, false);
    }
    int n;
    x = sc_reduce_fast(x, n);
    const double s = ((n & 3) == 1 || (n & 3) == 2) ? -1.0 : 1.0;
    return sc_poly(x * s, x * x, n, (n & 2) != 0);
}
__device__ __forceinline__ float glibc_cosf(float y) {
    double x = y;
    if (abstop12(y) < abstop12(0x1.921FB6p-1f)) {
        if (abstop12(y) < abstop12(0x1p-12f)) return 1.0f;
        return sc_poly(x, x * x, 1, false);
    }
    int n;
    x = sc_reduce_fast(x, n);
    const int m = (n + 1) & 3;
    const double s = (m == 1 || m == 2) ? -1.0 : 1.0;
    return sc_poly(x * s, x * x, n ^ 1, ((n + 1) & 2) != 0);
}

// ---------------------------------------------------------------------------------------------------------
// Environment transitions
// ---------------------------------------------------------------------------------------------------------
// CartPole::step, reference Environments/CartPole.cpp:47-94 (constants :6-17).  st = {x, x_dot, theta, theta_dot}.
// The part of CartPole::step behind the trigonometry: everything that depends on the action.  cartpole_step = sin / cos of the state + this; the
// fused rollout forms sin / cos ONCE per step and runs the tail for every possible action before the policy has chosen (kernels_rollout.hip).
__device__ __forceinline__ float cartpole_tail(float* st, int action, float cos_theta, float sin_theta, int& terminated) {
    const float gravity = 9.8f, mass_pole = 0.1f, total_mass = 0.1f + 1.0f, length = 0.5f;
    const float polemass_length = 0.1f * 0.5f, force_mag = 10.0f, tau = 0.02f;
    const float theta_thr = 0x1.aceeap-3f; /* (float)(12*2*M_PI/360) = bits 0x3e567750, CartPole.cpp:16 */
    const float x_thr = 2.4f;
    float x = st[0], x_dot = st[1], theta = st[2], theta_dot = st[3];
    float force = force_mag;
    if (action == 0) force = -force;
    const float temp = (force + polemass_length * theta_dot * theta_dot * sin_theta) / total_mass;
    const float theta_acc = (gravity * sin_theta - cos_theta * temp) /
                            (length * (4.0f / 3.0f - mass_pole * cos_theta * cos_theta / total_mass));
    const float x_acc = temp - polemass_length * theta_acc * cos_theta / total_mass;
    x = x + tau * x_dot;
    x_dot = x_dot + tau * x_acc;
    theta = theta + tau * theta_dot;
    theta_dot = theta_dot + tau * theta_acc;
    st[0] = x; st[1] = x_dot; st[2] = theta; st[3] = theta_dot;
    terminated = (x < -x_thr || x > x_thr || theta < -theta_thr || theta > theta_thr) ? 1 : 0;
    return terminated ? -1.0f : 1.0f;
}
// Position and angle of CartPole's next state, and with them the termination test, do NOT depend on the action: the explicit Euler step advances x and theta
// with the OLD velocities (CartPole.cpp:76-80; only x_dot and theta_dot see the force).  Same expressions as cartpole_tail, bit for bit; the fused rollout's
// trigonometry wave uses this to form sin / cos of the NEXT state's angle a whole step ahead (kernels_rollout.hip).
__device__ __forceinline__ void cartpole_next_pose(const float* st, float& x1, float& theta1, int& terminated) {
    const float tau = 0.02f, theta_thr = 0x1.aceeap-3f, x_thr = 2.4f;
    x1 = st[0] + tau * st[1];
    theta1 = st[2] + tau * st[3];
    terminated = (x1 < -x_thr || x1 > x_thr || theta1 < -theta_thr || theta1 > theta_thr) ? 1 : 0;
}
__device__ __forceinline__ float cartpole_step(float* st, int action, int& terminated) {
    const float cos_theta = glibc_cosf(st[2]), sin_theta = glibc_sinf(st[2]);
    return cartpole_tail(st, action, cos_theta, sin_theta, terminated);
}

// MountainCar::step, reference Environments/MountainCar.cpp:29-57 (constants :5-13).  st = {position, velocity}.
__device__ __forceinline__ float mountaincar_tail(float* st, int action, float cos3p, int& terminated) {
    const float min_position = -1.2f, max_position = 0.6f, max_speed = 0.07f, goal_position = 0.5f, goal_velocity = 0.0f;
    const float force = 0.001f, gravity = 0.0025f;
    float position = st[0], velocity = st[1];
    velocity += ((float)action - 1.0f) * force + cos3p * (-gravity);
    velocity = velocity < -max_speed ? -max_speed : (velocity > max_speed ? max_speed : velocity);
    position += velocity;
    position = position < min_position ? min_position : (position > max_position ? max_position : position);
    if (position == min_position && velocity < 0.0f) velocity = 0.0f;
    terminated = (position >= goal_position && velocity >= goal_velocity) ? 1 : 0;
    st[0] = position; st[1] = velocity;
    return -1.0f;
}
__device__ __forceinline__ float mountaincar_step(float* st, int action, int& terminated) {
    return mountaincar_tail(st, action, glibc_cosf(3.0f * st[0]), terminated);
}

// Pendulum-v1 (gymnasium's classic_control/pendulum.py; no reference counterpart: PPO_ENV_PENDULUM).  st = {theta, theta_dot}; a = the RAW action, clipped
// here to the torque range (the rollout keeps the raw sample).  Every operation rounds on its own (-ffp-contract=off), in exactly this association:
//   u      = min(max(a, -2), 2)
//   x      = theta + PI_F;  thn = (x - TWO_PI_F * floorf(x / TWO_PI_F)) - PI_F                    (gym's angle_normalize)
//   reward = -((thn * thn + 0.1f * (theta_dot * theta_dot)) + 0.001f * (u * u))
//   td'    = theta_dot + (15.0f * glibc_sinf(theta) + 3.0f * u) * 0.05f;  td' = min(max(td', -8), 8)    (3 g / (2 l) = 15, 3 / (m l^2) = 3, dt = 0.05)
//   th'    = theta + td' * 0.05f                                                                   (not wrapped, as in gym)
// The env never terminates; an episode ends at the time limit only.  |theta| grows by at most 8 * 0.05 a step, and glibc_sinf / glibc_cosf hold for
// |x| < 120: ppo_ctx_create bounds max_episode_steps accordingly (PENDULUM_MAX_EPISODE_STEPS).
constexpr float PEND_PI_F = 3.14159265358979323846f, PEND_TWO_PI_F = 6.28318530717958647692f;
constexpr int PENDULUM_MAX_EPISODE_STEPS = 290;   // pi + 290 * 0.4 = 119.14 < 120
__device__ __forceinline__ float pendulum_step(float* st, float a) {
    const float theta = st[0], theta_dot = st[1];
    const float u = a < -2.0f ? -2.0f : (a > 2.0f ? 2.0f : a);
    const float x = theta + PEND_PI_F;
    const float thn = (x - PEND_TWO_PI_F * floorf(x / PEND_TWO_PI_F)) - PEND_PI_F;
    const float reward = -((thn * thn + 0.1f * (theta_dot * theta_dot)) + 0.001f * (u * u));
    float td = theta_dot + (15.0f * glibc_sinf(theta) + 3.0f * u) * 0.05f;
    td = td < -8.0f ? -8.0f : (td > 8.0f ? 8.0f : td);
    st[0] = theta + td * 0.05f;
    st[1] = td;
    return reward;
}
// the observation of a state: (cos theta, sin theta, theta_dot)
__device__ __forceinline__ void pendulum_obs(const float* st, float* obs) {
    obs[0] = glibc_cosf(st[0]);
    obs[1] = glibc_sinf(st[0]);
    obs[2] = st[1];
}
// reset number k of global env e: MountainCar's keying, philox(seed; e, k, 0, 1); theta ~ U(-pi, pi) from word x, theta_dot ~ U(-1, 1) from word y
__device__ __forceinline__ void pendulum_reset(float* st, int k, int64_t seed, int64_t env_global) {
    const uint4 w = philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)env_global, (uint32_t)k, 0u, 1u);
    st[0] = canon_to_uniform(w.x, -PEND_PI_F, PEND_PI_F);
    st[1] = canon_to_uniform(w.y, -1.0f, 1.0f);
}
// One step of a Pendulum env with its bookkeeping (env_step_kernel's: episode sums, the time limit, the finished episode's numbers, auto-reset): ONE
// definition for the fused rollout and the stand-alone step.  Returns the reward; done / fin_len / fin_rew are the step's.
__device__ __forceinline__ float pendulum_step_episode(float* st, float a, int max_episode_steps, int64_t seed, int64_t env_global, int& ep_len, float& ep_rew,
                                                       int& resets, int& done, int& fin_len, float& fin_rew) {
    const float r = pendulum_step(st, a);
    ep_len += 1;
    ep_rew += r;
    done = ep_len == max_episode_steps ? 1 : 0;
    fin_len = 0;
    fin_rew = 0.0f;
    if (done) {
        fin_len = ep_len;
        fin_rew = ep_rew;
        pendulum_reset(st, resets++, seed, env_global);
        ep_len = 0;
        ep_rew = 0.0f;
    }
    return r;
}

// MountainCarContinuous-v0 (gymnasium's classic_control/continuous_mountain_car.py; no reference counterpart: PPO_ENV_MOUNTAINCAR_CONTINUOUS).  The discrete
// MountainCar's track with a real-valued force: st = {position, velocity}, and the observation IS the state.  a = the RAW action, clipped here to the force
// range (the rollout keeps the raw sample); the penalty is on the RAW action, as gym's math.pow(action[0], 2).  Every operation rounds on its own
// (-ffp-contract=off), in exactly this association:
//   u  = min(max(a, -1), 1)
//   v' = v + (u * 0.0015f - 0.0025f * glibc_cosf(3.0f * p));   v' = min(max(v', -0.07f), 0.07f)
//   p' = p + v';                                                p' = min(max(p', -1.2f), 0.6f)
//   if (p' == -1.2f && v' < 0) v' = 0
//   terminated = (p' >= 0.45f && v' >= 0.0f);   reward = (terminated ? 100.0f : 0.0f) - 0.1f * (a * a)
// The cosine's argument stays within [-3.6, 1.8].
__device__ __forceinline__ float mcc_step(float* st, float a, int& terminated) {
    const float min_position = -1.2f, max_position = 0.6f, max_speed = 0.07f, goal_position = 0.45f, goal_velocity = 0.0f;
    const float power = 0.0015f, gravity = 0.0025f;
    float position = st[0], velocity = st[1];
    const float u = a < -1.0f ? -1.0f : (a > 1.0f ? 1.0f : a);
    velocity = velocity + (u * power - gravity * glibc_cosf(3.0f * position));
    velocity = velocity < -max_speed ? -max_speed : (velocity > max_speed ? max_speed : velocity);
    position = position + velocity;
    position = position < min_position ? min_position : (position > max_position ? max_position : position);
    if (position == min_position && velocity < 0.0f) velocity = 0.0f;
    terminated = (position >= goal_position && velocity >= goal_velocity) ? 1 : 0;
    st[0] = position; st[1] = velocity;
    return (terminated ? 100.0f : 0.0f) - 0.1f * (a * a);
}
// reset number k of global env e: the discrete MountainCar's own (env_reset below): philox(seed; e, k, 0, 1).x mapped to [-0.6, -0.4), velocity 0
__device__ __forceinline__ void mcc_reset(float* st, int k, int64_t seed, int64_t env_global) {
    const uint4 w = philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)env_global, (uint32_t)k, 0u, 1u);
    st[0] = canon_to_uniform(w.x, -0.6f, -0.4f);
    st[1] = 0.0f;
}
// One step of a continuous MountainCar env with env_step_kernel's bookkeeping (the episode ends where the env terminates or its length reaches the limit):
// ONE definition for the fused rollout and the stand-alone step.  Returns the reward; done / fin_len / fin_rew are the step's.
__device__ __forceinline__ float mcc_step_episode(float* st, float a, int max_episode_steps, int64_t seed, int64_t env_global, int& ep_len, float& ep_rew,
                                                  int& resets, int& done, int& fin_len, float& fin_rew) {
    int term;
    const float r = mcc_step(st, a, term);
    ep_len += 1;
    ep_rew += r;
    done = (term || ep_len == max_episode_steps) ? 1 : 0;
    fin_len = 0;
    fin_rew = 0.0f;
    if (done) {
        fin_len = ep_len;
        fin_rew = ep_rew;
        mcc_reset(st, resets++, seed, env_global);
        ep_len = 0;
        ep_rew = 0.0f;
    }
    return r;
}

// What the fused Gaussian kernels need of a device env with real-valued actions (kernels_gauss_fused.hip: gauss_rollout_kernel, the stand-alone env kernels,
// gauss_trunc_fold_kernel, gauss_eval_kernel): the observation's width, the per-lane state (STATE floats), obs(state), the bare step (the raw action in,
// `terminated` out), the reset and step_episode.  OBS_IS_STATE: the fold and the evaluation's contract -- a stored observation is enough to step from.
struct GaussEnvPendulum {
    static constexpr int OBS = 3, STATE = 2;
    static constexpr bool OBS_IS_STATE = false;
    static constexpr bool OBS_ONE_HOT = false;   // cut_state_fold_kernel asks every trait
    __device__ static __forceinline__ void obs(const float* st, float* ob) { pendulum_obs(st, ob); }
    __device__ static __forceinline__ float step(float* st, float a, int& terminated) { terminated = 0; return pendulum_step(st, a); }
    __device__ static __forceinline__ void reset(float* st, int k, int64_t seed, int64_t env_global) { pendulum_reset(st, k, seed, env_global); }
    __device__ static __forceinline__ float step_episode(float* st, float a, int max_episode_steps, int64_t seed, int64_t env_global, int& ep_len, float& ep_rew,
                                                         int& resets, int& done, int& fin_len, float& fin_rew) {
        return pendulum_step_episode(st, a, max_episode_steps, seed, env_global, ep_len, ep_rew, resets, done, fin_len, fin_rew);
    }
};
struct GaussEnvMountainCarContinuous {
    static constexpr int OBS = 2, STATE = 2;
    static constexpr bool OBS_IS_STATE = true;
    static constexpr bool OBS_ONE_HOT = false;
    __device__ static __forceinline__ void obs(const float* st, float* ob) { ob[0] = st[0]; ob[1] = st[1]; }
    __device__ static __forceinline__ float step(float* st, float a, int& terminated) { return mcc_step(st, a, terminated); }
    __device__ static __forceinline__ void reset(float* st, int k, int64_t seed, int64_t env_global) { mcc_reset(st, k, seed, env_global); }
    __device__ static __forceinline__ float step_episode(float* st, float a, int max_episode_steps, int64_t seed, int64_t env_global, int& ep_len, float& ep_rew,
                                                         int& resets, int& done, int& fin_len, float& fin_rew) {
        return mcc_step_episode(st, a, max_episode_steps, seed, env_global, ep_len, ep_rew, resets, done, fin_len, fin_rew);
    }
};

// Acrobot-v1 (gymnasium's classic_control/acrobot.py, "book" dynamics, no torque noise; no reference counterpart: PPO_ENV_ACROBOT).  st = {th1, th2, w1, w2};
// action a in {0, 1, 2}, tau = (float)a - 1.0f.  Every operation rounds on its own (-ffp-contract=off), in exactly this association (ppo_hip.h repeats it;
// m1 = m2 = l1 = 1, lc1 = lc2 = 0.5, I1 = I2 = 1, g = 9.8, dt = 0.2; 4.9f = m2 lc2 g, 14.7f = (m1 lc1 + m2 l1) g):
//   dsdt:  c2 = cosr(th2);  s2 = sinr(th2)
//          d1   = (0.25f + (1.25f + c2)) + 2.0f
//          d2   = (0.25f + 0.5f * c2) + 1.0f
//          phi2 = 4.9f * cosr((th1 + th2) - HALF_PI_F)
//          phi1 = (((-0.5f * (w2 * w2)) * s2 - (w2 * w1) * s2) + 14.7f * cosr(th1 - HALF_PI_F)) + phi2
//          dw2  = (((tau + (d2 / d1) * phi1) - (0.5f * (w1 * w1)) * s2) - phi2) / (1.25f - (d2 * d2) / d1)
//          dw1  = -(d2 * dw2 + phi1) / d1
//          dsdt = (w1, w2, dw1, dw2)
//   RK4:   k1 = dsdt(s), k2 = dsdt(s + 0.1f * k1), k3 = dsdt(s + 0.1f * k2), k4 = dsdt(s + 0.2f * k3);  s' = s + DT6 * (((k1 + 2.0f * k2) + 2.0f * k3) + k4)
//   wrap th1', th2' into [-PI_F, PI_F] by gym's loops of -+ TWO_PI_F (capped at 1024 turns each: a non-finite input cannot hang a wave);
//   clip w1' to -+ (float)(4 pi), w2' to -+ (float)(9 pi);  terminated = ((-cosr(th1')) - cosr(th2' + th1') > 1.0f);  reward = terminated ? 0 : -1
// cosr / sinr: glibc_cosf / glibc_sinf hold for |x| < 120, and the RK4 stage angles leave that range in the corners of the state box (stage velocities of
// ~2000 rad/s): an argument of 64 or more is first reduced in binary64, x - TWO_PI_D * rint(x / TWO_PI_D), each operation rounded on its own, and rounded
// to f32.  1.25 - d2^2 / d1 >= 0.56 for every c2 in [-1, 1], so a finite state gives a finite step.
constexpr float ACRO_PI_F = 3.14159265358979323846f, ACRO_TWO_PI_F = 6.28318530717958647692f, ACRO_HALF_PI_F = 1.57079632679489661923f;
constexpr float ACRO_MAX_W1 = 12.566370614359172f, ACRO_MAX_W2 = 28.274333882308138f, ACRO_DT6 = (float)(0.2 / 6.0);
constexpr double ACRO_TWO_PI_D = 6.283185307179586476925;
__device__ __forceinline__ float acro_reduce(float x) {
    const double xd = (double)x;
    const double q = rint(xd / ACRO_TWO_PI_D);
    const double p = ACRO_TWO_PI_D * q;
    return (float)(xd - p);
}
__device__ __forceinline__ float acro_sinr(float x) { return glibc_sinf(fabsf(x) < 64.0f ? x : acro_reduce(x)); }
__device__ __forceinline__ float acro_cosr(float x) { return glibc_cosf(fabsf(x) < 64.0f ? x : acro_reduce(x)); }
__device__ __forceinline__ void acrobot_dsdt(const float* s, float tau, float* k) {
    const float th1 = s[0], th2 = s[1], w1 = s[2], w2 = s[3];
    const float c2 = acro_cosr(th2), s2 = acro_sinr(th2);
    const float d1 = (0.25f + (1.25f + c2)) + 2.0f;
    const float d2 = (0.25f + 0.5f * c2) + 1.0f;
    const float phi2 = 4.9f * acro_cosr((th1 + th2) - ACRO_HALF_PI_F);
    const float phi1 = (((-0.5f * (w2 * w2)) * s2 - (w2 * w1) * s2) + 14.7f * acro_cosr(th1 - ACRO_HALF_PI_F)) + phi2;
    const float dw2 = (((tau + (d2 / d1) * phi1) - (0.5f * (w1 * w1)) * s2) - phi2) / (1.25f - (d2 * d2) / d1);
    const float dw1 = -(d2 * dw2 + phi1) / d1;
    k[0] = w1; k[1] = w2; k[2] = dw1; k[3] = dw2;
}
__device__ __forceinline__ float acro_wrap(float x) {
    for (int i = 0; i < 1024 && x > ACRO_PI_F; i++) x -= ACRO_TWO_PI_F;
    for (int i = 0; i < 1024 && x < -ACRO_PI_F; i++) x += ACRO_TWO_PI_F;
    return x;
}
__device__ __forceinline__ float acrobot_step(float* st, int action, int& terminated) {
    const float tau = (float)action - 1.0f;
    float k1[4], k2[4], k3[4], k4[4], y[4];
    acrobot_dsdt(st, tau, k1);
#pragma unroll
    for (int i = 0; i < 4; i++) y[i] = st[i] + 0.1f * k1[i];
    acrobot_dsdt(y, tau, k2);
#pragma unroll
    for (int i = 0; i < 4; i++) y[i] = st[i] + 0.1f * k2[i];
    acrobot_dsdt(y, tau, k3);
#pragma unroll
    for (int i = 0; i < 4; i++) y[i] = st[i] + 0.2f * k3[i];
    acrobot_dsdt(y, tau, k4);
#pragma unroll
    for (int i = 0; i < 4; i++) y[i] = st[i] + ACRO_DT6 * (((k1[i] + 2.0f * k2[i]) + 2.0f * k3[i]) + k4[i]);
    const float th1 = acro_wrap(y[0]), th2 = acro_wrap(y[1]);
    const float w1 = y[2] < -ACRO_MAX_W1 ? -ACRO_MAX_W1 : (y[2] > ACRO_MAX_W1 ? ACRO_MAX_W1 : y[2]);
    const float w2 = y[3] < -ACRO_MAX_W2 ? -ACRO_MAX_W2 : (y[3] > ACRO_MAX_W2 ? ACRO_MAX_W2 : y[3]);
    st[0] = th1; st[1] = th2; st[2] = w1; st[3] = w2;
    terminated = ((-acro_cosr(th1)) - acro_cosr(th2 + th1) > 1.0f) ? 1 : 0;
    return terminated ? 0.0f : -1.0f;
}
// the observation of a state: (cos th1, sin th1, cos th2, sin th2, w1, w2)
__device__ __forceinline__ void acrobot_obs(const float* st, float* obs) {
    obs[0] = acro_cosr(st[0]);
    obs[1] = acro_sinr(st[0]);
    obs[2] = acro_cosr(st[1]);
    obs[3] = acro_sinr(st[1]);
    obs[4] = st[2];
    obs[5] = st[3];
}
// reset number k of global env e: MountainCar's keying, philox(seed; e, k, 0, 1); the four words, in state order, mapped to [-0.1, 0.1)
__device__ __forceinline__ void acrobot_reset(float* st, int k, int64_t seed, int64_t env_global) {
    const uint4 w = philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)env_global, (uint32_t)k, 0u, 1u);
    st[0] = canon_to_uniform(w.x, -0.1f, 0.1f);
    st[1] = canon_to_uniform(w.y, -0.1f, 0.1f);
    st[2] = canon_to_uniform(w.z, -0.1f, 0.1f);
    st[3] = canon_to_uniform(w.w, -0.1f, 0.1f);
}
// One step of an Acrobot env with env_step_kernel's bookkeeping (the episode ends where the env terminates or its length reaches the limit): ONE definition
// for the fused rollout and the stand-alone step.  Returns the reward; done / fin_len / fin_rew are the step's.
__device__ __forceinline__ float acrobot_step_episode(float* st, int action, int max_episode_steps, int64_t seed, int64_t env_global, int& ep_len, float& ep_rew,
                                                      int& resets, int& done, int& fin_len, float& fin_rew) {
    int term;
    const float r = acrobot_step(st, action, term);
    ep_len += 1;
    ep_rew += r;
    done = (term || ep_len == max_episode_steps) ? 1 : 0;
    fin_len = 0;
    fin_rew = 0.0f;
    if (done) {
        fin_len = ep_len;
        fin_rew = ep_rew;
        acrobot_reset(st, resets++, seed, env_global);
        ep_len = 0;
        ep_rew = 0.0f;
    }
    return r;
}
// What the fused categorical kernels need of a device env with integer actions (kernels_gauss_fused.hip: cat_rollout_kernel, the stand-alone env kernels,
// cat_eval_kernel): GaussEnv*'s members with an int action.  The env takes head 0's action.
struct CatEnvAcrobot {
    static constexpr int OBS = 6, STATE = 4, ACTIONS = 3, HOT = 0;
    static constexpr bool OBS_IS_STATE = false;
    static constexpr bool HAS_MASK = false;         // every action is always allowed: PPO_BUF_MASKS holds ones
    static constexpr bool STATE_FROM_OBS = false;   // the observation does not hold the angles: no truncation fold
    static constexpr bool OBS_ONE_HOT = false;
    __device__ static __forceinline__ void obs(const float* st, float* ob) { acrobot_obs(st, ob); }
    __device__ static __forceinline__ float step(float* st, int a, int& terminated) { return acrobot_step(st, a, terminated); }
    __device__ static __forceinline__ void reset(float* st, int k, int64_t seed, int64_t env_global) { acrobot_reset(st, k, seed, env_global); }
    __device__ static __forceinline__ float step_episode(float* st, int a, int max_episode_steps, int64_t seed, int64_t env_global, int& ep_len, float& ep_rew,
                                                         int& resets, int& done, int& fin_len, float& fin_rew) {
        return acrobot_step_episode(st, a, max_episode_steps, seed, env_global, ep_len, ep_rew, resets, done, fin_len, fin_rew);
    }
};

// Taxi-v3 (gymnasium's toy_text/taxi.py, no rain, no fickle passenger; no reference counterpart: PPO_ENV_TAXI; ppo_hip.h states the table).  st = {row, col,
// pass, dest}, small integers held exactly in f32: row, col in 0..4, pass in 0..4 (0..3 waiting at R, G, Y, B; 4 in the taxi), dest in 0..3.  Stands, as
// (row, col): R (0,0), G (0,4), Y (4,0), B (4,3).  The walls and stands are a few compares: no table in memory.  Every function converts and clamps each
// component into its range first (a NaN becomes 0), so a foreign state can index nothing outside the observation.
struct TaxiState { int r, c, p, d; };
__device__ __forceinline__ int taxi_clamp(float v, int hi) { return v >= 0.0f ? (v >= (float)hi ? hi : (int)v) : 0; }
__device__ __forceinline__ TaxiState taxi_load(const float* st) { return TaxiState{ taxi_clamp(st[0], 4), taxi_clamp(st[1], 4), taxi_clamp(st[2], 4), taxi_clamp(st[3], 3) }; }
__device__ __forceinline__ bool taxi_east_blocked(int r, int c) { return c == 4 || (r <= 1 && c == 1) || (r >= 3 && (c == 0 || c == 2)); }
__device__ __forceinline__ bool taxi_west_blocked(int r, int c) { return c == 0 || taxi_east_blocked(r, c - 1); }
// the stand the taxi is on, or -1
__device__ __forceinline__ int taxi_stand(int r, int c) { return r == 0 ? (c == 0 ? 0 : (c == 4 ? 1 : -1)) : (r == 4 ? (c == 0 ? 2 : (c == 3 ? 3 : -1)) : -1); }
// bit a: action a is allowed (exactly when it changes the state); never 0: south or north is always allowed
__device__ __forceinline__ uint32_t taxi_mask_bits(const float* st) {
    const TaxiState s = taxi_load(st);
    const int on = taxi_stand(s.r, s.c);
    return (s.r < 4 ? 1u : 0u) | (s.r > 0 ? 2u : 0u) | (taxi_east_blocked(s.r, s.c) ? 0u : 4u) | (taxi_west_blocked(s.r, s.c) ? 0u : 8u) |
           ((s.p < 4 && on == s.p) ? 16u : 0u) | ((s.p == 4 && on >= 0) ? 32u : 0u);
}
__device__ __forceinline__ float taxi_step(float* st, int action, int& terminated) {
    TaxiState s = taxi_load(st);
    const int a = action < 0 ? 0 : (action > 5 ? 5 : action);
    const int on = taxi_stand(s.r, s.c);
    float reward = -1.0f;
    terminated = 0;
    if (a == 0) s.r = s.r < 4 ? s.r + 1 : 4;
    else if (a == 1) s.r = s.r > 0 ? s.r - 1 : 0;
    else if (a == 2) { if (!taxi_east_blocked(s.r, s.c)) s.c += 1; }
    else if (a == 3) { if (!taxi_west_blocked(s.r, s.c)) s.c -= 1; }
    else if (a == 4) {
        if (s.p < 4 && on == s.p) s.p = 4;
        else reward = -10.0f;
    } else {
        if (s.p == 4 && on == s.d) { s.p = s.d; terminated = 1; reward = 20.0f; }
        else if (s.p == 4 && on >= 0) s.p = on;
        else reward = -10.0f;
    }
    st[0] = (float)s.r; st[1] = (float)s.c; st[2] = (float)s.p; st[3] = (float)s.d;
    return reward;
}
// the rows of the observation that hold 1.0f: one per one-hot group (row [0..4], col [5..9], pass [10..14], dest [15..18])
__device__ __forceinline__ void taxi_hot(const float* st, int* hot) {
    const TaxiState s = taxi_load(st);
    hot[0] = s.r; hot[1] = 5 + s.c; hot[2] = 10 + s.p; hot[3] = 15 + s.d;
}
__device__ __forceinline__ void taxi_obs(const float* st, float* ob) {
    int hot[4];
    taxi_hot(st, hot);
#pragma unroll
    for (int k = 0; k < 19; k++) ob[k] = (k == hot[0] || k == hot[1] || k == hot[2] || k == hot[3]) ? 1.0f : 0.0f;
}
// the state behind an observation: the index of the largest entry of each group, the first on ties (any 19 floats give a state inside the ranges)
__device__ __forceinline__ void taxi_state_of(const float* ob, float* st) {
    constexpr int lo[4] = { 0, 5, 10, 15 }, n[4] = { 5, 5, 5, 4 };
#pragma unroll
    for (int g = 0; g < 4; g++) {
        int best = 0;
#pragma unroll
        for (int k = 1; k < n[g]; k++) if (ob[lo[g] + k] > ob[lo[g] + best]) best = k;
        st[g] = (float)best;
    }
}
// reset number k of global env e: MountainCar's keying, philox(seed; e, k, 0, 1); uniform over gymnasium's 300 start states (passenger waiting, not at the
// destination): cell = (x * 25) >> 32, pass = (y * 4) >> 32, d = (z * 3) >> 32, dest = d + (d >= pass)
__device__ __forceinline__ void taxi_reset(float* st, int k, int64_t seed, int64_t env_global) {
    const uint4 w = philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)env_global, (uint32_t)k, 0u, 1u);
    const int cell = (int)(((uint64_t)w.x * 25u) >> 32);
    const int pass = (int)(((uint64_t)w.y * 4u) >> 32);
    const int d = (int)(((uint64_t)w.z * 3u) >> 32);
    st[0] = (float)(cell / 5); st[1] = (float)(cell % 5); st[2] = (float)pass; st[3] = (float)(d + (d >= pass ? 1 : 0));
}
// The second device env with integer actions (PPO_ENV_TAXI), the first with a mask that means something and with a state the fold can recover:
//   HAS_MASK        mask_bits(st): bit a = action a is allowed in st (cat_rollout_kernel / cat_eval_kernel draw under it when the policy is PPO_DIST_MASKED)
//   STATE_FROM_OBS  state_of(ob, st): the state behind a stored observation (cat_trunc_fold_kernel)
//   OBS_ONE_HOT     hot(st, rows): the observation is HOT ones, at these rows, over zeros -- a lane moves the ones in the X image, it keeps no observation
struct CatEnvTaxi {
    static constexpr int OBS = 19, STATE = 4, ACTIONS = 6, HOT = 4;
    static constexpr bool OBS_IS_STATE = false;
    static constexpr bool HAS_MASK = true;
    static constexpr bool STATE_FROM_OBS = true;
    static constexpr bool OBS_ONE_HOT = true;
    __device__ static __forceinline__ void obs(const float* st, float* ob) { taxi_obs(st, ob); }
    __device__ static __forceinline__ void hot(const float* st, int* rows) { taxi_hot(st, rows); }
    __device__ static __forceinline__ uint32_t mask_bits(const float* st) { return taxi_mask_bits(st); }
    __device__ static __forceinline__ void state_of(const float* ob, float* st) { taxi_state_of(ob, st); }
    __device__ static __forceinline__ float step(float* st, int a, int& terminated) { return taxi_step(st, a, terminated); }
    __device__ static __forceinline__ void reset(float* st, int k, int64_t seed, int64_t env_global) { taxi_reset(st, k, seed, env_global); }
    // env_step_kernel's bookkeeping, as acrobot_step_episode
    __device__ static __forceinline__ float step_episode(float* st, int a, int max_episode_steps, int64_t seed, int64_t env_global, int& ep_len, float& ep_rew,
                                                         int& resets, int& done, int& fin_len, float& fin_rew) {
        int term;
        const float r = taxi_step(st, a, term);
        ep_len += 1;
        ep_rew += r;
        done = (term || ep_len == max_episode_steps) ? 1 : 0;
        fin_len = 0;
        fin_rew = 0.0f;
        if (done) {
            fin_len = ep_len;
            fin_rew = ep_rew;
            taxi_reset(st, resets++, seed, env_global);
            ep_len = 0;
            ep_rew = 0.0f;
        }
        return r;
    }
};

// FrozenLake-v1 / FrozenLake8x8-v1 (gymnasium's toy_text/frozen_lake.py, is_slippery = True; no reference counterpart: PPO_ENV_FROZENLAKE, PPO_ENV_FROZENLAKE8X8;
// ppo_hip.h states the maps and the step).  The first device env whose transitions draw random numbers, and the state carries the randomness: st = {cell, j,
// k0, k1}, integers held exactly in f32 -- cell in 0..S-1 (row-major, S = SIDE * SIDE), j the steps taken in this episode, (k0, k1) the episode's 2 x 24-bit
// key, drawn at the reset.  A step's slip is a word of philox4x32_10(key = (k0, k1); counter = (j >> 2, 0, 0, 0x20)), so the step stays a pure function of
// (state, action): the stateless transition, the stand-alone step, the rollout and the evaluation share ONE definition and no seed or step index is passed.
// Holes and goal are compares against a bit mask: no table in memory.  Every function converts and clamps each component into its range first (a NaN becomes
// 0), so a foreign state can index nothing outside the observation.
constexpr int FROZENLAKE_WORD_MAX = (1 << 24) - 1;   // j, k0 and k1 are at most this: every integer up to it is an f32
constexpr uint32_t FROZENLAKE_SLIP_TAG = 0x20u;      // the Philox counter word that names this draw (no other draw of the library uses it)
template <int SIDE>
struct FrozenLakeMap;
template <>
struct FrozenLakeMap<4> {   // SFFF FHFH FFFH HFFG: holes {5, 7, 11, 12}
    static constexpr uint64_t HOLES = 0x18a0ull;
    static constexpr int SHIFT = 2;
};
template <>
struct FrozenLakeMap<8> {   // gymnasium's 8x8: holes {19, 29, 35, 41, 42, 46, 49, 52, 54, 59}
    static constexpr uint64_t HOLES = 0x0852460820080000ull;
    static constexpr int SHIFT = 3;
};
__device__ __forceinline__ int frozenlake_clamp(float v, int hi) { return v >= 0.0f ? (v >= (float)hi ? hi : (int)v) : 0; }
template <int SIDE>
__device__ __forceinline__ bool frozenlake_terminal(int cell) { return cell == SIDE * SIDE - 1 || ((FrozenLakeMap<SIDE>::HOLES >> cell) & 1ull) != 0; }
template <int SIDE>
__device__ __forceinline__ int frozenlake_cell(const float* st) { return frozenlake_clamp(st[0], SIDE * SIDE - 1); }
template <int SIDE>
__device__ __forceinline__ float frozenlake_step(float* st, int action, int& terminated) {
    constexpr int S = SIDE * SIDE, SH = FrozenLakeMap<SIDE>::SHIFT;
    int cell = frozenlake_clamp(st[0], S - 1);
    const int j = frozenlake_clamp(st[1], FROZENLAKE_WORD_MAX), k0 = frozenlake_clamp(st[2], FROZENLAKE_WORD_MAX), k1 = frozenlake_clamp(st[3], FROZENLAKE_WORD_MAX);
    const int a = action < 0 ? 0 : (action > 3 ? 3 : action);
    float reward = 0.0f;
    terminated = 1;
    if (!frozenlake_terminal<SIDE>(cell)) {   // a hole or the goal is reachable through an injected state only: nothing moves, nothing is drawn
        const uint4 w = philox4x32_10((uint32_t)k0, (uint32_t)k1, (uint32_t)(j >> 2), 0u, 0u, FROZENLAKE_SLIP_TAG);
        const uint32_t word = (j & 3) == 0 ? w.x : ((j & 3) == 1 ? w.y : ((j & 3) == 2 ? w.z : w.w));
        const int d = (int)(((uint64_t)word * 3u) >> 32);   // 0, 1, 2: one third each
        const int eff = (a + d + 3) & 3;                    // gym's [(a - 1) % 4, a, (a + 1) % 4]; 0 left, 1 down, 2 right, 3 up
        int row = cell >> SH, col = cell & (SIDE - 1);
        if (eff == 0) col = col > 0 ? col - 1 : 0;
        else if (eff == 1) row = row < SIDE - 1 ? row + 1 : SIDE - 1;
        else if (eff == 2) col = col < SIDE - 1 ? col + 1 : SIDE - 1;
        else row = row > 0 ? row - 1 : 0;
        cell = (row << SH) | col;
        terminated = frozenlake_terminal<SIDE>(cell) ? 1 : 0;
        reward = cell == S - 1 ? 1.0f : 0.0f;
    }
    st[0] = (float)cell;
    st[1] = (float)(j < FROZENLAKE_WORD_MAX ? j + 1 : FROZENLAKE_WORD_MAX);   // the cap is met by an injected j only: max_episode_steps ends an episode first
    st[2] = (float)k0;
    st[3] = (float)k1;
    return reward;
}
// reset number k of global env e: MountainCar's keying, philox(seed; e, k, 0, 1); the start cell, no steps taken, and the episode's key from the top 24 bits of x, y
__device__ __forceinline__ void frozenlake_reset(float* st, int k, int64_t seed, int64_t env_global) {
    const uint4 w = philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)env_global, (uint32_t)k, 0u, 1u);
    st[0] = 0.0f; st[1] = 0.0f; st[2] = (float)(w.x >> 8); st[3] = (float)(w.y >> 8);
}
// The third device env with integer actions (PPO_ENV_FROZENLAKE: SIDE 4, PPO_ENV_FROZENLAKE8X8: SIDE 8), the first whose step draws: nothing of the drawing
// shows in the traits -- step(st, a) reads its key and its count from st.  The observation is one one of `cell` over zeros (OBS_ONE_HOT, HOT 1); it holds the
// cell but neither j nor the key, so no state can be rebuilt from it (no STATE_FROM_OBS, no truncation fold).
template <int SIDE>
struct CatEnvFrozenLake {
    static constexpr int OBS = SIDE * SIDE, STATE = 4, ACTIONS = 4, HOT = 1;
    static constexpr bool OBS_IS_STATE = false;
    static constexpr bool HAS_MASK = false;
    static constexpr bool STATE_FROM_OBS = false;
    static constexpr bool OBS_ONE_HOT = true;
    __device__ static __forceinline__ void hot(const float* st, int* rows) { rows[0] = frozenlake_cell<SIDE>(st); }
    __device__ static __forceinline__ void obs(const float* st, float* ob) {
        const int cell = frozenlake_cell<SIDE>(st);
#pragma unroll
        for (int k = 0; k < OBS; k++) ob[k] = k == cell ? 1.0f : 0.0f;
    }
    __device__ static __forceinline__ float step(float* st, int a, int& terminated) { return frozenlake_step<SIDE>(st, a, terminated); }
    __device__ static __forceinline__ void reset(float* st, int k, int64_t seed, int64_t env_global) { frozenlake_reset(st, k, seed, env_global); }
    // env_step_kernel's bookkeeping, as acrobot_step_episode
    __device__ static __forceinline__ float step_episode(float* st, int a, int max_episode_steps, int64_t seed, int64_t env_global, int& ep_len, float& ep_rew,
                                                         int& resets, int& done, int& fin_len, float& fin_rew) {
        int term;
        const float r = frozenlake_step<SIDE>(st, a, term);
        ep_len += 1;
        ep_rew += r;
        done = (term || ep_len == max_episode_steps) ? 1 : 0;
        fin_len = 0;
        fin_rew = 0.0f;
        if (done) {
            fin_len = ep_len;
            fin_rew = ep_rew;
            frozenlake_reset(st, resets++, seed, env_global);
            ep_len = 0;
            ep_rew = 0.0f;
        }
        return r;
    }
};

// Blackjack-v1 (gymnasium's toy_text/blackjack.py, natural = False, sab = False, the infinite deck; no reference counterpart: PPO_ENV_BLACKJACK; ppo_hip.h
// states the cards and the step).  FrozenLake's mechanism with a NUMBER OF DRAWS THAT DEPENDS ON THE DATA: st = {hand, n, k0, k1}, integers held exactly in
// f32 -- hand = t + 32 * ace + 64 * show (t the player's total with aces as 1, ace whether the player holds one, show the dealer's showing card), n the index
// of the next card, (k0, k1) the episode's 2 x 24-bit key.  Card i of an episode is word i & 3 of philox4x32_10(key = (k0, k1); counter = (i >> 2, 0, 0,
// 0x21)): a hit draws card n, a stick plays the dealer out from (show, card 3) with cards n, n + 1, ..  The step stays a pure function of (state, action).
// Every function converts and clamps each component into its range first (a NaN becomes 0), so a foreign state can index nothing outside the observation,
// and the dealer's loop has a compile-time bound with a predicate: no state can spin a lane.
constexpr int BLACKJACK_WORD_MAX = (1 << 24) - 1;         // n, k0 and k1 are at most this: every integer up to it is an f32
constexpr int BLACKJACK_HAND_MAX = 31 + 32 + 64 * 10;     // 703: the largest hand word
constexpr uint32_t BLACKJACK_CARD_TAG = 0x21u;            // the Philox counter word that names this draw (no other draw of the library uses it)
constexpr int BLACKJACK_DEALER_DRAWS = 10;                // the most cards a dealer draws from any two-card start (enumerated in tests/test_blackjack_cpu.py)
struct BlackjackHand { int t, ace, show; };
__device__ __forceinline__ int blackjack_clamp(float v, int hi) { return v >= 0.0f ? (v >= (float)hi ? hi : (int)v) : 0; }
// the hand word clamped into 0..703, then its fields: t into 2..31, show into 1..10 (703 >> 6 = 10)
__device__ __forceinline__ BlackjackHand blackjack_hand(const float* st) {
    const int h = blackjack_clamp(st[0], BLACKJACK_HAND_MAX);
    const int t = h & 31, show = h >> 6;
    return BlackjackHand{ t < 2 ? 2 : t, (h >> 5) & 1, show < 1 ? 1 : show };
}
__device__ __forceinline__ int blackjack_usable(const BlackjackHand& h) { return (h.ace && h.t + 10 <= 21) ? 1 : 0; }
// gym's deck [1..10, 10, 10, 10]: thirteen equal buckets of a word, the last four are tens
__device__ __forceinline__ int blackjack_card(uint32_t word) {
    const int c = 1 + (int)(((uint64_t)word * 13u) >> 32);
    return c < 10 ? c : 10;
}
// the four words of one Philox call are kept while consecutive card indices share i >> 2 (blk = ~0: nothing kept; a card index is below 2^24 + 10)
struct BlackjackDeck { uint32_t k0, k1, blk; uint4 w; };
__device__ __forceinline__ int blackjack_draw(BlackjackDeck& d, uint32_t i) {
    if ((i >> 2) != d.blk) {
        d.blk = i >> 2;
        d.w = philox4x32_10(d.k0, d.k1, d.blk, 0u, 0u, BLACKJACK_CARD_TAG);
    }
    return blackjack_card((i & 3) == 0 ? d.w.x : ((i & 3) == 1 ? d.w.y : ((i & 3) == 2 ? d.w.z : d.w.w)));
}
__device__ __forceinline__ float blackjack_step(float* st, int action, int& terminated) {
    BlackjackHand h = blackjack_hand(st);
    const int n = blackjack_clamp(st[1], BLACKJACK_WORD_MAX), k0 = blackjack_clamp(st[2], BLACKJACK_WORD_MAX), k1 = blackjack_clamp(st[3], BLACKJACK_WORD_MAX);
    const int a = action < 0 ? 0 : (action > 1 ? 1 : action);
    uint32_t next = (uint32_t)n;
    float reward = -1.0f;
    terminated = 1;
    if (h.t <= 21) {   // a bust hand is reachable through an injected state only: nothing is drawn, the state stays
        BlackjackDeck deck{ (uint32_t)k0, (uint32_t)k1, ~0u, uint4{ 0u, 0u, 0u, 0u } };
        if (a == 1) {   // hit
            const int c = blackjack_draw(deck, next++);
            h.t += c;
            h.ace |= c == 1 ? 1 : 0;
            terminated = h.t > 21 ? 1 : 0;
            reward = h.t > 21 ? -1.0f : 0.0f;
        } else {        // stick: the dealer plays out from (show, card 3)
            const int hidden = blackjack_draw(deck, 3u);
            int dt = h.show + hidden, dace = (h.show == 1 || hidden == 1) ? 1 : 0;
#pragma unroll 1
            for (int d = 0; d < BLACKJACK_DEALER_DRAWS; d++) {
                if (dt + ((dace && dt + 10 <= 21) ? 10 : 0) < 17) {
                    const int c = blackjack_draw(deck, next++);
                    dt += c;
                    dace |= c == 1 ? 1 : 0;
                }
            }
            const int dealer = dt > 21 ? 0 : dt + ((dace && dt + 10 <= 21) ? 10 : 0);
            const int player = h.t + 10 * blackjack_usable(h);
            reward = player > dealer ? 1.0f : (player == dealer ? 0.0f : -1.0f);
        }
    }
    st[0] = (float)(h.t + 32 * h.ace + 64 * h.show);
    st[1] = (float)(next < (uint32_t)BLACKJACK_WORD_MAX ? (int)next : BLACKJACK_WORD_MAX);
    st[2] = (float)k0;
    st[3] = (float)k1;
    return reward;
}
// reset number k of global env e: MountainCar's keying, philox(seed; e, k, 0, 1) gives the episode's key; the key's first call deals cards 0 .. 3
__device__ __forceinline__ void blackjack_reset(float* st, int k, int64_t seed, int64_t env_global) {
    const uint4 w = philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)env_global, (uint32_t)k, 0u, 1u);
    const uint32_t k0 = w.x >> 8, k1 = w.y >> 8;
    const uint4 c = philox4x32_10(k0, k1, 0u, 0u, 0u, BLACKJACK_CARD_TAG);
    const int c0 = blackjack_card(c.x), c1 = blackjack_card(c.y), show = blackjack_card(c.z);
    st[0] = (float)(c0 + c1 + ((c0 == 1 || c1 == 1) ? 32 : 0) + 64 * show);
    st[1] = 4.0f;
    st[2] = (float)k0;
    st[3] = (float)k1;
}
// The fourth kind of device env with integer actions (PPO_ENV_BLACKJACK).  The observation is gymnasium's flattened Tuple(Discrete(32), Discrete(11),
// Discrete(2)): three ones over zeros (OBS_ONE_HOT, HOT 3) at sum, 32 + show and 43 + usable; it holds neither n nor the key (no STATE_FROM_OBS, no fold).
struct CatEnvBlackjack {
    static constexpr int OBS = 45, STATE = 4, ACTIONS = 2, HOT = 3;
    static constexpr bool OBS_IS_STATE = false;
    static constexpr bool HAS_MASK = false;
    static constexpr bool STATE_FROM_OBS = false;
    static constexpr bool OBS_ONE_HOT = true;
    __device__ static __forceinline__ void hot(const float* st, int* rows) {
        const BlackjackHand h = blackjack_hand(st);
        const int u = blackjack_usable(h);
        rows[0] = h.t + 10 * u; rows[1] = 32 + h.show; rows[2] = 43 + u;
    }
    __device__ static __forceinline__ void obs(const float* st, float* ob) {
        int rows[3];
        hot(st, rows);
#pragma unroll
        for (int k = 0; k < OBS; k++) ob[k] = (k == rows[0] || k == rows[1] || k == rows[2]) ? 1.0f : 0.0f;
    }
    __device__ static __forceinline__ float step(float* st, int a, int& terminated) { return blackjack_step(st, a, terminated); }
    __device__ static __forceinline__ void reset(float* st, int k, int64_t seed, int64_t env_global) { blackjack_reset(st, k, seed, env_global); }
    // env_step_kernel's bookkeeping, as acrobot_step_episode
    __device__ static __forceinline__ float step_episode(float* st, int a, int max_episode_steps, int64_t seed, int64_t env_global, int& ep_len, float& ep_rew,
                                                         int& resets, int& done, int& fin_len, float& fin_rew) {
        int term;
        const float r = blackjack_step(st, a, term);
        ep_len += 1;
        ep_rew += r;
        done = (term || ep_len == max_episode_steps) ? 1 : 0;
        fin_len = 0;
        fin_rew = 0.0f;
        if (done) {
            fin_len = ep_len;
            fin_rew = ep_rew;
            blackjack_reset(st, resets++, seed, env_global);
            ep_len = 0;
            ep_rew = 0.0f;
        }
        return r;
    }
};

// step_episode's sibling for a context with PPO_KERNEL_ENV_CUT_STATE, for every trait above (Action: float on a GaussEnv*, int on a CatEnv*): the trait's
// bare step and reset under the same bookkeeping, statement for statement (a Gaussian env's step reports terminated = 0 where it never terminates), and one
// thing more -- where the episode's length reaches the limit on this step, the state the env is in BEFORE the reset (Env::STATE words) and whether the env
// itself terminated (0.0f / 1.0f) are stored at rec[0], rec[stride], .., rec[Env::STATE * stride].  No other step stores anything.  The traits' own
// step_episode, which the stand-alone step kernels and the rollouts of every other context run, is not touched.
template <class Env, class Action>
__device__ __forceinline__ float step_episode_keep(float* st, Action a, int max_episode_steps, int64_t seed, int64_t env_global, int& ep_len, float& ep_rew,
                                                   int& resets, int& done, int& fin_len, float& fin_rew, float* rec, size_t stride) {
    int term;
    const float r = Env::step(st, a, term);
    ep_len += 1;
    ep_rew += r;
    done = (term || ep_len == max_episode_steps) ? 1 : 0;
    fin_len = 0;
    fin_rew = 0.0f;
    if (done) {
        fin_len = ep_len;
        fin_rew = ep_rew;
        if (ep_len == max_episode_steps) {
#pragma unroll
            for (int k = 0; k < Env::STATE; k++) rec[(size_t)k * stride] = st[k];
            rec[(size_t)Env::STATE * stride] = term ? 1.0f : 0.0f;
        }
        Env::reset(st, resets++, seed, env_global);
        ep_len = 0;
        ep_rew = 0.0f;
    }
    return r;
}

template <int ENV>
__device__ __forceinline__ float env_step(float* st, int action, int& terminated) {
    if constexpr (ENV == PPO_ENV_CARTPOLE) return cartpole_step(st, action, terminated);
    else return mountaincar_step(st, action, terminated);
}
// env_step in two halves: what depends on the state only (tr[0], tr[1]) ...
template <int ENV>
__device__ __forceinline__ void env_step_pre(const float* st, float* tr) {
    if constexpr (ENV == PPO_ENV_CARTPOLE) { tr[0] = glibc_cosf(st[2]); tr[1] = glibc_sinf(st[2]); }
    else { tr[0] = glibc_cosf(3.0f * st[0]); tr[1] = 0.0f; }
}
// ... and what depends on the action: env_step(st, a, t) == env_step_pre(st, tr) then env_step_tail(st, a, tr, t), bit for bit
template <int ENV>
__device__ __forceinline__ float env_step_tail(float* st, int action, const float* tr, int& terminated) {
    if constexpr (ENV == PPO_ENV_CARTPOLE) return cartpole_tail(st, action, tr[0], tr[1], terminated);
    else return mountaincar_tail(st, action, tr[0], terminated);
}

// CartPole::reset (CartPole.cpp:34-45): the k-th reset of ANY env reads words 4k..4k+3 of the one stream all envs share
// (every env is constructed with the same seed, PPO_Discrete.cpp:84-86).  MountainCar::reset (MountainCar.cpp:59-66,79-88)
// draws from std::random_device in the reference; the build keys it: philox(seed; global env, reset#, 0, 1).x.
template <int ENV>
__device__ __forceinline__ void env_reset(float* st, const float* __restrict__ reset_table, int k, int64_t seed, int64_t env_global) {
    if constexpr (ENV == PPO_ENV_CARTPOLE) {
        const float4 r = reinterpret_cast<const float4*>(reset_table)[k];
        st[0] = r.x; st[1] = r.y; st[2] = r.z; st[3] = r.w;
    } else {
        const uint4 w = philox4x32_10((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)env_global, (uint32_t)k, 0u, 1u);
        st[0] = canon_to_uniform(w.x, -0.6f, -0.4f);
        st[1] = 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Categorical / CategoricalMasked over one head of width A held in a small array (uniform across the wave or per-thread).
// reference Distributions/Categorical.cpp:28-39,92-119; CategoricalMasked.cpp:31-46,107-144.
//   z[a] in: raw logits; out: m_logits (log-probs).  p[a] out: m_probs.  returns entropy.
//   ZS: the stride (floats) between two elements of z and of p; 1 = a plain array.  The fused 2 x 64 kernels keep both as columns of [logit][sample]
//   LDS images (stride PPO_LDS_STRIDE), where a run-time index costs nothing; the arithmetic does not depend on it.
// ---------------------------------------------------------------------------------------------------------
template <int DIST, int ZS = 1>
__device__ __forceinline__ float categorical_head(float* z, float* p, const uint8_t* mask, int A) {
    float mx = -INFINITY;
    for (int a = 0; a < A; a++) {
        if (DIST == PPO_DIST_MASKED && mask && !mask[a]) z[a * ZS] = -1e8f;
        mx = z[a * ZS] > mx ? z[a * ZS] : mx;
    }
    float se = 0.0f;
    for (int a = 0; a < A; a++) { p[a * ZS] = expf(z[a * ZS] - mx); se += p[a * ZS]; }
    const float lse = logf(se) + mx;
    float ent = 0.0f;
    for (int a = 0; a < A; a++) {
        z[a * ZS] = z[a * ZS] - lse;
        p[a * ZS] = p[a * ZS] / se;
        if (DIST == PPO_DIST_CATEGORICAL) {
            const float l = z[a * ZS] > 1.17549435e-38f ? z[a * ZS] : 1.17549435e-38f;  // torch::clamp(m_logits, FLT_MIN), Categorical.cpp:115
            ent += l * p[a * ZS];
        } else {
            const float plp = z[a * ZS] * p[a * ZS];
            ent += (mask == nullptr || mask[a]) ? plp : 0.0f;
        }
    }
    return -ent;
}

// Inverse-CDF draw on m_probs with u in [0,1) (mirrors oracle/ppo_oracle.c:orc_act).  ZS: as above.
template <int ZS = 1>
__device__ __forceinline__ int sample_head(const float* p, int A, float u) {
    int a = 0, last = 0;
    float acc = 0.0f;
    bool hit = false;
    for (int k = 0; k < A; k++) {
        if (p[k * ZS] > 0.0f) last = k;
        acc += p[k * ZS];
        if (!hit && u < acc) { a = k; hit = true; }
    }
    return hit ? a : last;
}

// tanh for the update kernels: branch-free, ~3 ULP.  |x| >= 0.12: (1 - t) / (1 + t) with t = exp(-2|x|) on the hardware
// exp2 / rcp (v_exp_f32, v_rcp_f32); below that the odd Taylor polynomial to x^7 (truncation < 2e-9 relative at 0.12) avoids the
// cancellation in 1 - t.  The clamp keeps the exp2 argument inside the range where v_exp_f32 needs no denormal pre-scaling.
// exp / log on the hardware exp2 / log2 units (v_exp_f32, v_log_f32; ~1 ULP of the base-2 result).
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(fmaxf(x, -100.0f) * 1.4426950408889634f); }
__device__ __forceinline__ float fast_log(float x) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }

// tanh on the transcendental pipe: 1 - 2 / (1 + e^(2x)), five instructions (v_mul, v_exp, v_add, v_rcp, v_fma), absolute error
// <= ~2e-7 (the library tanhf costs ~40 and a sign-symmetric form 14; 64 tanh per lane per tile made them half of the kernel's
// vector instructions).  Saturates correctly: e = inf -> 1, e = 0 -> -1.
__device__ __forceinline__ float tanh_mufu(float x) {
    const float e = __builtin_amdgcn_exp2f(x * 2.885390081777927f);
    return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + e), 1.0f);
}

__device__ __forceinline__ float tanh_fast(float x) {
    const float ax = fminf(fabsf(x), 20.0f);
    const float t = __builtin_amdgcn_exp2f(ax * -2.885390081777927f);   // exp(-2|x|)
    const float big = (1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t);
    const float x2 = x * x;
    const float poly = __builtin_fmaf(x2, __builtin_fmaf(x2, __builtin_fmaf(x2, -17.0f / 315.0f, 2.0f / 15.0f), -1.0f / 3.0f), 1.0f);
    const float small = x * poly;
    const float bigs = __builtin_copysignf(big, x);
    return ax < 0.12f ? small : bigs;
}

// categorical_head on the hardware exp2 / log2 / rcp units (v_exp_f32, v_log_f32, v_rcp_f32: ~1 ULP each; log-probs within ~3e-7 of the
// library version): for kernels where one wave evaluates the heads on a step's critical path.
template <int DIST>
__device__ __forceinline__ float categorical_head_fast(float* z, float* p, const uint8_t* mask, int A) {
    float mx = -INFINITY;
    for (int a = 0; a < A; a++) {
        if (DIST == PPO_DIST_MASKED && mask && !mask[a]) z[a] = -1e8f;
        mx = z[a] > mx ? z[a] : mx;
    }
    float se = 0.0f;
    for (int a = 0; a < A; a++) { p[a] = fast_exp(z[a] - mx); se += p[a]; }
    const float lse = fast_log(se) + mx;
    const float rse = __builtin_amdgcn_rcpf(se);
    float ent = 0.0f;
    for (int a = 0; a < A; a++) {
        z[a] = z[a] - lse;
        p[a] = p[a] * rse;
        if (DIST == PPO_DIST_CATEGORICAL) {
            const float l = z[a] > 1.17549435e-38f ? z[a] : 1.17549435e-38f;
            ent += l * p[a];
        } else {
            const float plp = z[a] * p[a];
            ent += (mask == nullptr || mask[a]) ? plp : 0.0f;
        }
    }
    return -ent;
}

// Wave-wide float sum, result in every lane, on the DPP cross-lane network (no LDS crossbar round trips, which cost ~100+
// cycles each and are on the rollout's per-step dependency chain): butterfly inside each row of 16 lanes with
// quad_perm / row_half_mirror / row_mirror, then the four row sums are read through scalar registers.  Fixed order.
#define PPO_DPP_ADD(v, CTRL) ((v) + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (v)), (CTRL), 0xf, 0xf, false)))
__device__ __forceinline__ float wave_sum(float v) {
    v = PPO_DPP_ADD(v, 0xB1);    // quad_perm:[1,0,3,2]
    v = PPO_DPP_ADD(v, 0x4E);    // quad_perm:[2,3,0,1]
    v = PPO_DPP_ADD(v, 0x141);   // row_half_mirror
    v = PPO_DPP_ADD(v, 0x140);   // row_mirror: every lane of a row now holds the row's sum
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
    return ((r0 + r1) + r2) + r3;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// The same sum on the DPP network (no ds_bpermute round trips: a double butterfly through LDS costs twelve of them); result in
// every lane, fixed order (inside rows of 16 by butterfly, then the four row sums in order).
#define PPO_DPP_ADD_D(v, CTRL)                                                                                              \
    do {                                                                                                                    \
        const int lo_ = __builtin_amdgcn_update_dpp(0, __double2loint(v), (CTRL), 0xf, 0xf, false);                         \
        const int hi_ = __builtin_amdgcn_update_dpp(0, __double2hiint(v), (CTRL), 0xf, 0xf, false);                         \
        (v) += __hiloint2double(hi_, lo_);                                                                                  \
    } while (0)
__device__ __forceinline__ double wave_sum_d_dpp(double v) {
    PPO_DPP_ADD_D(v, 0xB1);    // quad_perm:[1,0,3,2]
    PPO_DPP_ADD_D(v, 0x4E);    // quad_perm:[2,3,0,1]
    PPO_DPP_ADD_D(v, 0x141);   // row_half_mirror
    PPO_DPP_ADD_D(v, 0x140);   // row_mirror: every lane of a row now holds the row's sum
    double r[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
        r[i] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 16 * i), __builtin_amdgcn_readlane(__double2loint(v), 16 * i));
    return ((r[0] + r[1]) + r[2]) + r[3];
}

// ---------------------------------------------------------------------------------------------------------
// clip_grad_norm_ + AdamW::step (PPO_Discrete.cpp:640-641) pieces shared by the stand-alone optimizer kernel and the update kernel's
// prologue (deferred step): ONE definition, so the two paths are bit-identical.
// ---------------------------------------------------------------------------------------------------------
// Total gradient norm from the per-workgroup sums of squares: wave w (< 4) adds the partials of the workgroups that touch tensors w, w + 4,
// w + 8 in a fixed order (all three loads in flight together, sums on the DPP network).  Every thread of the workgroup must call it
// (one barrier inside); n2s: 12 doubles of shared memory.
__device__ __forceinline__ float opt_total_norm(const NetLayout& L, const double* __restrict__ partial, double* n2s, int tid) {
    // The wave index as a SCALAR (it is wave-uniform; the compiler cannot know): L.tensor_off[w + 4 j] is then a scalar load out of the kernel arguments.  Indexed
    // by the per-lane value it was a VECTOR load from the argument segment with a wait behind it, and the partials' loads depended on it: three such pairs in a
    // row, six dependent memory round trips in a 5 us kernel (round 6, found in the assembly).  Now: the three tensors' block ranges first, then EVERY load of the
    // wave's three tensors (two per lane and tensor cover 128 workgroups of the slab reduction: more than any tensor of the reference's shapes spans) in one
    // batch, then the sums -- in the same order as before (a lane's blocks in index order), so the same bits.
    // Loads are UNCONDITIONAL with clamped addresses and the values selected afterwards: a load inside a divergent branch makes the compiler wait for it at
    // the join.  The thirteen offsets come as one batch of scalar loads and are picked by selects over a fixed bound, not by a dependent indexed load each.
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (w < 4) {
        int off[13];
#pragma unroll
        for (int t = 0; t < 13; t++) off[t] = L.tensor_off[t];
        int blo[3], bhi[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int t = w + 4 * j;
            int lo = 0, hi = 0;
#pragma unroll
            for (int tt = 0; tt < 12; tt++) { lo = tt == t ? off[tt] : lo; hi = tt == t ? off[tt + 1] : hi; }
            const bool have = t < L.n_tensors;
            blo[j] = have ? lo / 64 : 1;
            bhi[j] = have ? (hi - 1) / 64 : 0;
        }
        double v0[3], v1[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int t = w + 4 * j, b = blo[j] + lane;
            const int b0 = b <= bhi[j] ? b : 0, b1 = b + 64 <= bhi[j] ? b + 64 : 0;
            v0[j] = partial[(size_t)b0 * 12 + t];
            v1[j] = partial[(size_t)b1 * 12 + t];
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int t = w + 4 * j, b = blo[j] + lane;
            double v = 0.0;
            v += b <= bhi[j] ? v0[j] : 0.0;
            v += b + 64 <= bhi[j] ? v1[j] : 0.0;
            if (bhi[j] - blo[j] >= 128)   // wave-uniform; no tensor of the reference's shapes gets here
                for (int bb = b + 128; bb <= bhi[j]; bb += 64) v += partial[(size_t)bb * 12 + t];
            const double r = wave_sum_d_dpp(v);
            if (lane == 0) n2s[t] = r;
        }
    }
    __syncthreads();
    // total = || (||g_1||, ..., ||g_12||) ||_2 with float per-tensor norms (clip_grad.h:58-70).  Lane t forms tensor t's norm -- ONE binary64 square
    // root per wave instead of twelve in a row on every lane (a binary64 sqrt is a ~40-instruction sequence) -- and the squares are added in tensor
    // order through scalar registers: the same operations in the same order as before, every thread gets the same bits.
    double sq = 0.0;
    if (lane < 12) { const float nrm = (float)sqrt(n2s[lane]); sq = (double)nrm * nrm; }
    double tot = 0.0;
#pragma unroll
    for (int t = 0; t < 12; t++)
        tot += __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(sq), t), __builtin_amdgcn_readlane(__double2loint(sq), t));
    return (float)sqrt(tot);
}
__device__ __forceinline__ float opt_clip_coef(float total, float max_norm) {   // clip_grad.h:76-78
    const float c = max_norm / (total + 1e-6f);
    return c > 1.0f ? 1.0f : c;
}
__device__ __forceinline__ void adamw_apply(float g, float c, const AdamCoef& k, float& p, float& m, float& v) {
    const float b1 = 0.9f, b2 = 0.999f, omb1 = (float)(1.0 - 0.9), omb2 = (float)(1.0 - 0.999), eps = 1e-5f;
    const float gc = g * c;
    const float pi = p * k.decay;
    const float mi = __builtin_fmaf(gc, omb1, m * b1);
    const float vi = __builtin_fmaf(omb2 * gc, gc, v * b2);
    const float denom = sqrtf(vi) / k.sqrt_bc2 + eps;
    p = pi + (k.neg_step * mi) / denom;
    m = mi;
    v = vi;
}
// printPPOResults' inputs of one step (PPO_Discrete.cpp:700-774) from its loss sums; one thread
__device__ __forceinline__ void opt_write_stats(const double* ls, double cf0, double cf1, double global_M, const LossParams& hp, float total,
                                                StepStats* stats_out, double* clipfrac_accum) {
    const float pg = (float)(ls[0] / global_M);
    const float vl = 0.5f * (float)(ls[4] / global_M);
    const float el = (float)(ls[1] / global_M);
    StepStats o;
    o.pg_loss = pg;
    o.v_loss = vl;
    o.entropy_loss = el;
    o.approx_kl = (float)(ls[2] / global_M);
    o.clipfrac = (float)ls[3] / (float)global_M;
    o.loss = (pg - hp.ent_coef * el) + vl * hp.vf_coef;
    o.total_norm = total;
    o.pad = 0.0;
    *stats_out = o;
    if (clipfrac_accum) { clipfrac_accum[0] = cf0 + o.clipfrac; clipfrac_accum[1] = cf1 + 1.0; }
}
#endif  // __HIPCC__

// ---------------------------------------------------------------------------------------------------------
// Host-side launcher prototypes (each defined next to its kernels)
// ---------------------------------------------------------------------------------------------------------
struct RolloutArgs {
    // network
    const float* params;
    NetLayout L;
    int dist_kind;
    // env
    int env_kind;
    int N, T;
    int max_episode_steps;
    int64_t seed, env_offset, step_base;  // step_base: global index of rollout step 0 (sampling stream position)
    float* env_state;      // [O,N]
    int32_t* ep_len;       // [N]
    float* ep_rew;         // [N]
    int32_t* reset_count;  // [N]
    const float* reset_table;
    int reset_cap;
    int32_t* error_flag;
    // rollout buffers
    float* obs;            // [T,N,O]
    int32_t* actions;      // [T,N,H]
    float* logprobs;       // [T,N]
    float* rewards;        // [T,N]
    float* dones;          // [T,N]
    float* values;         // [T,N]
    uint8_t* masks;        // [T,N,A] or null
    int32_t* fin_len;      // [T,N]
    float* fin_rew;        // [T,N]
    float* next_obs;       // [N,O]
    int32_t* next_done;    // [N]
    float* next_value;     // [N]
    const int64_t* forced_actions;  // [T,N,H] or null
    int vector_kernel;     // PPO_KERNEL_ROLLOUT_VECTOR: rollout2_kernel for the single-head shapes
};

hipError_t launch_rollout(const RolloutArgs& a, hipStream_t s);
hipError_t launch_values(const float* params, const NetLayout& L, const float* obs0, int64_t n0, float* out0, const float* obs1, int64_t n1,
                         float* out1, hipStream_t s);
hipError_t launch_env_reset(int env_kind, int N, int64_t seed, int64_t env_offset, float* env_state, int32_t* ep_len, float* ep_rew,
                            int32_t* reset_count, const float* reset_table, int reset_cap, float* next_obs, int32_t* next_done,
                            int32_t* error_flag, hipStream_t s);
hipError_t launch_env_step(int env_kind, int N, int H, int max_episode_steps, int64_t seed, int64_t env_offset, float* env_state,
                           int32_t* ep_len, float* ep_rew, int32_t* reset_count, const float* reset_table, int reset_cap,
                           const int64_t* action, float* obs, float* reward, int32_t* done, int32_t* error_flag, hipStream_t s,
                           int32_t* fin_len = nullptr, float* fin_rew = nullptr);   // fin_*: the finished episodes' numbers of this step (a rollout's FIN_LEN / FIN_REW row)
hipError_t launch_env_transition(int env_kind, const float* state_in, const int64_t* action, int64_t n, float* next_state,
                                 float* reward, int32_t* terminated, hipStream_t s);
hipError_t launch_aos_to_soa(const float* aos, float* soa, int N, int O, bool to_soa, hipStream_t s);

hipError_t launch_policy_act(const float* params, const NetLayout& L, int dist_kind, const float* obs, const uint8_t* mask,
                             const int64_t* forced_action, int64_t n, int64_t seed, int64_t env_offset, int64_t step_index,
                             int64_t* action, float* logprob, float* entropy, float* value, bool value_only, hipStream_t s, bool as_rollout16 = false,
                             int32_t* error_flag = nullptr, bool greedy = false);   // as_rollout16: rollout16_kernel's arithmetic where that kernel serves the shape (policy_act16_serves); greedy: the heads' modes instead of draws (forced_action is ignored)
bool policy_act16_serves(const NetLayout& L);

// ppo_evaluate: whole episodes of the context's device env under the current policy as one launch (kernels_rollout.hip: eval16_kernel / evalv_kernel)
struct EvalArgs {
    const float* params;
    NetLayout L;
    int dist_kind, env_kind;
    int max_episode_steps;
    int greedy;                 // the heads' modes; 0: the sampler keyed (seed, episode, step of the episode, head)
    int vector_kernel;          // policy_act_kernel's arithmetic instead of policy_act16_kernel's (the choice ppo_rollout would make now)
    int64_t n_episodes, seed;
    const float* reset_table;   // CartPole: [n_episodes][4] = ppo_cartpole_reset_stream_h(seed, n_episodes); MountainCar: unused
    float* ep_return;           // [n_episodes]
    int32_t* ep_length;         // [n_episodes]
    int32_t* ep_trunc;          // [n_episodes] 1: the episode reached max_episode_steps
};
int eval_slots(const EvalArgs& a);   // episodes in flight (slot s runs episodes s, s + slots, ...)
hipError_t launch_evaluate(const EvalArgs& a, hipStream_t s);

// Caller-stepped environments (PPO_ENV_HOST; api.hip: ppo_host_*).  ppo_host_observe stages step t - 1's outputs of the caller's envs; the next
// launch COMMITS them (rewards / finished episodes of row t - 1, NEXT_DONE, NEXT_OBS, the per-env episode sums) and, in the act kernels, goes on to
// step t: OBS[t], DONES[t], MASKS[t], the actor forward + sample, ACTIONS[t], LOGPROBS[t] and the i64 actions where the host reads them.
struct HostStepArgs {
    const float* st_obs;        // [N,O] staged next observation (already the reset observation where done)
    const float* st_rew;        // [N]
    const int32_t* st_done;     // [N] (truncation included)
    const int32_t* st_fin_len;  // [N] length / reward of the episodes that finished (fin_given), else the context's running sums are used
    const float* st_fin_rew;
    int commit;                 // 1: step t - 1 is staged and not yet committed (0 at t = 0: the observation is NEXT_OBS)
    int fin_given;
    float* rewards_prev;        // REWARDS[t - 1], FIN_LEN[t - 1], FIN_REW[t - 1]
    int32_t* fin_len_prev;
    float* fin_rew_prev;
    int32_t* next_done;         // [N]
    float* next_obs;            // [N,O]
    int32_t* ep_len;            // [N] episode sums of the running episodes
    float* ep_rew;
    float* obs_t;               // OBS[t], DONES[t], MASKS[t] (null: not a masked policy), ACTIONS[t]; all null in the commit-only launch
    float* dones_t;
    uint8_t* masks_t;
    int32_t* actions_t;
    const float* st_rew_store;  // [N] or null: what the reward row receives in place of st_rew (reward normalisation); the episode sums always take st_rew
};
// commit + act of one step in ONE launch: rollout16_kernel's arithmetic (policy_act16_kernel) when as16 and the shape is one of its, else the vector
// form (policy_act_kernel).  mask: [N,A] of step t or null; action_h: i64 [N,H], device-visible host memory; logprob_t: LOGPROBS[t]
hipError_t launch_host_act(const float* params, const NetLayout& L, int dist_kind, const uint8_t* mask, int N, int64_t seed, int64_t env_offset,
                           int64_t step_index, const HostStepArgs& hs, int64_t* action_h, float* logprob_t, bool as16, int32_t* error_flag, hipStream_t s);
// commit only (ppo_host_rollout_end; the generic engine's per-step commit ahead of gen_forward)
hipError_t launch_host_commit(const HostStepArgs& hs, int N, int O, hipStream_t s);
// Env groups (ppo_host_rollout_begin_groups): group g owns rows [row0[g], row0[g + 1]) and steps through the rollout at its own pace.  A group's act launch
// is launch_host_act on the group's rows: every HostStepArgs pointer, the mask, the action block and logprob_t are offset to row row0[g] (and to the
// group's own step t_g), n = the group's row count and env_offset + row0[g] is the sampler's row origin -- the kernels index by row and a row's arithmetic
// does not depend on the tile or grid it sits in, so they run unchanged.  At the end of the rollout every group's last staged step is committed by ONE
// launch over all N rows; the only thing that differs between groups there is whether the caller passed the finished episodes' numbers (fin_given).
struct HostGroupTable {
    int n;                                       // groups, 1 .. PPO_HOST_MAX_GROUPS
    int32_t row0[PPO_HOST_MAX_GROUPS + 1];       // row0[0] = 0 < ... < row0[n] = N
    int32_t fin_given[PPO_HOST_MAX_GROUPS];
};
// hs: the whole context's rows at step T (commit = 1; fin_given is taken from the table)
hipError_t launch_host_commit_groups(const HostStepArgs& hs, const HostGroupTable& tab, int N, int O, hipStream_t s);
// Observation normalisation of caller-stepped envs (kernels_obsnorm.hip; ppo_obs_norm_* in ppo_hip.h).  stats: f64 [2 O] = mean[O] | var[O]; count: rows merged so far
// (kept by the host).  update_apply: Chan's merge of the batch src [N,O] into stats, then dst = clamp((src - mean) / sqrt(var + eps), +-clip) with the merged
// statistics, in one launch (dst may be src).  apply: the same map with the statistics as they stand; truncated / done non-null: only rows where both are
// non-zero are read and written.
hipError_t launch_obsnorm_update_apply(const float* src, float* dst, int64_t N, int O, double* stats, double count, float eps, float clip, hipStream_t s);
hipError_t launch_obsnorm_apply(const float* src, float* dst, int64_t N, int O, const double* stats, float eps, float clip, const int32_t* truncated,
                                const int32_t* done, hipStream_t s);
// Reward normalisation of caller-stepped envs (kernels_rewnorm.hip; ppo_reward_norm_* in ppo_hip.h).  ret: f64 [N] discounted-return accumulators;
// stats: f64 [2] = mean | var of the returns; count: returns merged so far (kept by the host).  update_apply: R = ret * gamma + rew, Chan's merge of the N
// values of R into stats, out = clamp(rew / sqrt(var + eps), +-clip) with the merged variance, ret = done ? 0 : R; one launch of one workgroup.  apply: the
// same map with the statistics as they stand.
hipError_t launch_rewnorm_update_apply(const float* rew, const int32_t* done, float* out, int64_t N, double* ret, double* stats, double count, float gamma,
                                       float eps, float clip, hipStream_t s);
hipError_t launch_rewnorm_apply(const float* rew, float* out, int64_t N, const double* stats, float eps, float clip, hipStream_t s);
// A whole rollout of a fused device env (PPO_KERNEL_ENV_REWARD_NORM), in place on rew [T, N] with done = (fin_len != 0): mode 1 leaves in rew, ret and stats
// the bits T launches of update_apply on rows 0 .. T - 1 would leave, in three launches whatever T is (the host advances its count by N per step, as there);
// mode 2 is the apply over all T N rewards, one launch.  ws: rewnorm_rollout_workspace(N, T) doubles of the context's own (mode 2 does not touch it).
size_t rewnorm_rollout_workspace(int64_t N, int T);
hipError_t launch_rewnorm_rollout(int mode, float* rew, const int32_t* fin_len, int64_t N, int T, double* ret, double* stats, double* ws, double count,
                                  float gamma, float eps, float clip, hipStream_t s);
hipError_t launch_categorical(int dist_kind, const float* logits, const uint8_t* mask, const int64_t* value, int64_t n, int A,
                              float* m_logits, float* m_probs, float* log_prob, float* entropy, int64_t* mode, hipStream_t s);

hipError_t launch_categorical_sample(const float* probs, int64_t n, int A, int64_t seed, int64_t row_offset, int64_t step_index, int head,
                                     int64_t* out, hipStream_t s);

// error_flag (may be null: the stateless entry points): device word that gets PPO_ERRFLAG_GAE_PROTOCOL when a bounded wait of the time-pipelined scan runs out
// (the affected strip's outputs are NaN either way)
hipError_t launch_gae(const float* rewards, const float* values, const float* dones, const float* next_value,
                      const int32_t* next_done, int64_t T, int64_t N, float gamma, float gae_lambda, float* adv, float* ret,
                      int32_t* error_flag, hipStream_t s);
hipError_t launch_gae_fast(const float* rewards, const float* values, const float* dones, const float* next_value,
                           const int32_t* next_done, int64_t T, int64_t N, float gamma, float gae_lambda, float* adv, float* ret,
                           hipStream_t s);
hipError_t launch_nstep(const float* rewards, const float* values, const float* dones, const float* next_value,
                        const int32_t* next_done, int64_t T, int64_t N, float gamma, float* adv, float* ret, int32_t* error_flag, hipStream_t s);

struct UpdateArgs {
    const float* params;
    NetLayout L;
    LossParams hp;
    // flattened batch views [B,...]
    const float* obs;
    const int32_t* actions;  // [B,H]
    const uint8_t* masks;    // [B,A] or null
    const float* logprobs;
    const float* advantages;
    const float* returns;
    const float* values;
    const float* rec_critic; // [B][8] packed sample records of the matrix-core kernel (launch_pack_records); the vector kernel reads the views above
    const float* rec_actor;  // [B][8]
    const int32_t* idx;      // [M]
    int M;                   // local minibatch rows
    double inv_global_M;     // 1 / (rows of the global minibatch)
    const AdvStat* adv_stat; // global sums for this minibatch (nullptr when !norm_adv)
    const float4* adv_norm;  // { mean, 1 / (std + 1e-8), std (Bessel), 0 } of this minibatch's advantages, formed ONCE per update from adv_stat (launch_adv_norm)
    double global_M;
    float* slab;             // [n_blocks, P_net_max] partial gradients
    double* stat_slab;       // [n_blocks, 8] partial loss sums
    int n_blocks[2];         // workgroups of the critic / of the actor; slab row = (net ? n_blocks[0] : 0) + workgroup
    unsigned long long* stamps;  // diagnostic build only: [2 nets][12 phases] cycle sums of wave 0 / workgroup 0
    int32_t* error_flag;     // the context's device error word (bit 0: reset table exhausted; PPO_ERRFLAG_UPDATE_PROTOCOL: a bounded wait of the wave-specialised update kernel ran out)
    int single_wave;         // 1: the one-wave-per-tile matrix-core kernel even for the reference's two shapes (A/B; ppo_config.kernel_flags)
};
// The update kernels' LEADING kernel parameters: copies of the UpdateArgs members at the head of their dependent chain (fetch_row's operands, the first
// record load, the weight staging's base), passed as scalars in front of the struct so that they are preloaded into SGPRs at wave launch (csrc/Makefile:
// kernel-argument preloading; a by-value struct never is).  4 pointers + 3 ints = 11 dwords.  The bodies take them as an UpdLead.
struct UpdLead { const int32_t* idx; const float* rec_critic; const float* rec_actor; const float* params; int M; int nb0; };
#define UPD_LEAD_PARAMS const int32_t* idx, const float* rec_critic, const float* rec_actor, const float* params, int M, int nb0, int nb1
#define UPD_LEAD_ARGS(a) (a).idx, (a).rec_critic, (a).rec_actor, (a).params, (a).M, (a).n_blocks[0], (a).n_blocks[1]
// UPD_LEAD_PARAMS as the kernel-argument segment lays them out, and where the struct behind them starts there.  kernels_update_mfma.hip holds the
// wave-specialised kernel's real signature to this image (a static_assert on its function type), so a leading parameter added or reordered in one place only
// does not compile.
struct UpdLeadImage { const int32_t* idx; const float* rec_critic; const float* rec_actor; const float* params; int M; int nb0; int nb1; };
constexpr size_t UPD_LEAD_DWORDS = (offsetof(UpdLeadImage, nb1) + sizeof(int)) / 4;
constexpr size_t UPD_ARGS_OFFSET = (UPD_LEAD_DWORDS * 4 + alignof(UpdateArgs) - 1) / alignof(UpdateArgs) * alignof(UpdateArgs);
constexpr int32_t PPO_ERRFLAG_UPDATE_PROTOCOL = 2;
constexpr int32_t PPO_ERRFLAG_GAE_PROTOCOL = 16;   // gae_pipe_kernel: a bounded wait between its mover waves and its walker ran out (that strip's advantages / returns are NaN)
constexpr int32_t PPO_ERRFLAG_UPDATE_RANGE = 8;    // a matrix-core update kernel met an observation that does not fit its fp16 operand (|obs| >= 65 504)
constexpr int32_t PPO_ERRFLAG_ROLLOUT_RANGE = 4;   // rollout16_kernel: |W3| does not fit the fp16 operand (pre-scaled by 2^8)
// NOT an error: the update's KL gate (kernels_earlystop.hip) found approx_kl above the context's target; raised and cleared inside one ppo_update, and
// masked out by every host-side reader of the word (PPO_ERRFLAG_NOT_ERRORS)
constexpr int32_t PPO_ERRFLAG_KL_STOP = 32;
constexpr int32_t PPO_ERRFLAG_NOT_ERRORS = PPO_ERRFLAG_KL_STOP;
constexpr int32_t PPO_ERRFLAG_SKIP_STEP = PPO_ERRFLAG_UPDATE_PROTOCOL | PPO_ERRFLAG_UPDATE_RANGE | PPO_ERRFLAG_GAE_PROTOCOL | PPO_ERRFLAG_KL_STOP;   // the optimizer does not apply a step behind these
int update_blocks_per_net(int M);
hipError_t launch_minibatch_fwd_bwd(const UpdateArgs& a, hipStream_t s);
// matrix-core version of the same kernel; sum(head_dims) <= 4, obs in {2, 4}: fp32 carried as two fp16 terms, three
// v_mfma_f32_32x32x16_f16 products per fp32 product (fp32 accuracy).  Gathers from the packed records.
void update_blocks_mfma(int M, int n_blocks[2]);
hipError_t launch_minibatch_fwd_bwd_mfma(const UpdateArgs& a, hipStream_t s);
hipError_t launch_pack_records(const NetLayout& L, const float* obs, const int32_t* actions, const uint8_t* masks, const float* logprobs,
                               const float* advantages, const float* returns, const float* values, int64_t B, float* rec_critic, float* rec_actor,
                               double* ev_sums, int32_t* error_flag, hipStream_t s);
// fp16 ranges of the matrix-core kernels of the 2 x 64 layout:
//   wr_dev[0..2] = the maxima of |parameter| by class -- [PPO_WR_W3] both nets' output layers (rollout16_kernel carries 2^8 W3 as fp16: |W3| < 255),
//   [PPO_WR_W2] both nets' hidden-to-hidden weights (the matrix-core update kernels carry c W2 and products through its columns as fp16 terms),
//   [PPO_WR_REST] everything else (c W1, c b1, ... < 65 504) -- as float bit patterns, recomputed from the parameters ONCE PER UPDATE by weight_range_kernel on a
//   stream of its own (api.hip: sweep_weight_range; no dependency on the update's stream, so it costs that stream nothing -- inside the AdamW kernel or the update
//   kernel's prologue the same few instructions cost 0.4 - 0.7 us per optimizer step, 1.5 % of the iteration, and as an extra workgroup of pack_records_kernel
//   7 us per update: the sweep's memory round trips and the write to the host were that kernel's tail) and, synchronously, after every host write of the parameters
//   (refresh_weight_range); wr_dev[4..6] mirrors what the pinned host words hold.  The HOST reads the mirror without synchronising, an update or two late --
//   AdamW moves a weight by about lr per step, hence thresholds at half the kernels' limits -- and takes the vector kernels for a launch whose weights do
//   not fit fp16 instead of failing.
// The optimizer kernels read the context's error word (OptGuard: one load that is in flight with the step's other loads) and do NOT apply a step the
// device already knows is garbage -- a bounded wait of the update kernel or of the scan ran out, or an observation left the fp16 range of the matrix-core
// update kernel (PPO_ERRFLAG_SKIP_STEP): parameters and moments stay as they were, the statistics are still written, the error stays sticky and
// ppo_read_stats reports it.  A gradient that is merely not finite is applied as the reference applies it (a 1-row minibatch gives NaN parameters there
// too, tests/test_gpu_parity.py): that is parity, not an error.
struct OptGuard {
    int32_t* error_flag = nullptr;
};
#ifdef __HIPCC__
// The error word as a VECTOR load: the address passes through a vector register the compiler cannot see through, so the load is issued in the same batch as
// the step's other vector loads and waited for with them.  Left to itself hipcc made it two DEPENDENT scalar loads (the pointer out of the kernel arguments,
// then the word) with a wait behind each at the very top of the kernel, in front of everything else: + 0.15 us on a 5 us launch (trace A/B, NOTES).
// error_flag is never null here: the launchers refuse a null word (no branch in the kernel: a branch made the compiler wait for the word on the spot).
__device__ __forceinline__ int32_t opt_guard_word(const int32_t* error_flag) {
    uintptr_t p = reinterpret_cast<uintptr_t>(error_flag);
    asm volatile("" : "+v"(p));
    return *reinterpret_cast<const __attribute__((address_space(1))) int32_t*>(p);
}
#endif
__device__ __forceinline__ int wr_class(const NetLayout& L, int p) {
    const bool w3 = (p >= L.w3[0] && p < L.b3[0]) || (p >= L.w3[1] && p < L.b3[1]);
    const bool w2 = (p >= L.w2[0] && p < L.b2[0]) || (p >= L.w2[1] && p < L.b2[1]);
    return w3 ? 0 : (w2 ? 1 : 2);
}
constexpr int PPO_WR_W3 = 0, PPO_WR_W2 = 1, PPO_WR_REST = 2;
// grads[p] = sum over blocks (fixed order); loss sums -> sums_out[8]
hipError_t launch_reduce_grads(const float* slab, const double* stat_slab, const int n_blocks[2], const NetLayout& L, float* grads,
                               double* sums_out, hipStream_t s);
hipError_t launch_clip_adamw(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const NetLayout& L, float max_grad_norm,
                             const AdamCoef* coef, const double* loss_sums, double global_M, LossParams hp, int world, bool do_step,
                             StepStats* stats_out, double* clipfrac_accum, double* norm2_scratch, hipStream_t s, OptGuard guard);
// Early stop at a target KL (ppo_target_kl_set; kernels_earlystop.hip).  The device's record of one update: the head is what the host reads (copied into a
// pinned EarlyStopHost behind the update's last launch), the tail what the unapplied steps overwrite.
struct EarlyStopHost {
    double kl_at_stop;       // approx_kl of the step that raised the stop (0 when none did)
    int64_t applied_total;   // optimizer steps applied so far, this update included
    int32_t epochs_run;      // epochs of this update whose steps were applied
    int32_t stopped;
};
struct EarlyStopDev : EarlyStopHost {
    StepStats saved;         // the statistics of the last applied step
    double cf[2];            // clipfrac_accum as that step left it
};
// behind the optimizer launch of the last minibatch of epoch `epoch`: step_stat = that step's statistics
hipError_t launch_kl_gate(const StepStats* step_stat, double target, int epoch, double* clipfrac_accum, int32_t* error_flag, EarlyStopDev* es, hipStream_t s);
// behind the update's last step: last_stat = the slot the host reads (ppo_ctx::last_stat_slot); applied_before = the applied steps before this update
hipError_t launch_kl_gate_end(StepStats* last_stat, double* clipfrac_accum, int32_t* error_flag, EarlyStopDev* es, int epochs, int n_mb, int64_t applied_before,
                              hipStream_t s);
// recomputes the three maxima of OptGuard from the parameters (after the host wrote them): wr_dev and wr_host both
hipError_t launch_weight_range(const float* params, const NetLayout& L, uint32_t* wr_dev, uint32_t* wr_host, hipStream_t s);
// partial-episode bootstrap (ppo_bootstrap_rewards): v = Critic(final_obs[k]), rewards[index[k]] += gamma * v (two roundings), value_out[k] = v (may be
// null), k < K; the critic arithmetic of launch_values_mfma (obs in {2, 4}) / launch_values (obs in {2, 4, 8}).  K <= 0: no launch.
hipError_t launch_bootstrap_values_mfma(const float* params, const NetLayout& L, const float* final_obs, const int32_t* index, int64_t K, float gamma,
                                        float* rewards, float* value_out, hipStream_t s);
hipError_t launch_bootstrap_values(const float* params, const NetLayout& L, const float* final_obs, const int32_t* index, int64_t K, float gamma,
                                   float* rewards, float* value_out, hipStream_t s);
// The same fold for caller-stepped envs that live on the device (ppo_dev_observe with truncation flags): nobody on the host knows how many rows of the
// step are flagged, so ONE launch over all N rows finds them.  A 256-thread workgroup owns env rows [256 b, 256 b + 256): every thread reads truncated[n]
// and done[n] of its row; a row counts when BOTH are non-zero (a flag on a row that is not done is ignored: the device call cannot refuse it without a
// host wait).  A workgroup without a flagged row ends there -- the common step: one pass over 2 N int32.  Otherwise the flagged rows are compacted inside
// the workgroup (wave ballot + mbcnt rank, the four waves' totals through LDS, the row list in LDS, ascending), the critic runs on those rows of
// final_obs only (other rows are never read: they may hold anything), and for each of them, i = t * N + n:
//   rewards[i] = f32(rewards[i] + f32(gamma * v));   (ev_index, ev_value)[base + k] = (i, v)
// base = ONE atomicAdd on *ev_count per workgroup that has events, k = the row's rank in the workgroup: the list's order across workgroups is arbitrary
// (ppo_host_truncations sorts it on the host; no result depends on it).  Entries at or beyond ev_cap are not stored (T * N holds a whole rollout).
struct DevFoldArgs {
    const int32_t* truncated;   // [N]     the caller's arrays of this step
    const int32_t* done;        // [N]
    const float* final_obs;     // [N,O]
    int N;
    int64_t tN;                 // t * N
    float gamma;
    float* rewards;             // PPO_BUF_REWARDS [T,N], step t committed by the launch in front
    int32_t* ev_count;          // the open rollout's event list
    int32_t* ev_index;
    float* ev_value;
    int64_t ev_cap;
};
constexpr int DEV_FOLD_THREADS = 256;
// The compaction every fold kernel shares (256 threads).  flag: this thread has a row to fold; item: what the list keeps for it.  list: LDS int [256], ascending
// by thread; wtot: LDS int [8] ([0..3] the waves' counts, [4] the workgroup's base in the event list); pos: the thread's place in the list (where flag).
// Returns the workgroup's number of flagged rows (the same in every thread; 0: nothing else was written, no atomic was issued).
__device__ __forceinline__ int fold_compact(bool flag, int item, int32_t* ev_count, int* list, int* wtot, int& pos) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) wtot[wave] = __popcll(b);
    __syncthreads();
    const int c0 = wtot[0], c1 = wtot[1], c2 = wtot[2], c3 = wtot[3];
    const int total = c0 + c1 + c2 + c3;
    pos = 0;
    if (total == 0) return 0;
    const int before = (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    pos = before + rank;
    if (flag) list[pos] = item;
    if (tid == 0) wtot[4] = atomicAdd(ev_count, total);
    __syncthreads();
    return total;
}
// the fold and the event record of one row (flat index i, value v, place e in the event list): one lane per row
__device__ __forceinline__ void fold_store(float* rewards, float gamma, int32_t* ev_index, float* ev_value, int64_t ev_cap, int64_t e, int64_t i, float v) {
    rewards[i] = __fadd_rn(rewards[i], __fmul_rn(gamma, v));
    if (e < ev_cap) { ev_index[e] = (int32_t)i; ev_value[e] = v; }
}
// The front end of the two ppo_dev_observe fold kernels: the flagged rows of the workgroup's 256 env rows.
__device__ __forceinline__ int dev_fold_compact(const DevFoldArgs& a, int* list, int* wtot) {
    const int64_t n = (int64_t)blockIdx.x * DEV_FOLD_THREADS + threadIdx.x;
    const bool flag = n < a.N && a.truncated[n] != 0 && a.done[n] != 0;
    int pos;
    return fold_compact(flag, (int)n, a.ev_count, list, wtot, pos);
}
// compacted row k (env row n, value v)
__device__ __forceinline__ void dev_fold_store(const DevFoldArgs& a, int base, int k, int n, float v) {
    fold_store(a.rewards, a.gamma, a.ev_index, a.ev_value, a.ev_cap, (int64_t)base + k, a.tN + n, v);
}
// the critic arithmetic of launch_bootstrap_values_mfma (obs in {2, 4}) / of launch_bootstrap_values (obs 8: the one shape ppo_bootstrap_rewards sends there)
hipError_t launch_dev_fold_mfma(const float* params, const NetLayout& L, const DevFoldArgs& a, hipStream_t s);
hipError_t launch_dev_fold(const float* params, const NetLayout& L, const DevFoldArgs& a, hipStream_t s);
// The same fold for the environments the library steps itself (ppo_env_truncation_bootstrap): ONE launch behind a rollout finds the episodes the time
// limit cut off -- FIN_LEN[i] == max_episode_steps, i = t * N + n -- and recomputes their last transition from what the rollout stored: for CartPole and
// MountainCar the observation IS the env state, so the final observation is env_step of OBS[i] under ACTIONS[i, 0].  Where the env itself terminated on
// that step the end is real and nothing happens; elsewhere v = Critic(final observation) is folded into REWARDS[i] and (i, v) joins the event list, as above.
struct EnvFoldArgs {
    const float* obs;           // PPO_BUF_OBS [B,O]
    const int32_t* actions;     // PPO_BUF_ACTIONS [B,H]
    const int32_t* fin_len;     // PPO_BUF_FIN_LEN [B]
    int64_t B;                  // T * N
    int H;
    int env_kind;
    int max_episode_steps;      // > 0
    float gamma;
    float* rewards;             // PPO_BUF_REWARDS [B]
    int32_t* ev_count;          // the context's event list, cleared in front of the launch
    int32_t* ev_index;
    float* ev_value;
    int64_t ev_cap;
};
// the critic arithmetic of launch_values_mfma, which fills PPO_BUF_VALUES for both envs (obs 4 and 2)
hipError_t launch_env_trunc_fold_mfma(const float* params, const NetLayout& L, const EnvFoldArgs& a, hipStream_t s);
// batched critic on the matrix cores (obs in {2, 4}); same contract as launch_values
hipError_t launch_values_mfma(const float* params, const NetLayout& L, const float* obs0, int64_t n0, float* out0, const float* obs1, int64_t n1,
                              float* out1, hipStream_t s);
// single-rank optimizer step: (slab reduction + per-workgroup sums of squares) then (norm from the partials + clip + AdamW)
int fused_opt_blocks(const NetLayout& L);
hipError_t launch_reduce_clip_adamw(const float* slab, const double* stat_slab, const int n_blocks[2], const NetLayout& L, float* grads,
                                    double* sums_out, float* params, float* exp_avg, float* exp_avg_sq, float max_grad_norm,
                                    const AdamCoef* coef, double global_M, LossParams hp, StepStats* stats_out, double* clipfrac_accum,
                                    double* partial, hipStream_t s, OptGuard guard);
hipError_t launch_reduce_exchange_clip_adamw(const float* slab, const double* stat_slab, const int n_blocks[2], const NetLayout& L, float* grads,
                                             double* sums_out, float* params, float* exp_avg, float* exp_avg_sq, float max_grad_norm, const AdamCoef* coef,
                                             double global_M, const LossParams& hp, StepStats* stats_out, double* clipfrac_accum, double* partial,
                                             void* const* peers, int rank, int n_ranks, size_t slot_bytes, uint64_t seq, int32_t* timeout_flag,
                                             hipStream_t s, OptGuard guard);
// Device-resident CircularBuffer(100) of finished episodes (reference Utils/Utils.h:30-79).
struct EpisodeRing {
    float rew[100];
    int32_t len[100];
    int32_t size, head;
    int64_t total;
    int64_t key[100];   // (absolute rollout step) * global_num_envs + global env index: the episode's position in the reference's push order
};
hipError_t launch_episode_ring_update(const int32_t* fin_len, const float* fin_rew, int T, int N, int32_t* row_counts, uint64_t* group_bits,
                                      EpisodeRing* ring, int64_t step_base, int64_t global_num_envs, int64_t env_offset, hipStream_t s);
// The same two jobs as workgroups of the rollout's critic launch (kernels_update_mfma.hip: values_ring_mfma_kernel): launch_episode_ring_update's arguments
// and `ticket`, one device word that is 0 between launches.  The T count workgroups each take a ticket behind their row; the one that draws the last does
// the push.  Nobody waits for anybody.
struct RingFuseArgs {
    const int32_t* fin_len;
    const float* fin_rew;
    int32_t* row_counts;
    uint64_t* group_bits;
    EpisodeRing* ring;
    unsigned int* ticket;
    int64_t step_base, global_num_envs, env_offset;
};
// launch_values_mfma over [T * N rows of obs0 | N rows of obs1] and launch_episode_ring_update(T, N) in ONE launch: workgroups [0, T) count a step row each
// (the push's serial walk is the longest chain of the launch, so its feeders start first), the rest run the critic's tiles with the block index and grid
// size launch_values_mfma gives them -- the values are that launch's, bit for bit.  The critic keeps the vector ALUs busy for ~24 us (4096 x 128); the
// ring's 20 us are one round trip and ONE wave walking rows, and hide behind it.
hipError_t launch_values_ring_mfma(const float* params, const NetLayout& L, const float* obs0, float* out0, const float* obs1, float* out1, int T, int N,
                                   const RingFuseArgs& r, hipStream_t s);
// launch_rollout with `ring`: its critic launch is launch_values_ring_mfma, and the rollout's finished episodes are in the ring behind it
hipError_t launch_rollout(const RolloutArgs& a, hipStream_t s, const RingFuseArgs* ring);
// launch_pack_records and launch_permutations_adv_stats in ONE launch (kernels_update_mfma.hip: pack_perm_stats_kernel): both need only the scan's output;
// the pack streams 64 B per sample with idle ALUs, the permutations are integer mixing and a cache-resident gather.  Workgroups [0, E * per_epoch *
// PPO_ADV_PARTS) form the permutations and the advantage sums with perm_adv_stats_kernel's (minibatch, part) -> element mapping, the next PPO_EV_BLOCKS pack
// with pack_records_kernel's grid-stride mapping; every sum keeps its order.  norm_out != nullptr (a context that is not sharded): the permutation
// workgroup that finishes last also does launch_adv_norm's job for all slots (the partial sums in order, in binary64) and clears zero2 -- `ticket` is its
// device word, 0 between launches.  norm_out == nullptr: the caller all-reduces the sums and launches launch_adv_norm.
struct PackPermArgs {
    // pack_records_kernel's
    const int32_t* actions; int n_heads; const uint8_t* masks; int A;
    const float* logprobs; const float* returns; const float* values;
    float4* rec_critic; float4* rec_actor; double* ev_out; int32_t* error_flag;
    // perm_adv_stats_kernel's
    int64_t update_index, rank_salt;
    AdvStat* stat_out;
    // adv_norm_kernel's
    int n_slots; float4* norm_out; double* zero2; unsigned int* ticket;
};
hipError_t launch_pack_perm_stats(const NetLayout& L, const float* obs, const float* advantages, int32_t* perm, int64_t B, int E, int64_t MB, int64_t seed,
                                  const PackPermArgs& a, hipStream_t s);
// this rank's contribution to the job-global statistics block (PPO_GSTAT_*): zeroes the block, then writes the head and the rank's own slot
hipError_t launch_gstats_pack(const double* ev_sums, const EpisodeRing* ring, int rank, double* gstats, hipStream_t s);
hipError_t launch_adv_stats(const float* advantages, const int32_t* perm, int64_t B, int64_t MB, int n_mb_total, AdvStat* out,
                            hipStream_t s);
hipError_t launch_permutations(int32_t* perm, int64_t B, int E, int64_t seed, int64_t update_index, int64_t rank_salt, hipStream_t s);
// the two above in one pass (ppo_update with norm_adv): perm[e][j] and the advantage sums of every minibatch of the update
// { mean, 1 / (std + 1e-8), std, 0 } of the advantages of minibatch slots [0, n) from their PPO_ADV_PARTS partial sums (PPO_Discrete.cpp:591-594); slot k is
// minibatch k % per_epoch of an epoch (rows min(MB, B - start) x world), or explicit_M x world rows when explicit_M > 0
// zero2 != nullptr: the launch also clears those two doubles (the update's clip-fraction accumulator)
hipError_t launch_adv_norm(const AdvStat* stats, int n, int per_epoch, int64_t B, int64_t MB, int64_t explicit_M, int world, float4* out, hipStream_t s, double* zero2 = nullptr);
hipError_t launch_permutations_adv_stats(const float* advantages, int32_t* perm, int64_t B, int E, int64_t MB, int64_t seed, int64_t update_index,
                                         int64_t rank_salt, AdvStat* out, hipStream_t s);
hipError_t launch_explained_variance(const float* returns, const float* values, int64_t B, double* sums4, hipStream_t s);
hipError_t launch_orthogonal_init(float* params, const NetLayout& L, int64_t seed, hipStream_t s);
