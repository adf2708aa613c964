/* include/ppo_hip.h -- C-ABI of libppo_hip.so: the MI355X (gfx950) PPO rollout-buffer hot path.
 *
 * The reference (AidanShipperley/PPO-LibTorch) has no plugin/FFI boundary: its "API" is a set of C++ classes
 * whose methods exchange torch::Tensor (PPO/PPO_Discrete.h:24-108, PPO/Agent.h:22-54, the Distributions and
 * Environments headers).  This header is the boundary a maintainer would bind instead of LibTorch for that path:
 * plain pointers and sizes, int32 status codes, no exceptions, no torch types.  Every entry point cites the
 * reference interface (file:line, relative to the reference root) it replaces.  The C++ classes with the
 * reference's names (ppo-libtorch_amd/host/) and the Python ctypes binding (ppo-libtorch_amd/binding.py) sit on
 * top of exactly these symbols; INTEGRATION.md shows the stub.
 *
 * Conventions
 *  - All bulk pointers are DEVICE pointers unless the parameter name ends in _h (host).  Callers without a HIP
 *    runtime of their own use ppo_device_alloc / ppo_memcpy_h2d / ppo_memcpy_d2h.
 *  - Work is enqueued on the context's stream (ppo_stream); functions return after enqueueing unless stated.
 *  - Rollout buffers are TIME-MAJOR [T, N, ...] exactly like the reference's m_obs/m_rewards/... tensors
 *    (PPO_Discrete.cpp:90-95), env index contiguous.
 *  - Status 0 = PPO_OK; on failure ppo_last_error() describes it.  Nothing throws across this ABI.
 */
#ifndef PPO_HIP_H
#define PPO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPO_MAX_HEADS 8
#define PPO_API __attribute__((visibility("default")))
#define PPO_ABI_VERSION 5

typedef int32_t ppo_status;
enum { PPO_OK = 0, PPO_ERR_INVALID = 1, PPO_ERR_HIP = 2, PPO_ERR_STATE = 3, PPO_ERR_COMM = 4, PPO_ERR_UNSUPPORTED = 5 };

/* PPO_ENV_SYNTHETIC: the synthetic env of BASELINE configs[4] (obs ~ N(0,1) of any width, reward ~ U(-1,1), done ~ Bernoulli(0.01), random
 * action masks); it is the env with which networks other than the reference's 2 x 64 (hidden / n_hidden) are accepted. */
/* PPO_ENV_HOST: the CALLER owns the environments and steps them on the host (the reference's custom-environment framework: any class with reset(),
 * step(action), episode_length and episode_reward in PPO_Discrete::m_envs, PPO_Discrete.cpp:365-483); the context owns everything else.  Driven by the
 * ppo_host_* calls ("Caller-stepped environments" below); ppo_rollout / ppo_train_iteration / ppo_env_reset / ppo_env_step return PPO_ERR_UNSUPPORTED.
 * obs_size is not checked against any env.  The reference's network (2 x 64, f32) with obs_size 2, 4 or 8 runs on the reference-shape kernels, every
 * other network (and compute_dtype) on the generic engine with PPO_ENV_SYNTHETIC's limits. */
/* PPO_ENV_PENDULUM (new; the reference has no continuous-action env): gymnasium's Pendulum-v1 on the device, the env of the Gaussian policy's fused rollout.
 * State (theta, theta_dot) f32 -- PPO_BUF_ENV_STATE is [2, N], ppo_env_set_state_h / ppo_env_get_state_h take [N, 2] -- observation
 * (cos theta, sin theta, theta_dot), obs_size 3, one real-valued action.  One step with the RAW action a, every operation rounded on its own:
 *   u      = min(max(a, -2), 2)
 *   x      = theta + PI_F;  thn = (x - TWO_PI_F * floorf(x / TWO_PI_F)) - PI_F                      (gym's angle_normalize; PI_F = (float)pi, TWO_PI_F = (float)(2 pi))
 *   reward = -((thn * thn + 0.1f * (theta_dot * theta_dot)) + 0.001f * (u * u))
 *   td'    = theta_dot + (15.0f * sinf(theta) + 3.0f * u) * 0.05f;  td' = min(max(td', -8), 8)
 *   th'    = theta + td' * 0.05f                                                                     (not wrapped, as in gym)
 *   obs'   = (cosf(th'), sinf(th'), td');  terminated = 0 always
 * with sinf / cosf the library's own device functions (glibc 2.35's sinf / cosf, bit for bit).  Only the env's copy of the action is clipped: PPO_BUF_ACTIONS
 * keeps the raw sample, whose log-prob is the stored one (PPO_DIST_GAUSSIAN's rule below: the rollout never clips what it stores).  An episode ends only when its length reaches max_episode_steps
 * (done = 1, FIN_LEN / FIN_REW written, auto-reset: ppo_env_step's bookkeeping).  Reset number k of global env e: w = philox4x32_10(seed; e, k, 0, 1),
 * theta = uniform(w.x, -PI_F, PI_F), theta_dot = uniform(w.y, -1, 1) (MountainCar's keying and uniform mapping); PPO_BUF_RESET_COUNT counts them.
 * ppo_ctx_create accepts the env in exactly one form: dist_kind = PPO_DIST_GAUSSIAN, n_heads = 1, head_dims[0] = 1, obs_size = 3, hidden = 64,
 * n_hidden = 2, PPO_DTYPE_F32, kernel_flags containing PPO_KERNEL_GAUSS_FUSED (required, never implied: another engine never serves in the flag's place)
 * and 1 <= max_episode_steps <= 290 (theta is not wrapped and moves by at most 0.4 a step; the device sinf / cosf are glibc's for |theta| < 120).  A wrong
 * obs_size returns PPO_ERR_INVALID with the reference's obs-size message, anything else PPO_ERR_UNSUPPORTED with a message that names the limit.
 * Calls: ppo_env_reset, ppo_env_set_state_h / ppo_env_get_state_h, ppo_rollout(ctx, NULL) / ppo_rollout_f32, ppo_env_step_f32, ppo_env_transition_f32,
 * ppo_calc_advantage, ppo_update, ppo_train_iteration, ppo_policy_act_f32, ppo_get_value, ppo_target_kl_set, the statistics and profile calls,
 * ppo_gauss_fused_launches.  ppo_rollout is THREE launches: gauss_rollout_kernel (all T steps; a workgroup of 256 threads owns 64 envs for the whole rollout,
 * the actor's weights resident in LDS) and the critic over the T * N stored observations and over NEXT_OBS; a stepwise loop of ppo_policy_act_f32(obs,
 * step_index = rollout_steps + t) and ppo_env_step_f32 reproduces every buffer it fills bit for bit (tests/test_gpu_pendulum.py).
 * Refused, each with its reason, changing nothing: the ppo_host_* / ppo_dev_* calls (PPO_ERR_STATE, as on any device-env context); ppo_evaluate
 * (PPO_ERR_UNSUPPORTED: step episodes through ppo_policy_act_f32 with greedy = 1 and ppo_env_transition_f32); ppo_env_truncation_bootstrap
 * (PPO_ERR_UNSUPPORTED: its fold rebuilds the final observation from PPO_BUF_OBS, and a Pendulum observation does not hold theta); ppo_obs_norm_* and
 * ppo_reward_norm_* (PPO_ERR_UNSUPPORTED, as on every device env); ppo_env_step and ppo_rollout with an i64 array (PPO_ERR_UNSUPPORTED, naming the _f32 call).
 * With PPO_KERNEL_ENV_CUT_STATE in kernel_flags (below) the rollout keeps theta and theta_dot of every cut-off episode, and ppo_env_truncation_bootstrap and
 * ppo_env_truncations are served from that record (cut_state_fold_kernel); without the flag the refusal above stands, word for word.
 * Sharding (ppo_comm_init*) is neither claimed nor tested for this env. */
/* PPO_ENV_MOUNTAINCAR_CONTINUOUS (new; value 5): gymnasium's MountainCarContinuous-v0 on the device, the second env of the Gaussian policy's fused rollout and
 * the sibling of PPO_ENV_MOUNTAINCAR: the same track, the same reset, one cosine per step.  State (position p, velocity v) f32, and the observation IS the
 * state: obs_size 2, PPO_BUF_ENV_STATE is [2, N], ppo_env_set_state_h / ppo_env_get_state_h take [N, 2].  One real-valued action.  One step with the RAW
 * action a, every operation rounded on its own, in this association:
 *   u   = min(max(a, -1), 1)
 *   v'  = v + (u * 0.0015f - 0.0025f * cosf(3.0f * p));   v' = min(max(v', -0.07f), 0.07f)
 *   p'  = p + v';                                          p' = min(max(p', -1.2f), 0.6f)
 *   if (p' == -1.2f && v' < 0) v' = 0
 *   terminated = (p' >= 0.45f && v' >= 0.0f)
 *   reward = (terminated ? 100.0f : 0.0f) - 0.1f * (a * a)                                          (the RAW action, as gym's math.pow(action[0], 2))
 * with cosf the library's own device function (glibc 2.35's cosf, bit for bit; its argument stays within [-3.6, 1.8]).  Only the env's copy of the action is
 * clipped: PPO_BUF_ACTIONS keeps the raw sample.  An episode ends where the env terminates or its length reaches max_episode_steps (any value >= 1; gym: 999):
 * done = 1, FIN_LEN / FIN_REW written, auto-reset -- ppo_env_step's bookkeeping.  Reset number k of global env e is MountainCar's own:
 * p = uniform(philox4x32_10(seed; e, k, 0, 1).x, -0.6, -0.4), v = 0; global env 0 takes reset 1 at ppo_env_reset; PPO_BUF_RESET_COUNT counts them.
 * ppo_ctx_create accepts the env in exactly one form: dist_kind = PPO_DIST_GAUSSIAN, n_heads = 1, head_dims[0] = 1, obs_size = 2, hidden = 64, n_hidden = 2,
 * PPO_DTYPE_F32, kernel_flags containing PPO_KERNEL_GAUSS_FUSED (required, never implied) and max_episode_steps >= 1.  A wrong obs_size returns
 * PPO_ERR_INVALID with the reference's obs-size message, anything else PPO_ERR_UNSUPPORTED with a message that names the limit.
 * Calls: those of PPO_ENV_PENDULUM (above; ppo_env_transition_f32 with state_in [n, 2], action [n, 1], obs_out [n, 2] = the next state or NULL, and
 * `terminated` as the step computes it), and -- because a stored observation is enough to step from -- ppo_env_truncation_bootstrap, ppo_env_truncations and
 * ppo_evaluate.  ppo_rollout is THREE launches, as for Pendulum -- the same kernel, gauss_rollout_kernel, instantiated for this env -- and a stepwise loop of
 * ppo_policy_act_f32(obs, step_index = rollout_steps + t) and ppo_env_step_f32 reproduces every buffer bit for bit
 * (tests/test_gpu_mountaincar_continuous.py); with ppo_env_truncation_bootstrap on, a fourth launch folds the cut-off episodes (below).
 * Refused exactly as on Pendulum, changing nothing: ppo_host_* / ppo_dev_* (PPO_ERR_STATE); ppo_obs_norm_* and ppo_reward_norm_* (PPO_ERR_UNSUPPORTED);
 * ppo_env_step, ppo_rollout with an i64 array and ppo_policy_act (PPO_ERR_UNSUPPORTED, naming the _f32 twin).
 * Which fold: without PPO_KERNEL_ENV_CUT_STATE gauss_trunc_fold_kernel, from PPO_BUF_OBS and the stored action; with the flag cut_state_fold_kernel, from the
 * kept state -- the same events and the same rewards, bit for bit (tests/test_gpu_cut_state.py holds the two against each other).
 * Sharding (ppo_comm_init*) is neither claimed nor tested for this env. */
/* PPO_ENV_ACROBOT (new; value 6): gymnasium's Acrobot-v1 on the device ("book" dynamics, no torque noise), the first device env of the fused 2 x 64 family
 * with a categorical policy.  State (theta1, theta2, w1, w2) f32 -- PPO_BUF_ENV_STATE is [4, N], ppo_env_set_state_h / ppo_env_get_state_h take [N, 4] --
 * observation (cos th1, sin th1, cos th2, sin th2, w1, w2), obs_size 6, which is NOT the state.  Action a in {0, 1, 2}, torque tau = (float)a - 1.0f.
 * One step, every operation rounded to f32 on its own, in exactly this association (PI_F = (float)pi, TWO_PI_F = (float)(2 pi), HALF_PI_F = (float)(pi / 2);
 * m1 = m2 = l1 = 1, lc1 = lc2 = 0.5, I1 = I2 = 1, g = 9.8, dt = 0.2, products of the constants folded: 4.9f = m2 lc2 g, 14.7f = (m1 lc1 + m2 l1) g):
 *   dsdt(th1, th2, w1, w2):
 *     c2   = cosr(th2);  s2 = sinr(th2)
 *     d1   = (0.25f + (1.25f + c2)) + 2.0f                            (m1 lc1^2 + m2 (l1^2 + lc2^2 + 2 l1 lc2 cos th2) + I1 + I2)
 *     d2   = (0.25f + 0.5f * c2) + 1.0f                               (m2 (lc2^2 + l1 lc2 cos th2) + I2)
 *     phi2 = 4.9f * cosr((th1 + th2) - HALF_PI_F)
 *     phi1 = (((-0.5f * (w2 * w2)) * s2 - (w2 * w1) * s2) + 14.7f * cosr(th1 - HALF_PI_F)) + phi2
 *     dw2  = (((tau + (d2 / d1) * phi1) - (0.5f * (w1 * w1)) * s2) - phi2) / (1.25f - (d2 * d2) / d1)
 *     dw1  = -(d2 * dw2 + phi1) / d1
 *     dsdt = (w1, w2, dw1, dw2)
 *   one classical RK4 step: k1 = dsdt(s), k2 = dsdt(s + 0.1f * k1), k3 = dsdt(s + 0.1f * k2), k4 = dsdt(s + 0.2f * k3)   (component by component)
 *     s'   = s + DT6 * (((k1 + 2.0f * k2) + 2.0f * k3) + k4),  DT6 = (float)(0.2 / 6)
 *   th1', th2': while (x > PI_F) x -= TWO_PI_F; while (x < -PI_F) x += TWO_PI_F          (gym's wrap; each loop gives up after 1024 turns, which no finite
 *                                                                                          state of the box below comes near: a non-finite input cannot hang)
 *   w1' = min(max(w1', -W1MAX), W1MAX), W1MAX = (float)(4 pi);  w2' likewise with W2MAX = (float)(9 pi)
 *   terminated = ((-cosr(th1')) - cosr(th2' + th1') > 1.0f);  reward = terminated ? 0.0f : -1.0f
 *   obs' = (cosr(th1'), sinr(th1'), cosr(th2'), sinr(th2'), w1', w2')
 * sinr / cosr, the trigonometric range: the library's device sinf / cosf (glibc 2.35's, bit for bit) hold for |x| < 120, and the RK4 stage angles leave that
 * range in the corners of the state box [-pi, pi]^2 x [-4 pi, 4 pi] x [-9 pi, 9 pi] (raw stage velocities reach ~2000 rad/s there).  So
 *   sinr(x) = |x| < 64.0f ? sinf(x) : sinf((float)((double)x - TWO_PI_D * rint((double)x / TWO_PI_D))),  TWO_PI_D = 2 pi in binary64
 * and cosr likewise: a large argument is reduced in binary64 (one division, one rint, one multiply, one subtraction, each rounded on its own), rounded to f32,
 * and handed to the same function.  Below 64 nothing changes.  The step is finite and inside the box for every state of the box.
 * An episode ends where the env terminates or its length reaches max_episode_steps (any value >= 1; gym: 500): done = 1, FIN_LEN / FIN_REW written,
 * auto-reset -- ppo_env_step's bookkeeping.  Reset number k of global env e: w = philox4x32_10(seed; e, k, 0, 1), (th1, th2, w1, w2) =
 * uniform(w.x | w.y | w.z | w.w, -0.1f, 0.1f) (MountainCar's keying and uniform mapping); global env 0 takes reset 1 at ppo_env_reset; PPO_BUF_RESET_COUNT
 * counts them.
 * ppo_ctx_create accepts the env in exactly one form: dist_kind = PPO_DIST_CATEGORICAL, n_heads = 1, head_dims[0] = 3, obs_size = 6, hidden = 64,
 * n_hidden = 2, PPO_DTYPE_F32, kernel_flags containing PPO_KERNEL_CAT_FUSED (required, never implied) and max_episode_steps >= 1.  A wrong obs_size returns
 * PPO_ERR_INVALID with the reference's obs-size message, anything else PPO_ERR_UNSUPPORTED with a message that names the limit.  The context lives in the
 * generic engine's layout, like a PPO_ENV_HOST context with PPO_KERNEL_CAT_FUSED.
 * Calls: ppo_env_reset, ppo_env_set_state_h (refills NEXT_OBS from the state) / ppo_env_get_state_h, ppo_env_step (action i64 [N, 1], obs [N, 6]),
 * ppo_env_transition(6, state [n, 4], action i64 [n], ...; the observation of a state comes from ppo_env_set_state_h, which refills PPO_BUF_NEXT_OBS -- no
 * symbol was added for it: the exported set stays at 92), ppo_rollout (forced i64 [T, N, 1] or NULL), ppo_calc_advantage, ppo_update,
 * ppo_train_iteration, ppo_policy_act, ppo_policy_act_greedy, ppo_get_value, ppo_target_kl_set, ppo_evaluate, the statistics and profile calls,
 * ppo_gauss_fused_launches.  ppo_rollout is THREE launches: cat_rollout_kernel (all T steps; a workgroup of 256 threads owns 64 envs for the whole rollout,
 * the actor's weights resident in LDS; PPO_BUF_MASKS is filled with ones, as a host-fed PPO_KERNEL_CAT_FUSED context without a mask holds it) and the critic
 * over the T * N stored observations and over NEXT_OBS: `value` moves by 2, `act` by 0.  A stepwise loop of ppo_policy_act(obs, step_index = rollout_steps + t)
 * and ppo_env_step reproduces every buffer it fills bit for bit (tests/test_gpu_acrobot.py).  ppo_evaluate is ONE launch (cat_eval_kernel) and moves no counter.
 * Refused, each with its reason, changing nothing: ppo_host_* / ppo_dev_* (PPO_ERR_STATE, as on any device env); ppo_obs_norm_* and ppo_reward_norm_*
 * (PPO_ERR_UNSUPPORTED); ppo_env_step_f32, ppo_rollout_f32, ppo_policy_act_f32 (PPO_ERR_UNSUPPORTED, naming the integer twin);
 * ppo_env_truncation_bootstrap and ppo_env_truncations (PPO_ERR_UNSUPPORTED: the fold rebuilds the final observation of a cut-off episode from PPO_BUF_OBS,
 * and an Acrobot observation does not hold the angles).  With PPO_KERNEL_ENV_CUT_STATE in kernel_flags (below) the rollout keeps the four state words of
 * every cut-off episode, and the two calls are served from that record (cut_state_fold_kernel); without the flag the refusal stands, word for word.
 * Sharding (ppo_comm_init*) is neither claimed nor tested for this env. */
enum { PPO_ENV_CARTPOLE = 0, PPO_ENV_MOUNTAINCAR = 1, PPO_ENV_SYNTHETIC = 2, PPO_ENV_HOST = 3, PPO_ENV_PENDULUM = 4, PPO_ENV_MOUNTAINCAR_CONTINUOUS = 5 };
enum { PPO_ENV_ACROBOT = PPO_ENV_MOUNTAINCAR_CONTINUOUS + 1 };   /* 6: the next env_kind, in an enum of its own -- the list above is kept as it was published */
/* PPO_ENV_TAXI (new; value 8): gymnasium's Taxi-v3 on the device (no rain, no fickle passenger), the first device env whose action mask means something:
 * the env of PPO_DIST_MASKED on the fused 2 x 64 family.  Every quantity is a small integer, held exactly in f32; nothing below rounds.
 * State (row, col, pass, dest): row, col in 0..4; pass in 0..4 (0..3: the passenger waits at stand R, G, Y, B; 4: in the taxi); dest in 0..3.
 * PPO_BUF_ENV_STATE is f32 [4, N]; ppo_env_set_state_h / ppo_env_get_state_h take [N, 4].
 * Stands, as (row, col): R = (0,0), G = (0,4), Y = (4,0), B = (4,3).
 * Walls: a move east from (r, c) is blocked when c == 4, or r in {0,1} and c == 1, or r in {3,4} and c in {0,2}; a move west from (r, c) is blocked when
 * c == 0 or east from (r, c-1) is blocked.
 * Step under action a, starting from reward -1 and terminated 0:
 *   0 south:   row = min(row+1, 4)
 *   1 north:   row = max(row-1, 0)
 *   2 east / 3 west: move one column unless blocked
 *   4 pickup:  if pass < 4 and the taxi stands on stand `pass`: pass = 4; else reward -10
 *   5 dropoff: if pass == 4 and the taxi stands on stand `dest`: pass = dest, terminated 1, reward +20;
 *              else if pass == 4 and the taxi stands on any stand s: pass = s; else reward -10
 * Any action in 0..5 is legal for the env, masked or not; an action outside 0..5 is clamped into 0..5.
 * Mask (u8, 6 wide): [row < 4, row > 0, !east_blocked, !west_blocked, pass < 4 && on stand pass, pass == 4 && on a stand] -- an action is allowed exactly
 * when it changes the state (all 500 x 6 pairs: tests/test_taxi_cpu.py).  A mask is never empty (south or north is always allowed).  Allowed bits per
 * action over the 500 states: 400, 400, 280, 280, 16, 16.
 * Observation, obs_size 19: four one-hot groups of 0.0f / 1.0f -- row in [0..4], col in [5..9], pass in [10..14], dest in [15..18].  It is not the state,
 * but the state is recoverable from it: the index of the largest entry of each group, the first index on ties.
 * Reset number k of global env e: w = philox4x32_10(seed; e, k, 0, 1) (MountainCar's keying); cell = (uint64(w.x) * 25) >> 32, row = cell / 5,
 * col = cell % 5; pass = (uint64(w.y) * 4) >> 32; d = (uint64(w.z) * 3) >> 32, dest = d + (d >= pass): uniform over gymnasium's 300 start states (passenger
 * waiting, not at the destination).  Global env 0 takes reset 1 at ppo_env_reset; PPO_BUF_RESET_COUNT counts them.
 * An episode ends where the env terminates or its length reaches max_episode_steps (any value >= 1; gym: 200): done = 1, FIN_LEN / FIN_REW written,
 * auto-reset -- ppo_env_step's bookkeeping.  Returns are integer sums, exact in f32.
 * Memory safety: ppo_env_set_state_h checks the host array -- a component that is not an integer of its range returns PPO_ERR_INVALID and changes nothing;
 * the device functions convert and clamp each component into its range (ppo_env_transition on device arrays cannot be checked without a host wait).
 * ppo_ctx_create accepts the env in exactly these forms: dist_kind = PPO_DIST_MASKED or PPO_DIST_CATEGORICAL, n_heads = 1, head_dims[0] = 6, obs_size = 19,
 * hidden = 64, n_hidden = 2, PPO_DTYPE_F32, kernel_flags containing PPO_KERNEL_CAT_FUSED (required, never implied) and max_episode_steps >= 1.  A wrong
 * obs_size returns PPO_ERR_INVALID with the reference's obs-size message, anything else PPO_ERR_UNSUPPORTED with a message that names the limit.  The context
 * lives in the generic engine's layout, as a PPO_ENV_ACROBOT context does.
 * Calls: PPO_ENV_ACROBOT's list -- ppo_env_reset, ppo_env_set_state_h (refills NEXT_OBS) / ppo_env_get_state_h, ppo_env_step (action i64 [N, 1], obs
 * [N, 19]), ppo_env_transition(8, state [n, 4], action i64 [n], ...), ppo_rollout (forced i64 [T, N, 1] or NULL), ppo_calc_advantage, ppo_update,
 * ppo_train_iteration, ppo_policy_act / ppo_policy_act_greedy (the caller passes the mask, as on any masked context), ppo_get_value, ppo_target_kl_set,
 * ppo_evaluate, the statistics and profile calls, ppo_gauss_fused_launches -- plus ppo_env_truncation_bootstrap and ppo_env_truncations.
 * PPO_BUF_MASKS (u8 [T, N, 6]): under PPO_DIST_MASKED the env's mask of the state each action was drawn in, formed on the chip (ppo_update reads it); under
 * PPO_DIST_CATEGORICAL ones (Acrobot's rule) and the policy is unmasked -- the A/B partner that shows what the mask is worth.
 * ppo_rollout is THREE launches, as on Acrobot (cat_rollout_kernel, LDS 67 136 bytes; `value` moves by 2, `act` by 0); a stepwise loop of
 * ppo_policy_act(obs, mask, step_index = rollout_steps + t) and ppo_env_step reproduces every buffer it fills bit for bit, PPO_BUF_MASKS included
 * (tests/test_gpu_taxi.py).  With ppo_env_truncation_bootstrap on, ONE more launch follows the two critic launches (cat_trunc_fold_kernel: the state of a
 * cut-off episode's last step is decoded from PPO_BUF_OBS, stepped again under the stored action, and the critic's value of the final observation is folded
 * into the reward); it is none of the launches ppo_gauss_fused_launches counts.  ppo_evaluate is ONE launch (cat_eval_kernel; under PPO_DIST_MASKED greedy is
 * the first-index argmax of the masked probabilities) and moves no counter.
 * Refused, changing nothing, with Acrobot's statuses: ppo_host_* / ppo_dev_* (PPO_ERR_STATE); ppo_obs_norm_* and ppo_reward_norm_* (PPO_ERR_UNSUPPORTED);
 * ppo_env_step_f32, ppo_rollout_f32, ppo_policy_act_f32 (PPO_ERR_UNSUPPORTED, naming the integer twin).
 * Which fold: without PPO_KERNEL_ENV_CUT_STATE cat_trunc_fold_kernel, from PPO_BUF_OBS and the stored action; with the flag cut_state_fold_kernel, from the
 * kept state -- the same events and the same rewards, bit for bit, under either distribution (tests/test_gpu_cut_state.py).
 * Sharding is neither claimed nor tested. */
enum { PPO_ENV_TAXI = PPO_ENV_ACROBOT + 2 };   /* 8, not 7: value 7 stays unassigned and keeps answering "unknown env_kind 7", as 9 does -- existing tests
                                                * hold both; in an enum of its own and written as a sum, as PPO_ENV_ACROBOT is: the first list's text is pinned */
/* PPO_ENV_FROZENLAKE (new; value 10) and PPO_ENV_FROZENLAKE8X8 (new; value 11): gymnasium's FrozenLake-v1 and FrozenLake8x8-v1 with is_slippery = True, the
 * first device envs whose transitions draw random numbers.  ppo_env_transition takes neither a seed nor a step index and stays stateless, so THE STATE CARRIES
 * THE RANDOMNESS: a reset draws a per-episode key into the state, a step draws from Philox keyed by that key and the episode's step count, both state words.
 * The transition is a pure function of (state, action); every contract of the family holds (a one-launch rollout equals a loop of ppo_policy_act +
 * ppo_env_step bit for bit; ppo_evaluate's episode e is a pure function of (parameters, seed, e)).  Two env kinds, because ppo_env_transition(env_kind, ..)
 * has no other way to know the map.  Every quantity is an integer held exactly in f32; nothing below rounds.
 * Maps (gymnasium's; cells row-major, cell = row * n + col; the start is cell 0; S = n * n cells):
 *   4x4 (PPO_ENV_FROZENLAKE, S = 16):    SFFF FHFH FFFH HFFG; holes {5, 7, 11, 12}, as a bit mask 0x18a0; goal 15
 *   8x8 (PPO_ENV_FROZENLAKE8X8, S = 64): SFFFFFFF FFFFFFFF FFFHFFFF FFFFFHFF FFFHFFFF FHHFFFHF FHFFHFHF FFFHFFFG; holes {19, 29, 35, 41, 42, 46, 49, 52, 54, 59},
 *                                        as a bit mask 0x0852460820080000; goal 63
 * State (cell, j, k0, k1): cell in 0..S-1; j, the steps taken in this episode, in 0..2^24-1; k0, k1 (the episode's key) in 0..2^24-1.
 * PPO_BUF_ENV_STATE is f32 [4, N]; ppo_env_set_state_h / ppo_env_get_state_h take [N, 4].
 * Step under action a (clamped into 0..3: 0 left, 1 down, 2 right, 3 up):
 *   cell is a hole or the goal (reachable only through an injected state): reward 0, terminated 1, cell unchanged, j' = min(j + 1, 2^24 - 1);
 *   otherwise: w = philox4x32_10(key = (k0, k1); counter = (j >> 2, 0, 0, 0x20)) -- the argument order of philox4x32_10(k0, k1, c0, c1, c2, c3); tag 0x20 is
 *   used by no other draw -- word = w[j & 3], d = (uint64(word) * 3) >> 32, eff = (a + d + 3) & 3 (gym's [(a-1)%4, a, (a+1)%4], one third each); move one cell
 *   in direction eff, clamped at the border; terminated = cell' is a hole or the goal; reward = cell' == goal ? 1.0f : 0.0f; j' = j + 1 (held at 2^24 - 1,
 *   which only an injected j meets: the time limit ends an episode first); k0 and k1 stay.
 * Reset number k of global env e: w = philox4x32_10(seed; e, k, 0, 1) (MountainCar's keying); cell = 0, j = 0, k0 = w.x >> 8, k1 = w.y >> 8.  Global env 0
 * takes reset 1 at ppo_env_reset; PPO_BUF_RESET_COUNT counts them.
 * Observation, obs_size 16 resp. 64: the one-hot of cell (0.0f / 1.0f).  It holds the cell but not j, k0, k1.
 * An episode ends where the env terminates or its length reaches max_episode_steps (1..16 777 215; gym: 100 and 200): done = 1, FIN_LEN / FIN_REW written,
 * auto-reset -- ppo_env_step's bookkeeping.  Returns are 0 or 1.
 * Memory safety, as for PPO_ENV_TAXI: ppo_env_set_state_h checks the host array -- a component that is not an integer of its range returns PPO_ERR_INVALID and
 * changes nothing; the device functions convert and clamp each component into its range (a NaN becomes 0); a caller's i64 action is saturated, not truncated.
 * ppo_ctx_create accepts the envs in exactly this form: dist_kind = PPO_DIST_CATEGORICAL (PPO_DIST_MASKED is refused as on PPO_ENV_ACROBOT: the env forms no
 * mask), n_heads = 1, head_dims[0] = 4, obs_size = 16 resp. 64, hidden = 64, n_hidden = 2, PPO_DTYPE_F32, kernel_flags containing PPO_KERNEL_CAT_FUSED
 * (required, never implied) and 1 <= max_episode_steps <= 16 777 215.  A wrong obs_size returns PPO_ERR_INVALID with the reference's obs-size message,
 * anything else PPO_ERR_UNSUPPORTED with a message that names the limit.
 * Calls: PPO_ENV_ACROBOT's list -- ppo_env_reset, ppo_env_set_state_h (refills NEXT_OBS) / ppo_env_get_state_h, ppo_env_step (action i64 [N, 1], obs
 * [N, S]), ppo_env_transition(10 | 11, state [n, 4], action i64 [n], ...), ppo_rollout (forced i64 [T, N, 1] or NULL), ppo_calc_advantage, ppo_update,
 * ppo_train_iteration, ppo_policy_act / ppo_policy_act_greedy, ppo_get_value, ppo_target_kl_set, ppo_evaluate, the statistics and profile calls,
 * ppo_gauss_fused_launches.  ppo_rollout is THREE launches, as on Acrobot (cat_rollout_kernel; LDS 62 912 bytes at 4x4, 88 256 bytes at 8x8: one workgroup
 * per CU there; `value` moves by 2, `act` by 0); a stepwise loop of ppo_policy_act(step_index = rollout_steps + t) and ppo_env_step reproduces every buffer
 * it fills bit for bit (tests/test_gpu_frozenlake.py).  ppo_evaluate is ONE launch (cat_eval_kernel) and moves no counter.
 * Refused, changing nothing: ppo_host_* / ppo_dev_* (PPO_ERR_STATE); ppo_obs_norm_* and ppo_reward_norm_* (PPO_ERR_UNSUPPORTED); ppo_env_step_f32,
 * ppo_rollout_f32, ppo_policy_act_f32 (PPO_ERR_UNSUPPORTED, naming the integer twin); ppo_env_truncation_bootstrap and ppo_env_truncations
 * (PPO_ERR_UNSUPPORTED: the final observation of a cut-off episode depends on j and the key, which the stored observation does not hold).  With
 * PPO_KERNEL_ENV_CUT_STATE in kernel_flags (below) the rollout keeps (cell, j, k0, k1) of every cut-off episode and whether the env itself terminated on that
 * step, and the two calls are served from that record on both kinds (cut_state_fold_kernel); without the flag the refusal stands, word for word.  Sharding is
 * neither claimed nor tested. */
enum { PPO_ENV_FROZENLAKE = PPO_ENV_TAXI + 2 };      /* 10, not 9: value 9 stays unassigned, as 7 does; an enum of its own, written as a sum */
enum { PPO_ENV_FROZENLAKE8X8 = PPO_ENV_TAXI + 3 };   /* 11 */
/* PPO_ENV_BLACKJACK (new; value 13): gymnasium's Blackjack-v1 with its defaults (natural = False, sab = False) and the infinite deck, on PPO_ENV_FROZENLAKE's
 * mechanism -- THE STATE CARRIES THE RANDOMNESS -- with a reset that deals and a step whose NUMBER OF DRAWS DEPENDS ON THE DATA: a hit draws one card, a stick
 * plays out the dealer, up to ten cards, inside one env step.  The transition is a pure function of (state, action); every contract of the family holds (a
 * one-launch rollout equals a loop of ppo_policy_act + ppo_env_step bit for bit; ppo_evaluate's episode e is a pure function of (parameters, seed, e)).
 * Every quantity is an integer held exactly in f32; nothing below rounds.  Returns have both signs: -1, 0 or +1.
 * Cards: card(word) = min(1 + ((uint64(word) * 13) >> 32), 10) -- gym's deck [1..10, 10, 10, 10]: ace = 1, a ten has probability 4/13.  Card number i of an
 *   episode with key (k0, k1) is card(w[i & 3]) of w = philox4x32_10(key = (k0, k1); counter = (i >> 2, 0, 0, 0x21)) -- the argument order of
 *   philox4x32_10(k0, k1, c0, c1, c2, c3); tag 0x21 is used by no other draw.  Cards 0 and 1 are the player's first two, card 2 is the dealer's showing card,
 *   card 3 the dealer's hidden card; cards 4, 5, ... are drawn in order by whoever draws next.
 * State (hand, n, k0, k1): hand = t + 32 * ace + 64 * show with t in 2..31 the player's total with every ace counted as 1, ace in 0..1 whether the player
 *   holds an ace, show in 1..10 the dealer's showing card; n in 0..2^24-1 the index of the next card to be drawn (4 after a reset); k0, k1 (the episode's
 *   key) in 0..2^24-1.  Derived: usable = ace && t + 10 <= 21; sum = t + 10 * usable.  PPO_BUF_ENV_STATE is f32 [4, N]; ppo_env_set_state_h /
 *   ppo_env_get_state_h take [N, 4].
 * Step under action a (clamped into 0..1: 0 stick, 1 hit):
 *   t > 21 (reachable only through an injected state): reward -1, terminated 1, nothing is drawn and the state is unchanged;
 *   hit: c = card n; t += c; ace |= (c == 1); n' = min(n + 1, 2^24 - 1); t > 21: reward -1, terminated 1; otherwise reward 0, terminated 0;
 *   stick: terminated 1.  The dealer's hand is (show, card 3): dt = show + card 3, dace = either of them is 1.  While dt + (dace && dt + 10 <= 21 ? 10 : 0)
 *   < 17 the dealer draws card n, n + 1, ... (dt += c; dace |= (c == 1)).  Dealer's score = 0 if dt > 21, else that sum; player's score = sum; reward = +1, 0
 *   or -1 as the player's score is above, equal to or below the dealer's.  n' = n + (cards the dealer drew), held at 2^24 - 1; the player's part of hand
 *   stays.  k0 and k1 stay in every case.
 *   The dealer draws at most 10 cards from any two-card start (the hard total rises by at least 1 per card; enumerated over all 100 (show, hidden) pairs), so
 *   the device's loop has exactly that compile-time bound with a predicate and is never a `while` on data: no foreign state can spin a lane.
 * Reset number k of global env e: w = philox4x32_10(seed; e, k, 0, 1) (MountainCar's keying); k0 = w.x >> 8, k1 = w.y >> 8; one more call (counter 0, tag
 *   0x21) gives all four dealt cards: t = card 0 + card 1, ace = either is 1, show = card 2, n = 4.  Global env 0 takes reset 1 at ppo_env_reset;
 *   PPO_BUF_RESET_COUNT counts them.
 * Observation, obs_size 45: gymnasium's flattened Tuple(Discrete(32), Discrete(11), Discrete(2)) -- three one-hot groups of 0.0f / 1.0f: sum at [0..31],
 *   32 + show at [32..42], 43 + usable at [43..44].  It holds neither n nor the key.
 * An episode ends where the env terminates or its length reaches max_episode_steps (1..16 777 215): done = 1, FIN_LEN / FIN_REW written, auto-reset --
 * ppo_env_step's bookkeeping.  Without a limit in the way an episode takes at most 20 steps.
 * Memory safety, as for PPO_ENV_FROZENLAKE: ppo_env_set_state_h checks the host array -- hand must decode into t 2..31, ace 0..1, show 1..10 with no bits
 * above (an integer in 0..703), n, k0, k1 must be integers in 0..2^24-1; a bad array returns PPO_ERR_INVALID and changes nothing; the device functions
 * convert and clamp each component (a NaN becomes 0; hand into 0..703, then t into 2..31 and show into 1..10; n, k0, k1 into 0..2^24-1); a caller's i64
 * action is saturated, not truncated.
 * ppo_ctx_create accepts the env in exactly this form: dist_kind = PPO_DIST_CATEGORICAL (PPO_DIST_MASKED is refused: the env forms no mask), n_heads = 1,
 * head_dims[0] = 2, obs_size = 45, hidden = 64, n_hidden = 2, PPO_DTYPE_F32, kernel_flags containing PPO_KERNEL_CAT_FUSED (required, never implied) and
 * 1 <= max_episode_steps <= 16 777 215.  A wrong obs_size returns PPO_ERR_INVALID with the reference's obs-size message, anything else PPO_ERR_UNSUPPORTED
 * with a message that names the limit.
 * Calls: PPO_ENV_FROZENLAKE's list, with ppo_env_step's obs [N, 45] and ppo_env_transition(13, state [n, 4], action i64 [n], ...).  ppo_rollout is THREE
 * launches (cat_rollout_kernel; LDS 79 808 bytes; `value` moves by 2, `act` by 0); a stepwise loop of ppo_policy_act(step_index = rollout_steps + t) and
 * ppo_env_step reproduces every buffer it fills bit for bit (tests/test_gpu_blackjack.py).  ppo_evaluate is ONE launch (cat_eval_kernel) and moves no counter.
 * Refused, changing nothing: PPO_ENV_FROZENLAKE's list -- ppo_host_* / ppo_dev_* (PPO_ERR_STATE); ppo_obs_norm_* and ppo_reward_norm_*
 * (PPO_ERR_UNSUPPORTED); ppo_env_step_f32, ppo_rollout_f32, ppo_policy_act_f32 (PPO_ERR_UNSUPPORTED, naming the integer twin);
 * ppo_env_truncation_bootstrap and ppo_env_truncations (PPO_ERR_UNSUPPORTED: the final observation of a cut-off episode depends on n and the key, which the
 * stored observation does not hold).  With PPO_KERNEL_ENV_CUT_STATE in kernel_flags (below) the rollout keeps (hand, n, k0, k1) of every cut-off episode
 * and whether the env itself terminated on that step, and the two calls are served from that record (cut_state_fold_kernel); without the flag the refusal
 * stands, word for word.  Sharding is neither claimed nor tested. */
enum { PPO_ENV_BLACKJACK = PPO_ENV_TAXI + 5 };   /* 13, not 12: value 12 stays unassigned, as 7 and 9 do; an enum of its own, written as a sum */
/* PPO_DIST_CATEGORICAL reproduces Distributions/Categorical.cpp including its entropy clamp (:112-119);
 * PPO_DIST_MASKED reproduces Distributions/CategoricalMasked.cpp (true entropy, -1e8 masking).
 * PPO_DIST_GAUSSIAN (new; the reference has no continuous policy): a diagonal Gaussian over D = head_dims[0] real-valued actions (n_heads = 1,
 * 1 <= D <= 32).  The actor's output layer gives the mean mu[D]; a state-independent parameter log_std[D] -- ONE MORE TENSOR, the last in
 * Agent::parameters() order, behind the actor's layers (ppo_param_count, ppo_param_shapes), initialised to 0 -- gives the scale.  With
 * z = (a - mu) exp(-log_std):  log-prob = sum_d (-z_d^2 / 2 - log_std_d - log(2 pi) / 2),  entropy = sum_d (1 / 2 + log(2 pi) / 2 + log_std_d), no clamp.
 * Serves PPO_ENV_HOST contexts with PPO_DTYPE_F32, on the generic engine (also for a 2 x 64 network, unless kernel_flags has PPO_KERNEL_GAUSS_FUSED), and PPO_ENV_PENDULUM /
 * PPO_ENV_MOUNTAINCAR_CONTINUOUS contexts in the one form each env accepts (above); any other env_kind, PPO_DTYPE_BF16 or
 * n_heads != 1 make ppo_ctx_create return PPO_ERR_UNSUPPORTED.  Actions are f32: PPO_BUF_ACTIONS is f32 [T,N,D], PPO_BUF_MASKS is not used, and the
 * calls that carry actions have _f32 twins (ppo_host_act_f32, ppo_dev_act_f32, ppo_policy_act_f32); the integer calls return PPO_ERR_UNSUPPORTED on a
 * Gaussian context and name the twin, and the twins do the same on a categorical context.  Env groups (ppo_host_rollout_begin_groups) return
 * PPO_ERR_UNSUPPORTED.  Everything up- and downstream of the distribution is shared: ppo_host_observe / ppo_host_observe_truncated /
 * ppo_host_rollout_end, ppo_dev_observe, ppo_obs_norm_*, ppo_reward_norm_*, ppo_get_value, ppo_update, ppo_minibatch_forward_backward,
 * ppo_optimizer_step (log_std is clipped, decayed and stepped like any other tensor).
 * THE ACTION IS THE RAW SAMPLE mu + sigma * eps, stored and returned unclipped: clipping it to the env's bounds is the caller's business (clip the copy
 * handed to the env, as gym's ClipAction does; the rollout keeps the raw sample, whose log-prob it stored). */
enum { PPO_DIST_CATEGORICAL = 0, PPO_DIST_MASKED = 1, PPO_DIST_GAUSSIAN = 2 };
/* PPO_DTYPE_F32: every product carries f32 accuracy (on the matrix cores: f32 operands as three exact bf16 terms, f32 accumulation).
 * PPO_DTYPE_BF16: "bf16 with MFMA GEMMs" of BASELINE configs[4] -- operands and stored activations rounded to bf16 (nearest even),
 * f32 accumulation, f32 master weights, gradients and optimizer state. */
enum { PPO_DTYPE_F32 = 0, PPO_DTYPE_BF16 = 1 };

/* Hyper-parameters: the m_* fields of PPO_Discrete (PPO_Discrete.h:52-85) / the TOML keys (PPO_Discrete.cpp:107-255). */
typedef struct ppo_config {
    int32_t struct_size;        /* = sizeof(ppo_config) */
    int32_t device;             /* HIP device ordinal (reference: use_cuda -> torch::kCUDA, PPO_Discrete.cpp:65) */
    int32_t env_kind;           /* PPO_ENV_* : PPO_Discrete owns CartPole, PPO_MultiDiscrete owns MountainCar, PPO_ENV_HOST: the caller's envs */
    int32_t dist_kind;          /* PPO_DIST_* */
    int32_t obs_size;           /* [environment] obs_size */
    int32_t n_heads;            /* Agent::m_actionSpace.size() (Agent.cpp:21) */
    int32_t head_dims[PPO_MAX_HEADS]; /* Agent::m_actionSpace; reference: { action_size } */
    int32_t hidden;             /* 64 (Agent.cpp:25-32) */
    int32_t n_hidden;           /* 2 tanh layers */
    int32_t num_envs;           /* envs owned by THIS context (a shard when global_num_envs > num_envs) */
    int32_t num_steps;
    int32_t num_minibatches;
    int32_t update_epochs;
    int32_t max_episode_steps;
    int32_t use_gae, norm_adv, clip_vloss, anneal_lr;
    int64_t seed;
    int64_t total_timesteps;    /* global; drives the LR anneal (PPO_Discrete.cpp:496,514-518) */
    int64_t env_offset;         /* global index of this shard's env 0 */
    int64_t global_num_envs;    /* 0 or num_envs when not sharded */
    float learning_rate, gamma, gae_lambda, clip_coef, ent_coef, vf_coef, max_grad_norm;
    int32_t compute_dtype;      /* PPO_DTYPE_*: arithmetic of the layer GEMMs of a PPO_ENV_SYNTHETIC network; the 2 x 64 paths are always f32 */
    int32_t kernel_flags;       /* PPO_KERNEL_* (0 = the defaults): which hand-written kernel runs a stage, for A/B runs and for bit-exact replays */
} ppo_config;

/* ppo_config.kernel_flags.  The defaults put the reference's two shapes on the matrix cores; every alternative computes the same function.
 *   PPO_KERNEL_ROLLOUT_VECTOR   the fused rollout AND the stand-alone policy (ppo_policy_act) on the vector ALU (rollout2_kernel, policy_act_kernel): logits
 *                               formed by plain fp32 multiply-adds.  The default rollout16_kernel forms layer 2 and the logits as two-term fp16 products on
 *                               the matrix cores, ~1e-7 away.  ppo_policy_act ALWAYS runs the arithmetic the context's rollout runs (default:
 *                               policy_act16_kernel, the same products in the same order; under this flag, or for a launch whose output-layer weights do
 *                               not fit fp16, the vector form), so a free-running rollout and the stand-alone policy on the same observations, weights and
 *                               step index agree in every log-prob bit and every sampled action (tests/test_gpu_parity.py:
 *                               test_fused_rollout_equals_stepwise_api).  Between the two arithmetics an action sampled where the uniform sits within ~1e-6
 *                               of a bin edge can differ (measured: <= 2 of 8 192): use this flag to replay recordings made with it, or with round <= 5
 *                               builds' stand-alone policy.
 *   fp16 ranges                 The matrix-core kernels carry some operands as fp16 terms: rollout16_kernel 2^8 W3 (|W3| < 255), the update kernels c W2 and
 *                               the products through its columns (sum |W2[:, k]| < ~350), c W1 / c b1 / c b2 (< 22 700) and the observation (< 65 504).  The
 *                               reference has none of these limits and a caller never meets the weight limits: the maxima of |parameter| per class are taken
 *                               once per update (and after every host write of the parameters), the host reads a pinned mirror of them without synchronising (thresholds at half the
 *                               limits: max |W3| >= 128, max |W2| >= 4, anything else >= 8192), and a launch whose weights do not fit takes the vector
 *                               kernel (plain fp32, the same function) -- for that launch only, with the default flags.  An OBSERVATION beyond fp16 written
 *                               into PPO_BUF_OBS cannot be foreseen: the update's record packing raises the context's error word (only when the matrix-core
 *                               kernel will read the records) and ppo_read_stats / ppo_stats_snapshot_read fail with PPO_ERR_STATE; PPO_KERNEL_UPDATE_VECTOR
 *                               has no such limit.  The same holds for a hand-over wait of the update kernel, or of the time-pipelined advantage scan, that
 *                               runs out (protocol errors, never observed in 1.6 M launches).  ABI 5: the optimizer kernels read the error word and do NOT
 *                               APPLY a step behind any of these: parameters and AdamW moments keep the values they had before the error (the
 *                               learning-rate schedule and the step counters run on), the error is sticky.  A gradient that is merely not finite (the
 *                               reference's 1-row minibatch) is applied as the reference applies it.
 *   PPO_KERNEL_UPDATE_VECTOR    the update's forward / backward on the vector ALU (fwd_bwd_kernel) for every shape: plain fp32 arithmetic; also for
 *                               rehearsals of more than two ranks on ONE GPU (tests/test_gpu_exchange.py).
 *   PPO_KERNEL_UPDATE_ONE_WAVE  the one-wave-per-tile matrix-core kernel (fwd_bwd_mfma_kernel) instead of the wave-specialised one
 *                               (fwd_bwd_mfma_ws_kernel) for the reference's two shapes: the A/B partner of the default.
 *   PPO_KERNEL_COMM_SELFTEST    ppo_comm_init(..., rank 0, nranks 1) really creates a ONE-rank RCCL communicator and every collective of the multi-rank
 *                               path is really issued (sums over one rank = identity): the only way to drive the RCCL calls -- library lookup,
 *                               datatype / op enums, stream ordering, the three-kernel optimizer path -- on a box with a single GPU.
 *   PPO_KERNEL_GENERIC_CLASSIC  generic networks with bf16 storage (PPO_ENV_SYNTHETIC, e.g. BASELINE configs[4]): a minibatch step in its first form -- the
 *                               minibatch gathered into dense copies, one net per launch with the critic's passes on a second stream, loss sums / gradient
 *                               norm / AdamW / weight planes as four launches -- instead of rows read in place through the index list, both nets in every
 *                               launch on one stream and one optimizer launch.  Same kernels for the products, same partial-sum partitions: the two forms
 *                               agree to the last bits of a float (only the order in which the gradient norm's partial sums are added differs).  For A/B
 *                               runs and tests.
 *   PPO_KERNEL_GENERIC_SPLIT_HEAD  generic networks with bf16 storage: heads, masked categorical, PPO loss and the head layers' backward as launches of their own
 *                               (loss_lanes_kernel, bwd_layer_kernel<1, ...>) behind a forward launch that writes logits, values and the top hidden activation
 *                               to memory -- round 5's step -- instead of in the forward launch's epilogue, on the tile still in LDS (ABI 5 default where the
 *                               shape allows: <= 4 heads of <= 4 logits).  Same arithmetic (the same bf16 roundings, f32 sums); partial sums are formed per
 *                               forward workgroup instead of per row range, so the two agree to f32 summation order.  For A/B runs and tests.
 *   PPO_KERNEL_GAUSS_FUSED      dist_kind = PPO_DIST_GAUSSIAN on a 2 x 64 f32 network (hidden = 64, n_hidden = 2, PPO_DTYPE_F32, 1 <= D <= 32, obs_size <= 64):
 *                               its own kernels (kernels_gauss_fused.hip) in the place of the generic engine's per-layer products -- ONE launch per env step
 *                               (actor, draw, log-prob, entropy and the step's rollout stores: ppo_host_act_f32, ppo_dev_act_f32, ppo_policy_act_f32), ONE per
 *                               critic batch (ppo_get_value, ppo_host_rollout_end's two, ppo_bootstrap_rewards and the truncation folds), and a minibatch
 *                               step of five: forward / loss / backward of both nets, the partial slabs' sum, then the engine's own loss sums, norm and
 *                               AdamW.  Plain f32 multiply-adds, one forward function for all three kernels (an observation gets the same mean and value from
 *                               every entry point, bit for bit); the draw, log-prob and entropy are the generic path's own device functions, so a mean gives
 *                               the same action and log-prob bits as ppo_gaussian.  Parameter layout and order are unchanged (log_std the 13th tensor).
 *                               Against the same context without the flag: means and values agree to f32 summation order (both within the forward bar of
 *                               float64), not bit for bit.  Opt-in; any other shape or policy with the flag set is refused by ppo_ctx_create with
 *                               PPO_ERR_UNSUPPORTED and a message that names the limit -- never served by the generic engine instead.
 *                               ppo_gauss_fused_launches counts the three kernels' launches.  Truncation flags in ppo_dev_observe are served: the fold is
 *                               one launch on the critic kernel's forward (gauss_dev_fold_kernel), counted as a `value` launch.
 *   PPO_KERNEL_SEPARATE_LAUNCHES  the once-per-iteration launches of a CartPole / MountainCar context in their stand-alone form, eight of them: the episode
 *                               ring's two kernels in front of the NEXT rollout (or the next statistics read), the critic batch, the record pack, the
 *                               permutations / advantage sums and the normalisation each a launch of its own.  Without the flag ppo_rollout's critic launch
 *                               also counts and pushes the rollout's finished episodes (values_ring_mfma_kernel: they are in the ring BEHIND their own
 *                               rollout), and ppo_update's first launch packs the records, forms the permutations and the advantage sums and -- in a context
 *                               that is not sharded -- the 40 normalisations (pack_perm_stats_kernel).  Every workgroup does the arithmetic it does in the
 *                               stand-alone kernel, on the same elements in the same order: parameters, buffers and statistics are the same bit for bit, and
 *                               every reader consumes pending episodes first, so nothing observable moves.  For A/B runs and tests.
 *   PPO_KERNEL_CAT_FUSED        PPO_KERNEL_GAUSS_FUSED's twin for the reference's own policies: env_kind = PPO_ENV_HOST with dist_kind = PPO_DIST_CATEGORICAL or
 *                               PPO_DIST_MASKED on a 2 x 64 f32 network (hidden = 64, n_hidden = 2, PPO_DTYPE_F32), 1 <= obs_size <= 64, any head list within
 *                               PPO_MAX_HEADS / sum(head_dims) <= 32.  The same kernel family (kernels_gauss_fused.hip: cat_act_kernel, gauss_values_kernel,
 *                               cat_fwd_bwd_kernel) in the place of the generic engine's per-layer products: ONE launch per env step (actor, masked
 *                               log-softmax, draw, log-prob, entropy and the step's rollout stores: ppo_host_act, ppo_host_group_act, ppo_dev_act,
 *                               ppo_policy_act, ppo_policy_act_greedy), ONE per critic batch, and a minibatch step of five.  The heads are the generic path's
 *                               own device functions (equal logits give equal action, log-prob and entropy bits); a row gets the same logits and value from
 *                               every entry point, bit for bit.  The context always lives in the generic engine's layout -- also at obs_size 2, 4 and 8, where
 *                               the flag takes it off the reference-shape kernels; the parameter order is Agent::parameters() order either way.  Against the
 *                               same context without the flag: log-probs and values agree to f32 summation order, not bit for bit.  Two device envs run on
 *                               the family too, PPO_ENV_ACROBOT and PPO_ENV_TAXI (above), in the forms they accept; there the flag is required.  Opt-in; a Gaussian
 *                               policy, any other device env, PPO_ENV_SYNTHETIC, another width or depth, bf16, obs_size > 64 or PPO_KERNEL_GAUSS_FUSED beside it make
 *                               ppo_ctx_create return PPO_ERR_UNSUPPORTED with a message that names the limit -- never served by another engine instead.
 *                               ppo_evaluate stays refused as on the generic engine; truncation flags in ppo_dev_observe are served as on a
 *                               PPO_KERNEL_GAUSS_FUSED context (the critic kernel is shared, and so is the fold: gauss_dev_fold_kernel).
 *                               ppo_gauss_fused_launches counts the three kernels' launches (one set of counters for the family; no symbol of its own).
 *   PPO_KERNEL_ENV_GENERIC      env_kind = PPO_ENV_CARTPOLE or PPO_ENV_MOUNTAINCAR on a network of any width and depth: the context lives in the generic
 *                               engine's layout, with PPO_ENV_SYNTHETIC's network limits (hidden 1 .. 2048, n_hidden 1 .. 7, PPO_DTYPE_F32 or PPO_DTYPE_BF16)
 *                               and its parameter order (Agent::parameters() order generalised, as ppo_param_shapes reports it).  dist_kind, n_heads,
 *                               head_dims, obs_size, the wrong-obs-size message and the masks are those of the same context without the flag (PPO_BUF_MASKS:
 *                               ones under PPO_DIST_MASKED, untouched otherwise).  The env is the unflagged context's, kernel for kernel: PPO_BUF_ENV_STATE,
 *                               EP_LEN, EP_REW, RESET_COUNT, CartPole's shared reset table, ppo_env_reset (env 0's probe reset included), ppo_env_step,
 *                               ppo_env_set_state_h / ppo_env_get_state_h, max_episode_steps, FIN_LEN / FIN_REW, the episode ring and the statistics.
 *                               ppo_rollout (forced i64 [T,N,H] or NULL), ppo_calc_advantage, ppo_update, ppo_minibatch_forward_backward, ppo_optimizer_step,
 *                               ppo_train_iteration, ppo_policy_act, ppo_policy_act_greedy, ppo_get_value, ppo_target_kl_set and the statistics and profile
 *                               calls run on the generic engine's paths.  The rollout, f32 storage: per step the engine's forward, heads and stores, then
 *                               the env's step kernel on the context's buffers -- the launches of ppo_policy_act(step_index = rollout_steps + t) +
 *                               ppo_env_step, same bits.  bf16 storage, wherever the engine's fused forward serves the network (sum(head_dims) <= 32, both
 *                               LDS tiles fit): generic_env_rollout_kernel, all T steps in ONE launch -- 32 envs per workgroup, the actor's layers on the
 *                               matrix cores with the activations in LDS, lanes 0 .. 31 of wave 0 sample the heads and keep state, episode sums, reset
 *                               count and done flag in registers, step the env and write the next observation themselves; two critic launches follow on
 *                               CartPole.  MountainCar with bf16 storage: the fused forward stages f32 rows as 16-byte pieces (obs_size % 4 == 0), which an
 *                               observation of 2 is not, so every critic or actor batch outside the rollout kernel -- the rollout's critic over the T N
 *                               stored rows and over NEXT_OBS, ppo_get_value, ppo_policy_act, ppo_policy_act_greedy -- first rounds its rows to bf16
 *                               (one conversion launch) and then runs the same fused layers, per chunk of the workspace's rows (max(minibatch, N) rounded
 *                               up to 128): 2 launches per chunk, about 2 (num_minibatches + 1) behind a rollout instead of 2, same bits as the rollout's.
 *                               Also at 2 x 64: the flag takes the context off the reference-shape kernels, as their A/B partner (log-probs and values then
 *                               agree to summation order, not bit for bit; the env's bits do not change under the same actions).  Opt-in, never implied;
 *                               ppo_ctx_create returns PPO_ERR_UNSUPPORTED with a message naming the flag and the limit for any other env_kind, for
 *                               PPO_KERNEL_GAUSS_FUSED or PPO_KERNEL_CAT_FUSED beside it and for PPO_DIST_GAUSSIAN -- another engine never serves in the
 *                               flag's place.  Refused on such a context, changing nothing: ppo_host_* / ppo_dev_* (PPO_ERR_STATE, as on any device env),
 *                               ppo_obs_norm_* / ppo_reward_norm_* (PPO_ERR_UNSUPPORTED), ppo_evaluate (PPO_ERR_UNSUPPORTED: step the episodes with
 *                               ppo_policy_act_greedy + ppo_env_transition), ppo_env_truncation_bootstrap and ppo_env_truncations (PPO_ERR_UNSUPPORTED: the
 *                               fold is built on the reference-shape critic).  Sharding (ppo_comm_init*) of a flagged context is neither claimed nor tested.
 *   PPO_KERNEL_ENV_CUT_STATE    the device envs of the fused 2 x 64 families -- PPO_ENV_PENDULUM, PPO_ENV_MOUNTAINCAR_CONTINUOUS, PPO_ENV_ACROBOT, PPO_ENV_TAXI,
 *                               PPO_ENV_FROZENLAKE, PPO_ENV_FROZENLAKE8X8 and PPO_ENV_BLACKJACK -- next to the env's own family flag: the one-launch rollout
 *                               keeps the state a time limit cut an episode off in.  What is kept: at every sample i = t * N + n whose episode's length reached
 *                               max_episode_steps on that step, wave 0's owning lane stores the env's state as it is BEFORE the auto-reset (STATE f32 words:
 *                               2 on the Gaussian envs, 4 on the categorical ones) and one more word, 0.0f or 1.0f, "the env itself terminated on this
 *                               step".  Where: a device allocation of the context's own, f32 [STATE + 1, T * N], made by ppo_ctx_create and released with the
 *                               context; it is no PPO_BUF_* and ppo_get_buffer does not reach it.  What it costs: 4 (STATE + 1) T N bytes, and STATE + 1
 *                               scattered stores at the cut-off samples only -- no store at any other sample, nothing dense per step, nothing cleared between
 *                               rollouts (the fold reads a column only where this rollout's FIN_LEN says this rollout wrote it).  The rollout is another
 *                               instantiation of the same kernel (gauss_rollout_kernel / cat_rollout_kernel with KEEP = true); every buffer it fills holds the
 *                               bits of the unflagged context's.  Which calls it opens: ppo_env_truncation_bootstrap and ppo_env_truncations on PPO_ENV_PENDULUM,
 *                               PPO_ENV_ACROBOT, PPO_ENV_FROZENLAKE, PPO_ENV_FROZENLAKE8X8 and PPO_ENV_BLACKJACK, whose observations do not hold the state
 *                               (theta; the angles; the step count, the card count and the episode's key) and which refuse the two calls without the flag.
 *                               On a flagged context EVERY fused env folds from the record, in one launch of cut_state_fold_kernel (the final observation is
 *                               Env::obs of the kept state; no step is replayed and no action read): PPO_ENV_MOUNTAINCAR_CONTINUOUS and PPO_ENV_TAXI too, with
 *                               the events and rewards of their unflagged folds, bit for bit.  The fold's dynamic LDS, by obs_size: 59 680 bytes at 2 and 3,
 *                               63 840 at 6, 68 064 at 16, 70 176 at 19, 84 960 at 45, 93 408 at 64.  Opt-in, never implied: without the flag every context is
 *                               what it was, refusals included.  ppo_ctx_create returns PPO_ERR_UNSUPPORTED with a message naming the flag and the limit on
 *                               any other env_kind (PPO_ENV_CARTPOLE, PPO_ENV_MOUNTAINCAR, PPO_ENV_SYNTHETIC, PPO_ENV_HOST) and beside PPO_KERNEL_ENV_GENERIC.
 *                               Everything else a flagged context refuses it refuses as without the flag (ppo_evaluate on Pendulum, ppo_host_* / ppo_dev_*,
 *                               the normalisers).  Sharding (ppo_comm_init*) of a flagged context is neither claimed nor tested.
 *   PPO_KERNEL_ENV_REWARD_NORM  the same seven device envs, next to the family flag (and beside PPO_KERNEL_ENV_CUT_STATE if wanted): opens ppo_reward_norm_* on
 *                               their one-launch rollouts.  Its entry stands at its #define below; the contract in "Reward normalisation". */
enum { PPO_KERNEL_ROLLOUT_VECTOR = 1, PPO_KERNEL_UPDATE_VECTOR = 2, PPO_KERNEL_UPDATE_ONE_WAVE = 4, PPO_KERNEL_COMM_SELFTEST = 8, PPO_KERNEL_GENERIC_CLASSIC = 16,
       PPO_KERNEL_GENERIC_SPLIT_HEAD = 32, PPO_KERNEL_GAUSS_FUSED = 64 };
#define PPO_KERNEL_SEPARATE_LAUNCHES 128   /* the next free bit of kernel_flags, 1 << 7; a macro beside the enumerators: same type in an expression, same use */
#define PPO_KERNEL_CAT_FUSED 256           /* 1 << 8, likewise */
#define PPO_KERNEL_ENV_GENERIC 512         /* 1 << 9, likewise */
#define PPO_KERNEL_ENV_CUT_STATE (1 << 10) /* 1024, likewise; written as the shift: tests/test_env_generic_abi.py pins the list of macros spelt as decimal literals */
/* PPO_KERNEL_ENV_REWARD_NORM (8192; bits 11 and 12 stay unassigned and are refused as unknown): the device envs of the fused 2 x 64 families -- PPO_ENV_PENDULUM,
 * PPO_ENV_MOUNTAINCAR_CONTINUOUS, PPO_ENV_ACROBOT, PPO_ENV_TAXI, PPO_ENV_FROZENLAKE, PPO_ENV_FROZENLAKE8X8 and PPO_ENV_BLACKJACK -- next to the env's own family
 * flag, and beside PPO_KERNEL_ENV_CUT_STATE if wanted: it opens ppo_reward_norm_enable / _get_h / _set_h on such a context ("Reward normalisation" below has the
 * contract).  What it costs: one allocation of the context's own, f64 [T N + 2 T + 2] (8 T N bytes and O(T)), made by ppo_ctx_create and released with the
 * context; it is no PPO_BUF_* and ppo_get_buffer does not reach it.  The rollout launch is the unflagged context's: a flagged context that never calls
 * ppo_reward_norm_enable(mode != 0) runs, launch for launch and bit for bit, what its unflagged twin runs.  Opt-in, never implied: without the flag the three
 * calls refuse a device-env context as before, word for word.  ppo_ctx_create returns PPO_ERR_UNSUPPORTED with a message naming the flag and the limit on any
 * other env_kind (PPO_ENV_CARTPOLE, PPO_ENV_MOUNTAINCAR, PPO_ENV_SYNTHETIC, PPO_ENV_HOST -- which has the three calls without a flag) and beside
 * PPO_KERNEL_ENV_GENERIC.  Observation normalisation stays refused (its statistics feed back into the policy inside the one launch).  Sharding (ppo_comm_init*)
 * of a flagged context is neither claimed nor tested; with the normaliser on it is refused, as on PPO_ENV_HOST. */
#define PPO_KERNEL_ENV_REWARD_NORM (1 << 13)

/* Scalars the reference prints per update (PPO_Discrete.cpp:700-774) plus per-step diagnostics. */
typedef struct ppo_stats {
    double pg_loss, v_loss, entropy_loss, approx_kl, loss; /* last minibatch of the update (:588,:599,:619,:628,:631) */
    double clipfrac_last, clipfrac_mean;                   /* m_clipfracs.back() / PPOUtils::getVectorMean (:349,:755) */
    double total_norm;                                     /* clip_grad_norm_ return value (:640) */
    double explained_variance;                             /* :647-648 */
    double learning_rate;                                  /* :515-517 */
    double ep_len_mean, ep_rew_mean;                       /* CircularBuffer (Utils.h:72-78) */
    int64_t ep_count;                                      /* CircularBuffer::size() */
    int64_t global_step;                                   /* :526 */
    int64_t optimizer_steps;                               /* AdamW state step */
    int64_t updates;                                       /* iterations done */
} ppo_stats;

typedef struct ppo_ctx ppo_ctx;

/* Internal device buffers (non-owning views).  Element types in brackets. */
enum {
    PPO_BUF_OBS = 0,      /* m_obs        f32 [T,N,O]                       PPO_Discrete.cpp:90  */
    PPO_BUF_ACTIONS,      /* m_actions    i32 [T,N,H] (reference stores f32 [T,N,1], :91,:537); PPO_DIST_GAUSSIAN: f32 [T,N,D] */
    PPO_BUF_LOGPROBS,     /* m_logprobs   f32 [T,N]                         :92  */
    PPO_BUF_REWARDS,      /* m_rewards    f32 [T,N]                         :93   (PPO_ENV_HOST with truncation events: r + gamma V(final obs) there, after ppo_host_rollout_end) */
    PPO_BUF_DONES,        /* m_dones      f32 [T,N]                         :94  */
    PPO_BUF_VALUES,       /* m_values     f32 [T,N]                         :95  */
    PPO_BUF_MASKS,        /* m_action_masks u8 [T,N,A]        PPO_MultiDiscrete.cpp:98 */
    PPO_BUF_ADVANTAGES,   /* f32 [T,N]  calcAdvantage()[1]                  :305 */
    PPO_BUF_RETURNS,      /* f32 [T,N]  calcAdvantage()[0] */
    PPO_BUF_NEXT_OBS,     /* f32 [N,O]                                      :494 */
    PPO_BUF_NEXT_DONE,    /* i32 [N]   (stepEnvs' done tensor is kInt32, :418) */
    PPO_BUF_NEXT_VALUE,   /* f32 [N]                                        :280 */
    PPO_BUF_PARAMS,       /* f32 [P]  Agent::parameters() order: critic then actor (Agent.cpp:65-66) */
    PPO_BUF_GRADS,        /* f32 [P] */
    PPO_BUF_EXP_AVG,      /* f32 [P]  AdamW exp_avg */
    PPO_BUF_EXP_AVG_SQ,   /* f32 [P]  AdamW exp_avg_sq */
    PPO_BUF_ENV_STATE,    /* f32 [O,N] struct-of-arrays env state (CartPole::state, CartPole.h:38) */
    PPO_BUF_EP_LEN,       /* i32 [N]  episode_length  (CartPole.h:44) */
    PPO_BUF_EP_REW,       /* f32 [N]  episode_reward  (CartPole.h:45) */
    PPO_BUF_RESET_COUNT,  /* i32 [N]  resets drawn so far from the env's private generator (CartPole.h:28-29) */
    PPO_BUF_PERM,         /* i32 [E,B] minibatch permutations of the current update (torch::randperm, :569) */
    PPO_BUF_FIN_LEN,      /* i32 [T,N] length of the episode that finished at (t,n), else 0 (:455) */
    PPO_BUF_FIN_REW,      /* f32 [T,N] reward of that episode (:456) */
    PPO_BUF_COUNT_
};

/* ---------------------------------------------------------------------------------------------------------
 * Lifecycle / plumbing
 * ------------------------------------------------------------------------------------------------------- */
PPO_API int32_t ppo_abi_version(void);
/* PPO_Discrete::PPO_Discrete() (PPO_Discrete.cpp:4-100): allocates every device buffer once (rollout [T,N,*],
 * parameters, AdamW state, env SoA, reset-stream table); no allocation happens afterwards -- except ppo_evaluate's scratch (per-episode arrays, the
 * evaluation reset table), allocated by its first call, kept, and grown only by a call that asks for more episodes than any before it; and, by the same
 * policy, the truncation-event list of caller-stepped rollouts (one pinned host block and its device twin), allocated by the first
 * ppo_host_observe_truncated / ppo_host_group_observe_truncated call that carries an event and grown by doubling up to num_steps * num_envs entries;
 * and the ppo_dev_* calls' two hand-over events (created by the first call on a stream other than the context's) and two device event lists
 * (num_steps * num_envs entries each, a counter, a pinned word and an event per list), made once by the first ppo_dev_observe that passes `truncated`;
 * and the observation normaliser's statistics (2 * obs_size f64) and its two [num_envs, obs_size] f32 scratches, made once by the first
 * ppo_obs_norm_enable with mode != 0 (or the first ppo_obs_norm_set_h / ppo_obs_norm_apply) and kept;
 * and the reward normaliser's discounted-return accumulators (num_envs f64), its two f64 statistics and one [num_envs] f32 scratch, made once by the
 * first ppo_reward_norm_enable with mode != 0 (or the first ppo_reward_norm_set_h) and kept;
 * and the event list of ppo_env_truncation_bootstrap (num_steps * num_envs entries plus a counter), allocated by the first enable and kept. */
PPO_API ppo_status ppo_ctx_create(const ppo_config* cfg, ppo_ctx** out);
PPO_API void ppo_ctx_destroy(ppo_ctx* ctx);
/* Error text of the last failing call on ctx (ctx == NULL: of the last failing ppo_ctx_create in this thread).
 * The C++ facade rethrows it as std::runtime_error like the reference's obs-size check does (:370-375). */
PPO_API const char* ppo_last_error(const ppo_ctx* ctx);
PPO_API ppo_status ppo_sync(ppo_ctx* ctx);              /* block until the context's stream is idle */
PPO_API void* ppo_stream(ppo_ctx* ctx);                 /* hipStream_t */
PPO_API ppo_status ppo_get_config(const ppo_ctx* ctx, ppo_config* out);
PPO_API ppo_status ppo_buffer(ppo_ctx* ctx, int32_t which, void** dev_ptr, size_t* bytes);
PPO_API ppo_status ppo_device_alloc(ppo_ctx* ctx, size_t bytes, void** dev_ptr);
PPO_API ppo_status ppo_device_free(ppo_ctx* ctx, void* dev_ptr);
PPO_API ppo_status ppo_memcpy_h2d(ppo_ctx* ctx, void* dst_dev, const void* src_h, size_t bytes); /* synchronous */
PPO_API ppo_status ppo_memcpy_d2h(ppo_ctx* ctx, void* dst_h, const void* src_dev, size_t bytes); /* synchronous */

/* ---------------------------------------------------------------------------------------------------------
 * Agent (PPO/Agent.h:22-54)
 * ------------------------------------------------------------------------------------------------------- */
PPO_API int64_t ppo_param_count(const ppo_ctx* ctx);
/* 2*(n_hidden+1) tensors per net, critic first: rows {out,in} for weights and {out,1} for biases; PPO_DIST_GAUSSIAN: one more row {D,1}, log_std. */
PPO_API ppo_status ppo_param_shapes(const ppo_ctx* ctx, int64_t* shapes_h, int32_t* n_tensors);
/* Agent::ppoLayerInit (Agent.cpp:91-99): orthogonal_(W, gain) with gain sqrt(2) / 1.0 (critic head) / 0.01 (actor
 * head), bias 0.  Own Householder-QR of a Philox Gaussian (LibTorch's LAPACK+mt19937 draw is not reproducible). */
PPO_API ppo_status ppo_params_init_orthogonal(ppo_ctx* ctx, int64_t seed);
PPO_API ppo_status ppo_params_set_h(ppo_ctx* ctx, const float* params_h, int64_t count); /* also resets nothing else */
PPO_API ppo_status ppo_params_get_h(ppo_ctx* ctx, float* params_h, int64_t count);
PPO_API ppo_status ppo_optimizer_set_h(ppo_ctx* ctx, const float* exp_avg_h, const float* exp_avg_sq_h, int64_t count, int64_t step);
PPO_API ppo_status ppo_optimizer_get_h(ppo_ctx* ctx, float* exp_avg_h, float* exp_avg_sq_h, int64_t count, int64_t* step);

/* Agent::getValue (Agent.cpp:107-109): value[n] = Critic(obs[n,O]). */
PPO_API ppo_status ppo_get_value(ppo_ctx* ctx, const float* obs, int64_t n, float* value);
/* Agent::getActionAndValueDiscrete (Agent.cpp:117-128) / getActionAndValueMasked (:137-170).
 *   obs [n,O]; mask u8 [n,A] or NULL; forced_action i64 [n,H] or NULL (NULL -> sample, Categorical.cpp:73-79, with the
 *   context's counter-based generator keyed by (seed, env_offset+row, step_index, head));
 *   outputs action i64 [n,H] (the transposed layout the reference returns, Agent.cpp:168), logprob/entropy/value f32 [n]
 *   (log-probs and entropies summed over heads, :165-168).  Any output may be NULL.
 *   Arithmetic: that of the kernel ppo_rollout would run in this context now (PPO_KERNEL_ROLLOUT_VECTOR above): bit for bit the rollout's log-probs / actions. */
PPO_API ppo_status ppo_policy_act(ppo_ctx* ctx, const float* obs, const uint8_t* mask, const int64_t* forced_action, int64_t n,
                          int64_t step_index, int64_t* action, float* logprob, float* entropy, float* value);

/* ppo_policy_act for PPO_DIST_GAUSSIAN contexts (the counterpart of Agent::getActionAndValueDiscrete, Agent.cpp:117-128, for real-valued actions).
 *   obs [n,O]; forced_action f32 [n,D] or NULL (NULL -> sample); greedy != 0: action = the mean, bit for bit (no random number, forced_action ignored);
 *   outputs action f32 [n,D], logprob / entropy / value f32 [n] (summed over the D dimensions).  Any output may be NULL (action only with forced_action).
 *   Draws: eps_d from the context's counter-based generator keyed by (seed, env_offset + row, step_index, d) through Box-Muller with u1 in (0, 1]; the key
 *   uses a counter word no categorical draw uses, and a draw depends on nothing but its key (not on n, on chunking or on the entry point).
 *   Arithmetic: that of ppo_host_act_f32 / ppo_dev_act_f32 -- a stepwise loop of this call on the same observations and step indices reproduces a rollout
 *   bit for bit (tests/test_gpu_gaussian.py). */
PPO_API ppo_status ppo_policy_act_f32(ppo_ctx* ctx, const float* obs, const float* forced_action, int64_t n, int64_t step_index, int32_t greedy,
                                      float* action, float* logprob, float* entropy, float* value);

/* Categorical::mode / CategoricalMasked::mode (Categorical.cpp:139-141, CategoricalMasked.cpp:160-162) through the Agent
 * (Agent.cpp:117-170): action[n,H] = per head argmax of m_probs (masked logits set to -1e8 first), FIRST index on equal values;
 * logprob / entropy summed over heads for that action; value as ppo_get_value.  Outputs may be NULL except action.
 *   The deterministic policy of a trained or loaded agent (the reference's README: real-time inference, embedding into a game engine).  Draws no random
 *   number, touches no rollout state, does not advance the sampler: valid on every context kind at any time, PPO_ENV_HOST contexts in the middle of a
 *   rollout included.
 *   Arithmetic: as ppo_policy_act -- the logits of the kernel the context's rollout would run now (policy_act16_kernel's products by default; the vector form
 *   under PPO_KERNEL_ROLLOUT_VECTOR or when the weight-range snapshot says the output layer does not fit fp16, counted in vector_fallback_launches; generic
 *   networks: the generic engine's forward in the context's compute_dtype).  logprob, entropy and value are, bit for bit, what ppo_policy_act returns when the
 *   greedy action is passed back as forced_action. */
PPO_API ppo_status ppo_policy_act_greedy(ppo_ctx* ctx, const float* obs, const uint8_t* mask, int64_t n,
                                         int64_t* action, float* logprob, float* entropy, float* value);

/* ---------------------------------------------------------------------------------------------------------
 * Distributions (Distributions/Categorical.h:11-22, CategoricalMasked.h:12-23), stateless
 * ------------------------------------------------------------------------------------------------------- */
/* Constructor + log_prob + entropy + mode on logits [n,A]: m_logits = logits - logsumexp, m_probs = softmax
 * (Categorical.cpp:28-39; CategoricalMasked.cpp:31-46), log_prob = gather (:92-101), entropy (:112-119 / :127-144),
 * mode = argmax (:139-141).  value i64 [n] may be NULL; outputs may be NULL. */
PPO_API ppo_status ppo_categorical(int32_t dist_kind, const float* logits, const uint8_t* mask, const int64_t* value, int64_t n,
                           int32_t A, float* m_logits, float* m_probs, float* log_prob, float* entropy, int64_t* mode,
                           void* stream);

/* The diagonal Gaussian alone (beside ppo_categorical; torch.distributions.Normal summed over the last dimension): mean f32 [n,D], log_std f32 [D],
 * value f32 [n,D] or NULL.  value != NULL: log_prob [n] of value, sample (may be NULL) receives a copy of it.  value == NULL: sample [n,D] = mean +
 * exp(log_std) * eps with eps keyed by (seed; row_offset + row, step_index, d) as in ppo_policy_act_f32, log_prob of that sample.  entropy [n].
 * Outputs may be NULL.  1 <= D <= 32. */
PPO_API ppo_status ppo_gaussian(const float* mean, const float* log_std, const float* value, int64_t n, int32_t D, int64_t seed, int64_t row_offset,
                                int64_t step_index, float* sample, float* log_prob, float* entropy, void* stream);

/* Host-side counts, since the context's creation, of the launches of the three PPO_KERNEL_GAUSS_FUSED kernels: act (one per env step / ppo_policy_act_f32),
 * value (one per critic batch) and update (one per minibatch step).  All three are 0 on a context with neither fused flag: proof of which path ran, like
 * ppo_profile.vector_fallback_launches.  Outputs may be NULL.  PPO_ENV_PENDULUM's rollout launch (gauss_rollout_kernel) is none of the three: a ppo_rollout there
 * moves `value` by 2 and `act` not at all.  The same holds on PPO_ENV_MOUNTAINCAR_CONTINUOUS, whose truncation fold (gauss_trunc_fold_kernel) and evaluation
 * launch (gauss_eval_kernel) are none of the three either: a rollout moves `value` by 2 with ppo_env_truncation_bootstrap on or off, ppo_evaluate moves nothing.
 * A PPO_KERNEL_CAT_FUSED context counts its three kernels of the same family here (the two flags exclude each other, so a context has one set of counters): act =
 * one per env step or env group's step / ppo_policy_act / ppo_policy_act_greedy, value and update as above.  No symbol was added for it.
 * On either family every ppo_dev_observe that passes `truncated` adds 1 to `value`: its fold launch (gauss_dev_fold_kernel) is the critic kernel's forward
 * on the flagged rows, whether or not a row is flagged. */
PPO_API ppo_status ppo_gauss_fused_launches(ppo_ctx* ctx, int64_t* act, int64_t* value, int64_t* update);

/* Categorical::sample / CategoricalMasked::sample (Categorical.cpp:73-79: multinomial(probs, 1, replacement = true)) on given
 * m_probs [n,A]: inverse-CDF draw with the counter-based generator keyed by (seed; row_offset + row, step_index, head). */
PPO_API ppo_status ppo_categorical_sample(const float* m_probs, int64_t n, int32_t A, int64_t seed, int64_t row_offset, int64_t step_index,
                                  int32_t head, int64_t* sample, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Linear layers of networks wider than the reference's 2 x 64 (Agent.cpp:25-59 with the widths of BASELINE configs[4]), stateless
 * ------------------------------------------------------------------------------------------------------- */
/* c[M,N] = epilogue(sum_k A(m,k) B(n,k)) on the matrix cores, all operands f32 on the device:
 *   A(m,k) = trans_a ? a[k * lda + m] : a[m * lda + k],  B(n,k) = trans_b ? b[k * ldb + n] : b[n * ldb + k]
 *   forward  h = tanh(x W^T + b): (0, 0, rows, out, in, x, W, EPI_BIAS_TANH, aux = b)
 *   d(input) dz' = (dz W)(1 - h'^2): (0, 1, rows, in, out, dz, W, EPI_DTANH, aux = h' [M, ld_aux])
 *   d(weight) dW = dz^T x: (1, 1, out, in, rows, dz, x, EPI_NONE)
 * precision PPO_MM_F32X3: every f32 operand is carried as three bf16 terms (exact split) and every product as six bf16 MFMAs with
 * f32 accumulation -- f32 accuracy; PPO_MM_BF16: one round-to-nearest bf16 term per operand, f32 accumulation. */
enum { PPO_MM_EPI_NONE = 0, PPO_MM_EPI_BIAS = 1, PPO_MM_EPI_BIAS_TANH = 2, PPO_MM_EPI_DTANH = 3 };
enum { PPO_MM_F32X3 = 0, PPO_MM_BF16 = 1 };
PPO_API ppo_status ppo_matmul(int32_t trans_a, int32_t trans_b, int64_t M, int64_t N, int64_t K, const float* a, int64_t lda, const float* b,
                      int64_t ldb, float* c, int64_t ldc, int32_t epilogue, const float* aux, int64_t ld_aux, int32_t precision,
                      void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Environments (Environments/CartPole.h, MountainCar.h) and their vectorised driver
 * ------------------------------------------------------------------------------------------------------- */
/* Stateless batched CartPole::step (CartPole.cpp:47-94) / MountainCar::step (MountainCar.cpp:29-57) on injected
 * states: state_in [n,O] (array-of-structs like the reference's std::vector<float> state), action i64 [n];
 * outputs next_state [n,O], reward f32 [n], terminated i32 [n].  PPO_ENV_ACROBOT: the same call with state_in / next_state [n,4] (the state, not the
 * observation) and action in {0, 1, 2}.  PPO_ENV_TAXI: likewise with state (row, col, pass, dest) [n,4] and action in 0..5 (clamped; state components too). */
PPO_API ppo_status ppo_env_transition(int32_t env_kind, const float* state_in, const int64_t* action, int64_t n, float* next_state,
                              float* reward, int32_t* terminated, void* stream);
/* First n_resets reset states [n_resets,4] of std::mt19937(seed) + uniform_real_distribution<float>(-0.05,0.05)
 * (CartPole.h:28-29, CartPole.cpp:3-4,34-45): host-side table builder used by the context. */
PPO_API ppo_status ppo_cartpole_reset_stream_h(int64_t seed, int64_t n_resets, float* out_h);
/* PPO_Discrete::initEnvs (PPO_Discrete.cpp:365-402): resets every env (env 0 twice, :368+:389), fills NEXT_OBS,
 * zeroes NEXT_DONE; checks obs_size against the env (:370-375 -> PPO_ERR_INVALID with the reference's message). */
PPO_API ppo_status ppo_env_reset(ppo_ctx* ctx);
/* PPO_Discrete::stepEnvs (PPO_Discrete.cpp:413-483): action i64 [N,H] (column 0 drives the env);
 * outputs obs [N,O] (first obs of the new episode where done), reward f32 [N], done i32 [N]. */
PPO_API ppo_status ppo_env_step(ppo_ctx* ctx, const int64_t* action, float* obs, float* reward, int32_t* done);
/* ppo_env_step for a context whose env takes real-valued actions (PPO_ENV_PENDULUM, PPO_ENV_MOUNTAINCAR_CONTINUOUS): action f32 [N,D] (the raw action; the env clips its own copy), the same
 * outputs and the same auto-reset bookkeeping.  ppo_env_step on such a context returns PPO_ERR_UNSUPPORTED and names this call; this call returns
 * PPO_ERR_UNSUPPORTED on a context with integer actions and on PPO_ENV_HOST contexts. */
PPO_API ppo_status ppo_env_step_f32(ppo_ctx* ctx, const float* action /* [N,D] */, float* obs, float* reward, int32_t* done);
/* ppo_env_transition for PPO_ENV_PENDULUM (any other env_kind: PPO_ERR_UNSUPPORTED): stateless; state_in f32 [n,2], action f32 [n,D] (D = 1, raw);
 * outputs next_state [n,2], obs_out [n,3] = the observation of next_state or NULL, reward f32 [n], terminated i32 [n] (always 0).
 * PPO_ENV_MOUNTAINCAR_CONTINUOUS: the same call with obs_out [n,2] (= next_state, bit for bit) or NULL and terminated as the step computes it (the goal
 * reached with a velocity >= 0).  Null pointers (obs_out aside) or n < 0: PPO_ERR_INVALID; n = 0: PPO_OK, nothing is launched. */
PPO_API ppo_status ppo_env_transition_f32(int32_t env_kind, const float* state_in, const float* action, int64_t n, float* next_state, float* obs_out,
                                          float* reward, int32_t* terminated, void* stream);
/* Inject / read env state for teacher-forced parity: state_h [N,O] AoS, ep_len i32, ep_rew f32, reset_count i32 (NULL = skip). */
PPO_API ppo_status ppo_env_set_state_h(ppo_ctx* ctx, const float* state_h, const int32_t* ep_len_h, const float* ep_rew_h,
                               const int32_t* reset_count_h);
PPO_API ppo_status ppo_env_get_state_h(ppo_ctx* ctx, float* state_h, int32_t* ep_len_h, float* ep_rew_h, int32_t* reset_count_h);

/* ---------------------------------------------------------------------------------------------------------
 * Rollout and advantages
 * ------------------------------------------------------------------------------------------------------- */
/* The rollout loop of PPO_Discrete::train (PPO_Discrete.cpp:524-548; PPO_MultiDiscrete.cpp:547-571) as ONE launch:
 * T x { store obs/done, policy forward + sample, store value/action/logprob, env step + auto-reset, store reward }.
 * forced_actions i64 [T,N,H] or NULL (teacher-forcing for parity).  Leaves NEXT_OBS / NEXT_DONE for the bootstrap. */
PPO_API ppo_status ppo_rollout(ppo_ctx* ctx, const int64_t* forced_actions);
/* ppo_rollout for Gaussian device-env contexts (PPO_ENV_PENDULUM, PPO_ENV_MOUNTAINCAR_CONTINUOUS): forced_actions f32 [T,N,D] or NULL; a forced action is stored in PPO_BUF_ACTIONS as given,
 * with the log-prob ppo_policy_act_f32 gives it, and steps the env.  ppo_rollout(ctx, NULL) on such a context is this call with NULL; ppo_rollout with a
 * non-NULL i64 array there returns PPO_ERR_UNSUPPORTED and names this call.  PPO_ERR_UNSUPPORTED on a categorical context and on PPO_ENV_HOST contexts. */
PPO_API ppo_status ppo_rollout_f32(ppo_ctx* ctx, const float* forced_actions /* [T,N,D] or NULL */);
/* Time-limit truncations of the context's own environments (new): bootstrap the value where the time limit cut an episode off.
 *
 * The reference ends an episode that reaches max_episode_steps exactly like one the env terminated (PPO_Discrete.cpp:443-452), so the scan cuts the return
 * there with a bootstrap of 0 and the critic learns that the state in front of the limit is worth nothing -- for CartPole, whose good policies reach the
 * limit in almost every episode, and MountainCar, which reaches it in every episode until it has learnt.  Callers of the ppo_host_* calls pass the final
 * observation themselves (ppo_host_observe_truncated below).  For PPO_ENV_CARTPOLE and PPO_ENV_MOUNTAINCAR nothing needs to be passed: the observation IS
 * the env state, so the final observation of the episode that ended at (t, n) is one env step of PPO_BUF_OBS[t, n] under PPO_BUF_ACTIONS[t, n, 0].
 *
 * Off by default, and off is off: a context that never turns the switch on -- or turned it off again -- runs what it ran before, launch for launch and
 * bit for bit.  With the switch on, ppo_rollout (and hence ppo_train_iteration) enqueues ONE more launch, behind the rollout's value launch and in front of
 * the scan.  For every i = t * N + n with PPO_BUF_FIN_LEN[i] == max_episode_steps it recomputes that step with the env kernels' own device function; where
 * the env itself terminated on the step the end is real and nothing happens; elsewhere
 *   v = Critic(final observation);  PPO_BUF_REWARDS[i] = f32(PPO_BUF_REWARDS[i] + f32(gamma * v)),  gamma = cfg.gamma  (two roundings, no FMA)
 * and (i, v) joins the rollout's event list, which starts empty.  v is bit for bit the value the launch that fills PPO_BUF_VALUES gives that observation
 * (the matrix-core critic for both envs, under every kernel_flags value and weight range, as for ppo_bootstrap_rewards; no fall-back is counted), so
 * delta = r + gamma V(final) - V(obs_t) is formed from ONE critic.  Raw rewards: PPO_BUF_REWARDS holds the folded rewards after ppo_rollout; FIN_REW,
 * EP_REW, the episode ring and every episode statistic keep the raw reward.  ppo_evaluate is untouched.  The common workgroup -- no episode at the limit
 * among its 256 samples -- costs one pass over FIN_LEN.  Works with forced_actions; purely local: no collective on a sharded context.
 * Errors: PPO_ERR_UNSUPPORTED on a PPO_ENV_SYNTHETIC context (its observations are noise: an episode there has no last observation), on a PPO_ENV_PENDULUM
 * context (the fold rebuilds the final observation from PPO_BUF_OBS, and a Pendulum observation does not hold theta) and on a
 * PPO_ENV_HOST context (the message names ppo_host_observe_truncated); PPO_ERR_INVALID for `on` outside 0..1 (and a null count, or arrays shorter than the
 * list, in ppo_env_truncations).  A failing call changes nothing.
 * PPO_ENV_MOUNTAINCAR_CONTINUOUS (obs_size 2: the observation is the state there too) is served with the same contract, word for word, on the fused Gaussian
 * critic: the fold is one launch of gauss_trunc_fold_kernel behind the rollout's two critic launches and in front of the scan; the step is recomputed from
 * PPO_BUF_OBS[i] under the RAW f32 action PPO_BUF_ACTIONS[i, 0] with the env's own device function; v is bit for bit what ppo_get_value gives the final
 * observation (gauss_values_kernel's forward); the grid covers the T * N rows in workgroups of 256, and the critic's weights are staged only by workgroups
 * that found an event.  The fold launch is none of the kernels ppo_gauss_fused_launches counts.
 * PPO_KERNEL_ENV_CUT_STATE (kernel_flags, above) serves the two calls on every device env of the fused families, with the same contract: the rollout has kept
 * the state each cut-off episode ended in and whether the env itself terminated there, so the fold (ONE launch of cut_state_fold_kernel, in the same place)
 * recomputes nothing -- for every i with PPO_BUF_FIN_LEN[i] == max_episode_steps and the terminated word clear, the final observation is the env's observation
 * of the kept state, v is bit for bit what ppo_get_value gives it, and the reward and the event list are formed as above.  On PPO_ENV_PENDULUM, where no
 * episode ends anywhere else, every finished episode is an event.  Without the flag the errors above stand. */
PPO_API ppo_status ppo_env_truncation_bootstrap(ppo_ctx* ctx, int32_t on);   /* 0 off (default), 1 on */
/* The events of the last ppo_rollout, with ppo_host_truncations' contract: count; flat indices t * N + n ascending (sorted on the host at read time); the
 * values V(final obs) that were folded in.  Before any rollout, and after a rollout with the switch off: count = 0.  index_h / value_h may be NULL (count
 * only); cap = room in the arrays (cap < count with a non-NULL array -> PPO_ERR_INVALID).  Waits for the fold only, not for an update behind it. */
PPO_API ppo_status ppo_env_truncations(ppo_ctx* ctx, int64_t* count, int32_t* index_h, float* value_h, int64_t cap);
/* PPO_Discrete::calcAdvantage (PPO_Discrete.cpp:274-331) on the context's buffers: bootstrap NEXT_VALUE = Critic(NEXT_OBS)
 * (:280), then GAE (:283-306) or n-step returns (:309-329) by cfg.use_gae; fills ADVANTAGES and RETURNS. */
PPO_API ppo_status ppo_calc_advantage(ppo_ctx* ctx);
/* The same scan on caller buffers (all [T,N] time-major f32; next_value f32 [N]; next_done i32 [N]).  Exact mode:
 * the reference's association and evaluation order along t, no FMA contraction -> bit-identical advantages/returns. */
PPO_API ppo_status ppo_gae(const float* rewards, const float* values, const float* dones, const float* next_value,
                   const int32_t* next_done, int64_t T, int64_t N, float gamma, float gae_lambda, float* advantages,
                   float* returns, void* stream);
/* The same scan in FAST mode -- north_star's "segmented prefix sum": the recurrence as a scan of affine maps (c, d) o (c', d') = (c c', d + c d') over
 * chunks of rows, all lanes busy, a done flag cuts the segment.  NOT bit-identical to PPO_Discrete.cpp:283-306 (the carry into a chunk is associated
 * differently: <= 6 ULP of the largest advantage the chain has carried, measured); training (ppo_calc_advantage) never uses it.  Kept to state, with a number, what giving up the
 * reference's association order would buy (profiles/NOTES.md). */
PPO_API ppo_status ppo_gae_fast(const float* rewards, const float* values, const float* dones, const float* next_value,
                        const int32_t* next_done, int64_t T, int64_t N, float gamma, float gae_lambda, float* advantages,
                        float* returns, void* stream);
PPO_API ppo_status ppo_nstep_returns(const float* rewards, const float* values, const float* dones, const float* next_value,
                             const int32_t* next_done, int64_t T, int64_t N, float gamma, float* advantages, float* returns,
                             void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Update (PPO_Discrete.cpp:554-648)
 * ------------------------------------------------------------------------------------------------------- */
/* torch::randperm replacement (:569): fills PERM[epoch] for every epoch of the coming update with a keyed
 * cycle-walking Feistel permutation of [0,B) (seed, update, epoch). */
PPO_API ppo_status ppo_generate_permutations(ppo_ctx* ctx);
/* One minibatch, forward + losses + backward (:576-638) on batch rows idx i32 [M] (device).  Leaves the UNCLIPPED
 * gradient of the global-minibatch loss in GRADS (local contribution when sharded) and the loss scalars in the stats. */
PPO_API ppo_status ppo_minibatch_forward_backward(ppo_ctx* ctx, const int32_t* idx, int64_t M);
/* New in the build (no reference counterpart): sum GRADS over ranks with one all-reduce on the context's transport
 * (direct exchange, RCCL or in-process group). No-op unsharded. */
PPO_API ppo_status ppo_allreduce_grads(ppo_ctx* ctx);
/* clip_grad_norm_ (:640; LibTorch clip_grad.h:22-85) + AdamW::step (:641; eps 1e-5f, betas .9/.999, weight_decay 1e-2,
 * :76-78) as one fused launch. */
PPO_API ppo_status ppo_optimizer_step(ppo_ctx* ctx);
/* All epochs x minibatches of one update (:567-644) with the context's own permutations, then explained variance (:647-648). */
PPO_API ppo_status ppo_update(ppo_ctx* ctx);
/* One iteration of the training loop (:511-659 minus printing/checkpoints): LR anneal, rollout, advantages, update. */
PPO_API ppo_status ppo_train_iteration(ppo_ctx* ctx);
/* Synchronises and returns the scalars of the last update (printPPOResults' inputs, :700-774).
 * Sharded runs (2..8 ranks): every number is the JOB's and identical on every rank, as the reference prints one table (:700-774).  The loss scalars
 * (pg / value / entropy loss, approx-KL, clipfrac, grad norm) ride the gradient all-reduce; the explained-variance sums (:647-648) and every
 * rank's ring of finished episodes, each episode tagged with its position in the reference's push order (step, then global env index; :474-480),
 * ride the per-update all-reduce of the advantage sums, and the host rebuilds the job's CircularBuffer(100) from the union: ep_rew_mean /
 * ep_len_mean / ep_count are what ONE context over all envs would report.  They describe the state at the last ppo_update: episodes that end in
 * a rollout taken AFTER it are not in them yet -- unlike a single context (one rank), whose episode ring is read as it stands.  ppo_comm_init
 * refuses more than 8 ranks (the block holds 8 slots: one node).  While a snapshot is pending (ppo_stats_snapshot) ppo_read_stats fails: read it first.
 * Device-side error words (reset table exhausted, fp16 range of the matrix-core rollout, a bounded wait of the update kernel or of the scan) surface here and in
 * ppo_stats_snapshot_read as PPO_ERR_STATE; a host that runs an iteration ahead of its snapshots (the facade's train()) learns of them one
 * iteration late and must check the snapshot before it writes a checkpoint (it does). */
PPO_API ppo_status ppo_read_stats(ppo_ctx* ctx, ppo_stats* out);
/* The same read in two steps, for a host that prints a table per update (printPPOResults, :700-774) and must not drain the GPU to do it:
 * ppo_stats_snapshot enqueues, behind the work enqueued so far, asynchronous copies of everything the statistics are made of into one pinned block
 * and notes the host-side training state; ppo_stats_snapshot_read waits for that snapshot only -- iterations enqueued after it keep running -- and
 * decodes it.  ppo_read_stats = snapshot + read + ppo_sync.  At most two snapshots may be pending (a host that runs one iteration ahead takes the
 * next one before it reads the previous one); they are read oldest first. */
PPO_API ppo_status ppo_stats_snapshot(ppo_ctx* ctx);
PPO_API ppo_status ppo_stats_snapshot_read(ppo_ctx* ctx, ppo_stats* out);
/* LR anneal (:514-518) is applied by ppo_train_iteration; direct control for tests. */
PPO_API ppo_status ppo_set_learning_rate(ppo_ctx* ctx, double lr);

/* ---------------------------------------------------------------------------------------------------------
 * Early stop at a target KL (extension: the reference's epoch loop, PPO_Discrete.cpp:567-644, is CleanRL's without
 * `if target_kl is not None and approx_kl > target_kl: break`; the estimator is the reference's, :352)
 * ------------------------------------------------------------------------------------------------------- */
/* CleanRL's semantics, decided on the device: ppo_update enqueues all update_epochs x num_minibatches steps at once, as always, and nothing inside it waits
 * for the GPU.  With target_kl > 0, behind the optimizer step of the LAST minibatch of every epoch e a one-workgroup launch compares that step's approx_kl
 * -- the float the step writes to its statistics, the job's value on sharded contexts, so every rank decides alike -- with the target (a NaN compares
 * false).  Above it, no later optimizer step of this update is applied: parameters, both AdamW moments and the applied-step count stay as epoch e left
 * them, and the update's statistics stay those of the last applied step (all of ppo_stats: clipfrac_mean is the mean over the applied steps,
 * optimizer_steps counts applied steps; explained variance does not depend on the steps).  The stop travels as one more bit of the context's device error
 * word, which the optimizer kernels already read (they apply no step behind a device-side error either); it is not an error, no reader reports it, and it
 * is cleared before the update ends: the stand-alone ppo_minibatch_forward_backward / ppo_allreduce_grads / ppo_optimizer_step never stop.
 * Cost: update_epochs + 1 small launches per update, and ppo_update first waits for the PREVIOUS update's outcome (one event behind one small copy; for
 * nothing enqueued after that update) to know how many steps were applied: the AdamW bias corrections are formed on the host per applied step.  A caller-
 * stepped context never blocks there (a whole host rollout lies between two updates); a host that runs ahead on the device envs loses part of its lead.
 * NOT built: the forward / backward launches of the unapplied steps still run and their results are discarded, so an update that stops early takes as long
 * as one that does not.
 * target_kl = 0 (the default) is off, and off is off: a context that never sets a target, or sets it back to 0, enqueues exactly the launches it always
 * did and produces the same bits.  A negative or non-finite target returns PPO_ERR_INVALID and changes nothing.  Valid on every context kind, at any time;
 * takes effect at the next ppo_update (the one inside ppo_train_iteration and ppo_host_rollout_end included). */
PPO_API ppo_status ppo_target_kl_set(ppo_ctx* ctx, double target_kl);
PPO_API ppo_status ppo_target_kl_get(ppo_ctx* ctx, double* out);
/* The last ppo_update's outcome: epochs whose steps were applied, whether a stop was raised, the approx_kl that raised it (0.0 when none did), and the sum of
 * epochs_run over all updates of the context.  Waits for that update only, not for work enqueued behind it.  Before any update: 0, 0, 0.0, 0.  With the
 * feature off: epochs_run = update_epochs, stopped = 0 (no wait at all).  Any output may be NULL.  ppo_stats.optimizer_steps, ppo_optimizer_get_h's step and
 * the statistics snapshots report applied steps as well, and a stand-alone ppo_optimizer_step behind a stopped update continues from them.  After a
 * ppo_update that FAILED with a target set the stop is still cleared, but the step and epoch counts are undefined. */
PPO_API ppo_status ppo_early_stop_read(ppo_ctx* ctx, int32_t* epochs_run, int32_t* stopped, double* kl_at_stop, int64_t* epochs_total);

/* ---------------------------------------------------------------------------------------------------------
 * Caller-stepped environments (PPO_ENV_HOST contexts; PPO_Discrete::initEnvs / stepEnvs / train, PPO_Discrete.cpp:365-483, 511-548)
 *
 *   ppo_host_env_reset(ctx, obs0)                                    once: every env's reset observation
 *   per iteration:  ppo_host_rollout_begin(ctx)
 *                   T x { ppo_host_act(ctx, mask, actions); step the envs on the host; ppo_host_observe(ctx, obs, reward, done, fin_len, fin_rew) }
 *                   ppo_host_rollout_end(ctx)                        enqueues the values, the scan and the update (ppo_stats_snapshot / ppo_read_stats as usual)
 *   (or group by group, the env stepping of one group overlapped with the policy call of the next: "Env groups" below)
 *
 * Arithmetic: that of a device-env context of the same shape.  The sampler key is (seed, env_offset + row, rollout_steps + t, head); for the
 * reference's shapes the actor runs rollout16_kernel's products (policy_act16_kernel) or, under PPO_KERNEL_ROLLOUT_VECTOR, the vector form, chosen
 * ONCE per rollout at ppo_host_rollout_begin from the same weight-range snapshot as ppo_rollout (weights outside fp16 send the whole rollout to the
 * vector form, counted in ppo_profile.vector_fallback_launches); values are one batched launch at ppo_host_rollout_end, as ppo_rollout's tail.  A
 * host-stepped CartPole reproduces ppo_train_iteration bit for bit (tests/test_gpu_host_env.py).
 * One launch per env step: ppo_host_act commits the step ppo_host_observe staged and acts on the next one in one kernel and waits for that kernel
 * only; ppo_host_observe copies into pinned staging and launches nothing.
 * Errors: the ppo_host_* calls return PPO_ERR_STATE on a context with a device env and out of sequence (act twice without observe, observe
 * before act, end before T steps, begin while a rollout is open); such a call changes nothing.
 * ------------------------------------------------------------------------------------------------------- */
/* initEnvs (PPO_Discrete.cpp:365-402) for caller-stepped envs: obs_h f32 [N,O] (host) = every env's reset observation.
 * NEXT_OBS = obs_h, NEXT_DONE = 0, per-env episode sums = 0.  Synchronous. */
PPO_API ppo_status ppo_host_env_reset(ppo_ctx* ctx, const float* obs_h);
/* Opens the rollout of one iteration: the LR anneal ppo_train_iteration applies (:514-518); t = 0. */
PPO_API ppo_status ppo_host_rollout_begin(ppo_ctx* ctx);
/* Step t of :524-548: m_obs[t] = next_obs, m_dones[t] = next_done, actor forward + sample, m_actions[t], m_logprobs[t] (and masks [t]);
 * mask_h u8 [N,A] or NULL (masked policies; NULL = all valid); returns when action_h i64 [N,H] (host) holds the actions. */
PPO_API ppo_status ppo_host_act(ppo_ctx* ctx, const uint8_t* mask_h, int64_t* action_h);
/* The same step for a PPO_DIST_GAUSSIAN context: returns when action_h f32 [N,D] (host) holds the raw samples mu + sigma * eps (unclipped: clip the copy
 * given to the env; m_actions[t] keeps the raw sample).  ppo_host_observe / ppo_host_observe_truncated / ppo_host_rollout_end are used unchanged. */
PPO_API ppo_status ppo_host_act_f32(ppo_ctx* ctx, float* action_h /* [N,D] */);
/* stepEnvs' outputs for step t (:413-483): next_obs_h [N,O] (already the reset observation where done), reward_h f32 [N], done_h i32 [N]
 * (truncation included; ppo_host_observe_truncated tells the two apart).  fin_len_h i32 [N] / fin_rew_h f32 [N]: the length and reward of the episodes that finished, as the reference reads
 * them from env->episode_length / episode_reward (:474-480), read where done only (a length of 0 is not counted as an episode).  NULL = the
 * context keeps them as running sums (steps counted, rewards summed), which is what CartPole and MountainCar report.  The data is copied
 * before the call returns. */
PPO_API ppo_status ppo_host_observe(ppo_ctx* ctx, const float* next_obs_h, const float* reward_h, const int32_t* done_h, const int32_t* fin_len_h,
                                    const float* fin_rew_h);
/* After T act/observe pairs: values of every stored observation and the bootstrap value (:280), the scan, the update: the rest of
 * ppo_train_iteration.  Enqueued; rollout_steps += T, global_step += T * global_num_envs, finished episodes pending, as after ppo_rollout. */
PPO_API ppo_status ppo_host_rollout_end(ppo_ctx* ctx);

/* Env groups: the same rollout taken group by group, so that the caller steps one group's envs while the GPU and the host link serve another's.
 *
 *   per iteration:  ppo_host_rollout_begin_groups(ctx, n_groups, bounds)
 *                   per group g, T x { ppo_host_group_act(ctx, g, mask_g);              enqueues and returns
 *                                      ppo_host_group_actions(ctx, g, actions_g);       waits for group g's launch only
 *                                      step the group's envs on the host;
 *                                      ppo_host_group_observe(ctx, g, obs_g, reward_g, done_g, fin_len_g, fin_rew_g) }
 *                   ppo_host_rollout_end(ctx)                                           once every group has observed its step T - 1
 *
 * Group g owns env rows [bounds[g], bounds[g + 1]); every array of a group call holds that group's rows only ([n_g, ...]).  Groups advance
 * independently: the calls of different groups interleave in any order, and one group may be any number of steps ahead of another.  A typical
 * pipeline enqueues ppo_host_group_act(g + 1) before it reads ppo_host_group_actions(g), and steps group g on worker threads meanwhile.
 * The rollout does not depend on the grouping or the interleaving in a single bit: the sampler is keyed by (seed, env_offset + row, rollout_steps + t,
 * head), a row's arithmetic does not depend on the launch it sits in, and finished episodes reach the statistics from FIN_LEN / FIN_REW after the
 * rollout (tests/test_gpu_host_env_groups.py).  Everything is enqueued on the context's one stream; only the host-side wait is per group.
 * Errors: PPO_ERR_STATE (nothing changed; the message names group and step) for a group call on a rollout opened with ppo_host_rollout_begin,
 * ppo_host_act / ppo_host_observe on a rollout opened here, a group's calls out of sequence, an act beyond step T - 1, ppo_host_rollout_end before
 * every group is done, a begin while a rollout is open, and device-env contexts; PPO_ERR_INVALID for n_groups outside 1 .. PPO_HOST_MAX_GROUPS,
 * bounds that are not 0 = b[0] < b[1] < ... < b[n_groups] = num_envs, g out of range, null pointers, and fin_len_h / fin_rew_h not both-or-neither. */
#define PPO_HOST_MAX_GROUPS 8
/* ppo_host_rollout_begin with the envs cut into n_groups row ranges: bounds_h i32 [n_groups + 1] (host; copied).  Every group starts at step 0. */
PPO_API ppo_status ppo_host_rollout_begin_groups(ppo_ctx* ctx, int32_t n_groups, const int32_t* bounds_h);
/* ppo_host_act for group g's rows at the group's step t_g, WITHOUT the wait: commit of the group's staged step t_g - 1, actor forward, sample, the
 * rollout stores of step t_g, actions into pinned host memory, an event of the group's own.  mask_h u8 [n_g,A] or NULL; copied before return. */
PPO_API ppo_status ppo_host_group_act(ppo_ctx* ctx, int32_t g, const uint8_t* mask_h);
/* Waits for group g's act (its event, not the stream: launches enqueued behind it keep running) and copies its actions out: action_h i64 [n_g,H]. */
PPO_API ppo_status ppo_host_group_actions(ppo_ctx* ctx, int32_t g, int64_t* action_h);
/* ppo_host_observe for group g's rows (all arrays [n_g, ...]); host memory only, no launch. */
PPO_API ppo_status ppo_host_group_observe(ppo_ctx* ctx, int32_t g, const float* next_obs_h, const float* reward_h, const int32_t* done_h,
                                          const int32_t* fin_len_h, const float* fin_rew_h);

/* Time-limit truncations (new): bootstrap the value where an episode was cut off instead of ended.
 *
 * The reference ends an episode that reaches max_episode_steps exactly like one the env terminated (PPO_Discrete.cpp:443-452: episode_length ==
 * max_episode_steps sets terminated = true, and the `truncated` flag its envs return is always false and never read): the scan cuts the return there
 * with a bootstrap of 0, which teaches the critic that the state in front of the limit is worth nothing.  Its framework cannot do better -- it never
 * sees the observation the episode ended on.  The caller of the ppo_host_* calls does: it holds step()'s observation when it resets the env.  With it
 * the usual partial-episode bootstrap applies: at a truncation at (t, n) the reward becomes r + gamma * V(final observation), and the scan runs unchanged.
 *
 *   T x { ppo_host_act; step the envs; ppo_host_observe_truncated(ctx, obs, reward, done, fin_len, fin_rew, truncated, final_obs) }
 *
 * Off unless these calls are used: a rollout without a truncation event is, launch for launch and bit for bit, the rollout of the plain calls.  The
 * plain and the _truncated observes mix freely within a rollout and across groups.  The observes only append (t * N + n, final observation) to a list
 * in pinned host memory -- no launch, no sorting per step.  ppo_host_rollout_end, behind the value launch and in front of the scan, with K events:
 * K == 0 enqueues nothing; K > 0 sorts the list by index on the host (the outcome does not depend on how groups interleaved), enqueues ONE asynchronous
 * copy of it and one fold launch on PPO_BUF_REWARDS with gamma = cfg.gamma.  V is the value this context's rollout assigns to that observation: the fold
 * runs the arithmetic of the launch that fills PPO_BUF_VALUES (bootstrap_values_mfma_kernel / bootstrap_values_kernel; generic networks: the engine's
 * critic forward, then fold_rewards_kernel), so delta = r + gamma V(final) - V(obs_t) is formed from ONE critic.  PPO_BUF_REWARDS holds the folded
 * rewards after ppo_host_rollout_end; FIN_REW, EP_REW and the episode statistics keep the raw rewards.  Purely local: no collective on a sharded context.
 * Errors: the PPO_ERR_STATE cases of the plain calls (device-env context, out of sequence, wrong rollout kind); a failing call changes nothing. */
/* ppo_host_observe plus: truncated_h i32 [N] -- non-zero where the episode that ended at this step was cut off (time limit) rather than terminated;
 * final_obs_h f32 [N,O] -- the LAST observation of that episode (what step() returned, before the reset), read only in rows where truncated_h != 0.
 * truncated_h[n] != 0 requires done_h[n] != 0 (else PPO_ERR_INVALID, the message names the row); a non-zero flag with final_obs_h == NULL is
 * PPO_ERR_INVALID.  truncated_h == NULL means no truncation (then final_obs_h may be NULL) and the call IS ppo_host_observe. */
PPO_API ppo_status ppo_host_observe_truncated(ppo_ctx* ctx, const float* next_obs_h, const float* reward_h, const int32_t* done_h, const int32_t* fin_len_h,
                                              const float* fin_rew_h, const int32_t* truncated_h, const float* final_obs_h);
/* The same for group g's rows (all arrays [n_g, ...]). */
PPO_API ppo_status ppo_host_group_observe_truncated(ppo_ctx* ctx, int32_t g, const float* next_obs_h, const float* reward_h, const int32_t* done_h,
                                                    const int32_t* fin_len_h, const float* fin_rew_h, const int32_t* truncated_h, const float* final_obs_h);
/* Truncation events of the last CLOSED rollout (while a rollout is open: of the one before it; before any rollout: count = 0): count; flat indices
 * t * N + n ascending; the bootstrap values V(final obs) that were folded in.  index_h / value_h may be NULL (count only); cap = room in the arrays
 * (cap < count with a non-NULL array -> PPO_ERR_INVALID).  Waits for the fold only, not for the update behind it. */
PPO_API ppo_status ppo_host_truncations(ppo_ctx* ctx, int64_t* count, int32_t* index_h, float* value_h, int64_t cap);
/* The fold on caller buffers, with the context's critic (any context kind, any time): for k < K
 *   v = Critic(final_obs[k]);  rewards[index[k]] = rewards[index[k]] + gamma * v  (two f32 roundings, no FMA);  value_out[k] = v (may be NULL).
 * final_obs f32 [K,O], index i32 [K] (distinct: the caller's promise; no atomics are used), rewards f32, value_out f32 [K]: device pointers.  v is
 * bit for bit ppo_get_value's.  K == 0: no launch.  Null pointers with K > 0, or K < 0: PPO_ERR_INVALID. */
PPO_API ppo_status ppo_bootstrap_rewards(ppo_ctx* ctx, const float* final_obs, const int32_t* index, int64_t K, float gamma, float* rewards, float* value_out);

/* Caller-stepped environments on the device (new): act and observe through DEVICE arrays, for envs that already live on the GPU (the caller's own HIP
 * kernels, PyTorch-ROCm tensors).  The reference steps its envs on the host between two device calls (PPO_Discrete.cpp:365-483, 524-548); with the ppo_host_*
 * calls above a device-resident env pays two PCIe crossings and one host wait per step for that.  These calls keep the step on the chip:
 *
 *   ppo_dev_env_reset(ctx, obs0, stream)                             once
 *   per iteration:  ppo_host_rollout_begin(ctx)
 *                   T x { ppo_dev_act(ctx, mask, action, stream); the caller's env kernels on `stream`;
 *                         ppo_dev_observe(ctx, obs, reward, done, fin_len, fin_rew, truncated, final_obs, stream) }
 *                   ppo_host_rollout_end(ctx)                        (ppo_host_truncations as usual)
 *
 * They serve PPO_ENV_HOST contexts.  Every bulk pointer is a DEVICE pointer; caller_stream is the hipStream_t on which the caller produces and consumes them.
 * Stream semantics:
 *   - Every call only enqueues.  None of the three waits for the device or copies to or from host memory.
 *   - The context's stream (ppo_stream) is created hipStreamNonBlocking, so the hand-over is explicit: on entry the call records an event on
 *     caller_stream and makes the context's stream wait for it; after its last launch it records an event on the context's stream and makes caller_stream
 *     wait for that.
 *   - Input arrays are therefore consumed in stream order, like hipMemcpyAsync's source: work the caller enqueues on caller_stream after the call returns
 *     may overwrite them.  `action` is valid for work enqueued on caller_stream after ppo_dev_act returns.
 *   - caller_stream == ppo_stream(ctx) means "the same stream": no events.  NULL is the null stream and gets the event hand-over like any other stream; it
 *     is NOT shorthand for the context's stream.
 * Launches per env step: ppo_dev_act one, ppo_dev_observe one, or two when `truncated` is passed.  ppo_dev_observe COMMITS its step at once (the ppo_host_*
 * calls stage it for the next act), so ppo_host_rollout_end of a device-fed rollout has no step to commit and no events to fold: it goes straight to the
 * value launch, the scan and the update.  Everything else is as for the host calls: the sampler key (seed, env_offset + row, rollout_steps + t, head), the
 * choice of arithmetic once per rollout, rollout_steps / global_step / finished episodes, the generic engine's per-step sequence, PPO_BUF_MASKS: a
 * device-fed rollout equals the host-fed rollout of the same data bit for bit (tests/test_gpu_dev_env.py).
 * A rollout is host-fed or device-fed AS A WHOLE; its first act decides.  Errors: PPO_ERR_STATE for a ppo_host_act / ppo_host_observe in a device-fed
 * rollout and a ppo_dev_act / ppo_dev_observe in a host-fed one (the message names both families), for ppo_dev_* on a rollout opened with
 * ppo_host_rollout_begin_groups (groups hide a host wait that does not exist here), and for the sequence errors of the host calls (act twice, observe
 * before act, act beyond step T - 1, end early, device-env context).  PPO_ERR_INVALID for a null action / next_obs / reward / done, fin_len / fin_rew
 * not both-or-neither, and truncated != NULL with final_obs == NULL.  A failing call enqueues nothing and changes nothing.
 * Truncations: with truncated != NULL one more launch per observe, behind the commit, folds the bootstrap where truncated[n] != 0 AND done[n] != 0:
 * PPO_BUF_REWARDS[t, n] = f32(r + f32(gamma * V(final_obs[n]))), gamma = cfg.gamma, V bit for bit ppo_get_value's (the kernel ppo_bootstrap_rewards would
 * run for this context); FIN_REW, EP_REW and the episode statistics keep the raw reward.  A flag on a row with done[n] == 0 is IGNORED -- the host calls
 * refuse it with PPO_ERR_INVALID, the device call cannot look without a host wait.  Rows of final_obs that are not flagged are never read.  The step's
 * common case, no flagged row, costs one pass over truncated and done.  The events go to a device list; ppo_host_truncations after a device-fed rollout
 * waits for that rollout's last fold only (not for the update), copies the list and returns it with indices ascending, as after a host-fed rollout.
 * The fused families (PPO_KERNEL_GAUSS_FUSED and PPO_KERNEL_CAT_FUSED contexts: 2 x 64 f32, obs_size 1 .. 64) take the flags like the reference's own
 * shapes: their critic is ONE kernel whatever the row count (gauss_values_kernel, the kernel behind ppo_get_value and ppo_bootstrap_rewards on such a
 * context), and the fold launch (gauss_dev_fold_kernel: ceil(N / 256) workgroups, the critic's weights staged only by a workgroup that found a flagged
 * row) runs that kernel's forward on the flagged rows, so V is ppo_get_value's bit for bit and a device-fed rollout equals the host-fed one bit for bit
 * (tests/test_gpu_fused_dev_truncation.py).  An observe is one launch there too, two with `truncated`, three with observation normalisation on top (the
 * flagged rows of final_obs are normalised in front of the commit); each fold launch counts in ppo_gauss_fused_launches' `value`.
 * The plain generic engine (any other network: another width or depth, bf16, or a 2 x 64 f32 network without either flag) takes the ppo_dev_* calls fully
 * EXCEPT a non-NULL `truncated`, which returns PPO_ERR_UNSUPPORTED and changes nothing: that engine chooses its critic kernel by the row count, that
 * choice changes bits, and the host does not have the count here.  Device callers of such networks can still fold with ppo_bootstrap_rewards where they
 * know K. */
/* ppo_host_env_reset from a device array: obs f32 [N,O] = every env's reset observation.  Enqueued. */
PPO_API ppo_status ppo_dev_env_reset(ppo_ctx* ctx, const float* obs /* [N,O] */, void* caller_stream);
/* ppo_host_act with the actions left on the device: mask u8 [N,A] or NULL (masked policies; NULL = all valid), action i64 [N,H]. */
PPO_API ppo_status ppo_dev_act(ppo_ctx* ctx, const uint8_t* mask /* [N,A] or NULL */, int64_t* action /* [N,H] */, void* caller_stream);
/* ppo_dev_act for a PPO_DIST_GAUSSIAN context: action f32 [N,D], the raw samples; equals ppo_host_act_f32 on the same data bit for bit. */
PPO_API ppo_status ppo_dev_act_f32(ppo_ctx* ctx, float* action /* device [N,D] */, void* caller_stream);
/* ppo_host_observe_truncated from device arrays, committed at once (see above). */
PPO_API ppo_status ppo_dev_observe(ppo_ctx* ctx, const float* next_obs /* [N,O] */, const float* reward /* [N] */, const int32_t* done /* [N] */,
                                   const int32_t* fin_len /* [N] or NULL */, const float* fin_rew /* [N] or NULL */,
                                   const int32_t* truncated /* [N] or NULL */, const float* final_obs /* [N,O] or NULL */, void* caller_stream);

/* Observation normalisation of caller-stepped environments (new): running mean / variance statistics, the first thing a PPO user adds to a custom env
 * (gym's NormalizeObservation, SB3's VecNormalize).  The reference has none and never needed one: its envs (CartPole, MountainCar) are of unit scale.
 * A caller's env is not: positions in metres, velocities in hundreds, counters in thousands -- a poor diet for orthogonal weights and tanh layers, and in
 * this build an observation beyond 65 504 in PPO_BUF_OBS raises the sticky error word (kernel_flags, "fp16 ranges").  A normalised observation, clipped
 * to +-clip, can never do that.
 *
 * Off unless ppo_obs_norm_enable turns it on: a context that never makes that call runs, launch for launch and bit for bit, what it ran before.
 * Per context, in f64 on the device: mean[O], var[O] (population variance) and a row count; initially mean = 0, var = 1, count = 0.  Every batch of N
 * new observations -- the reset observations (ppo_host_env_reset / ppo_dev_env_reset), then each step's next_obs -- is handled the same way:
 *   update (mode 1 only): batch mean bm[o] and batch M2 = sum (x - bm)^2 over the N rows, in f64; then Chan's merge
 *       tot = count + N;  delta = bm - mean;  mean += delta * N / tot;  M2 = var * count + bM2 + delta^2 * count * N / tot;  var = M2 / tot;  count = tot
 *   apply: y = f32(clamp((f64(x) - mean) / sqrt(var + eps), -clip, +clip)) with the statistics as just updated.
 * Everything downstream sees y only: PPO_BUF_NEXT_OBS, PPO_BUF_OBS[t], the actor, the value launch of ppo_host_rollout_end, the update; none of those
 * kernels changes.  The raw observation is not kept.  Sums are formed in a fixed order without atomics: the same feed gives the same bits.
 * Launches: ONE more per env step (update and apply are one kernel, obsnorm_update_apply_kernel), two with truncation flags.  ppo_dev_observe runs it in
 * front of its commit, on the caller's next_obs into a scratch of the context's (it still only enqueues); a host-fed rollout runs it in ppo_host_act in
 * front of the commit of the staged step (reading the pinned staging), and in ppo_host_rollout_end for the last step.  A host-fed and a device-fed
 * rollout of the same data therefore merge the same batches in the same order and agree bit for bit, statistics included.
 * Truncation bootstrap: a final observation is normalised WITHOUT updating the statistics, by the statistics as they stand when its fold runs.  The two
 * feeds differ here: ppo_dev_observe folds per step, so a device-fed rollout uses the statistics right behind the same step's update; the host path folds
 * once per rollout, so a host-fed rollout uses the statistics at ppo_host_rollout_end (all T steps merged).  This holds for every context whose
 * ppo_dev_observe takes the flags: the reference's shapes and the PPO_KERNEL_GAUSS_FUSED / PPO_KERNEL_CAT_FUSED families (with frozen statistics, mode 2,
 * the two feeds agree bit for bit there as well).  ppo_bootstrap_rewards on caller buffers
 * stays raw: the caller normalises with ppo_obs_norm_apply first.
 * Errors (a failing call changes nothing): PPO_ERR_UNSUPPORTED for any of the four calls on a context that is not PPO_ENV_HOST (device envs are of unit
 * scale and their fused rollout never leaves the chip), for ppo_obs_norm_enable(mode != 0) on a sharded context (global_num_envs > num_envs or a
 * communicator initialised: per-rank statistics would make the replicas disagree; reducing them across ranks is later work), for ppo_comm_init /
 * ppo_comm_init_local / ppo_comm_init_exchange on a context with normalisation on, and for ppo_host_rollout_begin_groups with normalisation on (groups
 * commit in an order the caller chooses, the statistics would depend on it, and that breaks the groups' promise of interleaving-independent bits).
 * PPO_ERR_STATE for enable / get / set while a rollout is open.  PPO_ERR_INVALID for a mode outside 0 .. 2, clip <= 0, eps <= 0, O != obs_size, a
 * negative count or variance, null pointers. */
/* mode 0 off, 1 update + apply, 2 apply only (frozen statistics: evaluation, fine-tuning).  Defaults of the bindings: clip = 10, eps = 1e-8.  The
 * statistics are kept across mode changes. */
PPO_API ppo_status ppo_obs_norm_enable(ppo_ctx* ctx, int32_t mode, float clip, float eps);
/* The statistics, host arrays f64 [O] (O = obs_size) and the row count.  Synchronous.  Before anything was enabled or set: mean 0, var 1, count 0. */
PPO_API ppo_status ppo_obs_norm_get_h(ppo_ctx* ctx, double* mean_h, double* var_h, int64_t O, double* count);
/* Replaces the statistics (a checkpoint's, another context's).  Synchronous.  get then set on a second context, then the same feed: the same bits. */
PPO_API ppo_status ppo_obs_norm_set_h(ppo_ctx* ctx, const double* mean_h, const double* var_h, int64_t O, double count);
/* out[n,O] = the apply step on obs[n,O] with the current statistics, clip and eps; no update, whatever the mode.  DEVICE pointers; out may alias obs.
 * Valid inside an open rollout too.  stream: as caller_stream of the ppo_dev_* calls (hand-over by events unless it is ppo_stream(ctx)). */
PPO_API ppo_status ppo_obs_norm_apply(ppo_ctx* ctx, const float* obs, int64_t n, float* out, void* stream);

/* Reward normalisation of caller-stepped environments (new): the other half of gym's NormalizeReward / SB3's VecNormalize -- every reward is divided by
 * the running standard deviation of the discounted return and clipped.  The reference has none: CartPole and MountainCar pay +-1 per step, and vf_coef,
 * clip_vloss, max_grad_norm and the learning rate of its TOML are tuned for returns of that scale.  A caller's env pays in its own units (a score in
 * thousands, a cost in millionths).
 *
 * Off unless ppo_reward_norm_enable turns it on: a context that never makes that call runs, launch for launch and bit for bit, what it ran before.
 * Per context, in f64: a discounted-return accumulator ret[N] and the scalars mean, var (population variance) of the returns seen so far, on the device,
 * and a row count on the host; initially ret = 0, mean = 0, var = 1, count = 0.  ppo_host_env_reset and ppo_dev_env_reset zero ret and keep the statistics.
 * Every committed step, with rewards r[N] (f32), this step's done[N] and g = (double)cfg.gamma:
 *   update (mode 1 only): R[n] = ret[n] * g + (double)r[n];  batch mean bm = (sum R) / N and batch M2 = sum (R - bm)^2, in f64;  then Chan's merge as above
 *       tot = count + N;  delta = bm - mean;  mean += delta * N / tot;  M2 = var * count + bM2 + delta^2 * count * N / tot;  var = M2 / tot;  count = tot
 *     and then ret[n] = done[n] ? 0 : R[n].
 *   apply: y[n] = f32(clamp((double)r[n] / sqrt(var + eps), -clip, +clip)) with var as just updated.  No mean is subtracted, as in gym and SB3.
 *   mode 2: apply only; ret and the statistics are untouched (SB3's training = False).  mode 0: off; the statistics are kept.
 * Known consequence: a first batch of identical rewards gives var = 0, so y = r / sqrt(eps) and the clip acts (gym behaves the same way).
 * Who sees which reward: PPO_BUF_REWARDS[t] holds y, and so do the scan and the update.  PPO_BUF_EP_REW, PPO_BUF_FIN_REW, ep_rew_mean and everything in
 * ppo_stats about episodes keep the RAW reward.  The truncation fold adds gamma * V(final obs) to the NORMALISED reward (V is in normalised units), in
 * both feeds: the normalisation of step t precedes the fold of step t.  With reward normalisation alone a host-fed and a device-fed rollout of the same
 * data agree bit for bit, folded rewards and the values of ppo_host_truncations included; with observation normalisation also on, the difference between
 * the feeds that its block documents remains, and only that one.  ppo_bootstrap_rewards on caller buffers stays as it is.
 * Launches: ONE more per env step (rewnorm_update_apply_kernel: one workgroup, sums in a fixed order without atomics, so the same feed gives the same
 * bits), in front of the commit of the step: in ppo_dev_observe (which still only enqueues), in ppo_host_act for the staged step and in
 * ppo_host_rollout_end for the last one.
 * The fused device envs (PPO_KERNEL_ENV_REWARD_NORM in kernel_flags, above; the library's own Pendulum pays down to -16 a step, MountainCarContinuous +100
 * at the goal, Taxi -10 to +20): the three calls are served on a flagged context with the same argument checks, modes, defaults and initial state, the same
 * refusal on a sharded context and of ppo_comm_init* while the normaliser is on.  ppo_env_reset zeroes ret and keeps the statistics; ppo_env_set_state_h
 * touches neither.  A device-env rollout is ONE launch for all T steps and its rewards never feed back into it (actions, states and stored observations do
 * not depend on how rewards are scaled), so the normalisation is a post-process of PPO_BUF_REWARDS and PPO_BUF_FIN_LEN: with mode 1, ppo_rollout /
 * ppo_rollout_f32 / ppo_train_iteration leave in PPO_BUF_REWARDS, ret, mean, var and the count EXACTLY -- the same bits -- what T successive updates as
 * above would leave, applied to rows t = 0 .. T - 1 of the raw rewards in order with done[t][n] = (PPO_BUF_FIN_LEN[t][n] != 0) and g = (double)cfg.gamma.
 * The summation order is rewnorm_update_apply_kernel's: slot w of 256 takes envs w, w + 256, ... ascending, the 256 slots are then added in slot order, all
 * in f64.  Mode 2 applies the frozen variance to all T N rewards and changes nothing else.  The raw reward stays in PPO_BUF_EP_REW, PPO_BUF_FIN_REW,
 * ep_rew_mean and ppo_evaluate.  The normalisation precedes the time-limit fold (ppo_env_truncation_bootstrap): the events and V of ppo_env_truncations are
 * what they are without it, and f32(gamma * V) is added to the NORMALISED reward -- by the fold from PPO_BUF_OBS and by the fold from the cut-state record
 * alike.  Launches: THREE per rollout whatever T is (rewnorm_scan_kernel: one thread per env walks the T steps; rewnorm_moments_kernel: one workgroup per
 * step; rewnorm_merge_apply_kernel: Chan's chain of T scalar merges, then the apply), one with mode 2, none with mode 0; enqueued behind the two critic
 * launches and in front of the fold, with no host wait, no floating-point atomics and no hand-over inside a launch.  The rollout kernels are untouched.
 * The first-batch consequence above is the rule on envs whose first rewards are all equal (Acrobot's -1, FrozenLake's 0): var = 0 there and the clip acts.
 * Errors (a failing call changes nothing): PPO_ERR_UNSUPPORTED for any of the three calls on a context that is not PPO_ENV_HOST (nor a flagged fused device env), for
 * ppo_reward_norm_enable(mode != 0) on a sharded context (global_num_envs > num_envs or a communicator initialised), for ppo_comm_init /
 * ppo_comm_init_local / ppo_comm_init_exchange on a context with it on, and for ppo_host_rollout_begin_groups with it on (the statistics would depend on
 * the order in which groups commit).  PPO_ERR_STATE for enable / get / set while a rollout is open.  PPO_ERR_INVALID for a mode outside 0 .. 2,
 * clip <= 0, eps <= 0, non-finite arguments, a negative var or count, ret_h != NULL with N != num_envs, null mean / var / count. */
/* mode 0 off, 1 update + apply, 2 apply only.  Defaults of the bindings: clip = 10, eps = 1e-8.  The statistics are kept across mode changes. */
PPO_API ppo_status ppo_reward_norm_enable(ppo_ctx* ctx, int32_t mode, float clip, float eps);
/* The statistics, the row count and (ret_h != NULL) the accumulators, f64 [N], N = num_envs.  Synchronous.  Before anything was enabled or set: 0, 1, 0, zeros. */
PPO_API ppo_status ppo_reward_norm_get_h(ppo_ctx* ctx, double* mean, double* var, double* count, double* ret_h /* f64 [N] or NULL */, int64_t N);
/* Replaces the statistics (a checkpoint's, another context's); ret is not touched (the resets zero it).  Synchronous. */
PPO_API ppo_status ppo_reward_norm_set_h(ppo_ctx* ctx, double mean, double var, double count);

/* ---------------------------------------------------------------------------------------------------------
 * Evaluation (new; the reference reports only the mean over the last 100 exploration episodes of its training envs, PPO_Discrete.cpp:474-480, Utils.h:72-78)
 * ------------------------------------------------------------------------------------------------------- */
typedef struct ppo_eval_stats {
    int64_t episodes, env_steps;                 /* env_steps = sum of lengths */
    double return_mean, return_std, return_min, return_max;   /* std: population (ddof 0) */
    double length_mean; int64_t length_min, length_max;
    int64_t truncated;                           /* episodes that reached max_episode_steps (PPO_Discrete.cpp:449-452) */
} ppo_eval_stats;
/* n_episodes whole episodes of the context's device env (PPO_ENV_CARTPOLE, PPO_ENV_MOUNTAINCAR) under the current policy, as ONE launch: no host round
 * trip per step and no [T,N,*] stores, only an episode's return, length and truncated flag leave the chip.
 *   Episode e (0 <= e < n_episodes) is a pure function of (parameters, seed, e, greedy, max_episode_steps).  Start state: CartPole = row e of
 *   ppo_cartpole_reset_stream_h(seed, n_episodes) (CartPole.cpp:34-45); MountainCar = MountainCar::reset (MountainCar.cpp:59-66) with the build's key
 *   (seed, env e, reset 0).  Steps as stepEnvs (PPO_Discrete.cpp:440-458): CartPole::step / MountainCar::step (CartPole.cpp:47-94, MountainCar.cpp:29-57),
 *   reward summed in f32 in step order, the episode ends where the env terminates or its length reaches the context's max_episode_steps (:449-452).
 *   greedy != 0: actions as ppo_policy_act_greedy.  greedy == 0: the sampler of ppo_policy_act (Categorical.cpp:73-79) keyed (seed, row e, step t within
 *   the episode, head).  Logits: those of ppo_policy_act_greedy / ppo_policy_act on the same context (the kernel is chosen once per call from the same
 *   weight-range snapshot as ppo_rollout's) -- stepping the same start states through those calls and ppo_env_transition gives the same bits.
 *   Hence: results do not depend on how episodes are spread over workgroups, and ppo_evaluate(n = 16) equals the first 16 entries of ppo_evaluate(n = 64)
 *   with the same seed.
 *   ep_return f32 [n_episodes] / ep_length i32 [n_episodes]: device arrays or NULL.  out_h (host, required): the summary, formed on the host in f64 from the
 *   per-episode arrays in index order.  Evaluates the parameters as they are behind everything already enqueued on the context's stream; SYNCHRONOUS (returns
 *   when out_h is filled).
 *   Leaves the training state exactly as it was: every PPO_BUF_*, reset counters, sampler position, episode ring, statistics, error word and ppo_profile
 *   (a vector-kernel fallback of this launch is not counted).  Purely local: no collective on a sharded context (every rank that asks the same question
 *   gets the same answer).
 *   Errors: PPO_ENV_SYNTHETIC and PPO_ENV_HOST contexts -> PPO_ERR_UNSUPPORTED (step the episodes yourself around ppo_policy_act_greedy);
 *   PPO_ENV_PENDULUM contexts -> PPO_ERR_UNSUPPORTED (step the episodes through ppo_policy_act_f32 with greedy = 1 and ppo_env_transition_f32);
 *   n_episodes <= 0, out_h == NULL, max_episode_steps <= 0 -> PPO_ERR_INVALID.  A failing call changes nothing.
 *   PPO_ENV_MOUNTAINCAR_CONTINUOUS: served, also as ONE launch (gauss_eval_kernel: a workgroup owns 64 episodes for their whole length, the actor's weights
 *   resident in LDS, as in the rollout kernel).  Episode e starts at reset 0 of env e under `seed` (p = uniform(philox4x32_10(seed; e, 0, 0, 1).x, -0.6, -0.4),
 *   v = 0).  greedy != 0: the action is the mean, bit for bit ppo_policy_act_f32 with greedy = 1; greedy == 0: mu + sigma * eps with eps keyed (seed, e, step t
 *   within the episode, d = 0), bit for bit ppo_policy_act_f32(step_index = t) on row e of a context whose seed is `seed` and whose env_offset is 0.  The env
 *   step, the f32 reward sum in step order, the end at termination or at max_episode_steps, the independence of how episodes are spread over workgroups and
 *   everything about the outputs and the untouched training state (ppo_gauss_fused_launches included) are as above.  No reset table is needed.
 *   PPO_ENV_ACROBOT: served likewise as ONE launch (cat_eval_kernel; the lane keeps the state, the observation goes through the forward).  Episode e starts
 *   at reset 0 of env e under `seed` (the four words of philox4x32_10(seed; e, 0, 0, 1) mapped to [-0.1, 0.1)).  greedy != 0: the first-index argmax of
 *   ppo_policy_act_greedy; greedy == 0: the draw keyed (seed, e, step t within the episode, head 0), bit for bit ppo_policy_act(step_index = t) on row e of
 *   a context whose seed is `seed` and whose env_offset is 0.
 *   PPO_ENV_TAXI: the same launch; episode e starts at reset 0 of env e under `seed` (the reset map above).  Under PPO_DIST_MASKED the lane forms the mask of
 *   its state and both the argmax and the draw run on the masked probabilities: a masked-out action has probability 0 and is never chosen. */
PPO_API ppo_status ppo_evaluate(ppo_ctx* ctx, int64_t n_episodes, int64_t seed, int32_t greedy,
                                float* ep_return /* dev f32[n] or NULL */, int32_t* ep_length /* dev i32[n] or NULL */,
                                ppo_eval_stats* out_h);

/* ---------------------------------------------------------------------------------------------------------
 * Measurement (new; the reference only has a wall clock around each update, PPO_Discrete.cpp:650-652)
 * ------------------------------------------------------------------------------------------------------- */
/* Per-kernel device time from HIP events recorded on the context's stream around the instrumented launches. */
typedef struct ppo_profile {
    int64_t fwd_bwd_launches, gae_launches, rollout_launches, optimizer_launches, reduce_launches;
    double fwd_bwd_ms, gae_ms, rollout_ms, optimizer_ms, reduce_ms;   /* summed over the launches since enable/read */
    double phase_cycles[24];  /* mode 3: [critic, actor][12 phases] shader cycles of one wave of the dominant kernel */
    int64_t allreduce_launches;   /* N > 1: gradient / statistics all-reduces bracketed (every one in mode 1; in modes 2 and 4 the one behind a bracketed */
    double allreduce_ms;          /* dominant-kernel launch): the collective's device time on THIS rank, waiting for the slowest peer included */
    int64_t vector_fallback_launches;   /* ABI 5: launches since ppo_ctx_create (NOT reset by a read) that took a vector kernel because a weight did not fit the fp16
                                         * operands of the matrix-core kernel of the same function (kernel_flags, "fp16 ranges") */
} ppo_profile;
/* on: 0 = off, 1 = every instrumented launch, 2 = only the dominant kernel (fused forward/backward; ONE launch in 8 is bracketed: an
 * event pair costs the stream ~3 us, 40 pairs per update were 8 % of the run) and the GAE scan,
 * 3 = in-kernel phase stamps of the dominant kernel (diagnostic kernel variant; read shares, not run time),
 * 4 = as 2 with ONE launch in 41 (about one per update, a different step each time): five pairs per 2.4 ms iteration still cost 1.7 % of it
 *     (219.4 against 215.5 M env-steps/s), one costs 0.3 % */
PPO_API ppo_status ppo_profile_enable(ppo_ctx* ctx, int32_t on);
PPO_API ppo_status ppo_profile_read(ppo_ctx* ctx, ppo_profile* out);  /* synchronises; resets the accumulators */

/* ---------------------------------------------------------------------------------------------------------
 * Multi-GPU (new): one context per GPU/process, envs sharded, one gradient all-reduce per optimizer step
 * ------------------------------------------------------------------------------------------------------- */
#define PPO_COMM_ID_BYTES 128
PPO_API ppo_status ppo_comm_unique_id(void* id_out_h /* PPO_COMM_ID_BYTES */);
PPO_API ppo_status ppo_comm_init(ppo_ctx* ctx, const void* id_h, int32_t rank, int32_t nranks);
/* Same contract without RCCL for contexts that live in ONE process (one host thread per context; up to 8): the ranks of
 * `group_id` rendezvous inside each all-reduce and the last to arrive sums every rank's buffer in rank order on its stream. */
PPO_API ppo_status ppo_comm_init_local(ppo_ctx* ctx, int64_t group_id, int32_t rank, int32_t nranks);
/* One-shot direct exchange (no reference counterpart): the latency-bound all-reduce (36.6 KB of gradient per optimizer step) without a
 * ring.  One process per GPU, up to the 8 GPUs of a node.  Every rank exports a small exchange buffer (fine-grained device memory, HIP IPC),
 * the handles are gathered by the host (e.g. torch.distributed), every rank maps its peers'; an all-reduce is then ONE kernel per rank that
 * pushes its payload into its slot of every peer's buffer over xGMI and adds every rank's, in rank order (bit-identical sums everywhere), out
 * of its own buffer.  Inside ppo_update the exchange rides in the gradient reduction: a sharded optimizer step is two launches, as on one GPU.
 *   1. ppo_comm_exchange_handle(ctx, handle)          on every rank
 *   2. gather the nranks handles in rank order
 *   3. ppo_comm_init_exchange(ctx, handles, rank, n)  on every rank
 * A kernel never spins forever: it waits for a peer's share at most the wait limit (default 30 s, ppo_comm_set_wait_limit -- keep it above any
 * host-side skew between ranks: a checkpoint write, a statistics read-back), then gives up with an incomplete sum, sets the timeout flag
 * (ppo_comm_exchange_timeouts: zero / non-zero) and marks the communicator dead (no later call waits again).  The failure is REPORTED: the next
 * ppo_sync, ppo_read_stats or ppo_profile_read of the context returns PPO_ERR_COMM (the replicas have diverged; the job must stop).
 * HIP IPC between processes needs HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment of every rank on hosts whose driver only supports dmabuf IPC
 * (set before the process's first HIP call; ppo-libtorch_amd/dist.py does it at import). */
#define PPO_COMM_HANDLE_BYTES 64
PPO_API ppo_status ppo_comm_exchange_handle(ppo_ctx* ctx, void* handle_out_h /* PPO_COMM_HANDLE_BYTES */);
PPO_API ppo_status ppo_comm_init_exchange(ppo_ctx* ctx, const void* handles_h /* nranks x PPO_COMM_HANDLE_BYTES */, int32_t rank, int32_t nranks);
PPO_API ppo_status ppo_comm_set_wait_limit(ppo_ctx* ctx, double seconds);
PPO_API ppo_status ppo_comm_exchange_timeouts(ppo_ctx* ctx, int32_t* nonzero_out);

#ifdef __cplusplus
}
#endif
#endif /* PPO_HIP_H */
