"""PPO_KERNEL_ENV_GENERIC: CartPole / MountainCar under networks of any width and depth (include/ppo_hip.h).  The env is the unflagged context's, the network
the generic engine's, so the yardsticks are the two the project already has: the unflagged 2 x 64 context for everything about the env (bit for bit, under
the same forced actions) and the oracle -- generic in width and depth, with both envs restated (oracle.VecEnv) -- for everything about the network, within
tests/test_gpu_generic.py's own bars for that engine (TOL).

Shapes: T = 16 steps, N in {1, 33, 70} (a lone env, a tile of 32 plus one, two tiles and a short one), max_episode_steps = 9 so that time-limit ends fall
inside a rollout, and injected states from which every fifth env ends by itself at the first step (CartPole: the pole beyond 12 degrees; MountainCar: the
car over the goal line).  CartPole runs with PPO_DIST_CATEGORICAL and MountainCar with PPO_DIST_MASKED, as the reference's two trainers do: MASKS is left
alone by the first and filled with ones by the second.
"""
import numpy as np
import pytest

import oracle as O
from __graft_entry__ import load_package
from test_gpu_generic import TOL

pytestmark = pytest.mark.gpu

T, MAXS, SEED = 16, 9, 7
NS = [1, 33, 70]
ENV_BUFS = ("OBS", "REWARDS", "DONES", "FIN_LEN", "FIN_REW", "NEXT_OBS", "NEXT_DONE", "MASKS")
ALL_BUFS = ENV_BUFS + ("ACTIONS", "LOGPROBS", "VALUES", "ADVANTAGES", "RETURNS", "NEXT_VALUE", "PARAMS", "GRADS", "EXP_AVG", "EXP_AVG_SQ", "ENV_STATE", "EP_LEN",
                       "EP_REW", "RESET_COUNT")
# f32 1 x 48 and 3 x 160 (one n tile with a ragged edge; two, the second ragged), bf16 2 x 128 and 4 x 256 (the one-launch rollout; 256: a whole pass of k steps)
SHAPES = [(0, 48, 1), (0, 160, 3), (1, 128, 2), (1, 256, 4)]
HP = dict(gamma=0.99, gae_lambda=0.95, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5)


@pytest.fixture(scope="module")
def P():
    return load_package()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def env_of(P, name):
    """(env_kind, oracle kind, obs, heads, masked)"""
    return (P.ENV_CARTPOLE, O.ENV_CARTPOLE, 4, (2,), False) if name == "cartpole" else (P.ENV_MOUNTAINCAR, O.ENV_MOUNTAINCAR, 2, (3,), True)


def make_ctx(P, name, N, flagged, hidden=64, n_hidden=2, dtype=0, **kw):
    kind, _, obs, heads, masked = env_of(P, name)
    args = dict(env_kind=kind, dist_kind=P.DIST_MASKED if masked else P.DIST_CATEGORICAL, obs_size=obs, head_dims=heads, hidden=hidden, n_hidden=n_hidden, num_envs=N,
                num_steps=T, num_minibatches=2, update_epochs=2, max_episode_steps=MAXS, seed=SEED, total_timesteps=64 * N * T, learning_rate=1e-3, anneal_lr=False,
                compute_dtype=dtype, kernel_flags=P.KERNEL_ENV_GENERIC if flagged else 0, **HP)
    args.update(kw)
    ctx = P.Context(P.make_config(**args))
    ctx.init_orthogonal(SEED)
    if flagged:   # a policy that is not uniform: the policy head (the last actor tensors) x 30, as tests/test_gpu_generic.py does
        p, A = ctx.get_params(), sum(heads)
        p[-(A * hidden + A):] *= 30.0
        ctx.set_params(p)
    return ctx


def inject(ctx, name):
    """ppo_env_reset, then states, episode lengths and returns of the test's own: every fifth env one step from its own end, lengths 0, 1, 2 so that the
    time limit (9) falls on steps 9, 8 and 7 of the first rollout and again in the second.  Returns NEXT_OBS, which ppo_env_set_state_h refilled."""
    N = ctx.N
    ctx.env_reset()
    rng = np.random.default_rng(11)
    n = np.arange(N)
    if name == "cartpole":
        st = rng.uniform(-0.05, 0.05, (N, 4)).astype(np.float32)
        st[n % 5 == 0, 2], st[n % 5 == 0, 3] = 0.205, 1.5
    else:
        st = np.stack([rng.uniform(-0.6, -0.4, N), np.zeros(N)], 1).astype(np.float32)
        st[n % 5 == 0] = (0.495, 0.06)
    ep_len = (n % 3).astype(np.int32)
    ep_rew = (ep_len if name == "cartpole" else -ep_len).astype(np.float32)
    ctx.env_set_state(state=st, ep_len=ep_len, ep_rew=ep_rew)
    obs = ctx.read("NEXT_OBS", (N, ctx.O))
    assert same(obs, st)
    return obs


def forced_actions(name, N, k):
    return np.random.default_rng(100 + k).integers(0, 2 if name == "cartpole" else 3, (T, N, 1)).astype(np.int64)


def env_state(ctx):
    return dict(zip(("ENV_STATE", "EP_LEN", "EP_REW", "RESET_COUNT"), ctx.env_get_state()))


# ---------------------------------------------------------------------------------------------------------
# 1. the env is the shipped engine's, bit for bit
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("name", ["cartpole", "mountaincar"])
@pytest.mark.parametrize("shape", [(0, 64, 2), (1, 128, 2)], ids=["f32 2x64", "bf16 2x128 one launch"])
def test_env_identical_to_the_unflagged_context(P, name, N, shape):
    dtype, hidden, n_hidden = shape
    a, b = make_ctx(P, name, N, False), make_ctx(P, name, N, True, hidden, n_hidden, dtype)
    assert same(inject(a, name), inject(b, name))
    for k in range(2):   # the second rollout carries the first one's done flags, episode sums and reset counts
        f = forced_actions(name, N, k)
        a.rollout(f)
        b.rollout(f)
        for buf in ENV_BUFS:
            assert same(a.read(buf), b.read(buf)), (k, buf)
        sa, sb = env_state(a), env_state(b)
        for key in sa:
            assert same(sa[key], sb[key]), (k, key)
        assert np.array_equal(b.read("ACTIONS", (T, N, 1)), f.astype(np.int32))
        fin = b.read("FIN_LEN", (T, N))
        if k == 0:
            assert (fin[0, np.arange(N) % 5 == 0] > 0).all()                      # the env's own end, at the first step
            assert (fin[1:] == MAXS).any()                                        # the time limit, inside the rollout
        masks = b.read("MASKS")
        assert (masks == (1 if name == "mountaincar" else 0)).all()
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------
# 2. other shapes against the oracle
# ---------------------------------------------------------------------------------------------------------
def replay(okind, N, state0, actions):
    """The stored actions through oracle.VecEnv from the injected state: the env buffers a rollout must hold."""
    env = O.VecEnv(okind, N, SEED, MAXS)
    env.init()
    s, l, r, k = state0
    env.set_state(state=s, ep_len=l, ep_rew=r, reset_count=k)
    out = {key: [] for key in ("OBS", "REWARDS", "DONES", "FIN_LEN", "FIN_REW")}
    x, done = s.copy(), np.zeros(N, np.int32)
    for t in range(actions.shape[0]):
        _, l0, r0, _ = env.get_state()
        out["OBS"].append(x)
        out["DONES"].append(done.astype(np.float32))
        x, r, done = env.step(actions[t, :, 0])
        out["REWARDS"].append(r)
        out["FIN_LEN"].append(np.where(done != 0, l0 + 1, 0).astype(np.int32))
        out["FIN_REW"].append(np.where(done != 0, r0 + r, np.float32(0)).astype(np.float32))
    res = {key: np.stack(v) for key, v in out.items()}
    res["NEXT_OBS"], res["NEXT_DONE"] = x, done
    return res, env


@pytest.mark.parametrize("name", ["cartpole", "mountaincar"])
@pytest.mark.parametrize("shape", SHAPES, ids=["f32 1x48", "f32 3x160", "bf16 2x128", "bf16 4x256"])
def test_shapes_against_the_oracle(P, name, shape):
    dtype, hidden, n_hidden = shape
    N, tol = 70, TOL[dtype]
    _, okind, obs_dim, heads, masked = env_of(P, name)
    A = sum(heads)
    ctx = make_ctx(P, name, N, True, hidden, n_hidden, dtype)
    net = O.Net.make(obs_dim, list(heads), hidden=hidden, n_hidden=n_hidden, dist_kind=O.DIST_MASKED if masked else O.DIST_CATEGORICAL, dtype=dtype)
    assert ctx.P == O.param_count(net) and np.array_equal(ctx.param_shapes(), O.param_shapes(net))
    params = ctx.get_params()
    inject(ctx, name)
    state0 = ctx.env_get_state()
    ctx.rollout()
    actions = ctx.read("ACTIONS", (T, N, 1)).astype(np.int64)
    want, env = replay(okind, N, state0, actions)
    for buf, w in want.items():
        assert same(ctx.read(buf).reshape(w.shape), w), buf
    for got, w in zip(ctx.env_get_state(), env.get_state()):
        assert np.array_equal(bits(got), bits(w.astype(got.dtype)))
    assert len(np.unique(actions)) > 1
    # ---- policy and critic against the oracle's forward, the sampler on every step's rows ----
    obs, logp, values = want["OBS"], ctx.read("LOGPROBS", (T, N)), ctx.read("VALUES", (T, N))
    mask = np.ones((T * N, A), np.uint8) if masked else None
    lp_o, _, v_o = O.evaluate(net, params, obs.reshape(T * N, obs_dim), actions.reshape(T * N, 1), mask)
    print("log-prob %.2e (bar %.0e), value %.2e (bar %.0e)" % (np.abs(logp.reshape(-1) - lp_o).max(), tol["fwd"], np.abs(values.reshape(-1) - v_o).max(), tol["fwd_v"]))
    np.testing.assert_allclose(logp.reshape(-1), lp_o, rtol=0, atol=tol["fwd"])
    np.testing.assert_allclose(values.reshape(-1), v_o, rtol=0, atol=tol["fwd_v"])
    next_value = ctx.read("NEXT_VALUE", (N,))
    np.testing.assert_allclose(next_value, O.get_value(net, params, want["NEXT_OBS"]), rtol=0, atol=tol["fwd_v"])
    a_o = np.stack([O.act(net, params, obs[t], SEED, t, 0, mask[:N] if masked else None)[0] for t in range(T)])
    print("sampler agreement %.4f (bar %.3f)" % ((a_o == actions).mean(), tol["agree"]))
    assert (a_o == actions).mean() >= tol["agree"]
    # ---- advantages / returns, bit for bit ----
    adv, ret = ctx.calc_advantage()
    adv_o, ret_o = O.gae(want["REWARDS"], values, want["DONES"], next_value, want["NEXT_DONE"], HP["gamma"], HP["gae_lambda"])
    assert same(adv, adv_o) and same(ret, ret_o)
    # ---- one minibatch step ----
    B = T * N
    idx = np.random.default_rng(1).permutation(B)[:B // 2].astype(np.int32)
    grads = ctx.minibatch_forward_backward(idx)
    st = ctx.stats()
    g_o, s_o = O.minibatch_grads(net, O.HParams(norm_adv=1, clip_vloss=1, **HP), params, obs.reshape(B, obs_dim), actions.reshape(B, 1).astype(np.float32), logp.reshape(B),
                                 adv.reshape(B), ret.reshape(B), values.reshape(B), idx.astype(np.int64), mask)[:2]
    for key, okey in (("pg_loss", "pg_loss"), ("v_loss", "v_loss"), ("entropy_loss", "entropy_loss"), ("approx_kl", "approx_kl"), ("clipfrac_last", "clipfrac"),
                      ("loss", "loss")):
        assert abs(st[key] - s_o[okey]) <= tol["loss"] * max(1.0, abs(s_o[okey])), (key, st[key], s_o[okey])
    print("gradient %.2e of max (bar %.0e)" % (np.abs(grads - g_o).max() / np.abs(g_o).max(), tol["grad"]))
    assert np.abs(grads - g_o).max() <= 1e-6 + tol["grad"] * np.abs(g_o).max()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 3. the rollout equals the stepwise API
# ---------------------------------------------------------------------------------------------------------
def stepwise_rollout(b, name, obs, done, step0, forced=None):
    """T x { ppo_policy_act(obs, step_index), ppo_env_step } on context b: the buffers a rollout would fill.  FIN_LEN / FIN_REW from the episode sums the
    context held in front of the step (f32 sum, the kernels' own operation)."""
    N, masked = b.N, name == "mountaincar"
    out = {k: [] for k in ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW")}
    for t in range(T):
        act, lp, _, _ = b.policy_act(obs, mask=np.ones((N, b.A), np.uint8) if masked else None, action=None if forced is None else forced[t], step_index=step0 + t)
        len0, rew0 = b.read("EP_LEN"), b.read("EP_REW")
        out["OBS"].append(obs)
        out["DONES"].append(done.astype(np.float32))
        obs, r, done = b.env_step(act)
        out["ACTIONS"].append(act.astype(np.int32))
        out["LOGPROBS"].append(lp)
        out["REWARDS"].append(r)
        out["FIN_LEN"].append(np.where(done != 0, len0 + 1, 0).astype(np.int32))
        out["FIN_REW"].append(np.where(done != 0, rew0 + r, np.float32(0)).astype(np.float32))
    res = {k: np.stack(v).reshape(-1) for k, v in out.items()}
    res["NEXT_OBS"], res["NEXT_DONE"] = obs.reshape(-1), done
    res["MASKS"] = np.full(T * N * b.A, 1 if masked else 0, np.uint8)
    return res, obs, done


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("name", ["cartpole", "mountaincar"])
def test_f32_rollout_equals_the_stepwise_api(P, name, N):
    """Free-running, f32 2 x 96: the rollout is the stepwise loop's launches on the same rows, so every buffer agrees bit for bit -- actions and log-probs
    included -- over two consecutive rollouts (the second runs step indices 16 .. 31)."""
    a, b = make_ctx(P, name, N, True, 96, 2), make_ctx(P, name, N, True, 96, 2)
    obs = inject(b, name)
    assert same(inject(a, name), obs)
    done = np.zeros(N, np.int32)
    fins = []
    for k in range(2):
        a.rollout()
        want, obs, done = stepwise_rollout(b, name, obs, done, k * T)
        for buf, w in want.items():
            assert same(a.read(buf), w), (k, buf, int((bits(a.read(buf)) != bits(w)).sum()))
        sa, sb = env_state(a), env_state(b)
        for key in sa:
            assert same(sa[key], sb[key]), (k, key)
        Ob = a.read("OBS", (T * N, a.O))
        assert same(a.read("VALUES"), a.get_value(Ob)) and same(a.read("NEXT_VALUE"), a.get_value(a.read("NEXT_OBS", (N, a.O))))
        fins.append((a.read("FIN_LEN"), a.read("FIN_REW")))
        a.calc_advantage()
        a.update()
        b.set_params(a.get_params())
        st = a.stats()
        assert st["global_step"] == (k + 1) * T * N      # rollout_steps advanced by T
        fl, fr = np.concatenate([f[0] for f in fins]), np.concatenate([f[1] for f in fins])
        n_done = min(int((fl > 0).sum()), 100)
        assert st["ep_count"] == n_done > 0
        assert abs(st["ep_len_mean"] - fl[fl > 0][-n_done:].astype(np.float64).mean()) <= 1e-6 * MAXS
        assert abs(st["ep_rew_mean"] - fr[fl > 0][-n_done:].astype(np.float64).mean()) <= 1e-6 * MAXS
    a.close()
    b.close()


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("name", ["cartpole", "mountaincar"])
def test_bf16_one_launch_rollout_equals_the_stepwise_api(P, name, N):
    """bf16 2 x 128 under forced actions (a last-bit log-prob difference would otherwise flip an action and send the two trajectories apart): the env
    buffers bit for bit; the log-probs within TOL[1]["same"] -- the logits are the same fused layers' on either side, the heads are evaluated on the hardware
    exp2 / log2 units in the one-launch kernel and by the library functions in ppo_policy_act.  That difference is also what tells generic_env_rollout_kernel
    from the per-step loop, which would run ppo_policy_act's own launches and give its bits (the f32 test above): over the 2 x 16 x 70 rows of N = 70 some
    log-prob differs in its last bits (measured: 1.2e-7 .. 2.4e-7 at N = 33 and 70, both envs)."""
    a, b = make_ctx(P, name, N, True, 128, 2, 1), make_ctx(P, name, N, True, 128, 2, 1)
    obs = inject(b, name)
    assert same(inject(a, name), obs)
    done = np.zeros(N, np.int32)
    differ = 0
    for k in range(2):
        f = forced_actions(name, N, k)
        a.rollout(f)
        want, obs, done = stepwise_rollout(b, name, obs, done, k * T, forced=f)
        lp = want.pop("LOGPROBS")
        differ += int((bits(a.read("LOGPROBS")) != bits(lp)).sum())
        for buf, w in want.items():
            assert same(a.read(buf), w), (k, buf)
        sa, sb = env_state(a), env_state(b)
        for key in sa:
            assert same(sa[key], sb[key]), (k, key)
        print("log-prob, one launch against stepwise: %.2e (bar %.0e)" % (np.abs(a.read("LOGPROBS") - lp).max(), TOL[1]["same"]))
        np.testing.assert_allclose(a.read("LOGPROBS"), lp, rtol=0, atol=TOL[1]["same"])
        np.testing.assert_allclose(a.read("VALUES"), a.get_value(a.read("OBS", (T * N, a.O))), rtol=0, atol=TOL[1]["same"])
        assert a.stats()["global_step"] == (k + 1) * T * N
    print("rows whose log-prob differs from the stepwise loop's in some bit: %d of %d" % (differ, 2 * T * N))
    assert differ > 0 or N < 70, "the rollout gave ppo_policy_act's bits on every row: the per-step loop ran in the one-launch kernel's place"
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------
# 4. training
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole", "mountaincar"])
@pytest.mark.parametrize("shape", SHAPES, ids=["f32 1x48", "f32 3x160", "bf16 2x128", "bf16 4x256"])
def test_three_iterations_train(P, name, shape):
    dtype, hidden, n_hidden = shape
    ctx = make_ctx(P, name, 70, True, hidden, n_hidden, dtype)
    ctx.env_reset()
    for _ in range(3):
        ctx.train_iteration()
    st = ctx.stats()
    assert np.isfinite(st["loss"]) and np.isfinite(ctx.get_params()).all()
    assert st["optimizer_steps"] == 3 * 2 * 2 and st["ep_count"] > 0 and st["global_step"] == 3 * T * 70
    ctx.close()


LEARN_ITERS = 30


def learning_curve(P, flagged, hidden):
    """CartPole, 256 envs x 32 steps, the reference's recommended settings (make_config's defaults), seed 2: ep_len_mean after every iteration."""
    ctx = P.Context(P.make_config(num_envs=256, num_steps=32, seed=2, total_timesteps=LEARN_ITERS * 256 * 32, hidden=hidden,
                                  kernel_flags=P.KERNEL_ENV_GENERIC if flagged else 0))
    ctx.init_orthogonal(2)
    ctx.env_reset()
    curve = []
    for _ in range(LEARN_ITERS):
        ctx.train_iteration()
        curve.append(ctx.stats()["ep_len_mean"])
    ctx.close()
    return np.array(curve)


def test_cartpole_learns_at_2x128(P):
    """The yardstick is the unflagged 2 x 64 context's gain in ep_len_mean over its first iteration, same hyper-parameters, seed and iteration count; the flagged
    2 x 128 f32 context must reach at least half of it (half: the seed-to-seed spread of such short runs is wide and the networks differ).  The iteration count
    is chosen so that the unflagged run at least doubles its first-iteration mean.
    Measured on an MI355X, 30 iterations (ep_len_mean after iterations 1, 6, 11, 16, 21, 26 and 30):
      unflagged 2 x 64 : 20.1 67.4 161.3 231.0 295.7 316.4 346.9   (gain 326.8, 17 times the first mean)
      flagged  2 x 128 : 20.1 68.9 165.2 247.2 314.0 342.9 366.0   (gain 345.9; the bar is 163.4)"""
    ref, got = learning_curve(P, False, 64), learning_curve(P, True, 128)
    print("unflagged 2 x 64 :", " ".join("%.1f" % x for x in ref[::5]), "last %.1f" % ref[-1])
    print("flagged  2 x 128 :", " ".join("%.1f" % x for x in got[::5]), "last %.1f" % got[-1])
    assert ref[-1] >= 2.0 * ref[0], "the yardstick run did not double its first-iteration mean: pick a longer run"
    assert got[-1] - got[0] >= 0.5 * (ref[-1] - ref[0]), (got[0], got[-1], ref[0], ref[-1])


# ---------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------
def test_ctx_create_refusals(P):
    F = P.KERNEL_ENV_GENERIC

    def refused(words, status, **kw):
        with pytest.raises(P.binding.PPOError) as e:
            P.Context(P.make_config(**kw))
        assert "status %d:" % status in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    flag = "PPO_KERNEL_ENV_GENERIC"
    refused((flag, "PPO_ENV_CARTPOLE and PPO_ENV_MOUNTAINCAR only"), 5, env_kind=P.ENV_SYNTHETIC, obs_size=8, head_dims=(3,), kernel_flags=F)
    refused((flag, "PPO_ENV_CARTPOLE and PPO_ENV_MOUNTAINCAR only"), 5, env_kind=P.ENV_HOST, obs_size=4, head_dims=(2,), kernel_flags=F)
    refused((flag, "PPO_ENV_CARTPOLE and PPO_ENV_MOUNTAINCAR only"), 5, env_kind=P.ENV_PENDULUM, dist_kind=P.DIST_GAUSSIAN, obs_size=3, head_dims=(1,), kernel_flags=F | P.KERNEL_GAUSS_FUSED)
    refused((flag, "PPO_ENV_CARTPOLE and PPO_ENV_MOUNTAINCAR only"), 5, env_kind=P.ENV_ACROBOT, obs_size=6, head_dims=(3,), kernel_flags=F | P.KERNEL_CAT_FUSED)
    refused((flag, "PPO_KERNEL_GAUSS_FUSED", "PPO_KERNEL_CAT_FUSED"), 5, kernel_flags=F | P.KERNEL_CAT_FUSED)
    refused((flag, "PPO_KERNEL_GAUSS_FUSED", "PPO_KERNEL_CAT_FUSED"), 5, env_kind=P.ENV_MOUNTAINCAR, obs_size=2, head_dims=(3,), kernel_flags=F | P.KERNEL_GAUSS_FUSED)
    refused((flag, "PPO_DIST_GAUSSIAN"), 5, dist_kind=P.DIST_GAUSSIAN, head_dims=(1,), kernel_flags=F)
    # a config that is invalid by itself is answered as such, flag or no flag
    refused(("unknown env_kind 9",), 1, env_kind=9, kernel_flags=F)
    refused(("unknown bits in kernel_flags",), 1, kernel_flags=F | 4096)
    refused(("unknown bits in kernel_flags",), 1, env_kind=P.ENV_SYNTHETIC, obs_size=8, head_dims=(3,), kernel_flags=F | 4096)
    # what the env accepts without the flag, and its limits with it
    refused(("observation of size 4", "expected observation size to be 2"), 1, obs_size=2, kernel_flags=F)
    refused(("observation of size 2", "expected observation size to be 4"), 1, env_kind=P.ENV_MOUNTAINCAR, obs_size=4, head_dims=(3,), kernel_flags=F)
    refused(("hidden 4096 (1..2048)",), 5, hidden=4096, kernel_flags=F)
    refused(("n_hidden 8 (1..7)",), 5, n_hidden=8, kernel_flags=F)
    # today's refusal of another network without the flag, in today's words
    refused(("only the reference architecture (2 hidden layers of 64", "got 4 x 256"), 5, hidden=256, n_hidden=4)
    refused(("PPO_DTYPE_BF16 applies to networks whose layers are GEMMs",), 5, compute_dtype=1)


def test_refused_calls_change_nothing(P):
    N, name = 40, "cartpole"
    ctx = make_ctx(P, name, N, True, 128, 2, 1)
    ctx.env_reset()
    ctx.train_iteration()
    ctx.rollout()
    ctx.sync()
    snap = lambda: ({k: ctx.read(k) for k in ALL_BUFS}, ctx.get_optimizer(), ctx.stats()["global_step"])   # noqa: E731
    before = snap()
    o, r, d = np.zeros((N, 4), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int32)
    d_o, d_r, d_d, d_a64 = ctx.dev(o), ctx.dev(r), ctx.dev(d), ctx.dev(np.zeros((N, 1), np.int64))
    flag = "PPO_KERNEL_ENV_GENERIC"
    calls = [
        # the caller-stepped families: PPO_ERR_STATE, as on any device-env context
        (3, "device environment", lambda: ctx.host_env_reset(o)),
        (3, "device environment", lambda: ctx.host_rollout_begin()),
        (3, "device environment", lambda: ctx.host_rollout_begin(groups=2)),
        (3, "device environment", lambda: ctx.host_act()),
        (3, "device environment", lambda: ctx.host_observe(o, r, d)),
        (3, "device environment", lambda: ctx.host_rollout_end()),
        (3, "device environment", lambda: ctx.dev_env_reset(d_o)),
        (3, "device environment", lambda: ctx.dev_act(d_a64)),
        (3, "device environment", lambda: ctx.dev_observe(d_o, d_r, d_d)),
        # the normalisers serve caller-stepped envs
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_enable(1)),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_get()),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_set(np.zeros(4), np.ones(4), 1.0)),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_apply(o)),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_enable(1)),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_get()),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_set(0.0, 1.0, 1.0)),
        # evaluation and the time-limit fold are built on the reference-shape kernels
        (5, "ppo_policy_act_greedy + ppo_env_transition", lambda: ctx.evaluate(8, 1)),
        (5, "reference-shape critic", lambda: ctx.env_truncation_bootstrap(True)),
        (5, "reference-shape critic", lambda: ctx.env_truncations()),
    ]
    for status, word, call in calls:
        with pytest.raises(P.binding.PPOError) as e:
            call()
        assert "status %d:" % status in str(e.value) and word in str(e.value) and flag in str(e.value), str(e.value)
    ctx.sync()
    after = snap()
    assert before[2] == after[2] and before[1][2] == after[1][2]
    for x, y in zip(before[1][:2], after[1][:2]):
        assert same(x, y)
    for k in ALL_BUFS:
        assert same(before[0][k], after[0][k]), k
    # and the context still trains
    ctx.train_iteration()
    assert np.isfinite(ctx.stats()["loss"])
    ctx.close()
