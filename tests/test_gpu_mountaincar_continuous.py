"""PPO_ENV_MOUNTAINCAR_CONTINUOUS (include/ppo_hip.h; ppo-libtorch_amd/csrc/kernels_gauss_fused.hip: gauss_rollout_kernel, gauss_trunc_fold_kernel,
gauss_eval_kernel) on the GPU through the C-ABI: the env against float64, the fused rollout against the stepwise API bit for bit, teacher forcing, the
truncation fold, the evaluation launch against a host loop, and every refusal.  Without the env none of these contexts can be created ("unknown env_kind 5").

Common setup (Pendulum's): orthogonal init, the actor's output layer scaled by 30 and log_std = 0.3 (samples leave the force range [-1, 1]),
max_episode_steps = 7 and T = 24: every env resets at least three times within a rollout, and the resets do not line up with T."""
import numpy as np
import pytest

from __graft_entry__ import load_package

from test_evaluate_abi import start_states

pytestmark = pytest.mark.gpu

T, MAXS = 24, 7
EPS = float(np.finfo(np.float32).eps)
ROLLOUT_BUFS = ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW", "NEXT_OBS", "NEXT_DONE", "VALUES", "NEXT_VALUE")
ALL_BUFS = ROLLOUT_BUFS + ("ADVANTAGES", "RETURNS", "PARAMS", "GRADS", "EXP_AVG", "EXP_AVG_SQ", "ENV_STATE", "EP_LEN", "EP_REW", "RESET_COUNT")
GOAL_START = (0.449, 0.05)   # one step from here reaches the goal with a positive velocity whatever the action: v' >= 0.05 - 0.0015 - 0.0025 > 0.045


@pytest.fixture(scope="module")
def P():
    return load_package()


@pytest.fixture(scope="module")
def O():
    import oracle   # Philox, for the evaluation's start states
    oracle.build()
    return oracle


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def mcc_cfg(P, N, **kw):
    d = dict(env_kind=P.ENV_MOUNTAINCAR_CONTINUOUS, dist_kind=P.DIST_GAUSSIAN, obs_size=2, head_dims=(1,), num_envs=N, num_steps=T, num_minibatches=2,
             update_epochs=2, max_episode_steps=MAXS, seed=5, total_timesteps=4 * N * T, learning_rate=1e-3, anneal_lr=True, gamma=0.99, gae_lambda=0.95,
             ent_coef=0.01, kernel_flags=P.KERNEL_GAUSS_FUSED)
    d.update(kw)
    return P.make_config(**d)


def common_params(ctx):
    """the common setup's parameters: the flat vector ends with the actor's output layer W3 [1, 64], b3 [1] and log_std [1]"""
    ctx.init_orthogonal(11)
    p = ctx.get_params()
    p[-66:-2] *= 30.0
    p[-1] = 0.3
    return p


def mcc_ctx(P, N, params=None, **kw):
    ctx = P.Context(mcc_cfg(P, N, **kw))
    ctx.set_params(common_params(ctx) if params is None else params)
    return ctx


def rollout_buffers(ctx):
    return {k: ctx.read(k) for k in ROLLOUT_BUFS}


def inject(ctx):
    """env_reset, then through ppo_env_set_state_h: every 5th env at GOAL_START (it terminates on its first step), every 7th env there with ep_len = 6
    (termination and the time limit fall on the same step).  Returns the observation, which is the state."""
    ctx.env_reset()
    state, ep_len, ep_rew, resets = ctx.env_get_state()
    n = np.arange(ctx.N)
    state[n % 5 == 0] = GOAL_START
    state[n % 7 == 0] = GOAL_START
    ep_len[n % 7 == 0] = MAXS - 1
    ctx.env_set_state(state, ep_len, ep_rew, resets)
    obs = ctx.read("NEXT_OBS", (ctx.N, 2))
    assert same(obs, state)
    return obs


# ---------------------------------------------------------------------------------------------------------
# 1. the transition against float64
# ---------------------------------------------------------------------------------------------------------
def transition_inputs():
    rng = np.random.default_rng(3)
    n = 4096
    p = rng.uniform(-1.2, 0.6, n).astype(np.float32)
    v = rng.uniform(-0.07, 0.07, n).astype(np.float32)
    a = rng.uniform(-1.5, 1.5, n).astype(np.float32)
    p[:512] = rng.uniform(0.40, 0.6, 512).astype(np.float32)
    p[512:1024] = rng.uniform(-1.2, -1.15, 512).astype(np.float32)
    return p, v, a


def transition_float64(p32, v32, a32):
    """The header's formulas in float64 on the f32 inputs (the constants are the f32 constants).  Per output the value and the bar, 8 x f32 epsilon x the
    largest intermediate magnitude of the output's formula (Pendulum's scheme); and the rows whose discontinuous parts -- the wall rule, `terminated`, the
    + 100 -- the bars cannot decide."""
    f = lambda x: float(np.float32(x))   # noqa: E731
    p, v, a = p32.astype(np.float64), v32.astype(np.float64), a32.astype(np.float64)
    u = np.minimum(np.maximum(a, -1.0), 1.0)
    t1, t2 = u * f(0.0015), f(0.0025) * np.cos(3.0 * p)
    acc = t1 - t2
    v_raw = v + acc
    v1 = np.minimum(np.maximum(v_raw, f(-0.07)), f(0.07))
    m_v = np.max(np.abs([v, t1, t2, acc, v_raw]), axis=0)
    p_raw = p + v1
    p1 = np.minimum(np.maximum(p_raw, f(-1.2)), f(0.6))
    m_p = np.maximum(m_v, np.max(np.abs([p, p_raw]), axis=0))
    wall = (p1 == f(-1.2)) & (v1 < 0)
    v2 = np.where(wall, 0.0, v1)
    term = (p1 >= f(0.45)) & (v2 >= 0.0)
    sq = a * a
    pen = f(0.1) * sq
    base = np.where(term, 100.0, 0.0)
    rew = base - pen
    m_r = np.max(np.abs([sq, pen, base, rew]), axis=0)
    bar_v, bar_p, bar_r = 8 * EPS * m_v, 8 * EPS * m_p, 8 * EPS * m_r
    undecided = (np.abs(p_raw - f(-1.2)) <= bar_p) | (np.abs(p1 - f(0.45)) <= bar_p) | ((np.abs(v1) <= bar_v) & ((p1 == f(-1.2)) | (p1 >= f(0.45))))
    return dict(v=(v2, bar_v), p=(p1, bar_p), reward=(rew, bar_r)), term, wall, undecided


def test_transition_against_float64(P):
    """ppo_env_transition_f32(5, ..) on 4096 rows -- 512 of them around the goal, 512 at the left wall -- against the header's formulas in numpy float64 on
    the f32 inputs.  Bar per output and row: 8 x f32 epsilon x the largest intermediate magnitude of that output's formula, computed in float64.  Only the
    two clips are continuous: a row whose float64 unclipped position lies within its bar of -1.2, whose clipped position lies within its bar of 0.45, or
    whose velocity lies within its bar of 0 at the wall or at / beyond the goal is left out (at most 1 % may be).  For these inputs the reference leaves out
    0 rows and has 394 terminating rows and 197 wall hits.  On the rows that stay `terminated` is the reference's exactly.
    Measured on an MI355X, the largest error as a fraction of its bar: v' 0.2169, p' 0.0825, reward 0.0399; 0 rows left out, 394 terminating on the device too."""
    p, v, a = transition_inputs()
    want, term64, wall64, undecided = transition_float64(p, v, a)
    ctx = mcc_ctx(P, 1)
    ns, ob, r, term = P.env_transition_f32(ctx, P.ENV_MOUNTAINCAR_CONTINUOUS, np.stack([p, v], 1), a)
    ns2, none, r2, term2 = P.env_transition_f32(ctx, P.ENV_MOUNTAINCAR_CONTINUOUS, np.stack([p, v], 1), a, want_obs=False)
    ctx.close()
    assert none is None and same(ns, ns2) and same(r, r2) and same(term, term2)
    assert ob.shape == (4096, 2) and same(ob, ns)
    keep = ~undecided
    print("left out %d rows; float64: %d terminating, %d wall hits; device: %d terminating" % (int(undecided.sum()), int(term64.sum()), int(wall64.sum()), int(term.sum())))
    assert undecided.sum() <= 0.01 * p.size
    assert term64[keep].sum() > 0 and wall64[keep].sum() > 0 and (~term64[keep]).sum() > 0
    got = dict(v=ns[:, 1], p=ns[:, 0], reward=r)
    worst = {k: float((np.abs(got[k].astype(np.float64) - exp)[keep] / bar[keep]).max()) for k, (exp, bar) in want.items()}
    print("largest error as a fraction of its bar:", {k: round(x, 4) for k, x in worst.items()})
    assert np.array_equal(term[keep] != 0, term64[keep])
    assert set(np.unique(term)) <= {0, 1}
    for k, x in worst.items():
        assert x <= 1.0, (k, x)
    # the wall rule and the goal, exactly, on the kept rows
    assert (ns[keep & wall64, 1] == 0).all() and (ns[keep & wall64, 0] == np.float32(-1.2)).all()
    assert (r[keep & term64] > 90).all() and (r[keep & ~term64] <= 0).all()


# ---------------------------------------------------------------------------------------------------------
# 2. the fused rollout against the stepwise API, bit for bit
# ---------------------------------------------------------------------------------------------------------
def stepwise_rollout(b, obs, done, step0):
    """T x { policy_act_f32(obs, step_index), env_step_f32 } on context b: the buffers a rollout would fill.  FIN_LEN / FIN_REW from the episode sums the
    context held in front of the step (f32 sum, the kernels' own operation)."""
    N = b.N
    out = {k: [] for k in ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW")}
    for t in range(T):
        act, lp, _, _ = b.policy_act_f32(obs, step_index=step0 + t)
        len0, rew0 = b.read("EP_LEN"), b.read("EP_REW")
        out["OBS"].append(obs)
        out["DONES"].append(done.astype(np.float32))
        obs, r, done = b.env_step_f32(act)
        out["ACTIONS"].append(act)
        out["LOGPROBS"].append(lp)
        out["REWARDS"].append(r)
        out["FIN_LEN"].append(np.where(done != 0, len0 + 1, 0).astype(np.int32))
        out["FIN_REW"].append(np.where(done != 0, rew0 + r, np.float32(0)).astype(np.float32))
        assert obs.shape == (N, 2)
    res = {k: np.stack(v).reshape(-1) for k, v in out.items()}
    res["NEXT_OBS"], res["NEXT_DONE"] = obs.reshape(-1), done
    return res, obs, done


@pytest.mark.parametrize("N", [1, 96, 200])
def test_fused_rollout_equals_stepwise_api(P, N):
    """N = 1: one lane; 96: a tile and a half; 200: three tiles and a bit.  Two rollouts: the second continues with step indices T .. 2 T - 1.  The injected
    states give the first rollout episodes the env ends itself, and ends where termination and the time limit coincide."""
    a, b = mcc_ctx(P, N), mcc_ctx(P, N)
    assert same(a.get_params(), b.get_params())
    obs = inject(b)
    assert same(inject(a), obs)
    done = np.zeros(N, np.int32)
    beyond = False
    for k in range(2):
        a.rollout()
        got = rollout_buffers(a)
        want, obs, done = stepwise_rollout(b, obs, done, k * T)
        for name, w in want.items():
            assert same(got[name], w), (k, name, int((bits(got[name]) != bits(w)).sum()))
        for x, y in zip(a.env_get_state(), b.env_get_state()):   # ENV_STATE, EP_LEN, EP_REW, RESET_COUNT
            assert same(x, y)
        O = got["OBS"].reshape(T * N, 2)
        assert same(got["VALUES"], a.get_value(O))
        assert same(got["NEXT_VALUE"], a.get_value(got["NEXT_OBS"].reshape(N, 2)))
        # the stored raw sample, forced through the stand-alone policy, gives the stored log-prob's bits
        fa, flp, _, _ = a.policy_act_f32(O, action=got["ACTIONS"].reshape(T * N, 1))
        assert same(fa.reshape(-1), got["ACTIONS"]) and same(flp, got["LOGPROBS"])
        beyond = beyond or bool((np.abs(got["ACTIONS"]) > 1).any())
        fin = got["FIN_LEN"].reshape(T, N)
        if k == 0:
            n = np.arange(N)
            assert (fin[0, n % 7 == 0] == MAXS).all()                     # termination and the time limit on the same step
            assert (fin[0, (n % 5 == 0) & (n % 7 != 0)] == 1).all()       # the env's own end
            assert (got["DONES"].reshape(T, N)[1] == (fin[0] > 0)).all()
            if N > 1:   # ends of both kinds
                assert (fin == MAXS).any() and ((fin > 0) & (fin < MAXS)).any()
                assert got["DONES"].sum() + got["NEXT_DONE"].sum() > N
    assert beyond or N == 1
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------
# 3. teacher forcing
# ---------------------------------------------------------------------------------------------------------
def test_teacher_forcing(P):
    """ppo_rollout_f32 with the actions of a free rollout reproduces it: every rollout buffer and the env's state, bit for bit"""
    N = 96
    free, forced = mcc_ctx(P, N), mcc_ctx(P, N)
    inject(free)
    inject(forced)
    free.rollout()
    got = rollout_buffers(free)
    forced.rollout(forced_actions=got["ACTIONS"].reshape(T, N, 1))
    rep = rollout_buffers(forced)
    for name in ROLLOUT_BUFS:
        assert same(got[name], rep[name]), name
    for x, y in zip(free.env_get_state(), forced.env_get_state()):
        assert same(x, y)
    assert (np.abs(got["ACTIONS"]) > 1).any() and got["DONES"].sum() > 0
    before = {k: forced.read(k) for k in ALL_BUFS}
    with pytest.raises(P.binding.PPOError, match=r"status 5: .*ppo_rollout_f32"):
        forced.rollout(forced_actions=np.zeros((T, N, 1), np.int64))
    assert all(same(before[k], forced.read(k)) for k in ALL_BUFS)
    free.close()
    forced.close()


# ---------------------------------------------------------------------------------------------------------
# 4. the truncation fold
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [96, 200])
def test_truncation_fold(P, N):
    """N = 96: the T * N = 2304 samples are 9 workgroups of the fold; 200: 18.75.  `never` never touched the switch, `off` turned it on and off again, `on`
    runs with it.  Same parameters, same injected states."""
    never, off, on = mcc_ctx(P, N), mcc_ctx(P, N), mcc_ctx(P, N)
    off.env_truncation_bootstrap(True)
    off.env_truncation_bootstrap(False)
    on.env_truncation_bootstrap(True)
    assert on.env_truncations()[0].size == 0   # no rollout yet
    counts = []
    for c in (never, off, on):
        inject(c)
        c0 = c.gauss_fused_launches()
        c.rollout()
        c1 = c.gauss_fused_launches()
        counts.append(tuple(y - x for x, y in zip(c0, c1)))
    assert counts == [(0, 2, 0)] * 3, counts   # the fold launch is none of the three kernels
    base, g_off, g_on = rollout_buffers(never), rollout_buffers(off), rollout_buffers(on)
    for name in ROLLOUT_BUFS:   # off is off, bit for bit
        assert same(base[name], g_off[name]), name
    assert off.env_truncations()[0].size == 0 and never.env_truncations()[0].size == 0

    # the events: FIN_LEN == max_episode_steps minus the rows whose recomputed step terminates
    at_limit = np.flatnonzero(base["FIN_LEN"] == MAXS)
    obs_i, act_i = base["OBS"].reshape(T * N, 2)[at_limit], base["ACTIONS"][at_limit]
    final, _, _, term = P.env_transition_f32(never, P.ENV_MOUNTAINCAR_CONTINUOUS, obs_i, act_i)
    expect = at_limit[term == 0]
    idx, val = on.env_truncations()
    assert idx.dtype == np.int32 and np.array_equal(idx, expect) and (np.diff(idx) > 0).all()
    coincident = np.flatnonzero(np.arange(N) % 7 == 0)   # t = 0: flat index = n
    assert (term != 0).sum() >= coincident.size and np.isin(coincident, at_limit).all() and not np.isin(coincident, idx).any()
    assert idx.size > N   # every env is cut off at least twice more within the rollout
    # each value is the critic's value of the final observation, bit for bit
    assert same(val, on.get_value(final[term == 0]))
    # REWARDS[i] = f32(r + f32(gamma * v)): two roundings
    gamma = np.float32(on.cfg.gamma)
    folded = base["REWARDS"].copy()
    folded[idx] = (base["REWARDS"][idx] + (gamma * val).astype(np.float32)).astype(np.float32)
    assert same(g_on["REWARDS"], folded) and not same(folded, base["REWARDS"])
    for name in ROLLOUT_BUFS:   # every other buffer is untouched: FIN_REW is raw
        if name != "REWARDS":
            assert same(base[name], g_on[name]), name
    for x, y in zip(never.env_get_state(), on.env_get_state()):   # EP_REW too
        assert same(x, y)
    idx2, val2 = on.env_truncations()   # reading twice gives the same list
    assert np.array_equal(idx, idx2) and same(val, val2)

    # an iteration with the switch on: finite, raw episode statistics, other advantages at the event rows
    for c in (never, on):
        c.train_iteration()
    s_never, s_on = never.stats(), on.stats()
    assert np.isfinite(s_on["loss"]) and np.isfinite(on.get_params()).all()
    assert s_on["ep_rew_mean"] == s_never["ep_rew_mean"] and s_on["ep_len_mean"] == s_never["ep_len_mean"] and s_on["ep_count"] == s_never["ep_count"] == 100
    assert same(never.read("FIN_REW"), on.read("FIN_REW")) and same(never.read("OBS"), on.read("OBS"))
    idx3, val3 = on.env_truncations()
    moved = idx3[val3 != 0]
    assert moved.size > 0 and (on.read("ADVANTAGES")[moved] != never.read("ADVANTAGES")[moved]).all()
    for c in (never, off, on):
        c.close()


# ---------------------------------------------------------------------------------------------------------
# 5. evaluation
# ---------------------------------------------------------------------------------------------------------
EVAL_SEED, EVAL_MAX, EVAL_N = 9, 100, 64


def pumping_params(ctx):
    """An actor that pushes the way the car moves: all zero except actor W1[0, 1] = 200, W2[0, 0] = 4, W3[0, 0] = 30, so mu = 30 tanh(4 tanh(200 v));
    a random critic; log_std = -1."""
    shapes = ctx.param_shapes()
    sizes = [int(r * c) for r, c in shapes]
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert [tuple(s) for s in shapes[6:9:2]] == [(64, 2), (64, 64)] and tuple(shapes[10]) == (1, 64) and off[-1] == ctx.P
    p = np.zeros(ctx.P, np.float32)
    p[:off[6]] = np.random.default_rng(8).normal(0, 0.3, off[6]).astype(np.float32)
    p[off[6] + 1] = 200.0
    p[off[8]] = 4.0
    p[off[10]] = 30.0
    p[-1] = -1.0
    return p


def host_episodes(P, ctx, states, greedy):
    """Whole episodes on the host: policy_act_f32 (greedy, or sampled with step_index = the episode's step) + env_transition_f32 on all rows, a finished row
    ignored; the f32 return in step order."""
    n = states.shape[0]
    st = states.copy()
    ret, length, alive = np.zeros(n, np.float32), np.zeros(n, np.int32), np.ones(n, bool)
    for t in range(EVAL_MAX):
        act = ctx.policy_act_f32(st, step_index=t, greedy=greedy)[0]
        ns, _, r, term = P.env_transition_f32(ctx, P.ENV_MOUNTAINCAR_CONTINUOUS, st, act, want_obs=False)
        ret[alive] = (ret[alive] + r[alive]).astype(np.float32)
        length[alive] += 1
        st[alive] = ns[alive]
        alive &= (term == 0) & (length < EVAL_MAX)
        if not alive.any():
            break
    return ret, length, (length == EVAL_MAX).astype(np.int32)


def test_evaluate(P, O):
    N = 32
    kw = dict(max_episode_steps=EVAL_MAX, seed=EVAL_SEED)
    ctx, ref, plain = P.Context(mcc_cfg(P, N, **kw)), P.Context(mcc_cfg(P, N, **kw)), P.Context(mcc_cfg(P, N, **kw))
    params = pumping_params(ctx)
    for c in (ctx, ref, plain):
        c.set_params(params)
        c.env_reset()
        c.rollout()
        c.sync()
    snap = lambda c: ({k: c.read(k) for k in ALL_BUFS}, c.get_optimizer()[2], c.gauss_fused_launches())   # noqa: E731
    before = snap(ctx)
    stats_g, ret_g, len_g = ctx.evaluate(EVAL_N, EVAL_SEED, greedy=True)
    stats_s, ret_s, len_s = ctx.evaluate(EVAL_N, EVAL_SEED, greedy=False)
    stats_16, ret_16, len_16 = ctx.evaluate(16, EVAL_SEED, greedy=True)
    stats_2, ret_2, len_2 = ctx.evaluate(EVAL_N, EVAL_SEED + 1, greedy=True)
    after = snap(ctx)
    assert before[1:] == after[1:]
    for k in ALL_BUFS:
        assert same(before[0][k], after[0][k]), k

    states = start_states(O, 1, EVAL_SEED, EVAL_N)
    assert states.shape == (EVAL_N, 2) and (states[:, 0] >= -0.6).all() and (states[:, 0] < -0.4).all()
    for greedy, (st, ret, length) in ((True, (stats_g, ret_g, len_g)), (False, (stats_s, ret_s, len_s))):
        h_ret, h_len, h_trunc = host_episodes(P, ref, states, greedy)
        print("greedy" if greedy else "sampled", "lengths %d..%d, truncated %d of %d" % (length.min(), length.max(), st["truncated"], EVAL_N))
        assert np.array_equal(length, h_len), (greedy, np.flatnonzero(length != h_len))
        assert same(ret, h_ret), (greedy, np.flatnonzero(bits(ret) != bits(h_ret)))
        assert st["truncated"] == int(h_trunc.sum()) and 0 < st["truncated"] < EVAL_N   # both kinds of end occur
        assert st["episodes"] == EVAL_N and st["env_steps"] == int(h_len.sum()) and st["length_max"] == EVAL_MAX
        assert abs(st["return_mean"] - h_ret.astype(np.float64).mean()) <= 1e-9 * max(1.0, abs(st["return_mean"]))
    assert not same(ret_g, ret_s)
    # results do not depend on how episodes are spread over workgroups
    assert same(ret_16, ret_g[:16]) and np.array_equal(len_16, len_g[:16]) and stats_16["episodes"] == 16
    # another seed, other start states
    assert not same(ret_2, ret_g) and not np.array_equal(len_2, len_g)
    states2 = start_states(O, 1, EVAL_SEED + 1, 4)
    first = ref.policy_act_f32(states2, greedy=True)[0]
    assert not same(states2, states[:4]) and np.isfinite(first).all()

    # the training state is untouched: an iteration afterwards is that of a context that never evaluated
    for c in (ctx, plain):
        c.train_iteration()
        c.sync()
    for k in ALL_BUFS:
        assert same(ctx.read(k), plain.read(k)), k
    assert ctx.stats() == plain.stats()
    for c in (ctx, ref, plain):
        c.close()


# ---------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,status,word", [
    (dict(obs_size=3), 1, "observation of size 2"),
    (dict(obs_size=4), 1, "observation of size 2"),
    (dict(dist_kind=0), 5, "PPO_DIST_GAUSSIAN"),
    (dict(dist_kind=1), 5, "PPO_DIST_GAUSSIAN"),
    (dict(head_dims=(2,)), 5, "head_dims[0] = 1"),
    (dict(head_dims=(1, 1)), 5, "n_heads = 1"),
    (dict(hidden=32), 5, "hidden = 64"),
    (dict(n_hidden=3), 5, "n_hidden = 2"),
    (dict(compute_dtype=1), 5, "PPO_DTYPE_F32"),
    (dict(kernel_flags=0), 5, "PPO_KERNEL_GAUSS_FUSED"),
    (dict(max_episode_steps=0), 5, "max_episode_steps"),
    (dict(max_episode_steps=-3), 5, "max_episode_steps"),
    (dict(env_kind=0, obs_size=4), 5, "PPO_ENV_HOST"),
    (dict(env_kind=1, obs_size=2), 5, "PPO_ENV_PENDULUM"),
    (dict(env_kind=2), 5, "PPO_ENV_MOUNTAINCAR_CONTINUOUS"),
])
def test_ctx_create_refusals(P, kw, status, word):
    with pytest.raises(P.binding.PPOError) as e:
        P.Context(mcc_cfg(P, 8, **kw))
    assert "status %d:" % status in str(e.value) and word in str(e.value), str(e.value)
    if "env_kind" in kw:   # Gaussian on CartPole, MountainCar and the synthetic env stays refused, and the message names every env that is served
        assert all(w in str(e.value) for w in ("PPO_ENV_HOST", "PPO_ENV_PENDULUM", "PPO_ENV_MOUNTAINCAR_CONTINUOUS"))


def test_any_time_limit_is_accepted(P):
    """no upper bound on max_episode_steps (the position is clipped to the track; gym's limit is 999)"""
    ctx = P.Context(mcc_cfg(P, 8, max_episode_steps=999))
    ctx.init_orthogonal(1)
    ctx.env_reset()
    ctx.rollout()
    assert (ctx.read("FIN_LEN") == 0).all() and (ctx.env_get_state()[1] == T).all()
    ctx.close()


def test_refused_calls_change_nothing(P):
    N = 40
    ctx = mcc_ctx(P, N)
    ctx.env_reset()
    ctx.train_iteration()
    ctx.rollout()
    ctx.sync()
    snap = lambda: ({k: ctx.read(k) for k in ALL_BUFS}, ctx.get_optimizer()[2], ctx.gauss_fused_launches())   # noqa: E731
    before = snap()
    o, r, d, a64 = np.zeros((N, 2), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int32), np.zeros((N, 1), np.int64)
    d_o, d_r, d_d, d_a, d_a64 = ctx.dev(o), ctx.dev(r), ctx.dev(d), ctx.dev(np.zeros((N, 1), np.float32)), ctx.dev(a64)
    calls = [
        # the caller-stepped families: PPO_ERR_STATE, as on any device-env context
        (3, "device environment", lambda: ctx.host_env_reset(o)),
        (3, "device environment", lambda: ctx.host_rollout_begin()),
        (3, "device environment", lambda: ctx.host_rollout_begin(groups=2)),
        (3, "device environment", lambda: ctx.host_act_f32()),
        (3, "device environment", lambda: ctx.host_act()),
        (3, "device environment", lambda: ctx.host_observe(o, r, d)),
        (3, "device environment", lambda: ctx.host_observe(o, r, d, truncated=d, final_obs=o)),
        (3, "device environment", lambda: ctx.host_rollout_end()),
        (3, "device environment", lambda: ctx.host_truncations()),
        (3, "device environment", lambda: ctx.dev_env_reset(d_o)),
        (3, "device environment", lambda: ctx.dev_act_f32(d_a)),
        (3, "device environment", lambda: ctx.dev_act(d_a64)),
        (3, "device environment", lambda: ctx.dev_observe(d_o, d_r, d_d)),
        # the normalisers serve caller-stepped envs
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_enable(1)),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_get()),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_set(np.zeros(2), np.ones(2), 1.0)),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_apply(o)),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_enable(1)),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_get()),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_set(0.0, 1.0, 1.0)),
        # the integer-action calls name their twins
        (5, "ppo_env_step_f32", lambda: ctx.env_step(a64)),
        (5, "ppo_rollout_f32", lambda: ctx.rollout(forced_actions=np.zeros((T, N, 1), np.int64))),
        (5, "ppo_policy_act_f32", lambda: ctx.policy_act(o)),
        # bad arguments of the calls this env does serve
        (1, "on must be 0 or 1", lambda: ctx.env_truncation_bootstrap(2)),
        (1, "n_episodes", lambda: ctx.evaluate(0, 1)),
    ]
    for status, word, call in calls:
        with pytest.raises(P.binding.PPOError) as e:
            call()
        assert "status %d:" % status in str(e.value) and word in str(e.value), str(e.value)
    ctx.sync()
    after = snap()
    assert before[1:] == after[1:]
    for k in ALL_BUFS:
        assert same(before[0][k], after[0][k]), k
    # and the context still works
    ctx.train_iteration()
    assert np.isfinite(ctx.stats()["loss"])
    ctx.close()


def test_pendulum_keeps_its_refusals(P):
    """PPO_ENV_PENDULUM's observation does not hold theta: its context still refuses the fold and the evaluation, with the same words"""
    cfg = P.make_config(env_kind=P.ENV_PENDULUM, dist_kind=P.DIST_GAUSSIAN, obs_size=3, head_dims=(1,), num_envs=8, num_steps=T, num_minibatches=2,
                        update_epochs=2, max_episode_steps=MAXS, seed=5, kernel_flags=P.KERNEL_GAUSS_FUSED)
    ctx = P.Context(cfg)
    ctx.init_orthogonal(1)
    ctx.env_reset()
    for word, call in (("ppo_evaluate is not built for PPO_ENV_PENDULUM", lambda: ctx.evaluate(4, 1)),
                       ("does not hold theta", lambda: ctx.env_truncation_bootstrap(True)),
                       ("does not hold theta", lambda: ctx.env_truncations())):
        with pytest.raises(P.binding.PPOError) as e:
            call()
        assert "status 5:" in str(e.value) and word in str(e.value), str(e.value)
    ctx.rollout()
    assert ctx.gauss_fused_launches() == (0, 2, 0)
    ctx.close()
