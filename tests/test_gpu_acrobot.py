"""PPO_ENV_ACROBOT (include/ppo_hip.h; ppo-libtorch_amd/csrc/kernels_gauss_fused.hip: cat_rollout_kernel, cat_eval_kernel, the cat_env_* kernels) on the GPU
through the C-ABI: the env against float64 (the yardstick is tests/acrobot_model.py, itself checked by tests/test_acrobot_cpu.py), the corners of the state
box, resets, the fused rollout against the stepwise API bit for bit, teacher forcing, the host-fed iteration, launch accounting, episode statistics, the
evaluation launch against a host loop, and every refusal.  Without the env none of these contexts can be created ("unknown env_kind 6").

Common setup: orthogonal init with the actor's output layer scaled by 300 (the three actions get visibly different probabilities), max_episode_steps = 5 and
T = 9: time-limit ends fall inside a rollout, and a second rollout starts at step index 9, so the Philox word select (& 3) and counter (>> 2) are both crossed.

The observation of a state has no symbol of its own (the exported set is pinned at 92): ppo_env_set_state_h refills NEXT_OBS from the state with the
rollout's own device function, and `observe` below reads it there."""
import importlib.util
import os

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package

import acrobot_model as M

pytestmark = pytest.mark.gpu

T, MAXS = 9, 5
ROLLOUT_BUFS = ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW", "NEXT_OBS", "NEXT_DONE", "VALUES", "NEXT_VALUE", "MASKS")
ALL_BUFS = ROLLOUT_BUFS + ("ADVANTAGES", "RETURNS", "PARAMS", "GRADS", "EXP_AVG", "EXP_AVG_SQ", "ENV_STATE", "EP_LEN", "EP_REW", "RESET_COUNT")
UPRIGHT = (3.0, 0.0, 0.0, 0.0)   # one step from here ends the episode whatever the action (tests/test_acrobot_cpu.py)


@pytest.fixture(scope="module")
def P():
    return load_package()


@pytest.fixture(scope="module")
def O():
    import oracle   # Philox, for the resets
    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def Y():
    return M.yardstick()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def acro_cfg(P, N, **kw):
    d = dict(env_kind=P.ENV_ACROBOT, dist_kind=P.DIST_CATEGORICAL, obs_size=6, head_dims=(3,), num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2,
             max_episode_steps=MAXS, seed=5, total_timesteps=4 * N * T, learning_rate=1e-3, anneal_lr=True, gamma=0.99, gae_lambda=0.95, ent_coef=0.01,
             kernel_flags=P.KERNEL_CAT_FUSED)
    d.update(kw)
    return P.make_config(**d)


def common_params(ctx):
    """the flat vector ends with the actor's output layer W3 [3, 64], b3 [3]"""
    ctx.init_orthogonal(11)
    p = ctx.get_params()
    p[-195:-3] *= 300.0
    return p


def acro_ctx(P, N, params=None, **kw):
    ctx = P.Context(acro_cfg(P, N, **kw))
    ctx.set_params(common_params(ctx) if params is None else params)
    return ctx


def rollout_buffers(ctx):
    return {k: ctx.read(k) for k in ROLLOUT_BUFS}


def observe(ctx, states):
    """The device's observation of ctx.N states: ppo_env_set_state_h refills NEXT_OBS from the state (the context's env state is overwritten)."""
    ctx.env_set_state(np.ascontiguousarray(states, np.float32))
    return ctx.read("NEXT_OBS", (ctx.N, 6))


def inject(ctx):
    """env_reset, then through ppo_env_set_state_h: every 5th env near the upright (it terminates on its first step), every 7th env there with
    ep_len = MAXS - 1 and the return of four steps (termination and the time limit fall on the same step).  Returns the observation."""
    ctx.env_reset()
    state, ep_len, ep_rew, resets = ctx.env_get_state()
    assert state.shape == (ctx.N, 4)
    n = np.arange(ctx.N)
    state[n % 5 == 0] = UPRIGHT
    state[n % 7 == 0] = UPRIGHT
    ep_len[n % 7 == 0] = MAXS - 1
    ep_rew[n % 7 == 0] = -(MAXS - 1.0)
    ctx.env_set_state(state, ep_len, ep_rew, resets)
    return ctx.read("NEXT_OBS", (ctx.N, 6))


def reset_states(O, seed, envs, k):
    """Reset number k[i] of global env envs[i]: the four words of philox4x32_10(seed; e, k, 0, 1) through canon_to_uniform(-0.1f, 0.1f), in state order."""
    f = np.float32
    a, b = f(-0.1), f(0.1)
    out = np.zeros((len(envs), 4), f)
    for i, (e, kk) in enumerate(zip(envs, k)):
        w = O.philox4x32(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, int(e), int(kk), 0, 1)
        for j in range(4):
            r = f(w[j]) / f(4294967296.0)
            if r >= f(1.0):
                r = np.nextafter(f(1.0), f(0.0))
            out[i, j] = f(r * f(b - a)) + a
    return out


# ---------------------------------------------------------------------------------------------------------
# 1. the transition and the observation against float64
# ---------------------------------------------------------------------------------------------------------
def test_transition_against_float64(P, Y):
    """ppo_env_transition(6, ..) on set A against the model in float64.  The bar per output is 8 x e_out, e_out the float32 model's own worst deviation,
    computed here, not written down: 8 because numpy's and glibc's sin / cos may differ in the last bit at 16 places per step and because e_out is a sample
    maximum.  Angles modulo 2 pi.  Reward and `terminated` exactly on the rows the float64 values do not leave out (tests/test_acrobot_cpu.py: <= 1 %)."""
    ctx = acro_ctx(P, 1)
    ns, r, term = P.env_transition(ctx, P.ENV_ACROBOT, Y["st"], Y["act"])
    ctx.close()
    assert ns.shape == (4096, 4) and ns.dtype == np.float32
    err = M.state_error(ns, Y["ref"]).max(axis=0)
    bar = 8 * Y["e_out"]
    print("worst / bar per output (th1, th2, w1, w2):", np.round(err / bar, 4), "e_out", Y["e_out"])
    assert (err <= bar).all(), (err, bar)
    keep = Y["keep"]
    assert keep.mean() >= 0.99
    assert np.array_equal(term[keep], Y["term"][keep]) and same(r[keep], Y["rew"][keep])
    assert set(np.unique(term)) <= {0, 1} and 0 < term.sum() < term.size
    assert (np.abs(ns[:, :2]) <= np.float32(np.pi)).all()


def test_observation_against_float64(P, Y):
    """The observation of set A's states (and of their successors): one ulp of the result; the inputs are the same float32 numbers on both sides, so no
    input error propagates.  The Pendulum case: the same path on a PPO_ENV_PENDULUM context, |theta| <= 100."""
    ctx = acro_ctx(P, 4096, num_steps=1, num_minibatches=1)
    for states in (Y["st"], Y["ns32"]):
        got = observe(ctx, states)
        ref = M.observation(states, np.float64)
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        worst = (np.abs(got.astype(np.float64) - ref) / ulp).max(axis=0)
        print("observation error in ulps of the result:", np.round(worst, 3))
        assert (worst <= 1.0).all(), worst
        assert same(got[:, 4:], np.ascontiguousarray(states[:, 2:]))
    ctx.close()
    pend = P.Context(P.make_config(env_kind=P.ENV_PENDULUM, dist_kind=P.DIST_GAUSSIAN, obs_size=3, head_dims=(1,), num_envs=4096, num_steps=1, num_minibatches=1,
                                   max_episode_steps=10, kernel_flags=P.KERNEL_GAUSS_FUSED))
    rng = np.random.default_rng(2)
    st = np.stack([rng.uniform(-100, 100, 4096), rng.uniform(-8, 8, 4096)], 1).astype(np.float32)
    pend.env_set_state(st)
    got = pend.read("NEXT_OBS", (4096, 3))
    ref = np.stack([np.cos(st[:, 0].astype(np.float64)), np.sin(st[:, 0].astype(np.float64)), st[:, 1].astype(np.float64)], 1)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - ref) <= ulp).all()
    pend.close()


# ---------------------------------------------------------------------------------------------------------
# 2. the corners of the state box
# ---------------------------------------------------------------------------------------------------------
def test_corners_of_the_state_box(P):
    """Set B: the 16 corners times the 3 actions plus 256 random rows at the full velocity range (304 rows: 4.75 tiles).  The RK4 stage angles leave the
    range of the device sinf / cosf there; with the header's large-argument rule the outputs are finite, inside the box and wrapped, and
    ppo_env_transition, ppo_env_step and a one-step rollout agree bit for bit."""
    st, act = M.set_b()
    n = st.shape[0]
    assert n == 304
    a = acro_ctx(P, n, num_steps=1, num_minibatches=1, max_episode_steps=1000)
    b = acro_ctx(P, n, num_steps=1, num_minibatches=1, max_episode_steps=1000)
    ns, r, term = P.env_transition(a, P.ENV_ACROBOT, st, act)
    f = np.float32
    assert np.isfinite(ns).all()
    assert (np.abs(ns[:, :2]) <= f(np.pi)).all() and (np.abs(ns[:, 2]) <= f(M.MAX_W1)).all() and (np.abs(ns[:, 3]) <= f(M.MAX_W2)).all()
    assert set(np.unique(r)) <= {f(0.0), f(-1.0)} and np.array_equal(r == 0, term == 1)
    # the float32 model agrees to rounding where the step is tame; in the corners it only has to be finite and inside (tests/test_acrobot_cpu.py)
    zero = np.zeros(n, np.int32)
    for c in (a, b):
        c.env_reset()
        c.env_set_state(st, zero, np.zeros(n, f), np.ones(n, np.int32))
    seer = acro_ctx(P, n, num_steps=1, num_minibatches=1)
    obs_ns = observe(seer, ns)
    seer.close()
    # ppo_env_step: the rows that did not terminate hold the transition's state; the others were reset
    o, r2, d = a.env_step(act.reshape(n, 1))
    s_a = a.env_get_state()
    assert same(r2, r) and np.array_equal(d, term)
    live = term == 0
    assert same(np.ascontiguousarray(s_a[0][live]), np.ascontiguousarray(ns[live])) and same(np.ascontiguousarray(o[live]), np.ascontiguousarray(obs_ns[live]))
    assert (np.abs(s_a[0][~live]) <= f(0.1)).all() and (s_a[3][~live] == 2).all() and (s_a[3][live] == 1).all()
    # a one-step rollout under the same (forced) actions
    b.rollout(forced_actions=act.reshape(1, n, 1))
    s_b = b.env_get_state()
    for x, y in zip(s_a, s_b):
        assert same(x, y)
    assert same(b.read("REWARDS"), r) and np.array_equal(b.read("NEXT_DONE"), term) and same(b.read("NEXT_OBS", (n, 6)), o)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------
# 3. resets
# ---------------------------------------------------------------------------------------------------------
def test_resets(P, O):
    N, K = 200, 70
    big, again, part = acro_ctx(P, N, max_episode_steps=3), acro_ctx(P, N), acro_ctx(P, N - K, env_offset=K, global_num_envs=N)
    obs = big.env_reset()
    st, ep_len, ep_rew, resets = big.env_get_state()
    assert (st >= np.float32(-0.1)).all() and (st < np.float32(0.1)).all()
    want = reset_states(O, 5, np.arange(N), [1] + [0] * (N - 1))   # global env 0 takes reset 1
    assert same(st, want)
    assert np.array_equal(resets, [2] + [1] * (N - 1)) and (ep_len == 0).all() and (ep_rew == 0).all() and (big.read("NEXT_DONE") == 0).all()
    assert same(obs, observe(other_ctx := acro_ctx(P, N), st))
    other_ctx.close()
    assert same(again.env_reset(), obs)                            # the same seed gives the same bits
    obs_p = part.env_reset()
    assert same(obs_p, np.ascontiguousarray(obs[K:])) and same(part.env_get_state()[0], np.ascontiguousarray(st[K:]))
    assert (part.env_get_state()[3] == 1).all()
    other = acro_ctx(P, N, seed=6)
    assert not same(other.env_reset(), obs)
    # the resets a rollout makes (max_episode_steps = 3, T = 9: every env has just finished its third episode): the state is reset RESET_COUNT - 1 of the env
    big.rollout()
    st2, _, _, resets2 = big.env_get_state()
    fresh = np.flatnonzero(big.read("NEXT_DONE") != 0)
    assert fresh.size == N and np.array_equal(resets2, resets + 3)
    assert same(np.ascontiguousarray(st2[fresh]), reset_states(O, 5, fresh, resets2[fresh] - 1))
    for c in (big, again, part, other):
        c.close()


# ---------------------------------------------------------------------------------------------------------
# 4. the fused rollout against the stepwise API, bit for bit
# ---------------------------------------------------------------------------------------------------------
def stepwise_rollout(b, obs, done, step0):
    """T x { policy_act(obs, step_index), env_step } on context b: the buffers a rollout would fill.  FIN_LEN / FIN_REW from the episode sums the context
    held in front of the step (f32 sum, the kernels' own operation)."""
    N = b.N
    out = {k: [] for k in ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW")}
    for t in range(T):
        act, lp, _, _ = b.policy_act(obs, step_index=step0 + t)
        len0, rew0 = b.read("EP_LEN"), b.read("EP_REW")
        out["OBS"].append(obs)
        out["DONES"].append(done.astype(np.float32))
        obs, r, done = b.env_step(act)
        out["ACTIONS"].append(act.astype(np.int32))
        out["LOGPROBS"].append(lp)
        out["REWARDS"].append(r)
        out["FIN_LEN"].append(np.where(done != 0, len0 + 1, 0).astype(np.int32))
        out["FIN_REW"].append(np.where(done != 0, rew0 + r, np.float32(0)).astype(np.float32))
        assert obs.shape == (N, 6)
    res = {k: np.stack(v).reshape(-1) for k, v in out.items()}
    res["NEXT_OBS"], res["NEXT_DONE"] = obs.reshape(-1), done
    res["MASKS"] = np.ones(T * N * 3, np.uint8)
    return res, obs, done


@pytest.mark.parametrize("N", [1, 96, 200])
def test_fused_rollout_equals_stepwise_api(P, N):
    """N = 1: one lane; 96: a full and a partial tile; 200: four workgroups.  Two rollouts in a row: the second runs step indices 9 .. 17, and carries the
    done flags and the episode sums of the first.  The injected states give the first rollout terminations at step 1 and an end where termination and the
    time limit coincide; max_episode_steps = 5 puts time-limit ends inside."""
    a, b = acro_ctx(P, N), acro_ctx(P, N)
    assert same(a.get_params(), b.get_params())
    obs = inject(b)
    assert same(inject(a), obs)
    done = np.zeros(N, np.int32)
    seen = set()
    for k in range(2):
        a.rollout()
        got = rollout_buffers(a)
        want, obs, done = stepwise_rollout(b, obs, done, k * T)
        for name, w in want.items():
            assert same(got[name], w), (k, name, int((bits(got[name]) != bits(w)).sum()))
        for x, y in zip(a.env_get_state(), b.env_get_state()):   # ENV_STATE, EP_LEN, EP_REW, RESET_COUNT
            assert same(x, y)
        Ob = got["OBS"].reshape(T * N, 6)
        assert same(got["VALUES"], a.get_value(Ob))
        assert same(got["NEXT_VALUE"], a.get_value(got["NEXT_OBS"].reshape(N, 6)))
        # the stored action, forced through the stand-alone policy, gives the stored log-prob's bits
        fa, flp, _, _ = a.policy_act(Ob, action=got["ACTIONS"].reshape(T * N, 1))
        assert np.array_equal(fa.reshape(-1), got["ACTIONS"]) and same(flp, got["LOGPROBS"])
        seen |= set(np.unique(got["ACTIONS"]).tolist())
        fin = got["FIN_LEN"].reshape(T, N)
        if k == 0:
            n = np.arange(N)
            assert (fin[0, n % 7 == 0] == MAXS).all()                     # termination and the time limit on the same step
            assert (fin[0, (n % 5 == 0) & (n % 7 != 0)] == 1).all()       # the env's own end, at step 1
            assert (got["REWARDS"].reshape(T, N)[0, n % 5 == 0] == 0).all()
            assert (got["DONES"].reshape(T, N)[1] == (fin[0] > 0)).all()
            if N > 1:
                assert (fin[1:] == MAXS).any()                            # time-limit ends inside the rollout
    assert seen == {0, 1, 2} or N == 1
    a.close()
    b.close()


def test_rows_do_not_depend_on_the_launch(P):
    big, small = acro_ctx(P, 200), acro_ctx(P, 64)
    for ctx in (big, small):
        ctx.env_reset()
        ctx.rollout()
    gb, gs = rollout_buffers(big), rollout_buffers(small)
    for name in ROLLOUT_BUFS:
        per_step = name not in ("NEXT_OBS", "NEXT_DONE", "NEXT_VALUE")
        x = gb[name].reshape((T, 200, -1) if per_step else (200, -1))
        y = gs[name].reshape((T, 64, -1) if per_step else (64, -1))
        assert same(np.ascontiguousarray(x[:, :64] if per_step else x[:64]), y), name
    big.close()
    small.close()


# ---------------------------------------------------------------------------------------------------------
# 5. teacher forcing
# ---------------------------------------------------------------------------------------------------------
def test_teacher_forcing(P):
    """forced actions are stored as given, with ppo_policy_act's log-prob; forcing a free rollout's actions reproduces it"""
    N = 96
    ctx = acro_ctx(P, N)
    ctx.env_reset()
    forced = np.random.default_rng(4).integers(0, 3, (T, N, 1)).astype(np.int64)
    ctx.rollout(forced_actions=forced)
    got = rollout_buffers(ctx)
    assert np.array_equal(got["ACTIONS"], forced.reshape(-1))
    _, lp, _, v = ctx.policy_act(got["OBS"].reshape(T * N, 6), action=forced.reshape(T * N, 1))
    assert same(lp, got["LOGPROBS"]) and same(v, got["VALUES"])
    free, rep = acro_ctx(P, N), acro_ctx(P, N)
    inject(free)
    inject(rep)
    free.rollout()
    g = rollout_buffers(free)
    rep.rollout(forced_actions=g["ACTIONS"].reshape(T, N, 1))
    r = rollout_buffers(rep)
    for name in ROLLOUT_BUFS:
        assert same(g[name], r[name]), name
    for x, y in zip(free.env_get_state(), rep.env_get_state()):
        assert same(x, y)
    for c in (ctx, free, rep):
        c.close()


# ---------------------------------------------------------------------------------------------------------
# 6. an iteration equals the host-fed iteration, bit for bit
# ---------------------------------------------------------------------------------------------------------
def test_iteration_equals_the_host_fed_iteration(P):
    """Both routes run ppo_update's one PPO_KERNEL_CAT_FUSED path (cat_fused_fwd_bwd, five launches per minibatch step) and the same scan; only the rollout
    differs.  So the comparison is bit for bit: two train_iterations of an Acrobot context against a PPO_ENV_HOST context (PPO_KERNEL_CAT_FUSED, obs 6,
    heads (3,), same parameters and seed) fed by host_act, a third context's env_step and host_observe."""
    N = 96
    dev = acro_ctx(P, N)
    host = P.Context(acro_cfg(P, N, env_kind=P.ENV_HOST))
    env = acro_ctx(P, N)
    params = dev.get_params()
    host.set_params(params)
    dev.env_reset()
    host.host_env_reset(env.env_reset())
    for _ in range(2):
        dev.train_iteration()
        host.host_rollout_begin()
        for _t in range(T):
            o, r, d = env.env_step(host.host_act())
            host.host_observe(o, r, d)
        host.host_rollout_end()
    sd, sh = dev.stats(), host.stats()
    for name in ("OBS", "ACTIONS", "LOGPROBS", "REWARDS", "DONES", "VALUES", "MASKS", "ADVANTAGES", "RETURNS"):
        assert same(dev.read(name), host.read(name)), name
    assert same(dev.get_params(), host.get_params()) and not same(dev.get_params(), params)
    (m0, v0, k0), (m1, v1, k1) = dev.get_optimizer(), host.get_optimizer()
    assert same(m0, m1) and same(v0, v1) and k0 == k1 == 2 * 2 * 2
    assert sd["loss"] == sh["loss"] and sd["global_step"] == sh["global_step"] == 2 * N * T
    for c in (dev, host, env):
        c.close()


# ---------------------------------------------------------------------------------------------------------
# 7. launch accounting, episode statistics
# ---------------------------------------------------------------------------------------------------------
def test_launch_accounting(P):
    ctx = acro_ctx(P, 96)
    ctx.env_reset()
    a0, v0, u0 = ctx.gauss_fused_launches()
    ctx.rollout()
    a1, v1, u1 = ctx.gauss_fused_launches()
    assert (a1 - a0, v1 - v0, u1 - u0) == (0, 2, 0)   # the rollout kernel is not an act launch; the critic over OBS and over NEXT_OBS
    ctx.calc_advantage()
    a2, v2, u2 = ctx.gauss_fused_launches()
    ctx.update()
    a3, v3, u3 = ctx.gauss_fused_launches()
    assert (a3 - a2, u3 - u2) == (0, ctx.cfg.update_epochs * ctx.cfg.num_minibatches)
    ctx.evaluate(16, 3)
    assert ctx.gauss_fused_launches() == (a3, v3, u3)  # ppo_evaluate moves nothing
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("N", [8, 96])
def test_episode_statistics(P, N):
    """N = 8: the ring is not full; N = 96: it keeps the last 100 in push order (step, then env).  The ring holds the FIN_REW values themselves."""
    ctx = acro_ctx(P, N)
    inject(ctx)
    ctx.rollout()
    ctx.calc_advantage()
    ctx.update()
    st = ctx.stats()
    fin_len, fin_rew = ctx.read("FIN_LEN"), ctx.read("FIN_REW")
    n_done = int(ctx.read("DONES").sum() + ctx.read("NEXT_DONE").sum())
    assert n_done == int((fin_len > 0).sum()) > 0
    k = min(n_done, 100)
    assert st["ep_count"] == k
    last_r, last_l = fin_rew[fin_len > 0][-k:].astype(np.float64), fin_len[fin_len > 0][-k:].astype(np.float64)
    assert abs(st["ep_rew_mean"] - last_r.mean()) <= 1e-6 * abs(last_r.mean()) and abs(st["ep_len_mean"] - last_l.mean()) <= 1e-6 * last_l.mean()
    # an episode's return is minus its length, plus one where the env ended it itself
    assert ((fin_rew[fin_len > 0] == -fin_len[fin_len > 0]) | (fin_rew[fin_len > 0] == 1 - fin_len[fin_len > 0])).all()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 8. evaluation
# ---------------------------------------------------------------------------------------------------------
EVAL_SEED, EVAL_N = 9, 64


def pumping_params(ctx):
    """An actor that pushes the way the second link turns -- logits (-c, -1, +c) h with h = tanh(4 tanh(200 w2)), c = 3 -- which swings the model up in 65
    to ~100 steps from the reset states (found with tests/acrobot_model.py: no rule tried there gets up in fewer than 65); a random critic."""
    shapes = ctx.param_shapes()
    sizes = [int(r * c) for r, c in shapes]
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert [tuple(s) for s in shapes[6:9:2]] == [(64, 6), (64, 64)] and tuple(shapes[10]) == (3, 64) and off[-1] == ctx.P
    p = np.zeros(ctx.P, np.float32)
    p[:off[6]] = np.random.default_rng(8).normal(0, 0.3, off[6]).astype(np.float32)
    p[off[6] + 5] = 200.0           # W1[0, 5]: w2
    p[off[8]] = 4.0                 # W2[0, 0]
    p[off[10]] = -3.0               # W3[0, 0]
    p[off[10] + 2 * 64] = 3.0       # W3[2, 0]
    p[off[11] + 1] = -1.0           # b3[1]
    return p


def host_episodes(P, ctx, states, greedy, max_steps):
    """Whole episodes on the host: the observation of the states, policy_act_greedy / policy_act(step_index = the episode's step) and env_transition on all
    rows, a finished row ignored; the f32 return in step order."""
    n = states.shape[0]
    st = states.copy()
    ret, length, alive = np.zeros(n, np.float32), np.zeros(n, np.int32), np.ones(n, bool)
    for t in range(max_steps):
        obs = observe(ctx, st)
        act = ctx.policy_act_greedy(obs)[0] if greedy else ctx.policy_act(obs, step_index=t)[0]
        ns, r, term = P.env_transition(ctx, P.ENV_ACROBOT, st, act)
        ret[alive] = (ret[alive] + r[alive]).astype(np.float32)
        length[alive] += 1
        st[alive] = ns[alive]
        alive &= (term == 0) & (length < max_steps)
        if not alive.any():
            break
    return ret, length, (length == max_steps).astype(np.int32)


@pytest.mark.parametrize("max_steps", [40, 80])
def test_evaluate(P, O, max_steps):
    """64 episodes, greedy and sampled, against the host loop.  max_episode_steps = 40: no policy swings Acrobot up from its reset states
    in 40 steps, so every episode is cut off there.  80: under the pumping policy some greedy episodes terminate and some are truncated."""
    N = 32
    kw = dict(max_episode_steps=max_steps, seed=EVAL_SEED)
    ctx, plain = P.Context(acro_cfg(P, N, **kw)), P.Context(acro_cfg(P, N, **kw))
    ref = P.Context(acro_cfg(P, EVAL_N, **kw))   # env_offset 0 and the same seed: row e of its policy_act is episode e's sampler
    params = pumping_params(ctx)
    for c in (ctx, ref, plain):
        c.set_params(params)
        c.env_reset()
    for c in (ctx, plain):
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

    states = reset_states(O, EVAL_SEED, np.arange(EVAL_N), [0] * EVAL_N)   # episode e starts at reset 0 of env e
    for greedy, (st, ret, length) in ((True, (stats_g, ret_g, len_g)), (False, (stats_s, ret_s, len_s))):
        h_ret, h_len, h_trunc = host_episodes(P, ref, states, greedy, max_steps)
        print("greedy" if greedy else "sampled", "lengths %d..%d, truncated %d of %d" % (length.min(), length.max(), st["truncated"], EVAL_N))
        assert np.array_equal(length, h_len), (greedy, np.flatnonzero(length != h_len))
        assert same(ret, h_ret), (greedy, np.flatnonzero(bits(ret) != bits(h_ret)))
        assert st["truncated"] == int(h_trunc.sum())
        assert st["episodes"] == EVAL_N and st["env_steps"] == int(h_len.sum()) and st["length_max"] == max_steps
        assert abs(st["return_mean"] - h_ret.astype(np.float64).mean()) <= 1e-9 * max(1.0, abs(st["return_mean"]))
    if max_steps == 80:
        assert 0 < stats_g["truncated"] < EVAL_N   # both kinds of end occur
        assert not same(ret_g, ret_s)
        assert not same(ret_2, ret_g)              # another seed differs
    else:
        assert stats_g["truncated"] == EVAL_N and (ret_g == -40).all()
    # results do not depend on how episodes are spread over workgroups
    assert same(ret_16, ret_g[:16]) and np.array_equal(len_16, len_g[:16]) and stats_16["episodes"] == 16
    assert not same(reset_states(O, EVAL_SEED + 1, range(4), [0] * 4), states[:4])

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
# 9. refusals
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,status,word", [
    (dict(obs_size=4), 1, "observation of size 6"),
    (dict(obs_size=8), 1, "observation of size 6"),
    (dict(dist_kind=1), 5, "PPO_DIST_CATEGORICAL"),
    (dict(dist_kind=2, head_dims=(1,)), 5, "PPO_DIST_CATEGORICAL"),
    (dict(head_dims=(2,)), 5, "head_dims[0] = 3"),
    (dict(head_dims=(3, 3)), 5, "n_heads = 1"),
    (dict(hidden=32), 5, "hidden = 64"),
    (dict(n_hidden=3), 5, "n_hidden = 2"),
    (dict(compute_dtype=1), 5, "PPO_DTYPE_F32"),
    (dict(kernel_flags=0), 5, "PPO_KERNEL_CAT_FUSED"),
    (dict(kernel_flags=64), 5, "PPO_KERNEL_CAT_FUSED"),
    (dict(max_episode_steps=0), 5, "max_episode_steps"),
    (dict(max_episode_steps=-3), 5, "max_episode_steps"),
])
def test_ctx_create_refusals(P, kw, status, word):
    with pytest.raises(P.binding.PPOError) as e:
        P.Context(acro_cfg(P, 8, **kw))
    assert "status %d:" % status in str(e.value) and word in str(e.value), str(e.value)


def test_pinned_refusals_still_hold(P):
    """What older tests pin: PPO_KERNEL_CAT_FUSED on the reference's envs and the synthetic env names the flag and PPO_ENV_HOST; a Gaussian policy on a
    discrete env names the three envs it serves; env_kind 7 is unknown; ppo_env_transition_f32(6, ..) is PPO_ERR_UNSUPPORTED."""
    def refused(words, status, **kw):
        with pytest.raises(P.binding.PPOError) as e:
            P.Context(P.make_config(**kw))
        assert "status %d" % status in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    refused(("PPO_KERNEL_CAT_FUSED", "PPO_ENV_HOST"), 5, env_kind=P.ENV_CARTPOLE, obs_size=4, head_dims=(2,), kernel_flags=P.KERNEL_CAT_FUSED)
    refused(("PPO_KERNEL_CAT_FUSED", "PPO_ENV_HOST"), 5, env_kind=P.ENV_MOUNTAINCAR, obs_size=2, head_dims=(3,), kernel_flags=P.KERNEL_CAT_FUSED)
    refused(("PPO_KERNEL_CAT_FUSED", "PPO_ENV_HOST"), 5, env_kind=P.ENV_SYNTHETIC, obs_size=6, head_dims=(3,), hidden=64, n_hidden=2, kernel_flags=P.KERNEL_CAT_FUSED)
    refused(("PPO_ENV_HOST", "PPO_ENV_PENDULUM", "PPO_ENV_MOUNTAINCAR_CONTINUOUS"), 5, env_kind=P.ENV_CARTPOLE, obs_size=4, head_dims=(1,), dist_kind=P.DIST_GAUSSIAN)
    refused(("unknown env_kind 7",), 1, env_kind=7, obs_size=6, head_dims=(3,), kernel_flags=P.KERNEL_CAT_FUSED)
    import ctypes as C
    buf, term = (C.c_float * 8)(), (C.c_int32 * 2)()
    assert P.binding.lib().ppo_env_transition_f32(6, buf, buf, 0, buf, None, buf, term, None) == 5


def test_refused_calls_change_nothing(P):
    N = 40
    ctx = acro_ctx(P, N)
    ctx.env_reset()
    ctx.train_iteration()
    ctx.rollout()
    ctx.sync()
    snap = lambda: ({k: ctx.read(k) for k in ALL_BUFS}, ctx.get_optimizer()[2], ctx.gauss_fused_launches())   # noqa: E731
    before = snap()
    o, r, d, af = np.zeros((N, 6), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int32), np.zeros((N, 3), np.float32)   # the binding shapes an f32 action [N, A]
    d_o, d_r, d_d, d_a, d_a64 = ctx.dev(o), ctx.dev(r), ctx.dev(d), ctx.dev(af), ctx.dev(np.zeros((N, 1), np.int64))
    L = P.binding.lib()
    calls = [
        # the caller-stepped families: PPO_ERR_STATE, as on any device-env context
        (3, "device environment", lambda: ctx.host_env_reset(o)),
        (3, "device environment", lambda: ctx.host_rollout_begin()),
        (3, "device environment", lambda: ctx.host_rollout_begin(groups=2)),
        (3, "device environment", lambda: ctx.host_act()),
        (3, "device environment", lambda: ctx.host_observe(o, r, d)),
        (3, "device environment", lambda: ctx.host_observe(o, r, d, truncated=d, final_obs=o)),
        (3, "device environment", lambda: ctx.host_rollout_end()),
        (3, "device environment", lambda: ctx.host_truncations()),
        (3, "device environment", lambda: ctx.dev_env_reset(d_o)),
        (3, "device environment", lambda: ctx.dev_act(d_a64)),
        (3, "device environment", lambda: ctx.dev_observe(d_o, d_r, d_d)),
        # the normalisers serve caller-stepped envs
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_enable(1)),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_get()),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_set(np.zeros(6), np.ones(6), 1.0)),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_apply(o)),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_enable(1)),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_get()),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_set(0.0, 1.0, 1.0)),
        # the real-valued calls name their integer twins
        (5, "ppo_env_step", lambda: ctx.env_step_f32(af)),
        (5, "ppo_rollout", lambda: P.binding._check(L.ppo_rollout_f32(ctx.h, d_a.ptr), ctx.h)),
        (5, "ppo_policy_act", lambda: ctx.policy_act_f32(o)),
        # the fold: an Acrobot observation does not hold the angles
        (5, "does not hold the angles", lambda: ctx.env_truncation_bootstrap(True)),
        (5, "does not hold the angles", lambda: ctx.env_truncations()),
        # bad arguments of a call this env does serve
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


def test_any_time_limit_is_accepted(P):
    """no upper bound on max_episode_steps: the angles are wrapped (gym's limit is 500)"""
    ctx = P.Context(acro_cfg(P, 8, max_episode_steps=500))
    ctx.init_orthogonal(1)
    ctx.env_reset()
    ctx.rollout()
    assert (ctx.read("FIN_LEN") == 0).all() and (ctx.env_get_state()[1] == T).all()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 10. the fused categorical path learns
# ---------------------------------------------------------------------------------------------------------
def test_acrobot_learns(P):
    """tools/acrobot_curve.py's run, one seed: 1024 envs x 64 steps, its default hyper-parameters, 50 iterations (0.15 s of training on an MI355X).  The tool
    measured, over seeds 1 .. 5, mean greedy returns over 256 fixed start states of -200.00 untrained (no episode swings up) and -81.79, -82.89, -83.31,
    -82.88, -82.96 trained: improvements of 118.21, 117.11, 116.69, 117.12 and 117.04 (profiles/NOTES.md).  The bar is half of the smallest: 58.34."""
    spec = importlib.util.spec_from_file_location("acrobot_curve", os.path.join(ROOT, "tools", "acrobot_curve.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse([])
    assert (args.iters, args.gamma, args.lr, args.epochs, args.minibatches, args.ent_coef) == (50, 0.99, 1e-3, 4, 4, 0.01)
    ctx = tool.make_ctx(P, 1, args)
    ctx.init_orthogonal(1)
    ctx.env_reset()
    untrained = tool.greedy_return(ctx)
    for _ in range(args.iters):
        ctx.train_iteration()
    trained = tool.greedy_return(ctx)
    print("greedy return: untrained %.2f, trained %.2f, improvement %.2f (bar 58.34)" % (untrained, trained, trained - untrained))
    ctx.close()
    assert untrained <= -199.0          # the untrained policy sits at or near -max_episode_steps
    assert trained - untrained >= 58.34
