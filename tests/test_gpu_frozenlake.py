"""PPO_ENV_FROZENLAKE / PPO_ENV_FROZENLAKE8X8 (include/ppo_hip.h; ppo-libtorch_amd/csrc/kernels_gauss_fused.hip: cat_rollout_kernel, cat_eval_kernel, the
cat_env_* kernels on CatEnvFrozenLake<4>, <8>) on the GPU through the C-ABI: the first device envs whose transitions draw random numbers, from a key the state
carries.  The env against the model (tests/frozenlake_model.py, itself checked by tests/test_frozenlake_cpu.py) on every (cell, action) pair, resets, the fused
rollout against the stepwise API and against the model, teacher forcing, the update against a host-fed context, launch accounting, the evaluation launch
against a host loop, every refusal, and learning.  Integer dynamics: every comparison is bit for bit.  Without the envs none of these contexts can be created
("unknown env_kind 10").

Common setup: N = 70 (one full tile and a short one), T = 9, max_episode_steps = 5 -- time-limit ends fall inside a rollout, and a second rollout starts at
step index 9, so the action draw's word select (& 3) and counter (>> 2) are both crossed; the env's own draw crosses its counter wherever an injected episode
starts at j = 2 or 3 -- orthogonal init with the actor's output layer scaled by 300 (the four actions get visibly different probabilities)."""
import importlib.util
import os

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package

import frozenlake_model as M

pytestmark = pytest.mark.gpu

N, T, MAXS = 70, 9, 5
ROLLOUT_BUFS = ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW", "NEXT_OBS", "NEXT_DONE", "VALUES", "NEXT_VALUE", "MASKS")
ALL_BUFS = ROLLOUT_BUFS + ("ADVANTAGES", "RETURNS", "PARAMS", "GRADS", "EXP_AVG", "EXP_AVG_SQ", "ENV_STATE", "EP_LEN", "EP_REW", "RESET_COUNT")
SIDES = pytest.mark.parametrize("side", [4, 8], ids=["4x4", "8x8"])
KEYS = ((0, 0), (11259375, 16777215))   # the two keys of the exhaustive rows (host_frozenlake_test.cpp uses the same)


@pytest.fixture(scope="module")
def P():
    return load_package()


@pytest.fixture(scope="module")
def O():
    import oracle   # Philox: the env's draws and the resets
    oracle.build()
    return oracle


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def kind_of(P, side):
    return P.ENV_FROZENLAKE8X8 if side == 8 else P.ENV_FROZENLAKE


def lake_cfg(P, side, n=N, **kw):
    d = dict(env_kind=kind_of(P, side), dist_kind=P.DIST_CATEGORICAL, obs_size=side * side, head_dims=(4,), num_envs=n, num_steps=T, num_minibatches=2,
             update_epochs=2, max_episode_steps=MAXS, seed=5, total_timesteps=4 * n * T, learning_rate=1e-3, anneal_lr=True, gamma=0.99, gae_lambda=0.95,
             ent_coef=0.01, kernel_flags=P.KERNEL_CAT_FUSED)
    d.update(kw)
    return P.make_config(**d)


def common_params(ctx):
    """the flat vector ends with the actor's output layer W3 [4, 64], b3 [4]"""
    ctx.init_orthogonal(11)
    p = ctx.get_params()
    p[-260:-4] *= 300.0
    return p


def lake_ctx(P, side, n=N, params=None, **kw):
    ctx = P.Context(lake_cfg(P, side, n, **kw))
    ctx.set_params(common_params(ctx) if params is None else params)
    return ctx


def rollout_buffers(ctx):
    return {k: ctx.read(k) for k in ROLLOUT_BUFS}


def istate(ctx):
    """the context's env states as the model's integers"""
    st = ctx.env_get_state()[0]
    assert st.shape == (ctx.N, 4) and (st == np.floor(st)).all()
    return st.astype(np.int64)


def inject(ctx, side):
    """env_reset, then through ppo_env_set_state_h: random non-terminal cells -- every other env next to a hole or the goal, so that terminations fall inside
    a rollout on the 8x8 map too -- step counts 0..3 and random keys (more than the start cell is visited, and the env's Philox counter j >> 2 is crossed
    inside an episode); every 7th env with ep_len = MAXS - 1.  Returns the observation."""
    ctx.env_reset()
    state, ep_len, ep_rew, resets = ctx.env_get_state()
    rng = np.random.default_rng(21 + side)
    live = np.flatnonzero(~M.terminal(side, np.arange(side * side)))
    n = np.arange(ctx.N)
    near = np.array([c for c in live if M.terminal(side, M.move(side, np.full(4, c), np.arange(4))).any()])
    state[:, 0] = live[rng.integers(0, live.size, ctx.N)]
    state[::2, 0] = near[rng.integers(0, near.size, (ctx.N + 1) // 2)]
    state[:, 1] = n % 4
    state[:, 2:] = rng.integers(0, M.WORD_MAX + 1, (ctx.N, 2))
    ep_len[:] = n % 4                       # the episode sums of an env that took j steps
    ep_len[n % 7 == 0] = MAXS - 1
    state[n % 7 == 0, 1] = MAXS - 1
    ctx.env_set_state(state, ep_len, ep_rew, resets)
    return ctx.read("NEXT_OBS", (ctx.N, side * side))


# ---------------------------------------------------------------------------------------------------------
# 1. transitions, exhaustive
# ---------------------------------------------------------------------------------------------------------
@SIDES
def test_transitions_against_the_model(P, O, side):
    S, kind = side * side, kind_of(P, side)
    ctx = lake_ctx(P, side, 8)
    # every (cell, action) pair, non-terminal and terminal, x j in 0..11 (every word of three Philox calls) x two keys
    rows = np.array([(c, j, k0, k1) for (k0, k1) in KEYS for j in range(12) for c in range(S) for _a in range(4)], np.int64)
    act = np.tile(np.arange(4), len(rows) // 4)
    ns, r, term = P.env_transition(ctx, kind, rows.astype(np.float32), act)
    m_ns, m_r, m_t = M.step(O, side, rows, act)
    assert ns.shape == (2 * 12 * S * 4, 4) and ns.dtype == np.float32
    assert same(ns, m_ns.astype(np.float32)) and same(r, m_r.astype(np.float32)) and np.array_equal(term, m_t.astype(np.int32))
    dead = M.terminal(side, rows[:, 0])
    assert (term[dead] == 1).all() and (r[dead] == 0).all() and (r == 1).any() and (term[~dead] == 0).any()
    # all three slips occur: from (row 2, col 1) under "down" the agent goes left, down and right
    c0 = 2 * side + 1
    ends = set(ns[(rows[:, 0] == c0) & (act == 1), 0].astype(int).tolist())
    assert ends == {c0 - 1, c0 + side, c0 + 1}, ends
    # j = 2^24 - 1: the count is held, the draw is that of counter (2^24 - 1) >> 2, word 3
    top = np.array([(c, M.WORD_MAX, k0, k1) for (k0, k1) in KEYS for c in range(S) for _a in range(4)], np.int64)
    act_t = np.tile(np.arange(4), len(top) // 4)
    ns, r, term = P.env_transition(ctx, kind, top.astype(np.float32), act_t)
    m_ns, m_r, m_t = M.step(O, side, top, act_t)
    assert same(ns, m_ns.astype(np.float32)) and same(r, m_r.astype(np.float32)) and np.array_equal(term, m_t.astype(np.int32))
    assert (ns[:, 1] == M.WORD_MAX).all()
    # actions -1, 7 and 2^40 are clamped (an i64 is saturated, not truncated: 2^40 is "up", not its low word 0, "left")
    base = np.array([(c, j, 123456, 654321) for c in range(S) for j in range(4)], np.int64)
    for bad, a in ((-1, 0), (7, 3), (1 << 40, 3)):
        ns, r, term = P.env_transition(ctx, kind, base.astype(np.float32), np.full(len(base), bad, np.int64))
        m_ns, m_r, m_t = M.step(O, side, base, np.full(len(base), a))
        assert same(ns, m_ns.astype(np.float32)) and same(r, m_r.astype(np.float32)) and np.array_equal(term, m_t.astype(np.int32)), bad
    # foreign states (NaN, -3, S + 5, 2^25 in each component): finite and inside the ranges -- and what the model makes of the clamped state
    odd = np.array([np.roll([np.nan, -3.0, S + 5.0, 2.0 ** 25], k) for k in range(4)] + [[2.9, 1.5, 3.99, 0.0]], np.float32)
    odd = np.repeat(odd, 4, axis=0)
    act_o = np.tile(np.arange(4), 5)
    ns, r, term = P.env_transition(ctx, kind, odd, act_o)
    assert np.isfinite(ns).all() and (ns == np.floor(ns)).all() and (ns >= 0).all() and (ns[:, 0] <= S - 1).all() and (ns[:, 1:] <= M.WORD_MAX).all()
    assert np.isin(r, (0.0, 1.0)).all() and np.isin(term, (0, 1)).all()
    m_ns, m_r, m_t = M.step(O, side, M.clamp(odd, side), act_o)
    assert same(ns, m_ns.astype(np.float32)) and same(r, m_r.astype(np.float32)) and np.array_equal(term, m_t.astype(np.int32))
    # ppo_env_set_state_h leaves the one-hot observations in NEXT_OBS
    cells = (np.arange(8) * 7) % S
    st = np.stack([cells, np.arange(8), np.full(8, 9), np.full(8, 10)], 1)
    ctx.env_reset()
    ctx.env_set_state(st.astype(np.float32))
    assert same(ctx.read("NEXT_OBS", (8, S)), M.obs(side, st))
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 2. resets
# ---------------------------------------------------------------------------------------------------------
@SIDES
def test_resets(P, O, side):
    S, K = side * side, 64
    big, again, part = lake_ctx(P, side, max_episode_steps=3), lake_ctx(P, side), lake_ctx(P, side, N - K, env_offset=K, global_num_envs=N)
    obs = big.env_reset()
    st, ep_len, ep_rew, resets = big.env_get_state()
    want = M.reset_states(O, 5, np.arange(N), [1] + [0] * (N - 1))   # global env 0 takes reset 1
    assert same(st, want.astype(np.float32)) and same(obs, M.obs(side, want)) and same(big.read("NEXT_OBS", (N, S)), obs)
    assert (obs[:, 0] == 1).all() and (obs.sum(axis=1) == 1).all()   # one-hot at the start cell
    assert len(set(map(tuple, want[:, 2:].tolist()))) == N            # every env drew its own key
    assert np.array_equal(resets, [2] + [1] * (N - 1)) and (ep_len == 0).all() and (ep_rew == 0).all() and (big.read("NEXT_DONE") == 0).all()
    assert same(again.env_reset(), obs) and same(again.env_get_state()[0], st)   # the same seed gives the same bits
    part.env_reset()
    assert same(part.env_get_state()[0], np.ascontiguousarray(st[K:])) and (part.env_get_state()[3] == 1).all()
    other = lake_ctx(P, side, seed=6)
    other.env_reset()
    assert not same(other.env_get_state()[0], st)
    # the resets a rollout makes (max_episode_steps = 3, T = 9: at least three episodes per env): every env's state behind a done step is reset
    # RESET_COUNT - 1 of the env, and RESET_COUNT counts the finished episodes
    big.rollout()
    st2, _, _, resets2 = big.env_get_state()
    fin = big.read("FIN_LEN").reshape(T, N)
    assert np.array_equal(resets2, resets + (fin > 0).sum(axis=0)) and ((fin > 0).sum(axis=0) >= 3).all()
    fresh = np.flatnonzero(big.read("NEXT_DONE") != 0)
    assert fresh.size >= N // 4
    assert same(np.ascontiguousarray(st2[fresh]), M.reset_states(O, 5, fresh, resets2[fresh] - 1).astype(np.float32))
    for c in (big, again, part, other):
        c.close()


# ---------------------------------------------------------------------------------------------------------
# 3. one launch against the loop, and against the model
# ---------------------------------------------------------------------------------------------------------
def stepwise_rollout(O, side, b, obs, done, step0, forced=None):
    """T x { policy_act(obs, step_index), env_step } on context b: the buffers a rollout would fill.  FIN_LEN / FIN_REW from the episode sums the context held
    in front of the step.  The env is held to the model at every step."""
    n, S = b.N, side * side
    out = {k: [] for k in ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW", "MASKS")}
    for t in range(T):
        state = istate(b)
        assert same(obs, M.obs(side, state))
        act, lp, _, _ = b.policy_act(obs, step_index=step0 + t, action=None if forced is None else forced[t])
        len0, rew0 = b.read("EP_LEN"), b.read("EP_REW")
        out["OBS"].append(obs)
        out["DONES"].append(done.astype(np.float32))
        out["MASKS"].append(np.ones((n, 4), np.uint8))
        m_ns, m_r, m_t = M.step(O, side, state, act.reshape(-1))
        obs, r, done = b.env_step(act)
        assert same(r, m_r.astype(np.float32)) and np.array_equal(done, ((m_t == 1) | (len0 + 1 == b.cfg.max_episode_steps)).astype(np.int32))
        assert np.array_equal(istate(b)[done == 0], m_ns[done == 0])
        out["ACTIONS"].append(act.astype(np.int32))
        out["LOGPROBS"].append(lp)
        out["REWARDS"].append(r)
        out["FIN_LEN"].append(np.where(done != 0, len0 + 1, 0).astype(np.int32))
        out["FIN_REW"].append(np.where(done != 0, rew0 + r, np.float32(0)).astype(np.float32))
        assert obs.shape == (n, S)
    res = {k: np.stack(v).reshape(-1) for k, v in out.items()}
    res["NEXT_OBS"], res["NEXT_DONE"] = obs.reshape(-1), done
    return res, obs, done


def model_rollout(O, side, state, ep_len, ep_rew, resets, actions, seed, n, max_steps):
    """The model alone under the stored actions: OBS, REWARDS, DONES (the flag in front of each step), FIN_LEN, FIN_REW of T steps, and the carried state."""
    state, ep_len, ep_rew, resets = state.copy(), ep_len.astype(np.int64), ep_rew.astype(np.float32), resets.astype(np.int64)
    out = {k: [] for k in ("OBS", "REWARDS", "FIN_LEN", "FIN_REW", "DONE_AFTER")}
    for t in range(actions.shape[0]):
        out["OBS"].append(M.obs(side, state))
        ns, r, term = M.step(O, side, state, actions[t])
        ep_len += 1
        ep_rew = (ep_rew + r.astype(np.float32)).astype(np.float32)
        done = (term == 1) | (ep_len == max_steps)
        out["REWARDS"].append(r.astype(np.float32))
        out["FIN_LEN"].append(np.where(done, ep_len, 0).astype(np.int32))
        out["FIN_REW"].append(np.where(done, ep_rew, np.float32(0)).astype(np.float32))
        out["DONE_AFTER"].append(done.astype(np.float32))
        idx = np.flatnonzero(done)
        ns[idx] = M.reset_states(O, seed, idx, resets[idx])
        resets[idx] += 1
        ep_len[idx] = 0
        ep_rew[idx] = 0
        state = ns
    return {k: np.stack(v) for k, v in out.items()}, (state, ep_len, ep_rew, resets)


@pytest.mark.parametrize("side,n", [(4, 70), (8, 70), (8, 130)], ids=["4x4-70", "8x8-70", "8x8-130"])
@pytest.mark.parametrize("force", [False, True], ids=["drawn", "forced"])
def test_fused_rollout_equals_stepwise_api_and_the_model(P, O, side, n, force):
    """N = 70: a full tile and a short one; N = 130 on the 8x8 map: three workgroups, the last with two envs.  Two rollouts in a row: the second runs step
    indices 9 .. 17 and carries the done flags and the episode sums of the first.  max_episode_steps = 5 puts time-limit ends inside; the injected states
    start from random non-terminal cells with random keys."""
    S = side * side
    a, b = lake_ctx(P, side, n), lake_ctx(P, side, n)
    assert same(a.get_params(), b.get_params())
    obs = inject(b, side)
    assert same(inject(a, side), obs)
    done = np.zeros(n, np.int32)
    carried = [x.copy() for x in a.env_get_state()]
    carried[0] = carried[0].astype(np.int64)
    seen_cells, seen_actions, early = set(), set(), 0
    rng = np.random.default_rng(4)
    for k in range(2):
        forced = rng.integers(0, 4, (T, n, 1)).astype(np.int64) if force else None
        prev_done = a.read("NEXT_DONE").astype(np.float32) if k else np.zeros(n, np.float32)
        a.rollout(forced_actions=forced)
        got = rollout_buffers(a)
        want, obs, done = stepwise_rollout(O, side, b, obs, done, k * T, forced)
        for name, w in want.items():
            assert same(got[name], w), (k, name, int((bits(got[name]) != bits(w)).sum()))
        for x, y in zip(a.env_get_state(), b.env_get_state()):   # ENV_STATE, EP_LEN, EP_REW, RESET_COUNT
            assert same(x, y)
        Ob = got["OBS"].reshape(T * n, S)
        assert same(got["VALUES"], a.get_value(Ob))
        assert same(got["NEXT_VALUE"], a.get_value(got["NEXT_OBS"].reshape(n, S)))
        assert (got["MASKS"] == 1).all() and got["MASKS"].size == T * n * 4
        if force:
            assert np.array_equal(got["ACTIONS"], forced.reshape(-1))
        # the model alone under the stored actions
        mod, carried = model_rollout(O, side, *carried, got["ACTIONS"].reshape(T, n), 5, n, MAXS)
        assert same(Ob, mod["OBS"].reshape(T * n, S)) and same(got["REWARDS"], mod["REWARDS"].reshape(-1))
        assert same(got["FIN_LEN"], mod["FIN_LEN"].reshape(-1)) and same(got["FIN_REW"], mod["FIN_REW"].reshape(-1))
        assert same(got["DONES"].reshape(T, n), np.concatenate([prev_done[None], mod["DONE_AFTER"][:-1]]))
        assert same(got["NEXT_DONE"].astype(np.float32), mod["DONE_AFTER"][-1])
        st_a, len_a, rew_a, res_a = a.env_get_state()
        assert same(st_a, carried[0].astype(np.float32)) and np.array_equal(len_a, carried[1]) and same(rew_a, carried[2]) and np.array_equal(res_a, carried[3])
        seen_cells |= set(Ob.argmax(axis=1).tolist())
        seen_actions |= set(np.unique(got["ACTIONS"]).tolist())
        assert (got["FIN_LEN"] == MAXS).any()                     # time-limit ends inside the rollout
        early += int(((got["FIN_LEN"] > 0) & (got["FIN_LEN"] < MAXS)).sum())
    # terminations too, counted over both rollouts: behind the first five steps every 8x8 episode starts in cell 0, five moves from the nearest hole, so the
    # second rollout alone need not hold one
    print("cells visited: %d of %d; actions: %s; episodes ended by the env: %d" % (len(seen_cells), S, sorted(seen_actions), early))
    assert early > 0 and len(seen_cells) > S // 4 and len(seen_actions) >= 2
    a.close()
    b.close()


@SIDES
def test_forcing_a_free_rollouts_actions_reproduces_it(P, side):
    free, rep = lake_ctx(P, side), lake_ctx(P, side)
    inject(free, side)
    inject(rep, side)
    free.rollout()
    g = rollout_buffers(free)
    rep.rollout(forced_actions=g["ACTIONS"].reshape(T, N, 1))
    r = rollout_buffers(rep)
    for name in ROLLOUT_BUFS:
        assert same(g[name], r[name]), name
    for x, y in zip(free.env_get_state(), rep.env_get_state()):
        assert same(x, y)
    free.close()
    rep.close()


# ---------------------------------------------------------------------------------------------------------
# 4. an iteration equals the host-fed iteration, bit for bit
# ---------------------------------------------------------------------------------------------------------
@SIDES
def test_iteration_equals_the_host_fed_iteration(P, side):
    """Two train_iterations against a PPO_ENV_HOST context (PPO_KERNEL_CAT_FUSED, PPO_DIST_CATEGORICAL, the same observation width, heads (4,), same
    parameters and seed) fed by host_act, a third context's env_step and host_observe: the same observations, actions, rewards and dones go into the same
    ppo_update, which ends with the same parameters and AdamW moments."""
    dev = lake_ctx(P, side)
    host = P.Context(lake_cfg(P, side, env_kind=P.ENV_HOST))
    env = lake_ctx(P, side)
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
    for name in ("OBS", "ACTIONS", "LOGPROBS", "REWARDS", "DONES", "VALUES", "ADVANTAGES", "RETURNS"):
        assert same(dev.read(name), host.read(name)), name
    assert same(dev.get_params(), host.get_params()) and not same(dev.get_params(), params)
    (m0, v0, k0), (m1, v1, k1) = dev.get_optimizer(), host.get_optimizer()
    assert same(m0, m1) and same(v0, v1) and k0 == k1 == 2 * 2 * 2
    assert sd["loss"] == sh["loss"] and sd["global_step"] == sh["global_step"] == 2 * N * T
    for c in (dev, host, env):
        c.close()


# ---------------------------------------------------------------------------------------------------------
# 5. launch accounting
# ---------------------------------------------------------------------------------------------------------
@SIDES
def test_launch_accounting(P, side):
    ctx = lake_ctx(P, side)
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
    ctx.evaluate(16, 3, greedy=False)
    assert ctx.gauss_fused_launches() == (a3, v3, u3)  # ppo_evaluate moves nothing
    ctx.sync()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 6. evaluation
# ---------------------------------------------------------------------------------------------------------
EVAL_SEED = 9


def host_episodes(P, O, side, ctx, states, greedy, max_steps):
    """Whole episodes on the host: the model's observation of the states, policy_act_greedy / policy_act(step_index = the episode's step) and
    ppo_env_transition on all rows, a finished row ignored; the device's transition is held to the model on the live rows."""
    n, kind = states.shape[0], kind_of(P, side)
    st = states.copy()
    ret, length, alive = np.zeros(n, np.float32), np.zeros(n, np.int32), np.ones(n, bool)
    for t in range(max_steps):
        obs = M.obs(side, st)
        act = ctx.policy_act_greedy(obs)[0] if greedy else ctx.policy_act(obs, step_index=t)[0]
        ns, r, term = P.env_transition(ctx, kind, st.astype(np.float32), act)
        if t < 8:
            m_ns, m_r, m_t = M.step(O, side, st[alive], act.reshape(-1)[alive])
            assert same(np.ascontiguousarray(ns[alive]), m_ns.astype(np.float32)) and same(np.ascontiguousarray(r[alive]), m_r.astype(np.float32))
        ret[alive] = (ret[alive] + r[alive]).astype(np.float32)
        length[alive] += 1
        st[alive] = ns[alive].astype(np.int64)
        alive &= (term == 0) & (length < max_steps)
        if not alive.any():
            break
    return ret, length, (length == max_steps).astype(np.int32)


@SIDES
@pytest.mark.parametrize("max_steps", [5, 100])
def test_evaluate(P, O, side, max_steps):
    """70 episodes, greedy and sampled, against the host loop in every return, length and truncated flag; n = 16 is the prefix of n = 70; another seed gives
    other episodes; the training state is untouched.  Plain orthogonal init (a near-uniform policy): episodes end in holes, at the goal and at the limit."""
    kw = dict(max_episode_steps=max_steps, seed=EVAL_SEED)
    ctx, plain, ref = P.Context(lake_cfg(P, side, 32, **kw)), P.Context(lake_cfg(P, side, 32, **kw)), P.Context(lake_cfg(P, side, N, **kw))
    ctx.init_orthogonal(3)
    params = ctx.get_params()
    for c in (ctx, ref, plain):
        c.set_params(params)
        c.env_reset()
    for c in (ctx, plain):
        c.rollout()
        c.sync()
    snap = lambda c: ({k: c.read(k) for k in ALL_BUFS}, c.get_optimizer()[2], c.gauss_fused_launches())   # noqa: E731
    before = snap(ctx)
    stats_g, ret_g, len_g = ctx.evaluate(N, EVAL_SEED, greedy=True)
    stats_s, ret_s, len_s = ctx.evaluate(N, EVAL_SEED, greedy=False)
    stats_16, ret_16, len_16 = ctx.evaluate(16, EVAL_SEED, greedy=True)
    s16_s, ret_16s, len_16s = ctx.evaluate(16, EVAL_SEED, greedy=False)
    stats_2, ret_2, len_2 = ctx.evaluate(N, EVAL_SEED + 1, greedy=False)
    stats_2g, ret_2g, len_2g = ctx.evaluate(N, EVAL_SEED + 1, greedy=True)
    after = snap(ctx)
    assert before[1:] == after[1:]
    for k in ALL_BUFS:
        assert same(before[0][k], after[0][k]), k
    states = M.reset_states(O, EVAL_SEED, np.arange(N), [0] * N)   # episode e starts at reset 0 of env e
    for greedy, (st, ret, length) in ((True, (stats_g, ret_g, len_g)), (False, (stats_s, ret_s, len_s))):
        h_ret, h_len, h_trunc = host_episodes(P, O, side, ref, states, greedy, max_steps)
        print("greedy" if greedy else "sampled", "lengths %d..%d, truncated %d of %d, reached the goal %d" % (length.min(), length.max(), st["truncated"], N, int(ret.sum())))
        assert np.array_equal(length, h_len), (greedy, np.flatnonzero(length != h_len))
        assert same(ret, h_ret), (greedy, np.flatnonzero(bits(ret) != bits(h_ret)))
        assert st["truncated"] == int(h_trunc.sum())
        assert st["episodes"] == N and st["env_steps"] == int(h_len.sum())
        assert abs(st["return_mean"] - h_ret.astype(np.float64).mean()) <= 1e-9
        assert np.isin(ret, (0.0, 1.0)).all()
    if max_steps == 100:   # (within 5 steps no 8x8 episode can end: all 70 are cut off with return 0, whatever the seed)
        # the greedy policy is the same in every episode, the slips are not: the episodes differ through their keys alone
        assert len(set(len_g.tolist())) > 1
        # another seed gives other episodes (other keys: other slips, greedy or not)
        assert not np.array_equal(len_2, len_s) and not np.array_equal(len_2g, len_g)
    # results do not depend on how episodes are spread over workgroups
    assert same(ret_16, ret_g[:16]) and np.array_equal(len_16, len_g[:16]) and stats_16["episodes"] == 16
    assert same(ret_16s, ret_s[:16]) and np.array_equal(len_16s, len_s[:16])
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
# 7. refusals
# ---------------------------------------------------------------------------------------------------------
@SIDES
@pytest.mark.parametrize("kw,status,word", [
    (dict(obs_size=4), 1, "observation of size"),
    (dict(obs_size=19), 1, "observation of size"),
    (dict(dist_kind=1), 5, "PPO_DIST_CATEGORICAL"),
    (dict(dist_kind=2, head_dims=(1,)), 5, "PPO_DIST_CATEGORICAL"),
    (dict(head_dims=(3,)), 5, "head_dims[0] = 4"),
    (dict(head_dims=(4, 4)), 5, "n_heads = 1"),
    (dict(hidden=32), 5, "hidden = 64"),
    (dict(n_hidden=3), 5, "n_hidden = 2"),
    (dict(compute_dtype=1), 5, "PPO_DTYPE_F32"),
    (dict(kernel_flags=0), 5, "PPO_KERNEL_CAT_FUSED"),
    (dict(kernel_flags=64), 5, "PPO_KERNEL_CAT_FUSED"),
    (dict(max_episode_steps=0), 5, "max_episode_steps"),
    (dict(max_episode_steps=-3), 5, "max_episode_steps"),
    (dict(max_episode_steps=1 << 24), 5, "max_episode_steps"),
    (dict(env_kind=7), 1, "unknown env_kind 7"),
    (dict(env_kind=9), 1, "unknown env_kind 9"),
    (dict(env_kind=12), 1, "unknown env_kind 12"),
])
def test_ctx_create_refusals(P, side, kw, status, word):
    with pytest.raises(P.binding.PPOError) as e:
        P.Context(lake_cfg(P, side, 8, **kw))
    assert "status %d:" % status in str(e.value) and word in str(e.value), str(e.value)
    if "obs_size" in kw:
        assert "observation of size %d" % (side * side) in str(e.value)


def test_the_other_maps_width_is_a_wrong_obs_size_and_the_limits_are_accepted(P):
    for side, other in ((4, 64), (8, 16)):
        with pytest.raises(P.binding.PPOError) as e:
            P.Context(lake_cfg(P, side, 8, obs_size=other))
        assert "status 1:" in str(e.value) and "observation of size %d" % (side * side) in str(e.value)
        for steps in (1, (1 << 24) - 1):
            P.Context(lake_cfg(P, side, 8, max_episode_steps=steps)).close()


@SIDES
def test_refused_calls_change_nothing(P, side):
    n, S = 40, side * side
    ctx = lake_ctx(P, side, n)
    ctx.env_reset()
    ctx.train_iteration()
    ctx.rollout()
    ctx.sync()
    snap = lambda: ({k: ctx.read(k) for k in ALL_BUFS}, ctx.get_optimizer()[2], ctx.gauss_fused_launches())   # noqa: E731
    before = snap()
    o, r, d, af = np.zeros((n, S), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 4), np.float32)
    d_o, d_r, d_d, d_a, d_a64 = ctx.dev(o), ctx.dev(r), ctx.dev(d), ctx.dev(af), ctx.dev(np.zeros((n, 1), np.int64))
    L = P.binding.lib()
    good = ctx.env_get_state()[0]

    def bad_state(i, j, v):
        s = good.copy()
        s[i, j] = v
        return s
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
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_set(np.zeros(S), np.ones(S), 1.0)),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_apply(o)),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_enable(1)),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_get()),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_set(0.0, 1.0, 1.0)),
        # the real-valued calls name their integer twins
        (5, "ppo_env_step", lambda: ctx.env_step_f32(af)),
        (5, "ppo_rollout", lambda: P.binding._check(L.ppo_rollout_f32(ctx.h, d_a.ptr), ctx.h)),
        (5, "ppo_policy_act", lambda: ctx.policy_act_f32(o)),
        # the time-limit fold: the stored observation holds neither the step count nor the key
        (5, "holds neither the step count nor the key", lambda: ctx.env_truncation_bootstrap(True)),
        (5, "holds neither the step count nor the key", lambda: ctx.env_truncation_bootstrap(False)),
        (5, "holds neither the step count nor the key", lambda: ctx.env_truncations()),
        # a state component outside its range, or not an integer: the host array is checked, nothing is copied
        (1, "state[3][0]", lambda: ctx.env_set_state(bad_state(3, 0, float(S)))),
        (1, "state[39][3]", lambda: ctx.env_set_state(bad_state(39, 3, 16777216.0))),
        (1, "state[0][2]", lambda: ctx.env_set_state(bad_state(0, 2, -1.0))),
        (1, "state[7][1]", lambda: ctx.env_set_state(bad_state(7, 1, 2.5))),
        (1, "state[7][1]", lambda: ctx.env_set_state(bad_state(7, 1, np.nan), np.zeros(n, np.int32))),
        # bad arguments of calls this env does serve
        (1, "n_episodes", lambda: ctx.evaluate(0, 1)),
    ]
    for status, word, call in calls:
        with pytest.raises(P.binding.PPOError) as e:
            call()
        assert "status %d:" % status in str(e.value) and word in str(e.value), str(e.value)
    import ctypes as C
    buf, term = (C.c_float * 8)(), (C.c_int32 * 2)()
    assert L.ppo_env_transition_f32(kind_of(P, side), buf, buf, 0, buf, None, buf, term, None) == 5
    ctx.sync()
    after = snap()
    assert before[1:] == after[1:]
    for k in ALL_BUFS:
        assert same(before[0][k], after[0][k]), k
    # the largest legal components are accepted, and the context still works
    top = good.copy()
    top[0] = (S - 1, M.WORD_MAX, M.WORD_MAX, M.WORD_MAX)
    ctx.env_set_state(top)
    assert same(ctx.env_get_state()[0], top) and ctx.read("NEXT_OBS", (n, S))[0, S - 1] == 1.0
    ctx.train_iteration()
    assert np.isfinite(ctx.stats()["loss"])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 8. learning (4x4)
# ---------------------------------------------------------------------------------------------------------
LEARN_ITERS = 40
RANDOM_SUCCESS = 0.0139398   # the model's uniformly random policy within 100 steps (tests/test_frozenlake_cpu.py)
LEARN_BAR = 0.3368           # half of the smallest improvement over the random policy that tools/frozenlake_curve.py showed across three seeds (below)


def test_frozenlake_learns(P):
    """tools/frozenlake_curve.py's settings, the 4x4 map, one seed: 512 envs x 64 steps, max_episode_steps 100, its default hyper-parameters, LEARN_ITERS
    iterations, then ppo_evaluate(512, sampled), whose return_mean is the success rate.  The tool measured on an MI355X, seeds 1 / 2 / 3: 0.0117 / 0.0098 /
    0.0117 untrained and 0.6895 / 0.6875 / 0.6934 after 40 iterations (0.09 s of training; the curves are in DESIGN.md): improvements over the random policy's
    0.0139 of 0.6756, 0.6736 and 0.6795.  The bar is half of the smallest, 0.3368 -- Acrobot's rule; the model's limit-100 optimum, the ceiling, is 0.7442."""
    spec = importlib.util.spec_from_file_location("frozenlake_curve", os.path.join(ROOT, "tools", "frozenlake_curve.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse([])
    assert (tool.N, tool.T, tool.MAXS[4], tool.EVAL_EPISODES, args.side) == (512, 64, 100, 512, 4)
    ctx = tool.make_ctx(P, 1, args)
    ctx.init_orthogonal(1)
    ctx.env_reset()
    untrained = tool.sampled_return(ctx)
    for _ in range(LEARN_ITERS):
        ctx.train_iteration()
    trained = tool.sampled_return(ctx)
    print("success rate over 512 episodes: untrained %.4f, trained %.4f, improvement over the random policy %.4f (bar %.4f; limit-100 optimum 0.7442)"
          % (untrained, trained, trained - RANDOM_SUCCESS, LEARN_BAR))
    ctx.close()
    assert args.iters == LEARN_ITERS
    assert untrained <= RANDOM_SUCCESS + 8 * np.sqrt(RANDOM_SUCCESS * (1 - RANDOM_SUCCESS) / 512)   # the untrained policy is a near-uniform one
    assert trained - RANDOM_SUCCESS >= LEARN_BAR
    assert trained <= 0.7442 + 8 * np.sqrt(0.7442 * (1 - 0.7442) / 512)                             # nothing beats the optimum but by sampling noise
