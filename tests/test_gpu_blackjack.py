"""PPO_ENV_BLACKJACK (include/ppo_hip.h; ppo-libtorch_amd/csrc/kernels_gauss_fused.hip: cat_rollout_kernel, cat_eval_kernel, the cat_env_* kernels on
CatEnvBlackjack) on the GPU through the C-ABI: the device env whose step draws a number of cards that depends on the data -- a hit one, a stick the dealer's
play-out of up to ten, a reset the deal -- from a key the state carries.  The env against the model (tests/blackjack_model.py, itself checked by
tests/test_blackjack_cpu.py) on every (t, ace, show, action) x card index x key, resets, the fused rollout against the stepwise API and against the model,
teacher forcing, the update against a host-fed context, launch accounting, the evaluation launch against a host loop, every refusal, and learning.  Integer
dynamics: every comparison is bit for bit.  Without the env none of these contexts can be created ("unknown env_kind 13").

Common setup: N = 70 (one full tile and a short one), T = 9, max_episode_steps 2 (time-limit ends fall inside a rollout: two hits that do not bust) or 100
(never met); a second rollout starts at step index 9, so the action draw's word select (& 3) and counter (>> 2) are both crossed; the env's own card index
crosses its counter inside an episode wherever a player hits or a dealer draws from n = 6, 7; orthogonal init with the actor's output layer scaled by 30
(both actions keep a probability that 630 draws show)."""
import importlib.util
import os

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package

import blackjack_model as M

pytestmark = pytest.mark.gpu

N, T, SEED = 70, 9, 5
OBS = 45
ROLLOUT_BUFS = ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW", "NEXT_OBS", "NEXT_DONE", "VALUES", "NEXT_VALUE", "MASKS")
ALL_BUFS = ROLLOUT_BUFS + ("ADVANTAGES", "RETURNS", "PARAMS", "GRADS", "EXP_AVG", "EXP_AVG_SQ", "ENV_STATE", "EP_LEN", "EP_REW", "RESET_COUNT")
LIMITS = pytest.mark.parametrize("max_steps", [2, 100], ids=["limit2", "limit100"])
# the two keys of the exhaustive rows, chosen on the CPU (host_blackjack_test.cpp uses the same): between them the dealer's play-outs take 0 and 7 cards
KEYS = ((11259375, 16777215), (20927, 3321251))


@pytest.fixture(scope="module")
def P():
    return load_package()


@pytest.fixture(scope="module")
def O():
    import oracle   # Philox: the env's cards and the resets
    oracle.build()
    return oracle


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def jack_cfg(P, n=N, **kw):
    d = dict(env_kind=P.ENV_BLACKJACK, dist_kind=P.DIST_CATEGORICAL, obs_size=OBS, head_dims=(2,), num_envs=n, num_steps=T, num_minibatches=2,
             update_epochs=2, max_episode_steps=100, seed=SEED, total_timesteps=4 * n * T, learning_rate=1e-3, anneal_lr=True, gamma=0.99, gae_lambda=0.95,
             ent_coef=0.01, kernel_flags=P.KERNEL_CAT_FUSED)
    d.update(kw)
    return P.make_config(**d)


def common_params(ctx):
    """the flat vector ends with the actor's output layer W3 [2, 64], b3 [2]"""
    ctx.init_orthogonal(11)
    p = ctx.get_params()
    p[-130:-2] *= 30.0
    return p


def jack_ctx(P, n=N, params=None, **kw):
    ctx = P.Context(jack_cfg(P, n, **kw))
    ctx.set_params(common_params(ctx) if params is None else params)
    return ctx


def rollout_buffers(ctx):
    return {k: ctx.read(k) for k in ROLLOUT_BUFS}


def istate(ctx):
    """the context's env states as the model's integers"""
    st = ctx.env_get_state()[0]
    assert st.shape == (ctx.N, 4) and (st == np.floor(st)).all()
    return st.astype(np.int64)


def check3(got, want, what=None):
    (ns, r, term), (m_ns, m_r, m_t) = got, want
    assert same(ns, m_ns.astype(np.float32)), what
    assert same(r, m_r.astype(np.float32)), what
    assert np.array_equal(term, m_t.astype(np.int32)), what


class ModelEnvs:
    """n envs of the model with ppo_env_step's bookkeeping: episode sums, the time limit, the auto-reset by reset number RESET_COUNT of the env"""

    def __init__(self, O, seed, n, max_steps, offset=0):
        self.O, self.seed, self.n, self.max_steps, self.offset = O, seed, n, max_steps, offset

    def reset(self):
        first = [1 if self.offset + e == 0 else 0 for e in range(self.n)]   # global env 0 takes reset 1
        self.state = M.reset_states(self.O, self.seed, self.offset + np.arange(self.n), first)
        self.ep_len, self.ep_rew = np.zeros(self.n, np.int64), np.zeros(self.n, np.float32)
        self.resets = np.array(first, np.int64) + 1
        return M.obs(self.state)

    def load(self, state, ep_len, ep_rew, resets):
        self.state, self.ep_len, self.ep_rew, self.resets = state.astype(np.int64), ep_len.astype(np.int64), ep_rew.astype(np.float32), resets.astype(np.int64)

    def step(self, actions):
        """-> (obs, reward f32, done i32, fin_len i32, fin_rew f32)"""
        ns, r, term = M.step(self.O, self.state, actions)
        self.ep_len += 1
        self.ep_rew = (self.ep_rew + r.astype(np.float32)).astype(np.float32)
        done = (term == 1) | (self.ep_len == self.max_steps)
        fin_len = np.where(done, self.ep_len, 0).astype(np.int32)
        fin_rew = np.where(done, self.ep_rew, np.float32(0)).astype(np.float32)
        idx = np.flatnonzero(done)
        if idx.size:
            ns[idx] = M.reset_states(self.O, self.seed, self.offset + idx, self.resets[idx])
        self.resets[idx] += 1
        self.ep_len[idx] = 0
        self.ep_rew[idx] = 0
        self.state = ns
        return M.obs(ns), r.astype(np.float32), done.astype(np.int32), fin_len, fin_rew


def inject(ctx, max_steps):
    """env_reset, then through ppo_env_set_state_h: random live hands (t 2..21, either ace flag, any showing card), episodes that took j hits so far (n = 4 +
    j, ep_len = j; j below the limit) and random keys -- more than dealt hands are visited, and card indices cross a Philox call inside an episode.  Returns
    the observation."""
    ctx.env_reset()
    state, ep_len, ep_rew, resets = ctx.env_get_state()
    rng = np.random.default_rng(21)
    n = np.arange(ctx.N)
    j = n % min(4, max_steps)
    state[:, 0] = M.pack(rng.integers(2, 22, ctx.N), rng.integers(0, 2, ctx.N), rng.integers(1, 11, ctx.N))
    state[:, 1] = 4 + j
    state[:, 2:] = rng.integers(0, M.WORD_MAX + 1, (ctx.N, 2))
    ep_len[:] = j
    ctx.env_set_state(state, ep_len, ep_rew, resets)
    return ctx.read("NEXT_OBS", (ctx.N, OBS))


# ---------------------------------------------------------------------------------------------------------
# 1. transitions, exhaustive
# ---------------------------------------------------------------------------------------------------------
def test_transitions_against_the_model(P, O):
    ctx = jack_ctx(P, 8)
    kind = P.ENV_BLACKJACK
    # every (t 2..31, ace, show 1..10) x both actions x n in 4..11 (every word of two Philox calls, the dealer's draws reaching into a third and fourth) x two keys
    rows = np.array([(int(M.pack(t, ace, show)), n, k0, k1) for (k0, k1) in KEYS for n in range(4, 12) for t in range(2, 32) for ace in (0, 1)
                     for show in range(1, 11) for _a in range(2)], np.int64)
    act = np.tile(np.arange(2), len(rows) // 2)
    assert len(rows) == 19200
    ns, r, term = P.env_transition(ctx, kind, rows.astype(np.float32), act)
    m_ns, m_r, m_t, drew = M.step(O, rows, act, with_draws=True)
    assert ns.shape == (19200, 4) and ns.dtype == np.float32
    check3((ns, r, term), (m_ns, m_r, m_t))
    t0 = M.unpack(rows[:, 0])[0]
    sticks = (act == 0) & (t0 <= 21)
    print("dealer play-outs among %d sticks: %s cards (count per length)" % (sticks.sum(), np.bincount(drew[sticks]).tolist()))
    assert (drew[sticks] == 0).any() and drew[sticks].max() >= 5                      # play-outs of no card and of at least five
    assert set(np.unique(r).tolist()) == {-1.0, 0.0, 1.0} and (term[act == 1] == 0).any() and (term[act == 0] == 1).all()
    assert (term[t0 > 21] == 1).all() and (r[t0 > 21] == -1).all() and same(np.ascontiguousarray(ns[t0 > 21]), rows[t0 > 21].astype(np.float32))
    # n = 2^24 - 1 and 2^24 - 2 under stick: the count is held, the cards are those of indices n, n + 1, ..
    top = np.array([(int(M.pack(t, ace, show)), n, k0, k1) for (k0, k1) in KEYS for n in (M.WORD_MAX, M.WORD_MAX - 1) for t in (4, 12, 16, 20) for ace in (0, 1)
                    for show in range(1, 11)], np.int64)
    for a in (0, 1):
        act_t = np.full(len(top), a)
        ns, r, term = P.env_transition(ctx, kind, top.astype(np.float32), act_t)
        m = M.step(O, top, act_t, with_draws=True)
        check3((ns, r, term), m[:3], a)
        assert (ns[:, 1] <= M.WORD_MAX).all() and (ns[:, 1] == M.WORD_MAX).any()
        if a == 0:
            assert (m[3] >= 2).any()                                                   # a play-out that would pass 2^24 - 1 from either n
    # actions -1, 7 and 2^40 are clamped (an i64 is saturated, not truncated: 2^40 is "hit", not its low word 0, "stick")
    base = np.array([(int(M.pack(t, ace, show)), n, 123456, 654321) for t in (5, 12, 15, 19, 21) for ace in (0, 1) for show in (1, 4, 10) for n in (4, 6, 7)], np.int64)
    for bad, a in ((-1, 0), (7, 1), (1 << 40, 1)):
        got = P.env_transition(ctx, kind, base.astype(np.float32), np.full(len(base), bad, np.int64))
        check3(got, M.step(O, base, np.full(len(base), a)), bad)
    # foreign states (NaN, -3, 708, 2^25 in each component; fractions; a hand word with t = 1 and show = 0): finite and inside the ranges -- and what the
    # model makes of the clamped state
    odd = np.array([np.roll([np.nan, -3.0, 708.0, 2.0 ** 25], k) for k in range(4)] + [[2.9, 1.5, 3.99, 0.0], [65.9, 7.2, 1.0, 2.0], [33.0, 4.0, 9.0, 9.0]], np.float32)
    odd = np.repeat(odd, 2, axis=0)
    act_o = np.tile(np.arange(2), len(odd) // 2)
    ns, r, term = P.env_transition(ctx, kind, odd, act_o)
    assert np.isfinite(ns).all() and (ns == np.floor(ns)).all() and (ns >= 0).all() and (ns[:, 0] <= M.HAND_MAX).all() and (ns[:, 1:] <= M.WORD_MAX).all()
    nt, _, nshow = M.unpack(ns[:, 0].astype(np.int64))
    assert (nt >= 2).all() and (nshow >= 1).all() and (nshow <= 10).all() and np.isin(r, (-1.0, 0.0, 1.0)).all() and np.isin(term, (0, 1)).all()
    check3((ns, r, term), M.step(O, M.clamp(odd), act_o))
    # ppo_env_set_state_h leaves the three one-hot groups in NEXT_OBS
    st = np.stack([M.pack([2, 11, 11, 12, 21, 31, 20, 10], [0, 1, 0, 1, 1, 1, 0, 1], [1, 2, 3, 4, 5, 6, 9, 10]), np.arange(8) + 4, np.full(8, 9), np.full(8, 10)], 1)
    ctx.env_reset()
    ctx.env_set_state(st.astype(np.float32))
    ob = ctx.read("NEXT_OBS", (8, OBS))
    assert same(ob, M.obs(st)) and (ob.sum(axis=1) == 3).all() and ob[1, 21] == 1 and ob[1, 44] == 1 and ob[3, 12] == 1 and ob[3, 43] == 1
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 2. resets
# ---------------------------------------------------------------------------------------------------------
def test_resets(P, O):
    K = 64
    big, again, part = jack_ctx(P, max_episode_steps=3), jack_ctx(P), jack_ctx(P, N - K, env_offset=K, global_num_envs=N)
    obs = big.env_reset()
    st, ep_len, ep_rew, resets = big.env_get_state()
    want = M.reset_states(O, SEED, np.arange(N), [1] + [0] * (N - 1))   # global env 0 takes reset 1
    assert same(st, want.astype(np.float32)) and same(obs, M.obs(want)) and same(big.read("NEXT_OBS", (N, OBS)), obs)
    t, ace, show = M.unpack(want[:, 0])
    assert (want[:, 1] == 4).all() and (t >= 2).all() and (t <= 20).all() and (show >= 1).all() and (show <= 10).all() and (obs.sum(axis=1) == 3).all()
    assert (t[ace == 1] <= 11).all() and np.array_equal(obs[:, 44] == 1, ace == 1)   # two cards with an ace: t <= 11, and the ace is usable
    assert len(set(map(tuple, want[:, 2:].tolist()))) == N and len(set(want[:, 0].tolist())) > 10   # every env drew its own key; the deals differ
    assert np.array_equal(resets, [2] + [1] * (N - 1)) and (ep_len == 0).all() and (ep_rew == 0).all() and (big.read("NEXT_DONE") == 0).all()
    assert same(again.env_reset(), obs) and same(again.env_get_state()[0], st)   # the same seed gives the same bits
    part.env_reset()                                                               # env_offset = 64: the last six envs of the same job
    assert same(part.env_get_state()[0], np.ascontiguousarray(st[K:])) and (part.env_get_state()[3] == 1).all()
    assert same(part.read("NEXT_OBS", (N - K, OBS)), np.ascontiguousarray(obs[K:]))
    other = jack_ctx(P, seed=6)
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
    assert same(np.ascontiguousarray(st2[fresh]), M.reset_states(O, SEED, fresh, resets2[fresh] - 1).astype(np.float32))
    for c in (big, again, part, other):
        c.close()


# ---------------------------------------------------------------------------------------------------------
# 3. one launch against the loop, and against the model
# ---------------------------------------------------------------------------------------------------------
def stepwise_rollout(O, b, obs, done, step0, forced=None):
    """T x { policy_act(obs, step_index), env_step } on context b: the buffers a rollout would fill.  FIN_LEN / FIN_REW from the episode sums the context held
    in front of the step.  The env is held to the model at every step."""
    n = b.N
    out = {k: [] for k in ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW", "MASKS")}
    for t in range(T):
        state = istate(b)
        assert same(obs, M.obs(state))
        act, lp, _, _ = b.policy_act(obs, step_index=step0 + t, action=None if forced is None else forced[t])
        len0, rew0 = b.read("EP_LEN"), b.read("EP_REW")
        out["OBS"].append(obs)
        out["DONES"].append(done.astype(np.float32))
        out["MASKS"].append(np.ones((n, 2), np.uint8))
        m_ns, m_r, m_t = M.step(O, state, act.reshape(-1))
        obs, r, done = b.env_step(act)
        assert same(r, m_r.astype(np.float32)) and np.array_equal(done, ((m_t == 1) | (len0 + 1 == b.cfg.max_episode_steps)).astype(np.int32))
        assert np.array_equal(istate(b)[done == 0], m_ns[done == 0])
        out["ACTIONS"].append(act.astype(np.int32))
        out["LOGPROBS"].append(lp)
        out["REWARDS"].append(r)
        out["FIN_LEN"].append(np.where(done != 0, len0 + 1, 0).astype(np.int32))
        out["FIN_REW"].append(np.where(done != 0, rew0 + r, np.float32(0)).astype(np.float32))
        assert obs.shape == (n, OBS)
    res = {k: np.stack(v).reshape(-1) for k, v in out.items()}
    res["NEXT_OBS"], res["NEXT_DONE"] = obs.reshape(-1), done
    return res, obs, done


def model_rollout(env, actions):
    """The model alone under the stored actions: OBS, REWARDS, FIN_LEN, FIN_REW and the done flag behind each of T steps; `env` carries the state on."""
    out = {k: [] for k in ("OBS", "REWARDS", "FIN_LEN", "FIN_REW", "DONE_AFTER")}
    for t in range(actions.shape[0]):
        out["OBS"].append(M.obs(env.state))
        _, r, done, fin_len, fin_rew = env.step(actions[t])
        out["REWARDS"].append(r)
        out["FIN_LEN"].append(fin_len)
        out["FIN_REW"].append(fin_rew)
        out["DONE_AFTER"].append(done.astype(np.float32))
    return {k: np.stack(v) for k, v in out.items()}


@LIMITS
@pytest.mark.parametrize("force", [False, True], ids=["drawn", "forced"])
def test_fused_rollout_equals_stepwise_api_and_the_model(P, O, max_steps, force):
    """N = 70: a full tile and a short one (a second, partial workgroup).  Two rollouts in a row: the second runs step indices 9 .. 17 and carries the done
    flags and the episode sums of the first.  The injected states start from random live hands with random keys."""
    a, b = jack_ctx(P, max_episode_steps=max_steps), jack_ctx(P, max_episode_steps=max_steps)
    assert same(a.get_params(), b.get_params())
    obs = inject(b, max_steps)
    assert same(inject(a, max_steps), obs)
    done = np.zeros(N, np.int32)
    env = ModelEnvs(O, SEED, N, max_steps)
    env.load(*a.env_get_state())
    seen = dict(resets=0, busts=0, sticks=0, truncations=0, hits_on=0)
    rng = np.random.default_rng(4)
    for k in range(2):
        forced = rng.integers(0, 2, (T, N, 1)).astype(np.int64) if force else None
        prev_done = a.read("NEXT_DONE").astype(np.float32) if k else np.zeros(N, np.float32)
        a.rollout(forced_actions=forced)
        got = rollout_buffers(a)
        want, obs, done = stepwise_rollout(O, b, obs, done, k * T, forced)
        for name, w in want.items():
            assert same(got[name], w), (k, name, int((bits(got[name]) != bits(w)).sum()))
        for x, y in zip(a.env_get_state(), b.env_get_state()):   # ENV_STATE, EP_LEN, EP_REW, RESET_COUNT
            assert same(x, y)
        Ob = got["OBS"].reshape(T * N, OBS)
        assert same(got["VALUES"], a.get_value(Ob))
        assert same(got["NEXT_VALUE"], a.get_value(got["NEXT_OBS"].reshape(N, OBS)))
        assert (got["MASKS"] == 1).all() and got["MASKS"].size == T * N * 2
        if force:
            assert np.array_equal(got["ACTIONS"], forced.reshape(-1))
        # the model alone under the stored actions
        mod = model_rollout(env, got["ACTIONS"].reshape(T, N))
        assert same(Ob, mod["OBS"].reshape(T * N, OBS)) and same(got["REWARDS"], mod["REWARDS"].reshape(-1))
        assert same(got["FIN_LEN"], mod["FIN_LEN"].reshape(-1)) and same(got["FIN_REW"], mod["FIN_REW"].reshape(-1))
        assert same(got["DONES"].reshape(T, N), np.concatenate([prev_done[None], mod["DONE_AFTER"][:-1]]))
        assert same(got["NEXT_DONE"].astype(np.float32), mod["DONE_AFTER"][-1])
        st_a, len_a, rew_a, res_a = a.env_get_state()
        assert same(st_a, env.state.astype(np.float32)) and np.array_equal(len_a, env.ep_len) and same(rew_a, env.ep_rew) and np.array_equal(res_a, env.resets)
        acts, rew, fin = got["ACTIONS"], got["REWARDS"], got["FIN_LEN"]
        seen["resets"] += int((fin > 0).sum())
        seen["busts"] += int(((acts == 1) & (rew == -1) & (fin > 0)).sum())
        seen["sticks"] += int((acts == 0).sum())
        seen["hits_on"] += int(((acts == 1) & (fin == 0)).sum())
        seen["truncations"] += int(((acts == 1) & (rew == 0) & (fin == max_steps)).sum())
        assert np.isin(rew, (-1.0, 0.0, 1.0)).all() and np.isin(got["FIN_REW"], (-1.0, 0.0, 1.0)).all() and (fin <= min(max_steps, 20)).all()
    print("in 2 x %d steps of %d envs: %s" % (T, N, seen))
    assert seen["resets"] > 0 and seen["busts"] > 0 and seen["sticks"] > 0 and seen["hits_on"] > 0
    assert (seen["truncations"] > 0) == (max_steps == 2)
    a.close()
    b.close()


def test_forcing_a_free_rollouts_actions_reproduces_it(P):
    free, rep = jack_ctx(P), jack_ctx(P)
    inject(free, 100)
    inject(rep, 100)
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
def test_iteration_equals_the_host_fed_iteration(P, O):
    """Two train_iterations against a PPO_ENV_HOST context (PPO_KERNEL_CAT_FUSED, PPO_DIST_CATEGORICAL, obs 45, heads (2,), same parameters and seed) fed by
    host_act, the MODEL's step with ppo_env_step's bookkeeping, and host_observe: the same observations, actions, rewards and dones go into the same
    ppo_update, which ends with the same parameters and AdamW moments."""
    dev = jack_ctx(P)
    host = P.Context(jack_cfg(P, env_kind=P.ENV_HOST))
    env = ModelEnvs(O, SEED, N, 100)
    params = dev.get_params()
    host.set_params(params)
    dev.env_reset()
    host.host_env_reset(env.reset())
    for _ in range(2):
        dev.train_iteration()
        host.host_rollout_begin()
        for _t in range(T):
            o, r, d, _, _ = env.step(host.host_act().reshape(-1))
            host.host_observe(o, r, d)
        host.host_rollout_end()
    sd, sh = dev.stats(), host.stats()
    for name in ("OBS", "ACTIONS", "LOGPROBS", "REWARDS", "DONES", "VALUES", "ADVANTAGES", "RETURNS"):
        assert same(dev.read(name), host.read(name)), name
    assert same(dev.get_params(), host.get_params()) and not same(dev.get_params(), params)
    (m0, v0, k0), (m1, v1, k1) = dev.get_optimizer(), host.get_optimizer()
    assert same(m0, m1) and same(v0, v1) and k0 == k1 == 2 * 2 * 2
    assert sd["loss"] == sh["loss"] and sd["global_step"] == sh["global_step"] == 2 * N * T
    assert same(dev.env_get_state()[0], env.state.astype(np.float32))
    for c in (dev, host):
        c.close()


# ---------------------------------------------------------------------------------------------------------
# 5. launch accounting
# ---------------------------------------------------------------------------------------------------------
def test_launch_accounting(P):
    ctx = jack_ctx(P)
    ctx.env_reset()
    a0, v0, u0 = ctx.gauss_fused_launches()
    ctx.rollout()
    a1, v1, u1 = ctx.gauss_fused_launches()
    assert (a1 - a0, v1 - v0, u1 - u0) == (0, 2, 0)   # the rollout kernel is not an act launch; the critic over OBS and over NEXT_OBS: three launches
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


def host_episodes(P, O, ctx, states, greedy, max_steps):
    """Whole episodes on the host: the model's observation of the states, policy_act_greedy / policy_act(step_index = the episode's step) and
    ppo_env_transition on all rows, a finished row ignored; the device's transition is held to the model on the live rows."""
    n = states.shape[0]
    st = states.copy()
    ret, length, alive = np.zeros(n, np.float32), np.zeros(n, np.int32), np.ones(n, bool)
    for t in range(max_steps):
        obs = M.obs(st)
        act = ctx.policy_act_greedy(obs)[0] if greedy else ctx.policy_act(obs, step_index=t)[0]
        ns, r, term = P.env_transition(ctx, P.ENV_BLACKJACK, st.astype(np.float32), act)
        m_ns, m_r, m_t = M.step(O, st[alive], act.reshape(-1)[alive])
        assert same(np.ascontiguousarray(ns[alive]), m_ns.astype(np.float32)) and same(np.ascontiguousarray(r[alive]), m_r.astype(np.float32))
        ret[alive] = (ret[alive] + r[alive]).astype(np.float32)
        length[alive] += 1
        st[alive] = ns[alive].astype(np.int64)
        alive &= (term == 0) & (length < max_steps)
        if not alive.any():
            break
    return ret, length, (length == max_steps).astype(np.int32)   # ppo_evaluate's flag: the episode's length reached the limit


@LIMITS
def test_evaluate(P, O, max_steps):
    """70 episodes, greedy and sampled, against the host loop in every return, length and truncated flag; n = 16 is the prefix of n = 70; another seed gives
    other episodes; the training state is untouched.  The common parameters (both actions are drawn): episodes end in busts, in sticks and, at limit 2, at
    the limit."""
    kw = dict(max_episode_steps=max_steps, seed=EVAL_SEED)
    ctx, plain, ref = jack_ctx(P, 32, **kw), jack_ctx(P, 32, **kw), jack_ctx(P, N, **kw)
    for c in (ctx, ref, plain):
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
        h_ret, h_len, h_trunc = host_episodes(P, O, ref, states, greedy, max_steps)
        print("greedy" if greedy else "sampled", "lengths %d..%d, truncated %d of %d, returns %s" %
              (length.min(), length.max(), st["truncated"], N, np.bincount((ret + 1).astype(int), minlength=3).tolist()))
        assert np.array_equal(length, h_len), (greedy, np.flatnonzero(length != h_len))
        assert same(ret, h_ret), (greedy, np.flatnonzero(bits(ret) != bits(h_ret)))
        assert st["truncated"] == int(h_trunc.sum())
        assert st["episodes"] == N and st["env_steps"] == int(h_len.sum())
        assert abs(st["return_mean"] - h_ret.astype(np.float64).mean()) <= 1e-9
        assert np.isin(ret, (-1.0, 0.0, 1.0)).all() and (length <= min(max_steps, 20)).all()
    assert len(set(ret_s.tolist())) > 1 and len(set(len_s.tolist())) > 1
    assert (stats_s["truncated"] > 0) == (max_steps == 2)
    # another seed gives other episodes (other keys: other deals and other decks, greedy or not)
    assert not np.array_equal(ret_2, ret_s) and not np.array_equal(ret_2g, ret_g)
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
@pytest.mark.parametrize("kw,status,word", [
    (dict(obs_size=4), 1, "observation of size"),
    (dict(obs_size=16), 1, "observation of size"),
    (dict(obs_size=44), 1, "observation of size"),
    (dict(dist_kind=1), 5, "PPO_DIST_CATEGORICAL"),
    (dict(dist_kind=2, head_dims=(1,)), 5, "PPO_DIST_CATEGORICAL"),
    (dict(head_dims=(3,)), 5, "head_dims[0] = 2"),
    (dict(head_dims=(2, 2)), 5, "n_heads = 1"),
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
    (dict(env_kind=14), 1, "unknown env_kind 14"),
])
def test_ctx_create_refusals(P, kw, status, word):
    with pytest.raises(P.binding.PPOError) as e:
        P.Context(jack_cfg(P, 8, **kw))
    assert "status %d:" % status in str(e.value) and word in str(e.value), str(e.value)
    if "obs_size" in kw:
        assert "observation of size 45" in str(e.value)


def test_the_limits_are_accepted(P):
    for steps in (1, (1 << 24) - 1):
        P.Context(jack_cfg(P, 8, max_episode_steps=steps)).close()


def test_refused_calls_change_nothing(P):
    n = 40
    ctx = jack_ctx(P, n)
    ctx.env_reset()
    ctx.train_iteration()
    ctx.rollout()
    ctx.sync()
    snap = lambda: ({k: ctx.read(k) for k in ALL_BUFS}, ctx.get_optimizer()[2], ctx.gauss_fused_launches())   # noqa: E731
    before = snap()
    o, r, d, af = np.zeros((n, OBS), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32)
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
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_set(np.zeros(OBS), np.ones(OBS), 1.0)),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_apply(o)),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_enable(1)),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_get()),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_set(0.0, 1.0, 1.0)),
        # the real-valued calls name their integer twins
        (5, "ppo_env_step", lambda: ctx.env_step_f32(af)),
        (5, "ppo_rollout", lambda: P.binding._check(L.ppo_rollout_f32(ctx.h, d_a.ptr), ctx.h)),
        (5, "ppo_policy_act", lambda: ctx.policy_act_f32(o)),
        # the time-limit fold: the stored observation holds neither the card count nor the key
        (5, "holds neither the card count nor the key", lambda: ctx.env_truncation_bootstrap(True)),
        (5, "holds neither the card count nor the key", lambda: ctx.env_truncation_bootstrap(False)),
        (5, "holds neither the card count nor the key", lambda: ctx.env_truncations()),
        # a state component outside its range, or not an integer: the host array is checked, nothing is copied
        (1, "state[3][0]", lambda: ctx.env_set_state(bad_state(3, 0, 704.0))),                       # show = 11
        (1, "state[4][0]", lambda: ctx.env_set_state(bad_state(4, 0, float(M.pack(1, 0, 5))))),      # t = 1
        (1, "state[5][0]", lambda: ctx.env_set_state(bad_state(5, 0, float(M.pack(12, 1, 0))))),     # show = 0
        (1, "state[6][0]", lambda: ctx.env_set_state(bad_state(6, 0, 1024.0 + 66.0))),               # a bit above the hand word
        (1, "state[39][3]", lambda: ctx.env_set_state(bad_state(39, 3, 16777216.0))),
        (1, "state[0][2]", lambda: ctx.env_set_state(bad_state(0, 2, -1.0))),
        (1, "state[7][1]", lambda: ctx.env_set_state(bad_state(7, 1, 2.5))),
        (1, "state[7][1]", lambda: ctx.env_set_state(bad_state(7, 1, np.nan), np.zeros(n, np.int32))),
        (1, "state[8][0]", lambda: ctx.env_set_state(bad_state(8, 0, np.nan))),
        # bad arguments of calls this env does serve
        (1, "n_episodes", lambda: ctx.evaluate(0, 1)),
    ]
    for status, word, call in calls:
        with pytest.raises(P.binding.PPOError) as e:
            call()
        assert "status %d:" % status in str(e.value) and word in str(e.value), str(e.value)
    import ctypes as C
    buf, term = (C.c_float * 8)(), (C.c_int32 * 2)()
    assert L.ppo_env_transition_f32(P.ENV_BLACKJACK, buf, buf, 0, buf, None, buf, term, None) == 5
    ctx.sync()
    after = snap()
    assert before[1:] == after[1:]
    for k in ALL_BUFS:
        assert same(before[0][k], after[0][k]), k
    # the largest legal components are accepted, and the context still works
    top = good.copy()
    top[0] = (M.HAND_MAX, M.WORD_MAX, M.WORD_MAX, M.WORD_MAX)
    top[1] = (float(M.pack(2, 0, 1)), 0, 0, 0)
    ctx.env_set_state(top)
    ob = ctx.read("NEXT_OBS", (n, OBS))
    assert same(ctx.env_get_state()[0], top) and ob[0, 31] == 1.0 and ob[0, 42] == 1.0 and ob[0, 43] == 1.0 and ob[1, 2] == 1.0 and ob[1, 33] == 1.0
    ctx.train_iteration()
    assert np.isfinite(ctx.stats()["loss"])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 8. learning
# ---------------------------------------------------------------------------------------------------------
LEARN_ITERS = 60
RANDOM_RETURN = -0.3958960   # the model's uniformly random policy (tests/test_blackjack_cpu.py)
OPTIMUM = -0.0465560         # the exact optimum from the deal (the same)
SE_MAX = 0.0079              # of a mean of 16 384 returns in [-1, 1]: at most 1 / sqrt(16 384) = 0.0078125
LEARN_BAR = 0.1720           # half of the smallest improvement over the random policy that tools/blackjack_curve.py showed across three seeds (below)


def test_blackjack_learns(P):
    """tools/blackjack_curve.py's settings, one seed: 512 envs x 64 steps, its default hyper-parameters, LEARN_ITERS iterations, then ppo_evaluate(16 384,
    sampled), whose return_mean has a standard error of at most 0.0079 (returns lie in [-1, 1]).  The tool measured on an MI355X, seeds 1 / 2 / 3 (mean sampled
    return over the 16 384 fixed episodes; the curves are in DESIGN.md): -0.4042 / -0.4054 / -0.4058 untrained, -0.0784 / -0.0715 / -0.0767 after 10 iterations,
    -0.0505 / -0.0511 / -0.0519 after 60 and -0.0497 / -0.0499 / -0.0528 after 100 (0.28 s of training): improvements over the random policy's -0.3958960 at
    iteration 60 of 0.3454, 0.3448 and 0.3440.  The bar is half of the smallest, 0.1720 -- a trained mean return of at least -0.2239, which always sticking
    (-0.1863677) would pass and the random policy would not; the exact optimum, the ceiling, is -0.0465560, and nothing beats it but by sampling noise."""
    spec = importlib.util.spec_from_file_location("blackjack_curve", os.path.join(ROOT, "tools", "blackjack_curve.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse([])
    assert (tool.N, tool.T, tool.MAXS, tool.EVAL_EPISODES) == (512, 64, 100, 16384)
    ctx = tool.make_ctx(P, 1, args)
    ctx.init_orthogonal(1)
    ctx.env_reset()
    untrained = tool.sampled_return(ctx)
    for _ in range(LEARN_ITERS):
        ctx.train_iteration()
    trained = tool.sampled_return(ctx)
    print("mean return over 16 384 episodes: untrained %.4f, trained %.4f, improvement over the random policy %.4f (bar %.4f; optimum %.4f)"
          % (untrained, trained, trained - RANDOM_RETURN, LEARN_BAR, OPTIMUM))
    ctx.close()
    assert args.iters == LEARN_ITERS
    assert abs(untrained - RANDOM_RETURN) <= 8 * SE_MAX + 0.05   # the untrained policy is a near-uniform one (0.05: what its small logits may move it)
    assert trained - RANDOM_RETURN >= LEARN_BAR
    assert trained <= OPTIMUM + 8 * SE_MAX                        # nothing beats the optimum but by sampling noise
