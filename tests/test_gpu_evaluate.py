"""Using a trained policy on the GPU: ppo_policy_act_greedy (Categorical::mode through the Agent, reference Categorical.cpp:139-141,
CategoricalMasked.cpp:160-162, Agent.cpp:117-170) and ppo_evaluate (whole episodes of the device env as one launch).

Yardsticks: ppo_policy_act with the greedy action forced (bit for bit), the oracle's logits (argmax wherever its top-two gap is >= 1e-5: three times the
3e-6 at which tests/test_gpu_parity.py holds teacher-forced log-probs to the reference), a host loop over the stand-alone entry points from the same start
states (bit for bit), the CPU reference loop of tests/test_evaluate_abi.py, and a context that trains without ever being evaluated (bit for bit).
"""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

import test_evaluate_abi as EA

pytestmark = pytest.mark.gpu

SEED = 123
ENVS = {"cartpole": dict(env_kind=0, dist_kind=0, obs_size=4, head_dims=(2,)), "mountaincar": dict(env_kind=1, dist_kind=1, obs_size=2, head_dims=(3,))}


@pytest.fixture(scope="module")
def P():
    return load_package()


@pytest.fixture(scope="module")
def O():
    import oracle
    oracle.build()
    return oracle


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def make_ctx(P, env, vector=False, **kw):
    cfg = dict(ENVS[env], num_envs=64, num_steps=128, num_minibatches=4, update_epochs=4, seed=SEED, max_episode_steps=500,
               kernel_flags=P.KERNEL_ROLLOUT_VECTOR if vector else 0)
    cfg.update(kw)
    return P.Context(P.make_config(**cfg))


_trained = {}


def trained_params(P, env):
    """~30 iterations at 64 x 128: CartPole episodes then spread up to the 500-step cap."""
    if env not in _trained:
        c = make_ctx(P, env, seed=1, total_timesteps=64 * 128 * 30, update_epochs=10)
        c.init_orthogonal(3)
        c.env_reset()
        for _ in range(30):
            c.train_iteration()
        c.stats()
        _trained[env] = c.get_params()
        c.close()
    return _trained[env]


def params_for(P, ctx, env, which):
    return EA.random_params(ctx.P) if which == "random" else trained_params(P, env)


# ---------------------------------------------------------------------------------------------- 3. greedy vs forced, 4. greedy vs oracle
SHAPES = {
    "cartpole": dict(env_kind=0, dist_kind=0, obs_size=4, head_dims=(2,)),
    "mountaincar_masked": dict(env_kind=1, dist_kind=1, obs_size=2, head_dims=(3,)),
    "generic_f32": dict(env_kind=2, dist_kind=1, obs_size=8, head_dims=(3, 3, 2), hidden=128, n_hidden=2, compute_dtype=0),
    "generic_bf16": dict(env_kind=2, dist_kind=1, obs_size=8, head_dims=(3, 3, 2), hidden=128, n_hidden=2, compute_dtype=1),
    "host": dict(env_kind=3, dist_kind=1, obs_size=8, head_dims=(3, 3, 2)),
}


def random_mask(rng, n, head_dims):
    """Random masks with at least one valid action per head; row 0: all but one action of every head masked."""
    cols, only = [], []
    for A in head_dims:
        m = rng.random((n, A)) < 0.6
        keep = rng.integers(0, A, n)
        m[np.arange(n), keep] = True
        m[0] = False
        m[0, keep[0]] = True
        only.append(int(keep[0]))
        cols.append(m)
    return np.concatenate(cols, axis=1).astype(np.uint8), only


@pytest.mark.parametrize("vector", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_greedy_equals_forced_policy_act(P, shape, vector):
    """policy_act_greedy then policy_act(action = greedy): log-prob, entropy and value agree bit for bit; a head with one valid action returns it; the call
    draws nothing (two calls agree) and, on a PPO_ENV_HOST context, works in the middle of an open rollout without disturbing it."""
    kw = dict(SHAPES[shape], num_envs=16, num_steps=4, num_minibatches=1, update_epochs=1, seed=5, kernel_flags=P.KERNEL_ROLLOUT_VECTOR if vector else 0)
    c = P.Context(P.make_config(**kw))
    rng = np.random.default_rng(11)
    c.set_params((np.random.default_rng(7).standard_normal(c.P) * 0.3).astype(np.float32))
    n = 1000   # a ragged last tile
    obs = rng.standard_normal((n, c.O)).astype(np.float32)
    masked = kw["dist_kind"] == 1
    mask, only = random_mask(rng, n, kw["head_dims"]) if masked else (None, None)
    if shape == "host":
        c.host_env_reset(rng.standard_normal((16, c.O)).astype(np.float32))
        c.host_rollout_begin()
        c.host_act()                     # mid-rollout: a step is acted on and not yet observed
    a, lp, en, v = c.policy_act_greedy(obs, mask)
    a2, lp2, en2, v2 = c.policy_act_greedy(obs, mask)
    assert np.array_equal(a, a2) and same(lp, lp2) and same(en, en2) and same(v, v2)
    fa, flp, fen, fv = c.policy_act(obs, mask=mask, action=a)
    assert same(lp, flp) and same(en, fen) and same(v, fv), (int((bits(lp) != bits(flp)).sum()), int((bits(en) != bits(fen)).sum()))
    assert a.shape == (n, len(kw["head_dims"])) and a.min() >= 0 and (a < np.asarray(kw["head_dims"])).all()
    if masked:
        assert list(a[0]) == only
        off = np.concatenate([[0], np.cumsum(kw["head_dims"])[:-1]])
        assert mask[np.arange(n)[:, None], a + off].all()      # never a masked action
    if len(kw["head_dims"]) == 1:   # the greedy action is the most probable one: no action has a larger log-prob
        for alt in range(kw["head_dims"][0]):
            _, olp, _, _ = c.policy_act(obs, mask=mask, action=np.full((n, 1), alt))
            assert (olp <= lp).all(), alt
    if shape == "host":
        c.host_observe(rng.standard_normal((16, c.O)).astype(np.float32), np.ones(16, np.float32), np.zeros(16, np.int32))
        for _ in range(3):
            c.host_act()
            c.host_observe(rng.standard_normal((16, c.O)).astype(np.float32), np.ones(16, np.float32), np.zeros(16, np.int32))
        c.host_rollout_end()
        assert np.isfinite(c.stats()["loss"])
    c.close()


@pytest.mark.parametrize("scale", [0.3, 0.01])
@pytest.mark.parametrize("shape", ["cartpole", "mountaincar_masked", "generic_f32"])
def test_greedy_equals_oracle_argmax(P, O, shape, scale):
    """Actions equal argmax of oracle.actor_logits on every row whose top-two oracle gap is >= 1e-5 in every head; at most 0.5 % of the rows may be left out
    (the oracle leaves out none for these parameters and observations)."""
    kw = dict(SHAPES[shape], num_envs=16, num_steps=4, num_minibatches=1, update_epochs=1, seed=5)
    c = P.Context(P.make_config(**kw))
    hd = list(kw["head_dims"])
    net = O.Net.make(kw["obs_size"], hd, hidden=kw.get("hidden", 64), n_hidden=kw.get("n_hidden", 2), dist_kind=kw["dist_kind"])
    params = EA.random_params(c.P, scale)
    assert O.param_count(net) == c.P
    c.set_params(params)
    obs = np.random.default_rng(7).standard_normal((8192, c.O)).astype(np.float32)
    a, _, _, _ = c.policy_act_greedy(obs)
    z = O.actor_logits(net, params, obs)
    ok = np.ones(8192, bool)
    want = np.zeros_like(a)
    off = 0
    for h, A in enumerate(hd):
        zh = z[:, off:off + A]
        top = np.sort(zh, axis=1)
        ok &= (top[:, -1] - top[:, -2]) >= EA.GAP
        want[:, h] = np.argmax(zh, axis=1)
        off += A
    left_out = 1.0 - ok.mean()
    print("rows left out: %.4f %%" % (100 * left_out))
    assert left_out <= 0.005
    assert np.array_equal(a[ok], want[ok]), int((a[ok] != want[ok]).any(axis=1).sum())
    c.close()


# ---------------------------------------------------------------------------------------------- 5. fused = stepwise
def stepwise_evaluate(P, ctx, env_kind, starts, greedy, max_steps):
    """The evaluation run through the stand-alone entry points: policy_act_greedy (or policy_act with step_index = t: ctx.cfg.seed is the evaluation seed
    and env_offset 0, so row e at step t draws with key (seed, e, t, head)) + env_transition, all rows every step; finished rows are frozen."""
    n = starts.shape[0]
    st = starts.copy()
    ret, length, trunc = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    alive = np.ones(n, bool)
    t = 0
    while alive.any():
        a = ctx.policy_act_greedy(st)[0] if greedy else ctx.policy_act(st, step_index=t)[0]
        ns, r, term = P.env_transition(ctx, env_kind, st, a[:, 0])
        st[alive] = ns[alive]
        ret[alive] = (ret[alive] + r[alive]).astype(np.float32)
        length[alive] += 1
        tr = length == max_steps
        trunc[alive] = tr[alive]
        alive &= (term == 0) & ~tr
        t += 1
    return ret, length, trunc


@pytest.mark.parametrize("which", ["random", "trained"])
@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("vector", [False, True])
@pytest.mark.parametrize("env", list(ENVS))
def test_fused_evaluation_equals_stepwise(P, O, env, vector, greedy, which):
    """Per-episode returns (f32 bits), lengths and the truncated count of ppo_evaluate equal the host loop over policy_act_greedy / policy_act +
    env_transition from the same start states, for n_episodes in {1, 7, 16, 33, 300}: ragged tiles, and (300 > 16 x 16) several tiles.  The stepwise loop
    runs once with 300 rows; episode e is the same function for every n (the prefix property), so each n is compared with its first n rows.
    Greedy runs are also held to the CPU reference loop on every episode whose oracle trajectory never saw a top-two gap below 1e-5.  Episodes left out:
    random parameters 0 allowed (observed 0); trained policy: at most 10 % allowed; observed on an MI355X: CartPole 0.67 % (2 of 300, both kernel forms),
    MountainCar 0 %."""
    kind = ENVS[env]["env_kind"]
    c = make_ctx(P, env, vector)
    params = params_for(P, c, env, which)
    c.set_params(params)
    starts = EA.start_states(O, kind, SEED, 300)
    s_ret, s_len, s_trunc = stepwise_evaluate(P, c, kind, starts, greedy, 500)
    for n in (1, 7, 16, 33, 300):
        st, ret, length = c.evaluate(n, SEED, greedy)
        assert same(ret, s_ret[:n]), (n, int((bits(ret) != bits(s_ret[:n])).sum()))
        assert np.array_equal(length, s_len[:n]), n
        assert st["truncated"] == int(s_trunc[:n].sum()) and st["episodes"] == n
    print("%s %s lengths %d..%d mean %.1f truncated %d / 300" % (env, which, s_len.min(), s_len.max(), s_len.mean(), s_trunc.sum()))
    if which == "trained" and env == "cartpole":
        assert s_len.max() > 100, "the trained CartPole policy should hold the pole for a while"
    if greedy:
        net = O.Net.make(c.O, list(ENVS[env]["head_dims"]), dist_kind=ENVS[env]["dist_kind"])
        o_ret, o_len, o_trunc, gap = EA.oracle_evaluate(O, net, params, kind, SEED, 300, 500)
        ok = gap >= EA.GAP
        left_out = 1.0 - ok.mean()
        print("%s %s vector=%d: episodes left out of the oracle comparison: %.2f %%" % (env, which, vector, 100 * left_out))
        assert left_out <= (0.0 if which == "random" else 0.10)
        assert same(s_ret[ok], o_ret[ok]) and np.array_equal(s_len[ok], o_len[ok]) and np.array_equal(s_trunc[ok], o_trunc[ok])
    c.close()


# ---------------------------------------------------------------------------------------------- 6. prefix and repeat, 8. summary
@pytest.mark.parametrize("greedy", [True, False])
@pytest.mark.parametrize("env", list(ENVS))
def test_prefix_repeat_and_summary(P, env, greedy):
    c = make_ctx(P, env)
    c.set_params(trained_params(P, env))
    st64, r64, l64 = c.evaluate(64, SEED, greedy)
    st16, r16, l16 = c.evaluate(16, SEED, greedy)
    assert same(r16, r64[:16]) and np.array_equal(l16, l64[:16])
    st64b, r64b, l64b = c.evaluate(64, SEED, greedy)
    assert same(r64, r64b) and np.array_equal(l64, l64b) and st64 == st64b
    for st, r, l in ((st64, r64, l64), (st16, r16, l16)):
        r8 = r.astype(np.float64)
        for key, want in (("return_mean", r8.mean()), ("return_std", r8.std()), ("return_min", r8.min()), ("return_max", r8.max()),
                          ("length_mean", l.astype(np.float64).mean())):
            assert abs(st[key] - want) <= 1e-12 * max(1.0, abs(want)), (key, st[key], want)
        assert st["env_steps"] == int(l.sum()) and st["length_min"] == l.min() and st["length_max"] == l.max() and st["episodes"] == len(l)
        assert l.min() >= 1 and l.max() <= 500
        if env == "mountaincar":
            assert st["truncated"] == int((l == 500).sum())
    c.close()


def test_more_episodes_than_slots(P):
    """65 536 + 5 episodes of the vector form's one-wave slots (16 384) and of the default form's 65 536 columns: slots take further episodes by the static
    rule, and the first 300 episodes are those of a run of 300."""
    for vector in (False, True):
        c = make_ctx(P, "cartpole", vector)
        c.set_params(EA.random_params(c.P))
        n = 65536 + 5
        st, r, l = c.evaluate(n, SEED, True)
        _, r300, l300 = c.evaluate(300, SEED, True)
        assert same(r[:300], r300) and np.array_equal(l[:300], l300)
        assert l.min() >= 1 and st["env_steps"] == int(l.sum()) and np.array_equal(r, (l - 2).astype(np.float32))
        c.close()


# ---------------------------------------------------------------------------------------------- 7. training undisturbed
STATE = ["OBS", "ACTIONS", "LOGPROBS", "VALUES", "REWARDS", "DONES", "ADVANTAGES", "RETURNS", "NEXT_VALUE", "NEXT_OBS", "NEXT_DONE", "FIN_LEN", "FIN_REW",
         "EP_LEN", "EP_REW", "ENV_STATE", "RESET_COUNT", "PERM", "GRADS", "MASKS"]


def assert_same_training_state(a, b, tag):
    for name in STATE:
        assert same(a.read(name), b.read(name)), (tag, name)
    assert same(a.get_params(), b.get_params()), (tag, "PARAMS")
    ma, va, sa = a.get_optimizer()
    mb, vb, sb = b.get_optimizer()
    assert sa == sb and same(ma, mb) and same(va, vb), (tag, "AdamW")
    assert a.stats() == b.stats(), tag
    assert a.profile_read()["vector_fallback_launches"] == b.profile_read()["vector_fallback_launches"], tag


@pytest.mark.parametrize("env", list(ENVS))
def test_training_is_undisturbed_by_evaluation(P, env):
    a, b = make_ctx(P, env, seed=4), make_ctx(P, env, seed=4)
    for c in (a, b):
        c.init_orthogonal(9)
        c.env_reset()
    for it in range(3):
        a.train_iteration()
        b.train_iteration()
        b.evaluate(64, SEED, True)
        b.evaluate(64, SEED, False)
        b.policy_act_greedy(np.zeros((5, b.O), np.float32))
    assert_same_training_state(a, b, env)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 9. refusals
def raw_evaluate(P, c, n, out=True):
    st = P.binding.EvalStats()
    code = P.binding.lib().ppo_evaluate(c.h, C.c_int64(n), C.c_int64(SEED), C.c_int32(1), None, None, C.byref(st) if out else None)
    return code, (P.binding.lib().ppo_last_error(c.h) or b"").decode()


def test_refusals_change_nothing(P):
    ERR_INVALID, ERR_UNSUPPORTED = 1, 5
    syn = P.Context(P.make_config(env_kind=2, dist_kind=1, obs_size=8, head_dims=(3, 2), hidden=128, num_envs=16, num_steps=4, num_minibatches=1, update_epochs=1))
    host = P.Context(P.make_config(env_kind=3, dist_kind=0, obs_size=4, head_dims=(2,), num_envs=16, num_steps=4, num_minibatches=1, update_epochs=1))
    for c in (syn, host):
        code, msg = raw_evaluate(P, c, 8)
        assert code == ERR_UNSUPPORTED and "ppo_policy_act_greedy" in msg, (code, msg)
        with pytest.raises(P.binding.PPOError):
            c.evaluate(8, SEED)
        c.close()
    a, b = make_ctx(P, "cartpole", seed=4), make_ctx(P, "cartpole", seed=4)
    for c in (a, b):
        c.init_orthogonal(9)
        c.env_reset()
        c.train_iteration()
    assert raw_evaluate(P, b, 0)[0] == ERR_INVALID
    assert raw_evaluate(P, b, -3)[0] == ERR_INVALID
    assert raw_evaluate(P, b, 8, out=False)[0] == ERR_INVALID
    a.train_iteration()
    b.train_iteration()
    assert_same_training_state(a, b, "after refused calls")
    a.close()
    b.close()
    z = make_ctx(P, "cartpole", max_episode_steps=0)
    assert raw_evaluate(P, z, 8)[0] == ERR_INVALID
    z.close()
