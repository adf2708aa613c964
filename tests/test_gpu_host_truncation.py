"""Time-limit truncations of caller-stepped environments (include/ppo_hip.h, "Time-limit truncations": ppo_host_observe_truncated /
ppo_host_group_observe_truncated / ppo_host_truncations / ppo_bootstrap_rewards) on the GPU.

The envs are scripted (tests/test_host_truncation_abi.py: ScriptedEnv, action-independent), so the truncation events of a rollout are known on the CPU
before the GPU runs.  What is checked: without an event the new calls ARE the plain ones, bit for bit; with events the rewards are folded as
f32(r + f32(gamma v)) exactly at the events, v being the value the context's own rollout assigns to that observation; the scan, the statistics and
the grouped form follow.
"""
import numpy as np
import pytest

from __graft_entry__ import load_package
from test_gpu_host_env import assert_same_state, bits
from test_host_truncation_abi import ScriptedEnv, Transitions

pytestmark = pytest.mark.gpu

T = 24
HEADS = {2: (3,), 4: (2,), 8: (4,)}


@pytest.fixture(scope="module")
def P():
    return load_package()


def make(P, N, O=4, steps=T, **kw):
    base = dict(env_kind=P.ENV_HOST, obs_size=O, head_dims=HEADS.get(O, (3, 2)), num_envs=N, num_steps=steps, num_minibatches=2, update_epochs=2, seed=5,
                total_timesteps=N * steps * 5)
    base.update(kw)
    return P.Context(P.make_config(**base))


def pair(P, N, O=4, steps=T, **kw):
    a, b = make(P, N, O, steps, **kw), make(P, N, O, steps, **kw)
    a.init_orthogonal(11)
    b.set_params(a.get_params())
    return a, b


def feed(ctx, tr, mode):
    """One iteration on the transitions tr.  mode: plain | flags | zeros | final_only"""
    ctx.host_rollout_begin()
    for t in range(ctx.T):
        ctx.host_act()
        o, r, d = tr.obs[t], tr.rew[t], tr.done[t]
        if mode == "plain":
            ctx.host_observe(o, r, d)
        elif mode == "flags":
            ctx.host_observe(o, r, d, truncated=tr.trunc[t], final_obs=tr.final[t])
        elif mode == "zeros":
            ctx.host_observe(o, r, d, truncated=np.zeros_like(tr.trunc[t]), final_obs=tr.final[t])
        else:
            ctx.host_observe(o, r, d, final_obs=tr.final[t])
    ctx.host_rollout_end()


def fold(r, v, gamma):
    return (r + (np.float32(gamma) * v).astype(np.float32)).astype(np.float32)


def check_fold(P, ctx, tr):
    """The event list, REWARDS at and off the events, and the scan on the folded rewards.  Returns (indices, values)."""
    Tn, N = ctx.T, ctx.N
    want = tr.events()
    idx, val = ctx.host_truncations()
    assert idx.dtype == np.int32 and np.array_equal(idx, want), (idx, want)
    assert val.shape == idx.shape and np.isfinite(val).all()
    rew = ctx.read("REWARDS")
    expect = tr.rew.ravel().copy()
    expect[idx] = fold(expect[idx], val, ctx.cfg.gamma)
    assert np.array_equal(bits(rew), bits(expect)), int((bits(rew) != bits(expect)).sum())
    if len(idx):
        assert (bits(rew[idx]) != bits(tr.rew.ravel()[idx])).any()
    shape = (Tn, N)
    adv, ret = P.gae(ctx, rew.reshape(shape), ctx.read("VALUES", shape), ctx.read("DONES", shape), ctx.read("NEXT_VALUE"), ctx.read("NEXT_DONE"),
                     ctx.cfg.gamma, ctx.cfg.gae_lambda)
    assert np.array_equal(bits(adv), bits(ctx.read("ADVANTAGES", shape))) and np.array_equal(bits(ret), bits(ctx.read("RETURNS", shape)))
    return idx, val


@pytest.mark.parametrize("N,O", [(7, 4), (33, 4), (33, 2), (33, 8)])
def test_without_an_event_the_truncated_calls_are_the_plain_ones(P, N, O):
    a, b = pair(P, N, O)
    env_a, env_b = ScriptedEnv(N, O), ScriptedEnv(N, O)
    a.host_env_reset(env_a.reset())
    b.host_env_reset(env_b.reset())
    for it, mode in enumerate(("zeros", "final_only")):
        feed(a, env_a.rollout(T), "plain")
        feed(b, env_b.rollout(T), mode)
        assert_same_state(a, b, tag=(it, mode))
        idx, val = b.host_truncations()
        assert idx.size == 0 and val.size == 0
    a.close()
    b.close()


@pytest.mark.parametrize("N,O", [(7, 4), (33, 4), (33, 2), (33, 8)])
def test_fold_bit_for_bit(P, N, O):
    a, b = pair(P, N, O)
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    tr = env.rollout(T)
    K, terminations = int(tr.trunc.sum()), int((tr.done != 0).sum() - tr.trunc.sum())
    assert K > 0 and terminations > 0
    for c, mode in ((a, "plain"), (b, "flags")):
        c.host_env_reset(obs0)
        feed(c, tr, mode)
    idx, _ = check_fold(P, b, tr)
    assert idx.size == K
    assert a.host_truncations()[0].size == 0
    # the finished episodes and their statistics keep the raw rewards
    assert np.array_equal(bits(a.read("FIN_REW")), bits(b.read("FIN_REW"))) and np.array_equal(a.read("FIN_LEN"), b.read("FIN_LEN"))
    assert np.array_equal(bits(a.read("EP_REW")), bits(b.read("EP_REW")))
    sa, sb = a.stats(), b.stats()
    assert sa["ep_count"] == sb["ep_count"] > 0 and sa["ep_rew_mean"] == sb["ep_rew_mean"] and sa["ep_len_mean"] == sb["ep_len_mean"]
    assert np.isfinite(sb["loss"]) and sb["updates"] == 1
    assert not np.array_equal(bits(a.read("ADVANTAGES")), bits(b.read("ADVANTAGES")))
    a.close()
    b.close()


@pytest.mark.parametrize("O", [2, 4, 8])
def test_same_critic_as_the_rollout(P, O):
    """final_obs = the observation the step was acted on (row (t, n) of OBS): every reported value is VALUES[t, n], bit for bit, and within the project's
    bar for values (3e-6) of ppo_get_value on the same rows."""
    N = 33
    b, twin = pair(P, N, O)
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    tr = env.rollout(T)
    acted_on = np.concatenate([obs0[None], tr.obs[:-1]])
    tr = Transitions(tr.obs, tr.rew, tr.done, tr.trunc, acted_on)
    b.host_env_reset(obs0)
    feed(b, tr, "flags")
    idx, val = b.host_truncations()
    assert idx.size == int(tr.trunc.sum()) > 32   # more than one 32-row tile
    assert np.array_equal(bits(b.read("OBS", (T * N, O))[idx]), bits(acted_on.reshape(T * N, O)[idx]))
    assert np.array_equal(bits(val), bits(b.read("VALUES")[idx]))
    ref = twin.get_value(acted_on.reshape(T * N, O)[idx])   # the twin keeps the parameters the rollout ran with
    assert np.abs(val - ref).max() <= 3e-6, np.abs(val - ref).max()
    b.close()
    twin.close()


def test_groups_equal_the_ungrouped_rollout(P):
    """3 groups with ragged bounds, group 0 two steps ahead of the others, group 1 on the plain observe whenever it has no event"""
    N = 33
    bounds = [0, 5, 6, N]
    a, b = pair(P, N)
    env = ScriptedEnv(N, 4)
    obs0 = env.reset()
    tr = env.rollout(T)
    a.host_env_reset(obs0)
    feed(a, tr, "flags")
    b.host_env_reset(obs0)
    b.host_rollout_begin(bounds)
    order = [0, 0] + [g for _ in range(T - 2) for g in (1, 2, 0)] + [1, 2, 1, 2]
    t_of = [0, 0, 0]
    plain_calls = 0
    for g in order:
        t, b0, b1 = t_of[g], bounds[g], bounds[g + 1]
        b.host_group_act(g)
        b.host_group_actions(g)
        if g == 1 and not tr.trunc[t, b0:b1].any():
            b.host_group_observe(g, tr.obs[t, b0:b1], tr.rew[t, b0:b1], tr.done[t, b0:b1])
            plain_calls += 1
        else:
            b.host_group_observe(g, tr.obs[t, b0:b1], tr.rew[t, b0:b1], tr.done[t, b0:b1], truncated=tr.trunc[t, b0:b1], final_obs=tr.final[t, b0:b1])
        t_of[g] += 1
        assert t_of[0] - min(t_of[1], t_of[2]) <= 2
    assert t_of == [T] * 3 and 0 < plain_calls < T and tr.trunc[:, 5].any()
    b.host_rollout_end()
    assert_same_state(a, b)
    ia, va = a.host_truncations()
    ib, vb = b.host_truncations()
    assert ia.size > 0 and np.array_equal(ia, ib) and np.array_equal(bits(va), bits(vb))
    check_fold(P, b, tr)
    a.close()
    b.close()


def pattern_transitions(N, steps, O, trunc, seed=3):
    """Random transitions whose episodes end exactly where `trunc` [steps, N] says, all by truncation, plus one termination where no event sits"""
    rng = np.random.default_rng(seed)
    trunc = np.asarray(trunc, np.int32)
    done = trunc.copy()
    free = np.argwhere(trunc == 0)
    if len(free):
        done[tuple(free[0])] = 1
    return Transitions(rng.standard_normal((steps, N, O)).astype(np.float32), rng.uniform(-1, 1, (steps, N)).astype(np.float32), done, trunc,
                       rng.standard_normal((steps, N, O)).astype(np.float32))


def edge(name):
    N, steps = (33, 4) if name == "tile_plus_one" else (7, 4)
    trunc = np.zeros((steps, N), np.int32)
    if name == "one":
        trunc[1, 3] = 1
    elif name == "tile_plus_one":
        trunc[2, :] = 1             # K = 33: one 32-row tile and one row
    elif name == "every_step":
        trunc[:] = 1                # K = T * N
    elif name == "last_step":
        trunc[steps - 1, [0, 6]] = 1
    return N, steps, trunc


@pytest.mark.parametrize("name", ["one", "tile_plus_one", "every_step", "last_step"])
def test_edges(P, name):
    N, steps, trunc = edge(name)
    b = make(P, N, 4, steps)
    b.init_orthogonal(11)
    tr = pattern_transitions(N, steps, 4, trunc)
    b.host_env_reset(np.zeros((N, 4), np.float32))
    feed(b, tr, "flags")
    idx, _ = check_fold(P, b, tr)
    assert idx.size == {"one": 1, "tile_plus_one": 33, "every_step": steps * N, "last_step": 2}[name]
    assert np.isfinite(b.stats()["loss"])
    b.close()


def test_events_in_one_iteration_and_none_in_the_next(P):
    """Iteration 1 with events, iteration 2 without: the second equals that of a twin that never saw a flag (given, after iteration 1, the parameters and
    AdamW state the fold led to), and the event list is empty again."""
    N, steps = 7, 4
    b, twin = pair(P, N, 4, steps)
    rng = np.random.default_rng(9)
    obs0 = rng.standard_normal((N, 4)).astype(np.float32)
    trunc = np.zeros((steps, N), np.int32)
    trunc[0, 2] = trunc[3, 5] = 1
    tr1 = pattern_transitions(N, steps, 4, trunc, seed=4)
    tr2 = pattern_transitions(N, steps, 4, np.zeros((steps, N), np.int32), seed=5)
    b.host_env_reset(obs0)
    twin.host_env_reset(obs0)
    feed(b, tr1, "flags")
    feed(twin, tr1, "plain")
    assert b.host_truncations()[0].size == 2
    twin.set_params(b.get_params())
    twin.set_optimizer(*b.get_optimizer())
    feed(b, tr2, "flags")
    feed(twin, tr2, "plain")
    assert_same_state(b, twin)
    idx, val = b.host_truncations()
    assert idx.size == 0 and val.size == 0
    b.close()
    twin.close()


def test_bootstrap_rewards_stand_alone(P):
    """On a CartPole device-env context: K = 45 rows (a 32-row tile and 13), distinct indices into 64 rewards"""
    c = P.Context(P.make_config(num_envs=8, num_steps=8, num_minibatches=2, update_epochs=1))
    c.init_orthogonal(3)
    rng = np.random.default_rng(7)
    K, gamma = 45, 0.97
    obs = rng.standard_normal((K, 4)).astype(np.float32)
    index = rng.permutation(64)[:K].astype(np.int32)
    r0 = rng.uniform(-1, 1, 64).astype(np.float32)
    d_r = c.dev(r0)
    v = c.bootstrap_rewards(obs, index, gamma, d_r)
    assert v.shape == (K,) and np.array_equal(bits(v), bits(c.get_value(obs)))
    expect = r0.copy()
    expect[index] = fold(r0[index], v, gamma)
    whole = d_r.download()
    assert np.array_equal(bits(whole), bits(expect))
    untouched = np.setdiff1d(np.arange(64), index)
    assert np.array_equal(bits(whole[untouched]), bits(r0[untouched])) and (bits(whole[index]) != bits(r0[index])).any()
    # 32 + 13 in two calls: the same bits
    d_r.upload(r0)
    v1 = c.bootstrap_rewards(obs[:32], index[:32], gamma, d_r)
    v2 = c.bootstrap_rewards(obs[32:], index[32:], gamma, d_r, want_values=True)
    assert np.array_equal(bits(np.concatenate([v1, v2])), bits(v)) and np.array_equal(bits(d_r.download()), bits(whole))
    # without values, and K = 0
    d_r.upload(r0)
    assert c.bootstrap_rewards(obs, index, gamma, d_r, want_values=False) is None
    assert np.array_equal(bits(d_r.download()), bits(whole))
    c.bootstrap_rewards(np.zeros((0, 4), np.float32), np.zeros(0, np.int32), gamma, d_r)
    assert np.array_equal(bits(d_r.download()), bits(whole))
    # the context's own buffer by name
    c.write("REWARDS", r0)
    c.bootstrap_rewards(obs, index, gamma, "REWARDS", want_values=False)
    assert np.array_equal(bits(c.read("REWARDS")), bits(whole))
    with pytest.raises(P.binding.PPOError, match="status 1"):
        P.binding._check(P.binding.lib().ppo_bootstrap_rewards(c.h, None, None, 3, 0.5, d_r.ptr, None), c.h)
    with pytest.raises(P.binding.PPOError, match="status 1"):
        P.binding._check(P.binding.lib().ppo_bootstrap_rewards(c.h, None, None, -1, 0.5, d_r.ptr, None), c.h)
    c.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_generic_engine(P, dtype):
    """obs 6, heads (3, 2): the generic engine.  The reported values are ppo_get_value's bits (both are the engine's critic forward)."""
    N, steps, O = 50, 12, 6
    kw = dict(compute_dtype=P.DTYPE_BF16 if dtype == "bf16" else P.DTYPE_F32, seed=3)
    b, twin = pair(P, N, O, steps, **kw)
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    tr = env.rollout(steps)
    assert tr.trunc.sum() > 0 and (tr.done - tr.trunc).sum() > 0
    b.host_env_reset(obs0)
    feed(b, tr, "flags")
    idx, val = check_fold(P, b, tr)
    assert np.array_equal(bits(val), bits(twin.get_value(tr.final.reshape(steps * N, O)[idx])))
    assert np.isfinite(b.stats()["loss"])
    b.close()
    twin.close()


def test_errors(P):
    N, steps = 7, 4
    a, b = pair(P, N, 4, steps)
    dev = P.Context(P.make_config(num_envs=N, num_steps=steps, num_minibatches=1, update_epochs=1))
    trunc = np.zeros((steps, N), np.int32)
    trunc[1, 2] = trunc[2, 4] = 1
    tr = pattern_transitions(N, steps, 4, trunc)
    obs0 = np.zeros((N, 4), np.float32)

    def status(fn, *args, **kw):
        with pytest.raises(P.binding.PPOError) as e:
            fn(*args, **kw)
        return str(e.value)

    a.host_env_reset(obs0)
    feed(a, tr, "flags")   # the clean run
    b.host_env_reset(obs0)
    assert b.host_truncations()[0].size == 0   # before any rollout
    b.host_rollout_begin()
    for t in range(steps):
        b.host_act()
        if t == 1:
            bad = tr.trunc[t].copy()
            bad[0] = 1   # row 0 is not done
            assert tr.done[t, 0] == 0
            msg = status(b.host_observe, tr.obs[t], tr.rew[t], tr.done[t], truncated=bad, final_obs=tr.final[t])
            assert "status 1" in msg and "row 0" in msg, msg
            # a set flag and no final observations
            null_final = P.binding.lib().ppo_host_observe_truncated(b.h, *(x.ctypes.data_as(P.binding.C.c_void_p) for x in (
                np.ascontiguousarray(tr.obs[t]), np.ascontiguousarray(tr.rew[t]), np.ascontiguousarray(tr.done[t]))), None, None,
                np.ascontiguousarray(tr.trunc[t]).ctypes.data_as(P.binding.C.c_void_p), None)
            assert null_final == 1
        b.host_observe(tr.obs[t], tr.rew[t], tr.done[t], truncated=tr.trunc[t], final_obs=tr.final[t])   # the correct call: nothing was harmed
        if t == 1:
            assert "status 3" in status(b.host_observe, tr.obs[t], tr.rew[t], tr.done[t], truncated=tr.trunc[t], final_obs=tr.final[t])   # out of sequence
            assert b.host_truncations()[0].size == 0   # a rollout is open: the last closed one's
    b.host_rollout_end()
    assert_same_state(a, b)
    ia, va = a.host_truncations()
    ib, vb = b.host_truncations()
    assert ia.size == 2 and np.array_equal(ia, ib) and np.array_equal(bits(va), bits(vb))
    # room for fewer events than there are
    k = P.binding.C.c_int64()
    small = np.empty(1, np.int32)
    assert P.binding.lib().ppo_host_truncations(b.h, P.binding.C.byref(k), small.ctypes.data_as(P.binding.C.c_void_p), None, 1) == 1
    assert P.binding.lib().ppo_host_truncations(b.h, P.binding.C.byref(k), None, None, 0) == 0 and k.value == 2
    # a device-env context
    assert "status 3" in status(dev.host_observe, obs0, np.zeros(N), np.zeros(N), truncated=np.zeros(N), final_obs=obs0)
    assert "status 3" in status(dev.host_truncations)
    for c in (a, b, dev):
        c.close()
