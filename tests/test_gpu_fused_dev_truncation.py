"""Time-limit truncations of device-fed rollouts on the two fused 2 x 64 families (PPO_KERNEL_GAUSS_FUSED / PPO_KERNEL_CAT_FUSED): ppo_dev_observe with
truncated / final_obs (include/ppo_hip.h, "Caller-stepped environments on the device"; csrc/kernels_gauss_fused.hip: gauss_dev_fold_kernel) on the GPU.

The yardstick is the host-fed rollout of the same data on a twin context (ppo_host_observe_truncated, folded at ppo_host_rollout_end through
ppo_bootstrap_rewards' launches), and every comparison is bit equality.  The transitions are scripted here and do not depend on the actions, so both contexts
see identical data by construction.  T = 8, 2 minibatches, 2 epochs; ppo_host_rollout_end runs the update.  Before the fused families took the flags every
case here failed with status 5 (PPO_ERR_UNSUPPORTED) at the first ppo_dev_observe.
"""
import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

T = 8
BUFS = ["OBS", "ACTIONS", "LOGPROBS", "VALUES", "REWARDS", "DONES", "ADVANTAGES", "RETURNS", "NEXT_VALUE", "NEXT_OBS", "NEXT_DONE", "FIN_LEN", "FIN_REW",
        "EP_LEN", "EP_REW"]
# (N, obs, D) and (N, obs, heads, masked): obs 16 / 20 / 64 sit below, at and above 64 KB of LDS for the fold kernel (65 024 dynamic bytes at obs 20, 66 080
# with the row list); obs 1, 3 and 11 are padded with zeros to a multiple of 4; N = 70 crosses a wave and a 64-row tile, N = 300 a 256-thread workgroup
GAUSS = [(7, 3, 1), (70, 16, 2), (70, 20, 6), (300, 64, 32)]
CAT = [(70, 11, (3, 2), True), (300, 1, (2,), False), (33, 64, (5, 3, 4), False)]


@pytest.fixture(scope="module")
def P():
    return load_package()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Transitions:
    """One rollout of env outputs, [T, N, ...]: obs (already the reset observation where done), rew, done, trunc (a subset of done) and final (the
    observation the step itself produced)."""

    def __init__(self, obs, rew, done, trunc, final):
        self.obs, self.rew, self.done, self.trunc, self.final = obs, rew, done, trunc, final

    def events(self):
        return np.flatnonzero((self.trunc.ravel() != 0) & (self.done.ravel() != 0)).astype(np.int32)


class ScriptedEnv:
    """Env n, step k (1-based) of its current episode: obs[e] = f32(cos(0.29 n + 0.13 k + 0.4 e + 0.017 episode)), reward f32(0.25 + 0.02 (n % 11) - 0.01 k);
    n % 4 == 0 terminates at k == 3 + n % 3, every other env is cut off by its time limit at k == 4 + n % 4.  Nothing depends on the action."""

    def __init__(self, N, O):
        self.N, self.O = N, O
        self.n = np.arange(N)
        self.k = np.zeros(N, np.int64)
        self.ep = np.zeros(N, np.int64)

    def _obs(self):
        e = np.arange(self.O)
        return np.cos(0.29 * self.n[:, None] + 0.13 * self.k[:, None] + 0.4 * e[None, :] + 0.017 * self.ep[:, None]).astype(np.float32)

    def reset(self):
        self.k[:] = 0
        return self._obs()

    def step(self):
        self.k += 1
        final = self._obs()
        rew = (0.25 + 0.02 * (self.n % 11) - 0.01 * self.k).astype(np.float32)
        term = (self.n % 4 == 0) & (self.k == 3 + self.n % 3)
        trunc = (self.n % 4 != 0) & (self.k == 4 + self.n % 4)
        done = term | trunc
        self.k[done] = 0
        self.ep[done] += 1
        return self._obs(), rew, done.astype(np.int32), trunc.astype(np.int32), final

    def rollout(self, steps=T):
        s = [self.step() for _ in range(steps)]
        return Transitions(*(np.stack([x[i] for x in s]) for i in range(5)))


def pattern_transitions(N, O, trunc, seed=3):
    """Random transitions whose episodes end exactly where `trunc` [T, N] says, all by truncation, plus one plain termination where no event sits"""
    rng = np.random.default_rng(seed)
    trunc = np.asarray(trunc, np.int32)
    done = trunc.copy()
    done[tuple(np.argwhere(trunc == 0)[0])] = 1
    return Transitions(rng.standard_normal((T, N, O)).astype(np.float32), rng.uniform(-1, 1, (T, N)).astype(np.float32), done, trunc,
                       rng.standard_normal((T, N, O)).astype(np.float32))


def make(P, N, O, D=None, heads=None, masked=False):
    kw = dict(env_kind=P.ENV_HOST, obs_size=O, num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2, seed=5, total_timesteps=N * T * 5)
    if D is not None:
        kw.update(dist_kind=P.DIST_GAUSSIAN, head_dims=(D,), kernel_flags=P.KERNEL_GAUSS_FUSED)
    else:
        kw.update(dist_kind=P.DIST_MASKED if masked else P.DIST_CATEGORICAL, head_dims=tuple(heads), kernel_flags=P.KERNEL_CAT_FUSED)
    return P.Context(P.make_config(**kw))


def group(P, n, *args, **kw):
    """n contexts of one shape with the same parameters"""
    ctxs = [make(P, *args, **kw) for _ in range(n)]
    ctxs[0].init_orthogonal(11)
    for c in ctxs[1:]:
        c.set_params(ctxs[0].get_params())
    return ctxs


def is_gauss(P, ctx):
    return ctx.cfg.dist_kind == P.DIST_GAUSSIAN


def make_masks(ctx, seed=17):
    """[T, N, A] for a masked context (actions disabled, never a whole head), None otherwise"""
    rng = np.random.default_rng(seed)
    masks = (rng.random((T, ctx.N, ctx.A)) < 0.6).astype(np.uint8)
    off = 0
    for h in range(ctx.H):
        dim = ctx.cfg.head_dims[h]
        masks[:, np.arange(ctx.N), off + np.arange(ctx.N) % dim] = 1
        off += dim
    assert (masks == 0).any()
    return masks


def host_feed(P, ctx, tr, flags=True, masks=None):
    """One host-fed iteration; returns the actions [T, N, .]"""
    acts = []
    ctx.host_rollout_begin()
    for t in range(T):
        acts.append(ctx.host_act_f32() if is_gauss(P, ctx) else ctx.host_act(None if masks is None else masks[t]))
        kw = dict(truncated=tr.trunc[t], final_obs=tr.final[t]) if flags else {}
        ctx.host_observe(tr.obs[t], tr.rew[t], tr.done[t], **kw)
    ctx.host_rollout_end()
    return np.stack(acts)


class DevArrays:
    """The caller's device arrays of one env step, allocated once and refilled"""

    def __init__(self, P, ctx):
        N, O = ctx.N, ctx.O
        self.obs, self.final = ctx.empty((N, O), np.float32), ctx.empty((N, O), np.float32)
        self.rew, self.done, self.trunc = ctx.empty(N, np.float32), ctx.empty(N, np.int32), ctx.empty(N, np.int32)
        self.act = ctx.empty((N, ctx.A), np.float32) if is_gauss(P, ctx) else ctx.empty((N, ctx.H), np.int64)
        self.mask = ctx.empty((N, ctx.A), np.uint8)


def dev_steps(P, ctx, d, tr, steps, flags=True, masks=None):
    acts = []
    for t in steps:
        if is_gauss(P, ctx):
            ctx.dev_act_f32(d.act)
        else:
            if masks is not None:
                d.mask.upload(masks[t])
            ctx.dev_act(d.act, mask=d.mask if masks is not None else None)
        acts.append(d.act.download())
        d.obs.upload(tr.obs[t]); d.rew.upload(tr.rew[t]); d.done.upload(tr.done[t])
        kw = {}
        if flags:
            d.trunc.upload(tr.trunc[t]); d.final.upload(tr.final[t])
            kw.update(truncated=d.trunc, final_obs=d.final)
        ctx.dev_observe(d.obs, d.rew, d.done, **kw)
    return acts


def dev_feed(P, ctx, d, tr, flags=True, masks=None):
    ctx.host_rollout_begin()
    acts = dev_steps(P, ctx, d, tr, range(T), flags, masks)
    ctx.host_rollout_end()
    return np.stack(acts)


def assert_same_state(P, a, b, tag=""):
    """every rollout buffer, ADVANTAGES and RETURNS, the parameters, both AdamW moments, the statistics, and the truncation events"""
    for name in BUFS + ([] if is_gauss(P, a) else ["MASKS"]):
        x, y = a.read(name), b.read(name)
        assert np.array_equal(bits(x), bits(y)), (tag, name, int((bits(x) != bits(y)).sum()))
    assert np.array_equal(bits(a.get_params()), bits(b.get_params())), (tag, "PARAMS")
    ma, va, sa = a.get_optimizer()
    mb, vb, sb = b.get_optimizer()
    assert sa == sb and np.array_equal(bits(ma), bits(mb)) and np.array_equal(bits(va), bits(vb)), (tag, "AdamW")
    st_a, st_b = a.stats(), b.stats()
    for k in st_a:
        assert np.array_equal(np.float64(st_a[k]).view(np.uint64), np.float64(st_b[k]).view(np.uint64)), (tag, k, st_a[k], st_b[k])
    ia, va = a.host_truncations()
    ib, vb = b.host_truncations()
    assert ib.dtype == np.int32 and np.array_equal(ia, ib) and (np.diff(ib) > 0).all(), (tag, ia.size, ib.size)
    assert np.array_equal(bits(va), bits(vb)), (tag, "event values")
    return st_a, ib, vb


def run_pair(P, tr, obs0, *shape, dev_tr=None, prepare=None, **kw):
    """Host-fed a and device-fed b (on dev_tr, default tr) from the same parameters, one iteration each, compared; w keeps the parameters the rollout ran with.
    Returns (b, w, event indices, event values)."""
    a, b, w = group(P, 3, *shape, **kw)
    for c in (a, b, w):
        if prepare:
            prepare(c)
    masks = make_masks(a) if kw.get("masked") else None
    a.host_env_reset(obs0)
    act_a = host_feed(P, a, tr, masks=masks)
    d = DevArrays(P, b)
    b.dev_env_reset(b.dev(obs0))
    act_b = dev_feed(P, b, d, dev_tr if dev_tr is not None else tr, masks=masks)
    assert act_a.dtype == act_b.dtype and np.array_equal(bits(act_a), bits(act_b))
    st, idx, val = assert_same_state(P, a, b, tag=shape)
    assert st["updates"] == 1 and np.isfinite(st["loss"])
    assert np.array_equal(idx, tr.events())
    a.close()
    return b, w, idx, val


def scripted(N, O):
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    tr = env.rollout()
    assert tr.trunc.sum() > 0 and (tr.done - tr.trunc).sum() > 0   # at least one truncation and at least one plain termination
    return env, obs0, tr


def check_events(P, b, w, tr, idx, val):
    """every event against the public calls: v = ppo_get_value of the final observation under the parameters of the rollout (w's: b's were updated by
    ppo_host_rollout_end), REWARDS at the events f32(r + f32(gamma v)) in float32 numpy, REWARDS elsewhere untouched"""
    N, O = b.N, b.O
    assert val.shape == idx.shape and np.isfinite(val).all()
    if idx.size:
        assert np.array_equal(bits(val), bits(w.get_value(tr.final.reshape(T * N, O)[idx])))
    expect = tr.rew.ravel().copy()
    expect[idx] = (expect[idx] + (np.float32(b.cfg.gamma) * val).astype(np.float32)).astype(np.float32)
    rew = b.read("REWARDS")
    assert np.array_equal(bits(rew), bits(expect)), int((bits(rew) != bits(expect)).sum())
    if idx.size:
        assert (bits(rew[idx]) != bits(tr.rew.ravel()[idx])).any()


# ---- 1 and 2. device-fed against host-fed, and every event against the public calls
@pytest.mark.parametrize("N,O,D", GAUSS)
def test_gaussian_device_fed_equals_host_fed(P, N, O, D):
    _, obs0, tr = scripted(N, O)
    b, w, idx, val = run_pair(P, tr, obs0, N, O, D)
    assert idx.size == int(tr.trunc.sum()) > 0
    check_events(P, b, w, tr, idx, val)
    b.close()
    w.close()


@pytest.mark.parametrize("N,O,heads,masked", CAT)
def test_categorical_device_fed_equals_host_fed(P, N, O, heads, masked):
    _, obs0, tr = scripted(N, O)
    b, w, idx, val = run_pair(P, tr, obs0, N, O, heads=heads, masked=masked)
    assert idx.size == int(tr.trunc.sum()) > 0
    check_events(P, b, w, tr, idx, val)
    if masked:
        assert np.array_equal(b.read("MASKS", (T, N, b.A)), make_masks(b))
    b.close()
    w.close()


# ---- 3. hand-built flag patterns
def test_hand_built_flag_patterns(P):
    """N = 300, obs 17, D 2.  Step 1: every row (workgroup 0 holds 256 flagged rows = four full tiles, workgroup 1 holds 44 = a partial tile); step 2: none;
    step 3: rows 0 .. 64 (a full tile and one row); step 5: rows 255 and 256 only (two workgroups, two atomics, either order); step T - 1: row 0."""
    N, O = 300, 17
    trunc = np.zeros((T, N), np.int32)
    trunc[1, :] = 1
    trunc[3, :65] = 1
    trunc[5, [255, 256]] = 1
    trunc[T - 1, 0] = 1
    tr = pattern_transitions(N, O, trunc)
    assert not tr.trunc[2].any() and tr.done[0].sum() == 1 and not tr.trunc[0].any()   # a termination where no event sits
    b, w, idx, val = run_pair(P, tr, np.zeros((N, O), np.float32), N, O, 2)
    assert idx.size == N + 65 + 2 + 1
    assert list(idx[N + 65:N + 67]) == [5 * N + 255, 5 * N + 256] and idx[-1] == (T - 1) * N
    check_events(P, b, w, tr, idx, val)
    b.close()
    w.close()


# ---- 4. rows flagged truncated with done == 0
def test_flag_without_done_is_ignored(P):
    N, O, D = 70, 17, 6
    _, obs0, tr = scripted(N, O)
    rng = np.random.default_rng(23)
    stray = (rng.random((T, N)) < 0.3) & (tr.done == 0)
    assert stray.sum() > 20
    final = tr.final.copy()
    final[~((tr.trunc != 0) & (tr.done != 0))] = np.nan   # rows that are not (truncated and done) are never read
    noisy = Transitions(tr.obs, tr.rew, tr.done, (tr.trunc | stray).astype(np.int32), final)
    b, w, idx, val = run_pair(P, tr, obs0, N, O, D, dev_tr=noisy)   # the host-fed twin runs without the stray flags
    check_events(P, b, w, tr, idx, val)
    rew = b.read("REWARDS")
    assert np.array_equal(bits(rew[stray.ravel()]), bits(tr.rew.ravel()[stray.ravel()]))   # the reward is untouched there
    for name in ("REWARDS", "ADVANTAGES", "RETURNS", "VALUES"):
        assert np.isfinite(b.read(name)).all(), name
    assert np.isfinite(b.get_params()).all() and np.isfinite(val).all()
    b.close()
    w.close()


# ---- 5. two rollouts back to back: the alternating lists; and the launch counter
@pytest.mark.parametrize("kind", ["gauss", "cat"])
def test_truncations_of_the_closed_rollout_while_the_next_is_open(P, kind):
    N, O = 70, 17
    a, b = group(P, 2, N, O, 6) if kind == "gauss" else group(P, 2, N, O, heads=(5, 3, 4))
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    tr1, tr2, tr3 = env.rollout(), env.rollout(), env.rollout()
    a.host_env_reset(obs0)
    d = DevArrays(P, b)
    b.dev_env_reset(b.dev(obs0))
    assert b.host_truncations()[0].size == 0   # before any rollout
    host_feed(P, a, tr1)
    i1, v1 = a.host_truncations()
    before = b.gauss_fused_launches()[1]
    dev_feed(P, b, d, tr1)
    # the value counter: one fold launch per dev_observe that passed flags, and the two critic launches of host_rollout_end
    assert b.gauss_fused_launches()[1] - before == T + 2
    host_feed(P, a, tr2)
    i2, v2 = a.host_truncations()
    assert i1.size > 0 and i2.size > 0 and not np.array_equal(i1, i2)
    b.host_rollout_begin()
    half = T // 2
    dev_steps(P, b, d, tr2, range(half))
    assert tr2.trunc[:half].any()
    ib, vb = b.host_truncations()   # the second rollout is open and has folded events: still the first rollout's
    assert np.array_equal(ib, i1) and np.array_equal(bits(vb), bits(v1))
    dev_steps(P, b, d, tr2, range(half, T))
    b.host_rollout_end()
    ib, vb = b.host_truncations()
    assert np.array_equal(ib, i2) and np.array_equal(bits(vb), bits(v2))
    assert_same_state(P, a, b, tag="second")
    # a third rollout without flags: no event, no fold launch, and the list of the second is no longer reported
    host_feed(P, a, tr3, flags=False)
    before = b.gauss_fused_launches()[1]
    dev_feed(P, b, d, tr3, flags=False)
    assert b.gauss_fused_launches()[1] - before == 2
    assert b.host_truncations()[0].size == 0 and a.host_truncations()[0].size == 0
    assert_same_state(P, a, b, tag="third")
    a.close()
    b.close()


# ---- 6. with the normalisations
def test_with_observation_and_reward_normalisation(P):
    """Obs-norm with frozen statistics (mode 2: the host feed normalises the final observations at the rollout's end, the device feed per step, and frozen
    statistics make the two alike) and reward-norm in mode 1 (the fold adds gamma * V to the normalised reward on both feeds)."""
    N, O, D = 70, 17, 6
    _, obs0, tr = scripted(N, O)
    rng = np.random.default_rng(31)
    mean, var = rng.uniform(-0.3, 0.3, O), rng.uniform(0.2, 1.5, O)

    def prepare(c):
        c.obs_norm_set(mean, var, 1000.0)
        c.obs_norm_enable(2)
        c.reward_norm_enable(1)

    b, w, idx, val = run_pair(P, tr, obs0, N, O, D, prepare=prepare)
    assert idx.size == int(tr.trunc.sum()) > 0
    # the folded value is the critic's on the NORMALISED final observation
    final_n = w.obs_norm_apply(tr.final.reshape(T * N, O)[idx])
    assert np.array_equal(bits(val), bits(w.get_value(final_n)))
    raw = tr.rew.ravel()
    rew = b.read("REWARDS")
    assert not np.array_equal(bits(rew), bits(raw))   # the rewards were normalised
    b.close()
    w.close()
