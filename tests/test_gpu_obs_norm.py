"""Observation normalisation of caller-stepped environments (include/ppo_hip.h, "Observation normalisation": ppo_obs_norm_*) on the GPU.

The oracle is a numpy f64 model of the header's semantics (Model below): Chan's merge of every batch -- the reset observations, then each step's
next_obs -- and y = f32(clamp((x - mean) / sqrt(var + eps), +-clip)) with the statistics as just updated.  The reference project has no normaliser.
The envs are scripted (tests/test_host_truncation_abi.py: ScriptedEnv), their observations scaled per column by 10^(e % 5) and shifted by 100 e, so
the columns differ in scale by four orders of magnitude.

Bounds.  Statistics: |mean - want| <= 1e-12 max|x| and |var - want| <= 1e-12 max|x|^2 per column; an f64 sum of N terms in any order is off by at most
about (N + 4) 2^-53 of the largest partial sum, times the merges of a run (13 here), times the scale: under 1e-13 at these sizes.  Outputs: one f32
ulp of the model's y -- the model rounds the same f64 expression, so a difference can only come from the last bits of the f64 sums.
"""
import numpy as np
import pytest

from __graft_entry__ import load_package
from test_gpu_dev_env import DevArrays, assert_untouched, dev_feed, host_feed, snapshot
from test_gpu_host_env import assert_same_state, bits
from test_gpu_host_truncation import check_fold, make, pair, pattern_transitions
from test_host_truncation_abi import ScriptedEnv, Transitions

pytestmark = pytest.mark.gpu

T = 6
CLIP, EPS = 10.0, 1e-8


@pytest.fixture(scope="module")
def P():
    return load_package()


class Model:
    """The header's semantics in numpy f64.  eps and clip pass through the ABI as floats."""

    def __init__(self, O, clip=CLIP, eps=EPS):
        self.mean, self.var, self.count = np.zeros(O), np.ones(O), 0.0
        self.clip, self.eps = float(np.float32(clip)), float(np.float32(eps))

    def update(self, x):
        x = np.asarray(x, np.float64)
        n = float(x.shape[0])
        bm = x.sum(axis=0) / n
        bm2 = ((x - bm) ** 2).sum(axis=0)
        tot = self.count + n
        delta = bm - self.mean
        self.mean = self.mean + delta * n / tot
        self.var = (self.var * self.count + bm2 + delta * delta * self.count * n / tot) / tot
        self.count = tot

    def apply(self, x):
        y = (np.asarray(x, np.float64) - self.mean) / np.sqrt(self.var + self.eps)
        return np.clip(y, -self.clip, self.clip).astype(np.float32)

    def fold(self, x):
        self.update(x)
        return self.apply(x)


def scaled(x):
    """columns scaled by 10^(e % 5) and shifted by 100 e, rounded to f32 once"""
    e = np.arange(x.shape[-1])
    return (np.asarray(x, np.float64) * 10.0 ** (e % 5) + 100.0 * e).astype(np.float32)


def scaled_transitions(tr):
    return Transitions(scaled(tr.obs), tr.rew, tr.done, tr.trunc, scaled(tr.final))


def within_one_ulp(got, want, tag):
    got, want = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bad = err > np.spacing(np.abs(want)).astype(np.float64)
    assert not bad.any(), (tag, int(bad.sum()), float(err.max()))


def check_stats(ctx, model, top, count, tag):
    mean, var, cnt = ctx.obs_norm_get()
    em, ev = np.abs(mean - model.mean), np.abs(var - model.var)
    print(tag, "mean err / max|x|: %.3g   var err / max|x|^2: %.3g" % ((em / top).max(), (ev / top ** 2).max()))
    assert (em <= 1e-12 * top).all(), (tag, "mean", (em / top).max())
    assert (ev <= 1e-12 * top ** 2).all(), (tag, "var", (ev / top ** 2).max())
    assert cnt == count == model.count, (tag, cnt, count)


SHAPES = [("7x4", 7, 4, {}), ("33x2", 33, 2, {}), ("70x8", 70, 8, {}), ("300x4", 300, 4, {}),
          ("generic_f32", 50, 6, dict(seed=3)), ("generic_bf16", 50, 6, dict(seed=3, bf16=True)),
          ("wide_33x67", 33, 67, dict(hidden=32, n_hidden=1))]


def make_kw(P, kw):
    kw = dict(kw)
    if kw.pop("bf16", False):
        kw["compute_dtype"] = P.DTYPE_BF16
    return kw


# ---- 1. statistics and outputs against numpy
@pytest.mark.parametrize("name,N,O,kw", SHAPES, ids=[s[0] for s in SHAPES])
def test_statistics_and_outputs_against_numpy(P, name, N, O, kw):
    """N = 7 is below any row split, 70 crosses a wave, 300 a 256-thread workgroup; O = 67 crosses the 16-column blocks and is no multiple of 4"""
    ctx = make(P, N, O, T, **make_kw(P, kw))
    ctx.init_orthogonal(11)
    ctx.obs_norm_enable()
    env = ScriptedEnv(N, O)
    model = Model(O)
    obs0 = scaled(env.reset())
    top = np.abs(obs0).max(axis=0).astype(np.float64)
    ctx.host_env_reset(obs0)
    last = model.fold(obs0)
    within_one_ulp(ctx.read("NEXT_OBS"), last, (name, "reset"))
    spike = (2, min(3, N - 1), 1)
    for it in range(2):
        tr = scaled_transitions(env.rollout(T))
        if it == 0:
            tr.obs[spike] *= np.float32(1e6)   # far beyond fp16: the clip is seen to act
            assert abs(tr.obs[spike]) > 1e6
        top = np.maximum(top, np.abs(tr.obs).max(axis=(0, 1)))
        host_feed(ctx, tr)
        want = [last]
        for t in range(T):
            want.append(model.fold(tr.obs[t]))
        last = want[-1]
        check_stats(ctx, model, top, (1 + (it + 1) * T) * N, (name, it))
        got = ctx.read("OBS", (T, N, O))
        within_one_ulp(got, np.stack(want[:-1]), (name, it, "OBS"))
        within_one_ulp(ctx.read("NEXT_OBS"), last, (name, it, "NEXT_OBS"))
        assert np.abs(got).max() <= model.clip
        if it == 0 and 4 * N >= 128:
            # (one outlier among n rows has a z-score of at most (n - 1) / sqrt(n), under 10 for n < 102: at N = 7 the clip cannot act, the spike is
            # merely normalised; there the point is the statistics read below)
            assert abs(want[spike[0] + 1][spike[1], spike[2]]) == model.clip and abs(got[spike[0] + 1, spike[1], spike[2]]) == model.clip
        st = ctx.stats()   # ppo_read_stats returns OK: no observation left the fp16 range
        assert np.isfinite(st["loss"]) and st["updates"] == it + 1
    ctx.close()


def test_the_same_data_without_normalisation_hits_the_fp16_limit(P):
    """what the feature buys: the raw spike in PPO_BUF_OBS raises the sticky error word of the matrix-core update (ppo_hip.h, "fp16 ranges")"""
    N, O = 7, 4
    ctx = make(P, N, O, T)
    ctx.init_orthogonal(11)
    env = ScriptedEnv(N, O)
    ctx.host_env_reset(scaled(env.reset()))
    tr = scaled_transitions(env.rollout(T))
    tr.obs[2, 3, 1] *= np.float32(1e6)
    host_feed(ctx, tr)
    with pytest.raises(P.binding.PPOError, match="status 3"):
        ctx.stats()
    ctx.close()


# ---- 2. device-fed equals host-fed, statistics included
def norm_bits(ctx):
    mean, var, count = ctx.obs_norm_get()
    return mean.view(np.uint64), var.view(np.uint64), count


def assert_same_norm(a, b, tag=""):
    (ma, va, ca), (mb, vb, cb) = norm_bits(a), norm_bits(b)
    assert np.array_equal(ma, mb) and np.array_equal(va, vb) and ca == cb, (tag, "statistics")


def random_masks(rng, ctx, steps, it):
    """disable actions, never a whole head"""
    N = ctx.N
    masks = (rng.random((steps, N, ctx.A)) < 0.6).astype(np.uint8)
    off = 0
    for h in range(ctx.H):
        dim = ctx.cfg.head_dims[h]
        masks[:, np.arange(N), off + (np.arange(N) + it) % dim] = 1
        off += dim
    return masks


DEV_CASES = [("33x4", 33, 4, T, {}), ("70x8", 70, 8, T, {}), ("generic_f32", 50, 6, 12, dict(seed=3)), ("generic_bf16", 50, 6, 12, dict(seed=3, bf16=True)),
             ("masked_multihead", 33, 4, T, dict(head_dims=(3, 2), masked=True))]


@pytest.mark.parametrize("name,N,O,steps,kw", DEV_CASES, ids=[c[0] for c in DEV_CASES])
def test_device_fed_equals_host_fed(P, name, N, O, steps, kw):
    kw = make_kw(P, kw)
    masked = kw.pop("masked", False)
    if masked:
        kw["dist_kind"] = P.DIST_MASKED
    a, b = pair(P, N, O, steps, **kw)
    a.obs_norm_enable()
    b.obs_norm_enable()
    env = ScriptedEnv(N, O)
    obs0 = scaled(env.reset())
    a.host_env_reset(obs0)
    d = DevArrays(b)
    b.dev_env_reset(b.dev(obs0))
    rng = np.random.default_rng(17)
    for it in range(2):
        tr = scaled_transitions(env.rollout(steps))
        masks = random_masks(rng, b, steps, it) if masked else None
        fin = it == 1
        act_a = host_feed(a, tr, fin=fin, masks=masks)
        act_b = dev_feed(b, d, tr, fin=fin, masks=masks)
        assert np.array_equal(act_a, act_b), (it, int((act_a != act_b).sum()))
        st = assert_same_state(a, b, tag=(name, it))
        assert_same_norm(a, b, (name, it))
    assert st["updates"] == 2 and a.obs_norm_get()[2] == (1 + 2 * steps) * N
    assert np.abs(a.read("OBS")).max() <= CLIP
    a.close()
    b.close()


# ---- 3. determinism
@pytest.mark.parametrize("N,O,kw", [(300, 4, {}), (33, 67, dict(hidden=32, n_hidden=1))], ids=["300x4", "33x67"])
def test_the_same_feed_twice_gives_the_same_bits(P, N, O, kw):
    a, b = pair(P, N, O, T, **kw)
    outs = []
    for c in (a, b):
        c.obs_norm_enable()
        env = ScriptedEnv(N, O)
        d = DevArrays(c)
        c.dev_env_reset(c.dev(scaled(env.reset())))
        outs.append([dev_feed(c, d, scaled_transitions(env.rollout(T))) for _ in range(2)])
    assert np.array_equal(np.stack(outs[0]), np.stack(outs[1]))
    assert_same_state(a, b)
    assert_same_norm(a, b)
    a.close()
    b.close()


# ---- 4. modes, the checkpoint round trip, the stand-alone apply
def test_modes(P):
    N, O = 33, 4
    ctx = make(P, N, O, T)
    ctx.init_orthogonal(11)
    ctx.obs_norm_enable(1)
    env = ScriptedEnv(N, O)
    model = Model(O)
    obs0 = scaled(env.reset())
    ctx.host_env_reset(obs0)
    model.update(obs0)
    tr1 = scaled_transitions(env.rollout(T))
    host_feed(ctx, tr1)
    for t in range(T):
        model.update(tr1.obs[t])
    frozen = norm_bits(ctx)
    # mode 2: the statistics stay, bit for bit, and the outputs follow them
    ctx.obs_norm_enable(2)
    tr2 = scaled_transitions(env.rollout(T))
    host_feed(ctx, tr2)
    after = norm_bits(ctx)
    assert np.array_equal(frozen[0], after[0]) and np.array_equal(frozen[1], after[1]) and frozen[2] == after[2] == (1 + T) * N
    within_one_ulp(ctx.read("OBS", (T, N, O))[1:], model.apply(tr2.obs[:-1]), "mode 2 OBS")
    within_one_ulp(ctx.read("NEXT_OBS"), model.apply(tr2.obs[-1]), "mode 2 NEXT_OBS")
    # the stand-alone apply on the raw observations with the final statistics: a host array, a device array in place, a device array into another
    raw = tr2.obs.reshape(T * N, O)
    want = model.apply(raw)
    within_one_ulp(ctx.obs_norm_apply(raw), want, "apply, host array")
    d_in, d_out = ctx.dev(raw), ctx.empty((T * N, O), np.float32)
    assert ctx.obs_norm_apply(d_in, out=d_out) is d_out
    ctx.sync()
    separate = d_out.download()
    assert np.array_equal(bits(d_in.download()), bits(raw))
    ctx.obs_norm_apply(d_in)   # out aliases obs
    ctx.sync()
    within_one_ulp(separate, want, "apply, device array")
    assert np.array_equal(bits(d_in.download()), bits(separate))
    after = norm_bits(ctx)
    assert np.array_equal(frozen[0], after[0]) and np.array_equal(frozen[1], after[1]) and frozen[2] == after[2]
    # mode 0: raw observations again (the statistics are kept)
    ctx.obs_norm_enable(0)
    tr3 = env.rollout(T)   # unit scale
    host_feed(ctx, tr3)
    assert np.array_equal(bits(ctx.read("OBS", (T, N, O))[1:]), bits(tr3.obs[:-1])) and np.array_equal(bits(ctx.read("NEXT_OBS", (N, O))), bits(tr3.obs[-1]))
    after = norm_bits(ctx)
    assert np.array_equal(frozen[0], after[0]) and np.array_equal(frozen[1], after[1]) and frozen[2] == after[2]
    ctx.close()


def test_set_get_round_trip_reproduces_a_context(P):
    """the checkpoint round trip: statistics of a trained context, set on two fresh ones -- on the second through get of the first"""
    N, O = 33, 4
    src = make(P, N, O, T)
    src.init_orthogonal(11)
    src.obs_norm_enable()
    env = ScriptedEnv(N, O)
    src.host_env_reset(scaled(env.reset()))
    host_feed(src, scaled_transitions(env.rollout(T)))
    mean, var, count = src.obs_norm_get()
    assert count == (1 + T) * N and (var > 1e-3).all()
    a, b = pair(P, N, O, T)
    assert a.obs_norm_get()[2] == 0 and (a.obs_norm_get()[1] == 1).all()   # before anything is enabled or set
    a.obs_norm_set(mean, var, count)
    got = a.obs_norm_get()
    assert np.array_equal(got[0].view(np.uint64), mean.view(np.uint64)) and np.array_equal(got[1].view(np.uint64), var.view(np.uint64)) and got[2] == count
    b.obs_norm_set(*got)
    obs0 = scaled(env.reset())
    tr = scaled_transitions(env.rollout(T))
    for c in (a, b):
        c.obs_norm_enable()
        c.host_env_reset(obs0)
        host_feed(c, tr)
    assert_same_state(a, b)
    assert_same_norm(a, b)
    assert a.obs_norm_get()[2] == count + (1 + T) * N
    for c in (src, a, b):
        c.close()


# ---- 5. truncations
def trunc_pattern(N):
    trunc = np.zeros((T, N), np.int32)
    trunc[1, :] = 1                   # every row
    trunc[3, [63, 64, 69]] = 1        # both sides of a wave's edge and the last row; step 2 has none
    trunc[T - 1, 0] = 1
    return trunc


@pytest.mark.parametrize("O", [4, 8])
def test_truncations(P, O):
    """Device-fed: a final observation is normalised by the statistics right behind its own step's update.  Host-fed: by those at the end of the rollout."""
    N = 70
    tr = scaled_transitions(pattern_transitions(N, T, O, trunc_pattern(N)))
    obs0 = scaled(np.zeros((N, O), np.float32))
    a, twin = pair(P, N, O, T)          # host-fed; the twin keeps the parameters the rollouts ran with
    b, c = pair(P, N, O, T)             # device-fed, and device-fed with NaN in the rows that are never read
    for x in (a, b, c):
        x.obs_norm_enable()
    a.host_env_reset(obs0)
    host_feed(a, tr, mode="flags")
    db, dc = DevArrays(b), DevArrays(c)
    b.dev_env_reset(b.dev(obs0))
    c.dev_env_reset(c.dev(obs0))
    dev_feed(b, db, tr, mode="flags")
    final = tr.final.copy()
    final[tr.trunc == 0] = np.nan
    dev_feed(c, dc, Transitions(tr.obs, tr.rew, tr.done, tr.trunc, final), mode="flags")
    ia, va = check_fold(P, a, tr)
    ib, vb = check_fold(P, b, tr)
    assert ia.size == N + 4 and np.array_equal(ia, ib)
    rows = tr.final.reshape(T * N, O)[ia]

    def critic(obs):
        """the fold's own critic launch on the twin (ppo_bootstrap_rewards), on a scratch reward array"""
        k = obs.shape[0]
        return twin.bootstrap_rewards(obs, np.arange(k), 0.5, twin.dev(np.zeros(k, np.float32)))

    # host-fed: the end-of-rollout statistics, replayed on the twin bit for bit
    twin.obs_norm_set(*a.obs_norm_get())
    assert np.array_equal(bits(va), bits(critic(twin.obs_norm_apply(rows))))
    # device-fed: the statistics after each step, from the numpy model (so: the project's bar for values, 3e-6 -- DESIGN section 0, rows a7-a10)
    model = Model(O)
    model.update(obs0)
    want = np.empty(ib.size, np.float32)
    for t in range(T):
        model.update(tr.obs[t])
        k = np.flatnonzero(ib // N == t)
        if k.size:
            twin.obs_norm_set(model.mean, model.var, model.count)
            want[k] = critic(twin.obs_norm_apply(rows[k]))
    err = np.abs(vb - want).max()
    print("device-fed fold against the model's per-step statistics: %.3g" % err)
    assert err <= 3e-6, err
    assert np.abs(va - vb).max() > 1e-4   # the documented difference between the two feeds
    # rows never read
    assert_same_state(b, c, tag="NaN rows")
    ic, vc = c.host_truncations()
    assert np.array_equal(ib, ic) and np.array_equal(bits(vb), bits(vc))
    assert_same_norm(b, c)
    assert_same_norm(a, b)   # the statistics themselves do not depend on the feed
    for x in (a, twin, b, c):
        x.close()


# ---- 6. errors, each leaving the state untouched
def test_errors(P):
    N, O = 7, 4
    a = make(P, N, O, T)
    a.init_orthogonal(11)
    cart = P.Context(P.make_config(num_envs=N, num_steps=T, num_minibatches=1, update_epochs=1))
    cart.env_reset()
    env = ScriptedEnv(N, O)
    L, C = P.binding.lib(), P.binding.C

    def status(ctx, fn, *args, **kw):
        before = snapshot(ctx)
        norm = norm_bits(ctx) if ctx is a and not a.host_open else None
        with pytest.raises(P.binding.PPOError) as e:
            fn(*args, **kw)
        assert_untouched(ctx, before, fn.__name__)
        if norm is not None:
            now = norm_bits(ctx)
            assert np.array_equal(norm[0], now[0]) and np.array_equal(norm[1], now[1]) and norm[2] == now[2]
        return str(e.value)

    a.host_open = False
    assert "status 5" in status(cart, cart.obs_norm_enable)               # a device-env context
    assert "status 1" in status(a, a.obs_norm_enable, 1, 0.0)             # clip = 0
    assert "status 1" in status(a, a.obs_norm_enable, 1, 10.0, 0.0)       # eps = 0
    assert "status 1" in status(a, a.obs_norm_enable, 3)
    a.obs_norm_enable()
    a.host_env_reset(scaled(env.reset()))
    msg = status(a, a.host_rollout_begin, 2)
    assert "status 5" in msg and "group" in msg, msg
    assert "status 5" in status(a, a.comm_init_local, 77, 0, 2)
    # get / set with a wrong O
    buf = np.zeros(2 * (O + 1))
    cnt = C.c_double()
    before, norm = snapshot(a), norm_bits(a)
    assert L.ppo_obs_norm_get_h(a.h, buf.ctypes.data_as(C.c_void_p), buf[O + 1:].ctypes.data_as(C.c_void_p), C.c_int64(O + 1), C.byref(cnt)) == 1
    assert L.ppo_obs_norm_set_h(a.h, buf.ctypes.data_as(C.c_void_p), buf[O + 1:].ctypes.data_as(C.c_void_p), C.c_int64(O + 1), C.c_double(5.0)) == 1
    assert_untouched(a, before, "wrong O")
    now = norm_bits(a)
    assert np.array_equal(norm[0], now[0]) and np.array_equal(norm[1], now[1]) and norm[2] == now[2] == N
    # inside an open rollout
    tr = scaled_transitions(env.rollout(T))
    a.host_rollout_begin()
    a.host_open = True
    a.host_act()
    assert "status 3" in status(a, a.obs_norm_enable, 0)
    assert "status 3" in status(a, a.obs_norm_get)
    assert "status 3" in status(a, a.obs_norm_set, np.zeros(O), np.ones(O), 0)
    y = a.obs_norm_apply(tr.obs[0])   # apply works inside a rollout
    assert y.shape == (N, O) and np.abs(y).max() <= CLIP
    a.host_observe(tr.obs[0], tr.rew[0], tr.done[0])
    for t in range(1, T):
        a.host_act()
        a.host_observe(tr.obs[t], tr.rew[t], tr.done[t])
    a.host_rollout_end()
    assert a.obs_norm_get()[2] == (1 + T) * N and np.isfinite(a.stats()["loss"])
    a.close()
    cart.close()


# ---- 7. off means off
def test_off_means_off(P):
    """enable never called and enable(0) called: identical bits over two iterations, host-fed and device-fed"""
    N, O = 33, 4
    a, b = pair(P, N, O, T)
    c, d = pair(P, N, O, T)
    c.set_params(a.get_params())
    d.set_params(a.get_params())
    b.obs_norm_enable(0)
    d.obs_norm_enable(0)
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    a.host_env_reset(obs0)
    b.host_env_reset(obs0)
    dc, dd = DevArrays(c), DevArrays(d)
    c.dev_env_reset(c.dev(obs0))
    d.dev_env_reset(d.dev(obs0))
    for it in range(2):
        tr = env.rollout(T)
        host_feed(a, tr, mode="flags")
        host_feed(b, tr, mode="flags")
        dev_feed(c, dc, tr, mode="flags")
        dev_feed(d, dd, tr, mode="flags")
        for other in (b, c, d):
            assert_same_state(a, other, tag=it)
        assert np.array_equal(bits(a.read("OBS", (T, N, O))[1:]), bits(tr.obs[:-1]))   # raw
    assert b.obs_norm_get()[2] == 0
    for x in (a, b, c, d):
        x.close()
