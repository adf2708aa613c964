"""Reward normalisation of caller-stepped environments (include/ppo_hip.h, "Reward normalisation": ppo_reward_norm_*) on the GPU.

The oracle is a numpy f64 model of the header's semantics (Model below): per committed step R = ret * gamma + r, Chan's merge of the N values of R,
ret = done ? 0 : R, and y = f32(clamp(r / sqrt(var + eps), +-clip)) with the variance as just updated.  The reference project has no normaliser.
The envs are scripted (tests/test_host_truncation_abi.py: ScriptedEnv), their rewards scaled by 1000 -- a score in thousands -- and, in the first
iteration, one entry (step 2) multiplied by 1e6.

Bounds.  Statistics: |mean - want| <= 1e-12 max|R| and |var - want| <= 1e-12 max|R|^2, the bounds derived in tests/test_gpu_obs_norm.py: an f64 sum of
N terms in any order is off by at most about (N + 4) 2^-53 of the largest partial sum, times the merges of a run (12 here), times the scale: under
1e-13 at these sizes.  ret: the same bound as the mean (one product and one sum per step, chained over at most 12 steps).  Outputs: one f32 ulp of the
model's y -- the model rounds the same f64 expression, so a difference can only come from the last bits of the f64 sums.

Why a small N cannot clip: the spike sits in step 2, when n = 3 N returns have been merged.  One outlier R among n values of negligible size has
variance R^2 (n - 1) / n^2, so y = r / std is about n / sqrt(n - 1): 4.7 at N = 7, and above the clip of 10 only from n = 99 on.  The clip is therefore
asserted at N >= 128 (n >= 384, y about 19.6 before the clip); below, the spike is merely normalised and the point is the statistics.
"""
import os
import re

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package
from test_gpu_dev_env import DevArrays, assert_untouched, dev_feed, host_feed, snapshot
from test_gpu_host_env import assert_same_state, bits
from test_gpu_host_truncation import check_fold, fold, make, pair, pattern_transitions
from test_gpu_obs_norm import make_kw, random_masks, trunc_pattern, within_one_ulp
from test_host_truncation_abi import ScriptedEnv, Transitions

pytestmark = pytest.mark.gpu

T = 6
CLIP, EPS = 10.0, 1e-8
# the update kernel's thread count: N = W + 1 gives exactly one thread a second row
W = int(re.search(r"constexpr int RN_THREADS = (\d+);", open(os.path.join(ROOT, "ppo-libtorch_amd", "csrc", "kernels_rewnorm.hip")).read()).group(1))


@pytest.fixture(scope="module")
def P():
    return load_package()


class Model:
    """The header's semantics in numpy f64.  gamma, eps and clip pass through the ABI as floats."""

    def __init__(self, N, gamma, clip=CLIP, eps=EPS):
        self.ret, self.mean, self.var, self.count = np.zeros(N), 0.0, 1.0, 0.0
        self.gamma, self.clip, self.eps = float(np.float32(gamma)), float(np.float32(clip)), float(np.float32(eps))
        self.top = 0.0   # max |R| seen

    def update(self, r, done):
        R = self.ret * self.gamma + np.asarray(r, np.float64)
        n = float(R.size)
        bm = R.sum() / n
        bm2 = ((R - bm) ** 2).sum()
        tot = self.count + n
        delta = bm - self.mean
        self.mean = self.mean + delta * n / tot
        self.var = (self.var * self.count + bm2 + delta * delta * self.count * n / tot) / tot
        self.count = tot
        self.ret = np.where(np.asarray(done) != 0, 0.0, R)
        self.top = max(self.top, float(np.abs(R).max()))

    def apply(self, r):
        y = np.asarray(r, np.float64) / np.sqrt(self.var + self.eps)
        return np.clip(y, -self.clip, self.clip).astype(np.float32)

    def step(self, r, done):
        self.update(r, done)
        return self.apply(r)

    def rollout(self, tr):
        return np.stack([self.step(tr.rew[t], tr.done[t]) for t in range(tr.rew.shape[0])])


def scaled_transitions(tr, spike=None):
    """rewards in thousands, rounded to f32 once; spike = (t, n): that entry times 1e6"""
    rew = (tr.rew.astype(np.float64) * 1000.0).astype(np.float32)
    if spike is not None:
        rew[spike] *= np.float32(1e6)
        assert abs(rew[spike]) > 1e8
    return Transitions(tr.obs, rew, tr.done, tr.trunc, tr.final)


def norm_bits(ctx):
    mean, var, count, ret = ctx.reward_norm_get(returns=True)
    return np.array([mean, var]).view(np.uint64), count, ret.view(np.uint64)


def same_bits(x, y):
    return np.array_equal(x[0], y[0]) and x[1] == y[1] and np.array_equal(x[2], y[2])


def assert_same_norm(a, b, tag=""):
    assert same_bits(norm_bits(a), norm_bits(b)), (tag, "reward statistics / ret")


def check_stats(ctx, model, count, last_done, tag):
    mean, var, cnt, ret = ctx.reward_norm_get(returns=True)
    top = model.top
    em, ev, er = abs(mean - model.mean), abs(var - model.var), np.abs(ret - model.ret).max()
    print(tag, "mean err / max|R|: %.3g   var err / max|R|^2: %.3g   ret err / max|R|: %.3g" % (em / top, ev / top ** 2, er / top))
    assert em <= 1e-12 * top, (tag, "mean", em / top)
    assert ev <= 1e-12 * top ** 2, (tag, "var", ev / top ** 2)
    assert er <= 1e-12 * top, (tag, "ret", er / top)
    assert (ret[last_done != 0] == 0.0).all() and (ret[last_done == 0] != 0.0).all(), (tag, "ret at the last done")
    assert cnt == count == model.count, (tag, cnt, count)


SHAPES = [("7x4", 7, 4, {}), ("33x4", 33, 4, {}), ("70x8", 70, 8, {}), ("300x4", 300, 4, {}), ("W+1", W + 1, 4, {}),
          ("generic_f32", 50, 6, dict(seed=3)), ("generic_bf16", 50, 6, dict(seed=3, bf16=True))]


# ---- 1. statistics and outputs against numpy
@pytest.mark.parametrize("name,N,O,kw", SHAPES, ids=[s[0] for s in SHAPES])
def test_statistics_and_outputs_against_numpy(P, name, N, O, kw):
    """N = 7 and 33 are below a wave, 70 crosses one, 300 and W + 1 give some threads of the one workgroup a second row"""
    ctx, raw = pair(P, N, O, T, **make_kw(P, kw))   # raw: the same feed with normalisation off
    ctx.reward_norm_enable()
    env = ScriptedEnv(N, O)
    model = Model(N, ctx.cfg.gamma)
    obs0 = env.reset()
    ctx.host_env_reset(obs0)
    raw.host_env_reset(obs0)
    spike = (2, min(3, N - 1))
    for it in range(2):
        tr = scaled_transitions(env.rollout(T), spike if it == 0 else None)
        host_feed(ctx, tr)
        host_feed(raw, tr)
        want = model.rollout(tr)
        check_stats(ctx, model, (it + 1) * T * N, tr.done[-1], (name, it))
        got = ctx.read("REWARDS", (T, N))
        within_one_ulp(got, want, (name, it, "REWARDS"))
        assert np.abs(got).max() <= model.clip
        if it == 0 and N >= 128:   # (the module docstring: below, the clip cannot act)
            assert want[spike] == model.clip and got[spike] == model.clip
        # the raw rewards are kept where episodes are counted
        assert np.array_equal(bits(raw.read("REWARDS", (T, N))), bits(tr.rew))
        for name_ in ("FIN_REW", "EP_REW"):
            assert np.array_equal(bits(ctx.read(name_)), bits(raw.read(name_))), (name, it, name_)
        assert np.array_equal(ctx.read("FIN_LEN"), raw.read("FIN_LEN"))
        st, st_raw = ctx.stats(), raw.stats()
        assert st["ep_count"] == st_raw["ep_count"] > 0 and st["ep_rew_mean"] == st_raw["ep_rew_mean"] and st["ep_len_mean"] == st_raw["ep_len_mean"]
        assert st["ep_rew_mean"] > 1000.0
        assert np.isfinite(st["loss"]) and st["updates"] == it + 1
    ctx.close()
    raw.close()


# ---- 2. constant reward
def test_constant_reward_clips(P):
    """The header's known consequence: a first batch of identical rewards has var = 0, y = r / sqrt(eps) = 1e4, and the clip acts.  A sum of N ones is
    exact in any order, so both sides are exact.  The statistics cannot be read inside a rollout, so the variance behind the first step is read off a
    context with gamma = 0: there R = r = 1 in every later step too, every term of Chan's M2 is non-negative, and the variance at the end of the
    rollout is 0 exactly when it was 0 (and the mean 1) behind the first step.  The context with the default gamma shows the first reward row."""
    N, O = 33, 4
    for kw in (dict(gamma=0.0), {}):
        ctx = make(P, N, O, T, **kw)
        ctx.init_orthogonal(11)
        ctx.reward_norm_enable()
        env = ScriptedEnv(N, O)
        ctx.host_env_reset(env.reset())
        tr = env.rollout(T)
        tr.rew = np.ones((T, N), np.float32)
        host_feed(ctx, tr)
        rew = ctx.read("REWARDS", (T, N))
        assert (rew[0] == np.float32(CLIP)).all()
        mean, var, count = ctx.reward_norm_get()
        assert count == T * N
        if kw:
            assert var == 0.0 and mean == 1.0 and (rew == np.float32(CLIP)).all()
        else:
            assert var > 0.0   # the returns of later steps differ between envs (episodes end at different steps)
        ctx.close()


# ---- 3. device-fed equals host-fed, statistics and ret included
DEV_CASES = [("33x4", 33, 4, T, {}), ("70x8", 70, 8, T, {}), ("generic_f32", 50, 6, 12, dict(seed=3)), ("generic_bf16", 50, 6, 12, dict(seed=3, bf16=True)),
             ("masked_multihead", 33, 4, T, dict(head_dims=(3, 2), masked=True)), ("33x4_obs_norm", 33, 4, T, dict(obs_norm=True))]


@pytest.mark.parametrize("name,N,O,steps,kw", DEV_CASES, ids=[c[0] for c in DEV_CASES])
def test_device_fed_equals_host_fed(P, name, N, O, steps, kw):
    kw = make_kw(P, kw)
    masked, obs_norm = kw.pop("masked", False), kw.pop("obs_norm", False)
    if masked:
        kw["dist_kind"] = P.DIST_MASKED
    a, b = pair(P, N, O, steps, **kw)
    for c in (a, b):
        c.reward_norm_enable()
        if obs_norm:   # no truncations here: the one documented difference between the feeds does not arise
            c.obs_norm_enable()
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    a.host_env_reset(obs0)
    d = DevArrays(b)
    b.dev_env_reset(b.dev(obs0))
    rng = np.random.default_rng(17)
    for it in range(2):
        tr = scaled_transitions(env.rollout(steps), (2, 3) if it == 0 else None)
        masks = random_masks(rng, b, steps, it) if masked else None
        fin = it == 1
        act_a = host_feed(a, tr, fin=fin, masks=masks)
        act_b = dev_feed(b, d, tr, fin=fin, masks=masks)
        assert np.array_equal(act_a, act_b), (it, int((act_a != act_b).sum()))
        st = assert_same_state(a, b, tag=(name, it))
        assert_same_norm(a, b, (name, it))
    assert st["updates"] == 2 and a.reward_norm_get()[2] == 2 * steps * N
    assert np.abs(a.read("REWARDS")).max() <= CLIP
    if obs_norm:
        ma, mb = a.obs_norm_get(), b.obs_norm_get()
        assert np.array_equal(ma[0].view(np.uint64), mb[0].view(np.uint64)) and np.array_equal(ma[1].view(np.uint64), mb[1].view(np.uint64)) and ma[2] == mb[2]
    a.close()
    b.close()


# ---- 4. truncations: the fold adds gamma * V(final obs) to the NORMALISED reward, in both feeds
def test_truncations(P):
    N, O = 70, 4
    tr = scaled_transitions(pattern_transitions(N, T, O, trunc_pattern(N)))
    obs0 = np.zeros((N, O), np.float32)
    a, b = pair(P, N, O, T)        # host-fed and device-fed, with flags
    twin = make(P, N, O, T)        # the same feed without flags: the unfolded normalised rewards
    twin.set_params(a.get_params())
    for x in (a, b, twin):
        x.reward_norm_enable()
    a.host_env_reset(obs0)
    twin.host_env_reset(obs0)
    host_feed(a, tr, mode="flags")
    host_feed(twin, tr)
    db = DevArrays(b)
    b.dev_env_reset(b.dev(obs0))
    dev_feed(b, db, tr, mode="flags")
    y = twin.read("REWARDS", (T, N))
    within_one_ulp(y, Model(N, a.cfg.gamma).rollout(tr), "unfolded")
    assert twin.host_truncations()[0].size == 0
    # REWARDS = y off the events and f32(y + f32(gamma v)) at them, v the reported value; the scan runs on that (check_fold)
    unfolded = Transitions(tr.obs, y, tr.done, tr.trunc, tr.final)
    ia, va = check_fold(P, a, unfolded)
    ib, vb = check_fold(P, b, unfolded)
    assert ia.size == N + 4
    assert np.array_equal(ia, ib) and np.array_equal(bits(va), bits(vb))
    ra, rb = a.read("REWARDS"), b.read("REWARDS")
    assert np.array_equal(bits(ra), bits(rb))
    assert np.array_equal(bits(ra[ia]), bits(fold(y.ravel()[ia], va, a.cfg.gamma)))
    assert_same_state(a, b, tag="flags")
    # the statistics do not see the fold, and ret is zero behind a truncated step
    assert_same_norm(a, b)
    assert_same_norm(a, twin)
    ret = a.reward_norm_get(returns=True)[3]
    assert tr.trunc[T - 1, 0] == 1 and ret[0] == 0.0
    assert (ret[tr.done[T - 1] != 0] == 0.0).all() and (ret[tr.done[T - 1] == 0] != 0.0).all()
    for x in (a, b, twin):
        x.close()


# ---- 5. determinism
@pytest.mark.parametrize("N", [300, W + 1], ids=["300", "W+1"])
def test_the_same_feed_twice_gives_the_same_bits(P, N):
    O = 4
    a, b = pair(P, N, O, T)
    outs = []
    for c in (a, b):
        c.reward_norm_enable()
        env = ScriptedEnv(N, O)
        d = DevArrays(c)
        c.dev_env_reset(c.dev(env.reset()))
        outs.append([dev_feed(c, d, scaled_transitions(env.rollout(T), (2, 3) if it == 0 else None)) for it in range(2)])
    assert np.array_equal(np.stack(outs[0]), np.stack(outs[1]))
    assert_same_state(a, b)
    assert_same_norm(a, b)
    assert a.reward_norm_get()[2] == 2 * T * N
    a.close()
    b.close()


# ---- 6. modes and the checkpoint round trip
def test_modes(P):
    N, O = 33, 4
    ctx = make(P, N, O, T)
    ctx.init_orthogonal(11)
    ctx.reward_norm_enable(1)
    env = ScriptedEnv(N, O)
    model = Model(N, ctx.cfg.gamma)
    ctx.host_env_reset(env.reset())
    tr1 = scaled_transitions(env.rollout(T))
    host_feed(ctx, tr1)
    model.rollout(tr1)
    frozen = norm_bits(ctx)
    assert frozen[1] == T * N
    # mode 2: the statistics and ret stay, bit for bit, and the outputs follow the frozen variance
    ctx.reward_norm_enable(2)
    tr2 = scaled_transitions(env.rollout(T), (2, 3))
    host_feed(ctx, tr2)
    assert same_bits(frozen, norm_bits(ctx))
    within_one_ulp(ctx.read("REWARDS", (T, N)), model.apply(tr2.rew), "mode 2 REWARDS")
    assert abs(ctx.read("REWARDS", (T, N))[2, 3]) == model.clip
    # mode 0: raw rewards again (the statistics are kept)
    ctx.reward_norm_enable(0)
    tr3 = scaled_transitions(env.rollout(T))
    host_feed(ctx, tr3)
    assert np.array_equal(bits(ctx.read("REWARDS", (T, N))), bits(tr3.rew))
    assert same_bits(frozen, norm_bits(ctx))
    ctx.close()


def test_set_get_round_trip_reproduces_a_context(P):
    """the checkpoint round trip: statistics of a trained context, set on two fresh ones -- on the second through get of the first"""
    N, O = 33, 4
    src = make(P, N, O, T)
    src.init_orthogonal(11)
    src.reward_norm_enable()
    env = ScriptedEnv(N, O)
    src.host_env_reset(env.reset())
    host_feed(src, scaled_transitions(env.rollout(T)))
    mean, var, count = src.reward_norm_get()
    assert count == T * N and var > 1e4
    a, b = pair(P, N, O, T)
    assert a.reward_norm_get() == (0.0, 1.0, 0.0) and (a.reward_norm_get(returns=True)[3] == 0).all()   # before anything is enabled or set
    a.reward_norm_set(mean, var, count)
    got = a.reward_norm_get()
    assert np.array_equal(np.array(got).view(np.uint64), np.array([mean, var, count]).view(np.uint64))
    b.reward_norm_set(*got)
    obs0 = env.reset()
    tr = scaled_transitions(env.rollout(T))
    for c in (a, b):
        c.reward_norm_enable()
        c.host_env_reset(obs0)
        host_feed(c, tr)
    assert_same_state(a, b)
    assert_same_norm(a, b)
    assert a.reward_norm_get()[2] == count + T * N
    # a reset zeroes ret and keeps the statistics
    before = norm_bits(a)
    assert before[2].any()
    a.host_env_reset(obs0)
    after = norm_bits(a)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1] and not after[2].any()
    for c in (src, a, b):
        c.close()


# ---- 7. errors, each leaving the state and the statistics untouched
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
            assert same_bits(norm, norm_bits(ctx))
        return str(e.value)

    a.host_open = False
    assert "status 5" in status(cart, cart.reward_norm_enable)               # a device-env context
    assert "status 5" in status(cart, cart.reward_norm_get)
    assert "status 5" in status(cart, cart.reward_norm_set, 0.0, 1.0, 0.0)
    assert "status 1" in status(a, a.reward_norm_enable, 1, 0.0)             # clip = 0
    assert "status 1" in status(a, a.reward_norm_enable, 1, 10.0, 0.0)       # eps = 0
    assert "status 1" in status(a, a.reward_norm_enable, 3)
    assert "status 1" in status(a, a.reward_norm_enable, 1, float("inf"))
    assert "status 1" in status(a, a.reward_norm_set, 0.0, -1.0, 0.0)        # a negative variance, a negative count, a non-finite mean
    assert "status 1" in status(a, a.reward_norm_set, 0.0, 1.0, -1.0)
    assert "status 1" in status(a, a.reward_norm_set, float("nan"), 1.0, 0.0)
    a.reward_norm_enable()
    a.host_env_reset(env.reset())
    tr = scaled_transitions(env.rollout(T))
    host_feed(a, tr)
    msg = status(a, a.host_rollout_begin, 2)
    assert "status 5" in msg and "group" in msg and "reward" in msg, msg
    assert "status 5" in status(a, a.comm_init_local, 77, 0, 2)
    # ret_h with a wrong N; null mean / var / count
    buf = np.zeros(N + 1)
    m, v, cnt = C.c_double(), C.c_double(), C.c_double()
    before, norm = snapshot(a), norm_bits(a)
    assert L.ppo_reward_norm_get_h(a.h, C.byref(m), C.byref(v), C.byref(cnt), buf.ctypes.data_as(C.c_void_p), C.c_int64(N + 1)) == 1
    assert not buf.any()
    assert L.ppo_reward_norm_get_h(a.h, None, C.byref(v), C.byref(cnt), None, C.c_int64(N)) == 1
    assert L.ppo_reward_norm_get_h(a.h, C.byref(m), C.byref(v), None, None, C.c_int64(N)) == 1
    assert L.ppo_reward_norm_get_h(a.h, C.byref(m), C.byref(v), C.byref(cnt), None, C.c_int64(0)) == 0 and cnt.value == T * N   # N is not looked at without ret_h
    assert_untouched(a, before, "wrong N")
    assert same_bits(norm, norm_bits(a))
    # inside an open rollout
    tr = scaled_transitions(env.rollout(T))
    a.host_rollout_begin()
    a.host_open = True
    a.host_act()
    assert "status 3" in status(a, a.reward_norm_enable, 0)
    assert "status 3" in status(a, a.reward_norm_get)
    assert "status 3" in status(a, a.reward_norm_set, 0.0, 1.0, 0.0)
    a.host_observe(tr.obs[0], tr.rew[0], tr.done[0])
    for t in range(1, T):
        a.host_act()
        a.host_observe(tr.obs[t], tr.rew[t], tr.done[t])
    a.host_rollout_end()
    assert a.reward_norm_get()[2] == 2 * T * N and np.isfinite(a.stats()["loss"])
    a.close()
    cart.close()


# ---- 8. off means off
def test_off_means_off(P):
    """enable never called and enable(0) called: identical bits over two iterations, host-fed and device-fed, with truncation flags"""
    N, O = 33, 4
    a, b = pair(P, N, O, T)
    c, d = pair(P, N, O, T)
    c.set_params(a.get_params())
    d.set_params(a.get_params())
    b.reward_norm_enable(0)
    d.reward_norm_enable(0)
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
        off_events = tr.trunc.ravel() == 0
        assert np.array_equal(bits(a.read("REWARDS"))[off_events], bits(tr.rew.ravel())[off_events])   # raw
    assert b.reward_norm_get() == (0.0, 1.0, 0.0) and d.reward_norm_get() == (0.0, 1.0, 0.0)
    for x in (a, b, c, d):
        x.close()
