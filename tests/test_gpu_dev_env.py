"""Caller-stepped environments on the device (include/ppo_hip.h: ppo_dev_env_reset / ppo_dev_act / ppo_dev_observe) on the GPU.

The yardstick is the host-fed rollout of the same data on a twin context (ppo_host_act / ppo_host_observe), itself tied to the device-env rollout by
tests/test_gpu_host_env.py.  The envs are scripted (tests/test_host_truncation_abi.py: ScriptedEnv, action-independent), so both contexts see identical
data by construction, and every comparison is bit equality: every rollout buffer, the parameters, AdamW, the statistics, every step's actions, and the
truncation events with their values.
"""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package
from test_gpu_host_env import BUFS, NumpyFin, assert_same_state, bits
from test_gpu_host_truncation import check_fold, make, pair, pattern_transitions
from test_host_truncation_abi import ScriptedEnv, Transitions

pytestmark = pytest.mark.gpu

T = 24


@pytest.fixture(scope="module")
def P():
    return load_package()


class DevArrays:
    """The caller's device arrays of one env step, allocated once and refilled (DeviceArray.upload is synchronous)."""

    def __init__(self, ctx):
        N, O = ctx.N, ctx.O
        self.obs, self.final = ctx.empty((N, O), np.float32), ctx.empty((N, O), np.float32)
        self.rew, self.fin_rew = ctx.empty(N, np.float32), ctx.empty(N, np.float32)
        self.done, self.fin_len, self.trunc = ctx.empty(N, np.int32), ctx.empty(N, np.int32), ctx.empty(N, np.int32)
        self.act = ctx.empty((N, ctx.H), np.int64)
        self.mask = ctx.empty((N, ctx.A), np.uint8)


def fins(tr, use):
    """fin_len / fin_rew [T, N] as a user env reports them, or (None, None)"""
    if not use:
        return None, None
    f = NumpyFin(tr.rew.shape[1])
    out = [f.step(tr.rew[t], tr.done[t]) for t in range(tr.rew.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def host_feed(ctx, tr, mode="plain", fin=False, masks=None):
    """One host-fed iteration; returns the actions [T, N, H]."""
    fl, fr = fins(tr, fin)
    acts = []
    ctx.host_rollout_begin()
    for t in range(ctx.T):
        acts.append(ctx.host_act(None if masks is None else masks[t]))
        kw = dict(fin_len=fl[t], fin_rew=fr[t]) if fin else {}
        if mode == "flags":
            kw.update(truncated=tr.trunc[t], final_obs=tr.final[t])
        ctx.host_observe(tr.obs[t], tr.rew[t], tr.done[t], **kw)
    ctx.host_rollout_end()
    return np.stack(acts)


def dev_steps(ctx, d, tr, steps, mode="plain", fin=False, masks=None, fl=None, fr=None):
    """Device-fed steps of the open rollout from uploaded arrays; returns their actions, read back from the device."""
    acts = []
    for t in steps:
        if masks is not None:
            d.mask.upload(masks[t])
        ctx.dev_act(d.act, mask=d.mask if masks is not None else None)
        acts.append(d.act.download())
        d.obs.upload(tr.obs[t]); d.rew.upload(tr.rew[t]); d.done.upload(tr.done[t])
        kw = {}
        if fin:
            d.fin_len.upload(fl[t]); d.fin_rew.upload(fr[t])
            kw.update(fin_len=d.fin_len, fin_rew=d.fin_rew)
        if mode in ("flags", "zeros"):
            d.trunc.upload(tr.trunc[t] if mode == "flags" else np.zeros_like(tr.trunc[t]))
            d.final.upload(tr.final[t])
            kw.update(truncated=d.trunc, final_obs=d.final)
        ctx.dev_observe(d.obs, d.rew, d.done, **kw)
    return acts


def dev_feed(ctx, d, tr, mode="plain", fin=False, masks=None):
    fl, fr = fins(tr, fin)
    ctx.host_rollout_begin()
    acts = dev_steps(ctx, d, tr, range(ctx.T), mode, fin, masks, fl, fr)
    ctx.host_rollout_end()
    return np.stack(acts)


def snapshot(ctx):
    s = {name: ctx.read(name).copy() for name in BUFS}
    s["PARAMS"] = ctx.get_params()
    return s


def assert_untouched(ctx, before, tag):
    after = snapshot(ctx)
    for k in before:
        assert np.array_equal(bits(before[k]), bits(after[k])), (tag, k)


# ---- 1. device-fed equals host-fed
def device_equals_host(P, N, O, steps=T, masked=False, **kw):
    a, b = pair(P, N, O, steps, **kw)
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    a.host_env_reset(obs0)
    d = DevArrays(b)
    b.dev_env_reset(b.dev(obs0))
    rng = np.random.default_rng(17)
    for it in range(2):
        tr = env.rollout(steps)
        masks = None
        if masked:   # disable actions, never a whole head
            masks = (rng.random((steps, N, b.A)) < 0.6).astype(np.uint8)
            off = 0
            for h in range(b.H):
                dim = b.cfg.head_dims[h]
                keep = (np.arange(N) + it) % dim
                masks[:, np.arange(N), off + keep] = 1
                off += dim
            assert (masks == 0).any()
        fin = it == 1   # fin_len / fin_rew both NULL in the first iteration, both given in the second
        act_a = host_feed(a, tr, fin=fin, masks=masks)
        act_b = dev_feed(b, d, tr, fin=fin, masks=masks)
        assert act_a.dtype == act_b.dtype == np.int64 and np.array_equal(act_a, act_b), (it, int((act_a != act_b).sum()))
        st = assert_same_state(a, b, tag=it)
        if masked:
            assert np.array_equal(b.read("MASKS", (steps, N, b.A)), masks)
    assert st["updates"] == 2 and st["ep_count"] > 0
    assert b.host_truncations()[0].size == 0
    a.close()
    b.close()


@pytest.mark.parametrize("N,O", [(7, 4), (33, 4), (33, 2), (33, 8)])
def test_device_fed_equals_host_fed(P, N, O):
    device_equals_host(P, N, O)


def test_device_fed_equals_host_fed_vector_rollout(P):
    device_equals_host(P, 33, 4, kernel_flags=P.KERNEL_ROLLOUT_VECTOR)


def test_device_fed_equals_host_fed_masked_multihead(P):
    device_equals_host(P, 33, 4, masked=True, head_dims=(3, 2), dist_kind=P.DIST_MASKED)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_device_fed_equals_host_fed_generic(P, dtype):
    """obs 6, heads (3, 2), 50 envs x 12 steps: the generic engine at the shape tests/test_gpu_host_truncation.py feeds it from the host"""
    device_equals_host(P, 50, 6, steps=12, compute_dtype=P.DTYPE_BF16 if dtype == "bf16" else P.DTYPE_F32, seed=3)


# ---- 2. stream-ordered hand-over
class Hip:
    """The HIP runtime libppo_hip.so is linked against, by its soname (already in the process), for the caller's side of the hand-over: a stream of the
    caller's own, pinned host memory and asynchronous copies on that stream."""
    H2D, D2D, NON_BLOCKING = 1, 3, 1

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so.7")
        self.lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.lib.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        self.lib.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.lib.hipStreamDestroy.argtypes = [C.c_void_p]
        self.lib.hipHostFree.argtypes = [C.c_void_p]
        self.pinned = []

    def ok(self, status):
        assert status == 0, "HIP status %d" % status

    def stream(self):
        s = C.c_void_p()
        self.ok(self.lib.hipStreamCreateWithFlags(C.byref(s), C.c_uint(self.NON_BLOCKING)))
        return s

    def pin(self, a):
        """a's bytes in pinned host memory; returns the address"""
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        self.ok(self.lib.hipHostMalloc(C.byref(p), C.c_size_t(a.nbytes), C.c_uint(0)))
        C.memmove(p, a.ctypes.data, a.nbytes)
        self.pinned.append(p)
        return p.value

    def copy(self, dst, src, nbytes, kind, stream):
        self.ok(self.lib.hipMemcpyAsync(dst, src, nbytes, kind, stream))

    def close(self):
        for p in self.pinned:
            self.lib.hipHostFree(p)


@pytest.mark.parametrize("which", ["side", "context", "null"])
def test_stream_ordered_handover(P, which):
    """The caller's arrays are reused in place every step: step t + 1's data is copied over step t's right behind dev_observe, and the actions are consumed
    by an asynchronous copy right behind dev_act (and then scribbled over), all on the caller's stream and without a host wait inside the rollout.  The
    result is the host-fed state, for a side stream of the caller's, for the context's own stream (stream=None) and for the null stream.
    The caller's side is plain HIP through ctypes, not torch tensors on a torch.cuda.Stream: a PyTorch-ROCm wheel that bundles its own HIP runtime
    cannot share a stream or an event with a library linked against the system's, and this suite must not depend on which of the two a machine has."""
    N, O = 33, 4
    a, b = pair(P, N, O)
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    tr = env.rollout(T)
    a.host_env_reset(obs0)
    act_a = host_feed(a, tr, mode="flags")
    hip = Hip()
    own = hip.stream() if which == "side" else None
    s = own if which == "side" else (C.c_void_p(b.stream()) if which == "context" else C.c_void_p(0))
    arg = s if which == "side" else (None if which == "context" else 0)   # None = ppo_stream(ctx): no events; 0 = the null stream: the event hand-over
    src = [tr.obs, tr.rew, tr.done, tr.trunc, tr.final]
    step_bytes = [x[0].nbytes for x in src]
    pinned = [hip.pin(x) for x in src]
    cur = [b.empty(x.shape[1:], x.dtype) for x in src]
    d_obs0, act, log = b.empty((N, O), np.float32), b.empty((N, b.H), np.int64), b.empty((T, N, b.H), np.int64)
    act_bytes = N * b.H * 8

    def load(t):
        for c, p, n in zip(cur, pinned, step_bytes):
            hip.copy(c.ptr, p + t * n, n, Hip.H2D, s)

    hip.copy(d_obs0.ptr, hip.pin(obs0), obs0.nbytes, Hip.H2D, s)
    b.dev_env_reset(d_obs0, stream=arg)
    load(0)
    b.host_rollout_begin()
    for t in range(T):
        b.dev_act(act, stream=arg)
        hip.copy(log.ptr.value + t * act_bytes, act.ptr, act_bytes, Hip.D2D, s)    # the actions, consumed right behind the call
        hip.ok(hip.lib.hipMemsetAsync(act.ptr, 0xFF, act_bytes, s))               # ... and scribbled over: the next act writes behind this
        b.dev_observe(cur[0], cur[1], cur[2], truncated=cur[3], final_obs=cur[4], stream=arg)
        if t + 1 < T:
            load(t + 1)                                                             # over step t's arrays: they were consumed in stream order
        else:
            for c, n in zip(cur, step_bytes):
                hip.ok(hip.lib.hipMemsetAsync(c.ptr, 0xFF, n, s))                  # NaN / -1 everywhere
    b.host_rollout_end()
    hip.ok(hip.lib.hipStreamSynchronize(s))
    b.sync()
    assert np.array_equal(log.download(), act_a)
    assert_same_state(a, b, tag=which)
    ia, va = a.host_truncations()
    ib, vb = b.host_truncations()
    assert ia.size > 0 and np.array_equal(ia, ib) and np.array_equal(bits(va), bits(vb))
    if own is not None:
        hip.ok(hip.lib.hipStreamDestroy(own))
    hip.close()
    a.close()
    b.close()


# ---- 3. truncation fold, device against host
def fold_device_against_host(P, N, O, tr, obs0):
    a, b = pair(P, N, O)
    a.host_env_reset(obs0)
    host_feed(a, tr, mode="flags")
    d = DevArrays(b)
    b.dev_env_reset(b.dev(obs0))
    dev_feed(b, d, tr, mode="flags")
    assert_same_state(a, b, tag=(N, O))   # REWARDS, ADVANTAGES, RETURNS, the parameters, AdamW, the statistics (and the rest)
    ia, va = a.host_truncations()
    ib, vb = b.host_truncations()
    assert ib.dtype == np.int32 and np.array_equal(ia, ib) and np.array_equal(bits(va), bits(vb)), (ia.size, ib.size)
    assert np.array_equal(ib, tr.events()) and (np.diff(ib) > 0).all()
    check_fold(P, b, tr)
    a.close()
    b.close()
    return ib


@pytest.mark.parametrize("N,O", [(7, 4), (33, 2), (33, 8), (70, 4), (70, 8), (300, 2), (300, 4), (300, 8)])
def test_truncation_fold_device_against_host(P, N, O):
    """N = 70 crosses a wave, N = 300 a 256-thread workgroup"""
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    tr = env.rollout(T)
    assert tr.trunc.sum() > 0 and (tr.done - tr.trunc).sum() > 0
    fold_device_against_host(P, N, O, tr, obs0)


@pytest.mark.parametrize("O", [2, 4, 8])
def test_truncation_fold_hand_built_patterns_n70(P, O):
    """a step where every row is flagged (two 32-row tiles and 6 rows; 18 rounds of four waves), steps where none is, flags only in rows 63, 64, 69"""
    N = 70
    trunc = np.zeros((T, N), np.int32)
    trunc[1, :] = 1
    trunc[3, [63, 64, 69]] = 1
    trunc[T - 1, 0] = 1
    tr = pattern_transitions(N, T, O, trunc)
    assert not tr.trunc[2].any() and tr.done[0].sum() == 1   # a termination where no event sits
    idx = fold_device_against_host(P, N, O, tr, np.zeros((N, O), np.float32))
    assert idx.size == N + 4


@pytest.mark.parametrize("O", [4, 8])
def test_truncation_fold_rows_255_and_256(P, O):
    """one flagged row in each of two workgroups: two atomicAdds, either order"""
    N = 300
    trunc = np.zeros((T, N), np.int32)
    trunc[5, [255, 256]] = 1
    tr = pattern_transitions(N, T, O, trunc)
    idx = fold_device_against_host(P, N, O, tr, np.zeros((N, O), np.float32))
    assert list(idx) == [5 * N + 255, 5 * N + 256]


# ---- 4. two rollouts back to back: the alternating lists
def test_truncations_of_the_closed_rollout_while_the_next_is_open(P):
    N, O = 70, 4
    a, b = pair(P, N, O)
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    tr1, tr2, tr3 = env.rollout(T), env.rollout(T), env.rollout(T)
    a.host_env_reset(obs0)
    d = DevArrays(b)
    b.dev_env_reset(b.dev(obs0))
    assert b.host_truncations()[0].size == 0   # before any rollout
    host_feed(a, tr1, mode="flags")
    i1, v1 = a.host_truncations()
    dev_feed(b, d, tr1, mode="flags")
    host_feed(a, tr2, mode="flags")
    i2, v2 = a.host_truncations()
    assert i1.size > 0 and i2.size > 0 and not np.array_equal(i1, i2)
    b.host_rollout_begin()
    half = T // 2
    dev_steps(b, d, tr2, range(half), mode="flags")
    assert tr2.trunc[:half].any()
    ib, vb = b.host_truncations()   # the second rollout is open and has folded events: still the first rollout's
    assert np.array_equal(ib, i1) and np.array_equal(bits(vb), bits(v1))
    dev_steps(b, d, tr2, range(half, T), mode="flags")
    b.host_rollout_end()
    ib, vb = b.host_truncations()
    assert np.array_equal(ib, i2) and np.array_equal(bits(vb), bits(v2))
    assert_same_state(a, b, tag="second")
    # a third rollout without flags passed: no event, and the list of the second is no longer reported
    host_feed(a, tr3)
    dev_feed(b, d, tr3)
    assert b.host_truncations()[0].size == 0 and a.host_truncations()[0].size == 0
    assert_same_state(a, b, tag="third")
    a.close()
    b.close()


# ---- 5. rows flagged truncated with done == 0
@pytest.mark.parametrize("O", [4, 8])
def test_flag_without_done_is_ignored(P, O):
    N = 70
    a, b = pair(P, N, O)
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    tr = env.rollout(T)
    rng = np.random.default_rng(23)
    stray = (rng.random((T, N)) < 0.3) & (tr.done == 0)
    assert stray.sum() > 20
    trunc = (tr.trunc | stray).astype(np.int32)
    final = tr.final.copy()
    final[~((tr.trunc != 0) & (tr.done != 0))] = np.nan   # rows that are not (truncated and done) are never read
    noisy = Transitions(tr.obs, tr.rew, tr.done, trunc, final)
    a.host_env_reset(obs0)
    host_feed(a, tr, mode="flags")   # the run without those flags
    d = DevArrays(b)
    b.dev_env_reset(b.dev(obs0))
    dev_feed(b, d, noisy, mode="flags")
    assert_same_state(a, b, tag=O)
    ia, va = a.host_truncations()
    ib, vb = b.host_truncations()
    assert np.array_equal(ia, ib) and np.array_equal(bits(va), bits(vb)) and np.array_equal(ib, tr.events())
    rew = b.read("REWARDS")
    assert np.array_equal(bits(rew[stray.ravel()]), bits(tr.rew.ravel()[stray.ravel()]))   # the reward is untouched there
    a.close()
    b.close()


# ---- 6. truncated = zeros, truncated = None and the plain host rollout
@pytest.mark.parametrize("O", [4, 8])
def test_zero_flags_and_no_flags_are_the_plain_rollout(P, O):
    N = 33
    a, b = pair(P, N, O)
    c = make(P, N, O)
    c.set_params(a.get_params())
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    a.host_env_reset(obs0)
    db, dc = DevArrays(b), DevArrays(c)
    b.dev_env_reset(b.dev(obs0))
    c.dev_env_reset(c.dev(obs0))
    for it in range(2):
        tr = env.rollout(T)
        host_feed(a, tr)
        dev_feed(b, db, tr, mode="zeros")
        dev_feed(c, dc, tr, mode="plain")
        assert_same_state(a, b, tag=(it, "zeros"))
        assert_same_state(a, c, tag=(it, "none"))
        assert b.host_truncations()[0].size == 0 and c.host_truncations()[0].size == 0
    for x in (a, b, c):
        x.close()


# ---- 7. errors, each leaving the state untouched
def test_errors(P):
    N, steps, O = 7, 4, 4
    a, b = pair(P, N, O, steps)
    cart = P.Context(P.make_config(num_envs=N, num_steps=steps, num_minibatches=1, update_epochs=1))
    gen = make(P, N, 6, steps)
    gen.init_orthogonal(11)
    trunc = np.zeros((steps, N), np.int32)
    trunc[1, 2] = trunc[2, 4] = 1
    tr = pattern_transitions(N, steps, O, trunc)
    obs0 = np.zeros((N, O), np.float32)

    def status(ctx, fn, *args, **kw):
        before = snapshot(ctx)
        with pytest.raises(P.binding.PPOError) as e:
            fn(*args, **kw)
        assert_untouched(ctx, before, fn.__name__)
        return str(e.value)

    a.host_env_reset(obs0)
    host_feed(a, tr, mode="flags")   # the clean run
    d = DevArrays(b)
    for x in (d.obs, d.final):
        x.upload(obs0)
    for x in (d.rew, d.fin_rew):
        x.upload(np.zeros(N, np.float32))
    for x in (d.done, d.fin_len, d.trunc):
        x.upload(np.zeros(N, np.int32))

    # a device-env context
    dc = DevArrays(cart)
    cart.env_reset()
    assert "status 3" in status(cart, cart.dev_env_reset, dc.obs)
    assert "status 3" in status(cart, cart.dev_act, dc.act)
    assert "status 3" in status(cart, cart.dev_observe, dc.obs, dc.rew, dc.done)

    assert "status 1" in status(b, b.dev_env_reset, None)
    b.dev_env_reset(b.dev(obs0))
    assert "status 3" in status(b, b.dev_act, d.act)                      # no rollout is open
    b.host_rollout_begin()
    assert "status 3" in status(b, b.dev_env_reset, d.obs)                # a rollout is open
    assert "status 3" in status(b, b.dev_observe, d.obs, d.rew, d.done)   # observe before any act
    assert "status 1" in status(b, b.dev_act, None)                       # null action
    for t in range(steps):
        b.dev_act(d.act)
        if t == 1:
            assert "status 3" in status(b, b.dev_act, d.act)              # act twice in a row
            msg = status(b, b.host_observe, tr.obs[t], tr.rew[t], tr.done[t])   # the other family
            assert "status 3" in msg and "ppo_host_" in msg and "ppo_dev_" in msg, msg
            msg = status(b, b.host_act)
            assert "status 3" in msg and "ppo_host_" in msg and "ppo_dev_" in msg, msg
            assert "status 1" in status(b, b.dev_observe, None, d.rew, d.done)
            assert "status 1" in status(b, b.dev_observe, d.obs, None, d.done)
            assert "status 1" in status(b, b.dev_observe, d.obs, d.rew, None)
            assert "status 1" in status(b, b.dev_observe, d.obs, d.rew, d.done, fin_len=d.fin_len)
            assert "status 1" in status(b, b.dev_observe, d.obs, d.rew, d.done, fin_rew=d.fin_rew)
            assert "status 1" in status(b, b.dev_observe, d.obs, d.rew, d.done, truncated=d.trunc)   # flags without final observations
            assert "status 3" in status(b, b.host_rollout_end)            # end early
        dev_steps_observe(b, d, tr, t)
    assert "status 3" in status(b, b.dev_act, d.act)                      # beyond step T - 1
    b.host_rollout_end()
    assert_same_state(a, b)   # nothing was harmed
    ia, va = a.host_truncations()
    ib, vb = b.host_truncations()
    assert ia.size == 2 and np.array_equal(ia, ib) and np.array_equal(bits(va), bits(vb))

    # a host-fed rollout refuses the device calls, and a grouped one too
    b.host_rollout_begin()
    b.host_act()
    msg = status(b, b.dev_observe, d.obs, d.rew, d.done)
    assert "status 3" in msg and "ppo_host_" in msg and "ppo_dev_" in msg, msg
    msg = status(b, b.dev_act, d.act)
    assert "status 3" in msg and "ppo_host_" in msg and "ppo_dev_" in msg, msg
    b.host_observe(tr.obs[0], tr.rew[0], tr.done[0])
    assert "status 3" in status(b, b.dev_act, d.act)
    for t in range(1, steps):
        b.host_act()
        b.host_observe(tr.obs[t], tr.rew[t], tr.done[t])
    b.host_rollout_end()
    b.host_rollout_begin(2)
    msg = status(b, b.dev_act, d.act)
    assert "status 3" in msg and "group" in msg, msg
    assert "status 3" in status(b, b.dev_observe, d.obs, d.rew, d.done)

    # a generic network takes the calls, but not the flags
    dg = DevArrays(gen)
    for x, v in ((dg.obs, np.zeros((N, 6), np.float32)), (dg.final, np.zeros((N, 6), np.float32)), (dg.rew, np.zeros(N, np.float32)),
                 (dg.done, np.zeros(N, np.int32)), (dg.trunc, np.zeros(N, np.int32))):
        x.upload(v)
    gen.dev_env_reset(dg.obs)
    gen.host_rollout_begin()
    gen.dev_act(dg.act)
    msg = status(gen, gen.dev_observe, dg.obs, dg.rew, dg.done, truncated=dg.trunc, final_obs=dg.final)
    assert "status 5" in msg and "ppo_bootstrap_rewards" in msg, msg
    gen.dev_observe(dg.obs, dg.rew, dg.done)   # the same step without flags goes through
    for c in (a, b, cart, gen):
        c.close()


def dev_steps_observe(ctx, d, tr, t):
    d.obs.upload(tr.obs[t]); d.rew.upload(tr.rew[t]); d.done.upload(tr.done[t]); d.trunc.upload(tr.trunc[t]); d.final.upload(tr.final[t])
    ctx.dev_observe(d.obs, d.rew, d.done, truncated=d.trunc, final_obs=d.final)
