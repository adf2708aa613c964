"""The life cycle of the device event lists (ppo-libtorch_amd/csrc/api.hip: DevEventList) on the GPU: the list of the context's own env
(ppo_env_truncation_bootstrap / ppo_env_truncations) and the two lists of device-fed rollouts (ppo_dev_observe / ppo_host_truncations).

What the sibling suites do not pin: one context that alternates between device-fed and host-fed rollouts, a second read of a list that was fetched
already, and the refusal of a read whose arrays are too short -- which must write nothing and leave the list readable.
"""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package
from test_gpu_dev_env import DevArrays, ScriptedEnv, assert_same_state, bits, dev_feed, host_feed, pair

pytestmark = pytest.mark.gpu

T = 24
SENTINEL = -7


@pytest.fixture(scope="module")
def P():
    return load_package()


def same_events(x, y):
    return x[0].dtype == y[0].dtype == np.int32 and np.array_equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1]))


def test_one_context_both_feeds(P):
    """b: device-fed with flags, host-fed with flags, device-fed with flags, host-fed without flags; a: the same transitions host-fed"""
    N, O = 7, 4
    a, b = pair(P, N, O, T)
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    a.host_env_reset(obs0)
    d = DevArrays(b)
    b.dev_env_reset(b.dev(obs0))
    for it, (device, mode) in enumerate([(True, "flags"), (False, "flags"), (True, "flags"), (False, "plain")]):
        tr = env.rollout(T)
        host_feed(a, tr, mode=mode)
        if device:
            dev_feed(b, d, tr, mode=mode)
        else:
            host_feed(b, tr, mode=mode)
        assert_same_state(a, b, tag=it)
        ea, eb = a.host_truncations(), b.host_truncations()
        assert same_events(ea, eb), (it, ea[0].size, eb[0].size)
        if it < 3:
            assert eb[0].size > 0 and np.array_equal(eb[0], tr.events()), it
        else:
            assert ea[0].size == 0 and eb[0].size == 0 and ea[1].size == 0 and eb[1].size == 0
        if it == 2:   # the list was fetched by the read above: the second read is served from the host copy
            assert same_events(eb, b.host_truncations())
    a.close()
    b.close()


def short_room(P, ctx, fn, want):
    """The three calls of a reader on a list of K >= 2 events: arrays one short, no arrays, arrays of the exact size"""
    idx, val = want
    K = idx.size
    assert K >= 2
    k = C.c_int64(SENTINEL)
    short = np.full(K - 1, SENTINEL, np.int32)
    assert fn(ctx.h, C.byref(k), short.ctypes.data_as(C.c_void_p), None, C.c_int64(K - 1)) == 1
    assert (short == SENTINEL).all() and k.value == SENTINEL
    assert b"room for" in P.binding.lib().ppo_last_error(ctx.h)
    assert fn(ctx.h, C.byref(k), None, None, C.c_int64(0)) == 0 and k.value == K
    k = C.c_int64(SENTINEL)
    i2, v2 = np.full(K, SENTINEL, np.int32), np.zeros(K, np.float32)
    assert fn(ctx.h, C.byref(k), i2.ctypes.data_as(C.c_void_p), v2.ctypes.data_as(C.c_void_p), C.c_int64(K)) == 0 and k.value == K
    assert same_events((i2, v2), want)


def test_short_room_on_a_device_fed_list(P):
    """N = 70: the events come from two waves"""
    N, O = 70, 4
    a, b = pair(P, N, O, T)
    a.close()
    env = ScriptedEnv(N, O)
    obs0 = env.reset()
    tr = env.rollout(T)
    d = DevArrays(b)
    b.dev_env_reset(b.dev(obs0))
    dev_feed(b, d, tr, mode="flags")
    want = b.host_truncations()
    assert np.array_equal(want[0], tr.events()) and (tr.trunc[:, 64:] != 0).any() and (tr.trunc[:, :64] != 0).any()
    short_room(P, b, P.binding.lib().ppo_host_truncations, want)
    b.close()


def test_short_room_on_the_env_list_and_the_switch(P):
    """CartPole cut off at 12 steps (tests/test_gpu_env_truncation.py: test_off_is_off, which has something to fold)"""
    c = P.Context(P.make_config(num_envs=33, num_steps=T, num_minibatches=2, update_epochs=2, seed=5, total_timesteps=33 * T * 5, max_episode_steps=12))
    c.init_orthogonal(11)
    c.env_truncation_bootstrap(True)
    c.env_reset()
    c.train_iteration()
    want = c.env_truncations()
    assert (np.diff(want[0]) > 0).all()
    short_room(P, c, P.binding.lib().ppo_env_truncations, want)
    c.env_truncation_bootstrap(False)
    c.train_iteration()
    assert (c.read("FIN_LEN") == 12).any()   # there was something to fold
    k = C.c_int64(SENTINEL)
    assert P.binding.lib().ppo_env_truncations(c.h, C.byref(k), None, None, C.c_int64(0)) == 0 and k.value == 0
    c.close()
