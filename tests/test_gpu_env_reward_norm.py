"""Reward normalisation of the fused device envs (include/ppo_hip.h: PPO_KERNEL_ENV_REWARD_NORM and the "Reward normalisation" block;
ppo-libtorch_amd/csrc/kernels_rewnorm.hip: rewnorm_scan_kernel, rewnorm_moments_kernel, rewnorm_merge_apply_kernel) on the GPU through the C-ABI.

The oracle is the path that was already in the tree: a PPO_ENV_HOST context with reward normalisation on, device-fed (ppo_dev_observe) the raw rewards
and FIN_LEN != 0 rows that an unflagged twin of the device-env context left, runs rewnorm_update_apply_kernel once per step.  The whole-rollout kernels
must leave the same BITS in PPO_BUF_REWARDS, mean, var, the count and ret[N].  Beside it the numpy f64 Model of tests/test_gpu_reward_norm.py with that
file's bounds (1e-12 max|R| on the statistics and ret, one f32 ulp on the outputs), and the fold's own f32 arithmetic (fold_store: f32(y + f32(gamma v))).
Without the flag's bit none of the flagged contexts can be created ("unknown bits in kernel_flags").

Shapes (W = RN_THREADS = 256 slots): Pendulum 70 x 7 with a limit of 3 -- dones inside the rollout, a ragged second 64-env rollout workgroup, 186 slots
without a row; Blackjack 300 x 6 -- natural terminations, rewards of both signs, 44 slots with two rows; masked Taxi 257 x 5 -- W + 1 rows."""
import numpy as np
import pytest

from __graft_entry__ import load_package
from test_gpu_cut_state import EPISODE_STATS, SEED, bits, envs, read_all, same
from test_gpu_dev_env import DevArrays, dev_feed
from test_gpu_host_truncation import fold, make
from test_gpu_obs_norm import within_one_ulp
from test_gpu_reward_norm import CLIP, Model, W, norm_bits, same_bits
from test_host_truncation_abi import Transitions

pytestmark = pytest.mark.gpu

GAMMA = 0.99
SHAPES = [("pendulum", 70, 7, 3), ("blackjack", 300, 6, 100), ("taxi_masked", W + 1, 5, 4)]
IDS = ["%s-%dx%d" % s[:3] for s in SHAPES]


@pytest.fixture(scope="module")
def P():
    return load_package()


def make_ctx(P, env, n, t, max_steps, flags=0, params=None):
    """a fused device env, reset; flags: KERNEL_ENV_REWARD_NORM and / or KERNEL_ENV_CUT_STATE beside the family flag"""
    kind, dist, obs, actions, family, gauss = envs(P)[env]
    cfg = P.make_config(env_kind=kind, dist_kind=dist, obs_size=obs, head_dims=(actions,), num_envs=n, num_steps=t, num_minibatches=1, update_epochs=2,
                        max_episode_steps=max_steps, seed=SEED, total_timesteps=8 * n * t, learning_rate=1e-3, anneal_lr=True, gamma=GAMMA, gae_lambda=0.95,
                        ent_coef=0.01, kernel_flags=family | flags)
    ctx = P.Context(cfg)
    if params is None:   # as tests/test_gpu_cut_state.py: an output layer scaled so that the draws show every action
        ctx.init_orthogonal(11)
        params = ctx.get_params()
        if gauss:
            params[-66:-2] *= 30.0
            params[-1] = 0.3
        else:
            params[-(actions * 65):-actions] *= 30.0
    ctx.set_params(params)
    ctx.env_reset()
    return ctx


def twins(P, env, n, t, max_steps, extra=0):
    plain = make_ctx(P, env, n, t, max_steps, extra)
    flagged = make_ctx(P, env, n, t, max_steps, extra | P.KERNEL_ENV_REWARD_NORM, plain.get_params())
    return plain, flagged


class HostOracle:
    """The existing route: a PPO_ENV_HOST context (2 x 64, four observation words that play no part) with reward normalisation on, device-fed one rollout
    of raw rewards and dones at a time"""

    def __init__(self, P, n, t):
        self.ctx = make(P, n, 4, t, gamma=GAMMA, num_minibatches=1)
        self.ctx.init_orthogonal(11)
        self.ctx.reward_norm_enable()
        self.d = DevArrays(self.ctx)
        self.obs = np.zeros((t, n, 4), np.float32)
        self.ctx.dev_env_reset(self.ctx.dev(self.obs[0]))

    def feed(self, raw, done):
        tr = Transitions(self.obs, raw, done, np.zeros_like(done), self.obs)
        dev_feed(self.ctx, self.d, tr)
        return tr


def raw_and_done(plain, t, n):
    return plain.read("REWARDS", (t, n)).copy(), (plain.read("FIN_LEN", (t, n)) != 0).astype(np.int32)


def assert_rest_equal(flagged, plain, tag):
    got, want = read_all(flagged), read_all(plain)
    for k in want:
        if k != "REWARDS":
            assert same(got[k], want[k]), (tag, k)
    sa, sp = flagged.stats(), plain.stats()
    assert all(sa[k] == sp[k] for k in EPISODE_STATS), (tag, sa, sp)


# ---- 1. the bits of the per-step path, and the numpy model
@pytest.mark.parametrize("env,n,t,limit", SHAPES, ids=IDS)
def test_bits_of_the_per_step_path(P, env, n, t, limit):
    plain, flagged = twins(P, env, n, t, limit)
    assert flagged.reward_norm_get(returns=True)[:3] == (0.0, 1.0, 0.0)
    flagged.reward_norm_enable()
    host = HostOracle(P, n, t)
    model = Model(n, GAMMA)
    dones = 0
    for r in range(2):   # the second rollout with no update between: ret and the statistics carry over
        plain.rollout()
        flagged.rollout()
        raw, done = raw_and_done(plain, t, n)
        tr = host.feed(raw, done)
        dones += int(done.sum())
        got, want = flagged.read("REWARDS", (t, n)), host.ctx.read("REWARDS", (t, n))
        assert same(got, want), (env, r, np.flatnonzero(bits(got) != bits(want))[:8])
        assert same_bits(norm_bits(flagged), norm_bits(host.ctx)), (env, r, flagged.reward_norm_get(), host.ctx.reward_norm_get())
        assert_rest_equal(flagged, plain, (env, r))
        # the numpy f64 model, with the bounds of tests/test_gpu_reward_norm.py
        y = model.rollout(tr)
        mean, var, cnt, ret = flagged.reward_norm_get(returns=True)
        top = model.top
        em, ev, er = abs(mean - model.mean), abs(var - model.var), np.abs(ret - model.ret).max()
        print(env, r, "mean err / max|R|: %.3g   var err / max|R|^2: %.3g   ret err / max|R|: %.3g   dones %d" % (em / top, ev / top ** 2, er / top, done.sum()))
        assert em <= 1e-12 * top and ev <= 1e-12 * top ** 2 and er <= 1e-12 * top
        assert cnt == (r + 1) * t * n == model.count
        assert (ret[done[-1] != 0] == 0.0).all()
        within_one_ulp(got, y, (env, r, "REWARDS"))
        assert np.abs(got).max() <= CLIP and not same(got, raw)
    assert dones > 0, "no episode ended inside the rollouts"
    if env == "blackjack":
        assert (raw > 0).any() and (raw < 0).any()
    for c in (plain, flagged, host.ctx):
        c.close()


# ---- 2. the fold adds f32(gamma V) to the NORMALISED reward, from PPO_BUF_OBS and from the cut-state record
@pytest.mark.parametrize("env,cut", [("mcc", False), ("pendulum", True)], ids=["mcc-fold-from-obs", "pendulum-cut-state"])
def test_fold_on_the_normalised_reward(P, env, cut):
    n, t, limit = 70, 7, 3
    extra = P.KERNEL_ENV_CUT_STATE if cut else 0
    plain, flagged = twins(P, env, n, t, limit, extra)            # plain: the fold on raw rewards -- its events and V
    unfolded = make_ctx(P, env, n, t, limit, extra | P.KERNEL_ENV_REWARD_NORM, plain.get_params())   # normalised, not folded: y
    raw_ctx = make_ctx(P, env, n, t, limit, extra, plain.get_params())                                # neither
    plain.env_truncation_bootstrap(True)
    flagged.env_truncation_bootstrap(True)
    flagged.reward_norm_enable()
    unfolded.reward_norm_enable()
    model = Model(n, GAMMA)
    for r in range(2):
        for c in (plain, flagged, unfolded, raw_ctx):
            c.rollout()
        (i0, v0), (i1, v1) = plain.env_truncations(), flagged.env_truncations()
        assert i0.size > 0 and np.array_equal(i0, i1) and same(v0, v1), (env, r)
        y = unfolded.read("REWARDS")
        raw, done = raw_and_done(raw_ctx, t, n)
        within_one_ulp(y.reshape(t, n), model.rollout(Transitions(None, raw, done, None, None)), (env, r, "y"))
        want = y.copy()
        want[i1] = fold(y[i1], v1, flagged.cfg.gamma)   # fold_store: __fadd_rn(y, __fmul_rn(gamma, v)) and no other rounding
        got = flagged.read("REWARDS")
        assert same(got, want), (env, r, np.flatnonzero(bits(got) != bits(want))[:8])
        assert (bits(got[i1]) != bits(y[i1])).any()
        # the statistics do not see the fold
        assert same_bits(norm_bits(flagged), norm_bits(unfolded)), (env, r)
        assert_rest_equal(flagged, plain, (env, r))
    for c in (plain, flagged, unfolded, raw_ctx):
        c.close()


# ---- 3. modes
def test_modes(P):
    env, n, t, limit = "pendulum", 70, 7, 3
    plain, ctx = twins(P, env, n, t, limit)
    model = Model(n, GAMMA)
    ctx.reward_norm_enable(1)
    plain.rollout()
    ctx.rollout()
    raw, done = raw_and_done(plain, t, n)
    model.rollout(Transitions(None, raw, done, None, None))
    frozen = norm_bits(ctx)
    assert frozen[1] == t * n and frozen[2].any()
    # mode 2: the statistics, the count and ret stay, bit for bit, and all T N rewards follow the frozen variance
    ctx.reward_norm_enable(2)
    plain.rollout()
    ctx.rollout()
    raw2 = plain.read("REWARDS", (t, n))
    assert same_bits(frozen, norm_bits(ctx))
    within_one_ulp(ctx.read("REWARDS", (t, n)), model.apply(raw2), "mode 2 REWARDS")
    assert_rest_equal(ctx, plain, "mode 2")
    # mode 0 behind mode 1: raw rewards again, the statistics are kept
    ctx.reward_norm_enable(0)
    plain.rollout()
    ctx.rollout()
    assert same(ctx.read("REWARDS"), plain.read("REWARDS"))
    assert same_bits(frozen, norm_bits(ctx))
    assert_rest_equal(ctx, plain, "mode 0")
    plain.close()
    ctx.close()


@pytest.mark.parametrize("env,limit", [("pendulum", 3), ("acrobot", 3), ("blackjack", 2)])
def test_a_flagged_context_never_enabled_is_the_unflagged_one(P, env, limit):
    n, t = 70, 7
    plain, never = twins(P, env, n, t, limit)
    back = make_ctx(P, env, n, t, limit, P.KERNEL_ENV_REWARD_NORM, plain.get_params())
    back.reward_norm_enable(0)
    for r in range(2):
        for c in (plain, never, back):
            c.rollout()
        want = read_all(plain)
        for c in (never, back):
            got = read_all(c)
            for k in want:
                assert same(got[k], want[k]), (env, r, k)
            assert c.gauss_fused_launches() == plain.gauss_fused_launches()
            assert c.reward_norm_get() == (0.0, 1.0, 0.0)
    for c in (plain, never, back):
        c.train_iteration()
    assert same(never.get_params(), plain.get_params()) and same(back.get_params(), plain.get_params())
    for c in (plain, never, back):
        c.close()


@pytest.mark.parametrize("env,n,t,limit", SHAPES[1:], ids=IDS[1:])
def test_the_same_run_twice_gives_the_same_bits(P, env, n, t, limit):
    a = make_ctx(P, env, n, t, limit, P.KERNEL_ENV_REWARD_NORM)
    b = make_ctx(P, env, n, t, limit, P.KERNEL_ENV_REWARD_NORM, a.get_params())
    for c in (a, b):
        c.reward_norm_enable()
        c.rollout()
        c.rollout()
    assert same(a.read("REWARDS"), b.read("REWARDS")) and same_bits(norm_bits(a), norm_bits(b))
    assert a.reward_norm_get()[2] == 2 * t * n
    a.close()
    b.close()


def test_set_get_round_trip_and_reset(P):
    env, n, t, limit = "pendulum", 70, 7, 3
    src = make_ctx(P, env, n, t, limit, P.KERNEL_ENV_REWARD_NORM)
    src.reward_norm_enable()
    src.rollout()
    mean, var, count = src.reward_norm_get()
    assert count == t * n and var > 1.0
    a = make_ctx(P, env, n, t, limit, P.KERNEL_ENV_REWARD_NORM, src.get_params())
    b = make_ctx(P, env, n, t, limit, P.KERNEL_ENV_REWARD_NORM, src.get_params())
    a.reward_norm_set(mean, var, count)
    got = a.reward_norm_get()
    assert np.array_equal(np.array(got).view(np.uint64), np.array([mean, var, count]).view(np.uint64))
    b.reward_norm_set(*got)
    for c in (a, b):
        c.reward_norm_enable()
        c.rollout()
    assert same(a.read("REWARDS"), b.read("REWARDS")) and same_bits(norm_bits(a), norm_bits(b))
    assert a.reward_norm_get()[2] == count + t * n
    # ppo_env_reset zeroes ret and keeps the statistics; ppo_env_set_state_h touches neither
    before = norm_bits(a)
    assert before[2].any()
    state, ep_len, ep_rew, resets = a.env_get_state()
    a.env_set_state(state, ep_len, ep_rew, resets)
    assert same_bits(before, norm_bits(a))
    a.env_reset()
    after = norm_bits(a)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1] and not after[2].any()
    # the argument checks are PPO_ENV_HOST's
    for call in (lambda: a.reward_norm_enable(3), lambda: a.reward_norm_enable(1, 0.0), lambda: a.reward_norm_set(0.0, -1.0, 0.0)):
        with pytest.raises(P.binding.PPOError) as e:
            call()
        assert "status 1:" in str(e.value), str(e.value)
    assert same_bits(after, norm_bits(a))
    for c in (src, a, b):
        c.close()


def test_without_the_flag_the_refusals_stand(P):
    plain = make_ctx(P, "pendulum", 8, 4, 3)
    for call in (lambda: plain.reward_norm_enable(1), lambda: plain.reward_norm_get(), lambda: plain.reward_norm_set(0.0, 1.0, 0.0)):
        with pytest.raises(P.binding.PPOError) as e:
            call()
        assert "status 5:" in str(e.value) and "reward normalisation serves PPO_ENV_HOST contexts" in str(e.value), str(e.value)
    plain.close()
    flagged = make_ctx(P, "pendulum", 8, 4, 3, P.KERNEL_ENV_REWARD_NORM)
    with pytest.raises(P.binding.PPOError) as e:
        flagged.obs_norm_enable(1)
    assert "status 5:" in str(e.value) and "PPO_ENV_HOST" in str(e.value)
    flagged.reward_norm_enable()
    with pytest.raises(P.binding.PPOError) as e:
        flagged.comm_init_local(77, 0, 2)
    assert "status 5:" in str(e.value) and "reward normalisation is on" in str(e.value)
    flagged.close()


# ---- 4. two train iterations
def test_train_iterations_on_pendulum(P):
    n, t = 64, 16
    ctx = make_ctx(P, "pendulum", n, t, t, P.KERNEL_ENV_REWARD_NORM)   # a limit of T: 2 N episodes of T steps end inside the two rollouts
    ctx.reward_norm_enable()
    for _ in range(2):
        ctx.train_iteration()
    st = ctx.stats()
    assert np.isfinite(st["loss"]) and st["updates"] == 2
    mean, var, count = ctx.reward_norm_get()
    assert count == 2 * t * n and var > 0.0 and np.isfinite([mean, var]).all()
    assert np.abs(ctx.read("REWARDS")).max() <= CLIP
    # raw units: an episode is T steps at -(theta^2 + 0.1 theta_dot^2 + 0.001 u^2) >= -16.2736 each, about -6 on average from a uniform start -- of
    # order 10^2 at T = 16.  In normalised units a step is r / std(return), the return's std being tens: an episode would sum to a few units
    print("ep_rew_mean", st["ep_rew_mean"], "mean", mean, "var", var)
    assert st["ep_count"] > 0 and -16.2736 * t <= st["ep_rew_mean"] < -1.0 * t
    ctx.close()
