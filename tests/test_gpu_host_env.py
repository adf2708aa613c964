"""Caller-stepped environments (PPO_ENV_HOST, include/ppo_hip.h ppo_host_*): the reference's custom-environment framework, where the user's env
class sits in PPO_Discrete::m_envs and stepEnvs steps it on the host (reference PPO_Discrete.cpp:365-483).

The yardstick is the device-env context of the same shape.  Context A trains on its own device env (ppo_train_iteration); context B is a PPO_ENV_HOST
context whose envs are stepped by the test through context C (the same device env, driven one step at a time: env_reset / env_step).  After every
iteration every rollout buffer, the parameters, the AdamW moments and every statistic of B must be A's, bit for bit.
"""
import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

BUFS = ["OBS", "ACTIONS", "LOGPROBS", "VALUES", "REWARDS", "DONES", "ADVANTAGES", "RETURNS", "NEXT_VALUE", "NEXT_OBS", "NEXT_DONE", "FIN_LEN",
        "FIN_REW", "EP_LEN", "EP_REW", "MASKS"]


@pytest.fixture(scope="module")
def P():
    return load_package()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_state(a, b, buffers=BUFS, tag=""):
    for name in buffers:
        x, y = a.read(name), b.read(name)
        assert np.array_equal(bits(x), bits(y)), (tag, name, int((bits(x) != bits(y)).sum()))
    assert np.array_equal(bits(a.get_params()), bits(b.get_params())), (tag, "PARAMS")
    ma, va, sa = a.get_optimizer()
    mb, vb, sb = b.get_optimizer()
    assert sa == sb and np.array_equal(bits(ma), bits(mb)) and np.array_equal(bits(va), bits(vb)), (tag, "AdamW")
    st_a, st_b = a.stats(), b.stats()
    assert st_a == st_b, (tag, st_a, st_b)
    return st_a


class NumpyFin:
    """The finished episodes' length and reward as a user env reports them (episode_length / episode_reward), kept in numpy."""

    def __init__(self, n):
        self.len = np.zeros(n, np.int32)
        self.rew = np.zeros(n, np.float32)

    def step(self, rew, done):
        self.len += 1
        self.rew = (self.rew + rew.astype(np.float32)).astype(np.float32)
        d = done != 0
        fl, fr = np.where(d, self.len, 0).astype(np.int32), np.where(d, self.rew, 0).astype(np.float32)
        self.len[d] = 0
        self.rew[d] = 0
        return fl, fr


def host_iteration(b, env, mask=None, fin=None):
    b.host_rollout_begin()
    for _ in range(b.T):
        act = b.host_act(mask)
        obs, rew, done = env.env_step(act)
        if fin is None:
            b.host_observe(obs, rew, done)
        else:
            fl, fr = fin.step(rew, done)
            b.host_observe(obs, rew, done, fl, fr)
    b.host_rollout_end()


def run_against_device(P, env_kind, N, T, iters=3, vector=False, explicit_fin=False, params_hook=None, masked=False, **kw):
    flags = P.KERNEL_ROLLOUT_VECTOR if vector else 0
    base = dict(num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2, seed=5, total_timesteps=N * T * 5, kernel_flags=flags, **kw)
    if env_kind == P.ENV_MOUNTAINCAR:
        base.update(obs_size=2, head_dims=(3,), dist_kind=P.DIST_MASKED if masked else P.DIST_CATEGORICAL)
    a = P.Context(P.make_config(env_kind=env_kind, **base))
    env = P.Context(P.make_config(env_kind=env_kind, **base))
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    a.init_orthogonal(11)
    params = a.get_params()
    if params_hook is not None:
        params_hook(params)
    a.set_params(params)
    b.set_params(params)
    a.env_reset()
    b.host_env_reset(env.env_reset())
    fin = NumpyFin(N) if explicit_fin else None
    mask = np.ones((N, b.A), np.uint8) if masked else None   # MountainCar::getActionMask: every action valid
    dones = 0
    for it in range(iters):
        a.train_iteration()
        host_iteration(b, env, mask, fin)
        st = assert_same_state(a, b, tag=it)
        dones += int(a.read("DONES").sum())
    assert dones > 0   # episode ends (termination or truncation) and auto-resets were exercised
    out = (a.profile_read()["vector_fallback_launches"], b.profile_read()["vector_fallback_launches"], st)
    for c in (a, b, env):
        c.close()
    return out


@pytest.mark.parametrize("vector", [False, True])
@pytest.mark.parametrize("N", [7, 96])
def test_host_cartpole_reproduces_train_iteration(P, N, vector):
    fa, fb, st = run_against_device(P, P.ENV_CARTPOLE, N, 24, vector=vector, max_episode_steps=20)
    assert fa == fb == 0 and st["updates"] == 3


def test_host_cartpole_explicit_finished_episodes(P):
    """fin_len / fin_rew passed by the caller (the reference reads env->episode_length / episode_reward, :474-480), computed in numpy."""
    _, _, st = run_against_device(P, P.ENV_CARTPOLE, 33, 24, explicit_fin=True, max_episode_steps=15)
    assert st["ep_count"] > 0


def test_host_cartpole_weights_outside_rollout16_range(P):
    """An actor output weight of 300 does not fit rollout16_kernel's fp16 operand: the whole host-stepped rollout takes the vector form, as ppo_rollout
    does, the fall-back is counted, and the bits are still the device rollout's."""
    def hook(p):
        p[-130] = 300.0
    fa, fb, _ = run_against_device(P, P.ENV_CARTPOLE, 48, 16, params_hook=hook, max_episode_steps=12)
    assert fb == fa and fb >= 3


@pytest.mark.parametrize("vector", [False, True])
def test_host_mountaincar_masked_reproduces_train_iteration(P, vector):
    run_against_device(P, P.ENV_MOUNTAINCAR, 40, 20, vector=vector, masked=True, max_episode_steps=25, gamma=0.99, ent_coef=0.01)


def test_host_generic_engine_reproduces_synthetic_rollout(P):
    """obs 6 (a width the reference-shape kernels are not built for): the generic engine, whose per-step functions are the synthetic rollout's."""
    N, T = 50, 12
    base = dict(obs_size=6, head_dims=(3, 2), num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2, seed=3, total_timesteps=N * T * 4,
                max_episode_steps=9)
    a = P.Context(P.make_config(env_kind=P.ENV_SYNTHETIC, **base))
    env = P.Context(P.make_config(env_kind=P.ENV_SYNTHETIC, **base))
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    a.init_orthogonal(4)
    b.set_params(a.get_params())
    a.env_reset()
    b.host_env_reset(env.env_reset())
    for it in range(3):
        a.train_iteration()
        host_iteration(b, env)
        assert_same_state(a, b, tag=it)
    for c in (a, b, env):
        c.close()


def test_host_generic_bf16_matches_policy_act(P):
    """bf16 at configs[4]'s widths (obs 376, 4 x 256, heads [3, 3, 3, 2], masked): the host-stepped rollout's actions and log-probs are ppo_policy_act's on
    the stored observations and masks at the same step indices, its values ppo_get_value's (a twin context with the same parameters that never trains)."""
    N, T = 64, 4
    base = dict(obs_size=376, head_dims=(3, 3, 3, 2), hidden=256, n_hidden=4, compute_dtype=P.DTYPE_BF16, dist_kind=P.DIST_MASKED, num_envs=N,
                num_steps=T, num_minibatches=2, update_epochs=1, seed=7, total_timesteps=N * T * 2)
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    twin = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    b.init_orthogonal(9)
    twin.set_params(b.get_params())
    rng = np.random.default_rng(1)
    masks = (rng.random((T, N, b.A)) < 0.7).astype(np.uint8)
    masks[..., 0] = 1
    b.host_env_reset(rng.standard_normal((N, 376)).astype(np.float32))
    b.host_rollout_begin()
    acts = []
    for t in range(T):
        acts.append(b.host_act(masks[t]))
        b.host_observe(rng.standard_normal((N, 376)).astype(np.float32), rng.uniform(-1, 1, N).astype(np.float32), (rng.random(N) < 0.1).astype(np.int32))
    b.host_rollout_end()
    obs, lp, val = b.read("OBS", (T, N, 376)), b.read("LOGPROBS", (T, N)), b.read("VALUES", (T, N))
    assert np.array_equal(b.read("MASKS", (T, N, b.A)), masks)
    assert np.array_equal(b.read("ACTIONS", (T, N, 4)), np.stack(acts).astype(np.int32))
    for t in range(T):
        a_t, lp_t, _, _ = twin.policy_act(obs[t], mask=masks[t], step_index=t)
        assert np.array_equal(a_t, acts[t]), t
        assert np.array_equal(bits(lp_t), bits(lp[t])), t
    assert np.array_equal(bits(twin.get_value(obs.reshape(T * N, 376))), bits(val.ravel()))
    assert np.isfinite(b.stats()["loss"])
    b.close()
    twin.close()


class NumpyCartPole6:
    """A vectorised env the library has no kernel for: CartPole physics (gym's constants) observed as [x, x_dot, cos th, sin th, th_dot, t / 500]."""

    def __init__(self, n, seed):
        self.n, self.rng = n, np.random.default_rng(seed)
        self.s = np.zeros((n, 4))
        self.t = np.zeros(n, np.int32)
        self.ret = np.zeros(n, np.float32)

    def _reset(self, idx):
        self.s[idx] = self.rng.uniform(-0.05, 0.05, (len(idx), 4))
        self.t[idx] = 0
        self.ret[idx] = 0

    def obs(self):
        x, xd, th, thd = self.s.T
        return np.stack([x, xd, np.cos(th), np.sin(th), thd, self.t / 500.0], 1).astype(np.float32)

    def reset(self):
        self._reset(np.arange(self.n))
        return self.obs()

    def step(self, action):
        g, mc, mp, l, fmag, tau = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
        x, xd, th, thd = self.s.T
        f = np.where(action.ravel() == 1, fmag, -fmag)
        ct, st = np.cos(th), np.sin(th)
        temp = (f + mp * l * thd ** 2 * st) / (mc + mp)
        tha = (g * st - ct * temp) / (l * (4.0 / 3.0 - mp * ct ** 2 / (mc + mp)))
        xa = temp - mp * l * tha * ct / (mc + mp)
        self.s = np.stack([x + tau * xd, xd + tau * xa, th + tau * thd, thd + tau * tha], 1)
        self.t += 1
        rew = np.ones(self.n, np.float32)
        self.ret += rew
        done = (np.abs(self.s[:, 0]) > 2.4) | (np.abs(self.s[:, 2]) > 0.2095) | (self.t >= 500)
        fin_len, fin_rew = np.where(done, self.t, 0).astype(np.int32), np.where(done, self.ret, 0).astype(np.float32)
        idx = np.nonzero(done)[0]
        if len(idx):
            self._reset(idx)
        return self.obs(), rew, done.astype(np.int32), fin_len, fin_rew


def test_host_env_learns_a_numpy_env(P):
    """An env written here in numpy, stepped only through the host path (obs 6: the generic engine): ep_len_mean climbs as in
    test_training_learns_cartpole (256 envs x 128 steps x 25 updates)."""
    N, T, U = 256, 128, 25
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, obs_size=6, num_envs=N, num_steps=T, num_minibatches=4, update_epochs=4, seed=2,
                                total_timesteps=N * T * U, ent_coef=0.0, learning_rate=1e-3))
    b.init_orthogonal(2)
    env = NumpyCartPole6(N, 0)
    b.host_env_reset(env.reset())
    first = None
    for u in range(U):
        b.host_rollout_begin()
        for _ in range(T):
            b.host_observe(*env.step(b.host_act()))
        b.host_rollout_end()
        st = b.stats()
        assert np.isfinite(st["loss"])
        if first is None:
            first = st["ep_len_mean"]
    assert st["updates"] == U and st["global_step"] == N * T * U
    assert st["ep_len_mean"] > max(100.0, 3 * first), (first, st)
    b.close()


def test_host_env_errors_leave_the_context_unchanged(P):
    N, T = 16, 8
    base = dict(num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2, seed=5, total_timesteps=N * T * 4, max_episode_steps=6)
    a = P.Context(P.make_config(**base))
    env = P.Context(P.make_config(**base))
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    a.init_orthogonal(3)
    b.set_params(a.get_params())

    def status(fn, *args):
        with pytest.raises(P.binding.PPOError) as e:
            fn(*args)
        return str(e.value)

    # the device env's entry points on a host-env context: PPO_ERR_UNSUPPORTED, naming the ppo_host_* calls
    for fn, args in ((b.env_reset, ()), (b.env_step, (np.zeros(N, np.int64),)), (b.rollout, ()), (b.train_iteration, ())):
        msg = status(fn, *args)
        assert "status 5" in msg and "ppo_host_act" in msg, msg
    # the ppo_host_* calls on a device-env context: PPO_ERR_STATE
    for fn, args in ((a.host_env_reset, (np.zeros((N, 4)),)), (a.host_rollout_begin, ()), (a.host_act, ()),
                     (a.host_observe, (np.zeros((N, 4)), np.zeros(N), np.zeros(N))), (a.host_rollout_end, ())):
        assert "status 3" in status(fn, *args)
    a.env_reset()
    obs0 = env.env_reset()
    b.host_env_reset(obs0)
    # out of sequence
    assert "status 3" in status(b.host_act)                                   # no rollout open
    assert "status 3" in status(b.host_rollout_end)
    b.host_rollout_begin()
    assert "status 3" in status(b.host_rollout_begin)                         # begin while open
    assert "status 3" in status(b.host_observe, obs0, np.zeros(N), np.zeros(N))   # observe before act
    act = b.host_act()
    assert "status 3" in status(b.host_act)                                   # act twice
    assert "status 3" in status(b.host_env_reset, obs0)                       # reset while open
    obs, rew, done = env.env_step(act)
    b.host_observe(obs, rew, done)
    assert "status 3" in status(b.host_rollout_end)                           # end before T steps
    for _ in range(T - 1):
        obs, rew, done = env.env_step(b.host_act())
        b.host_observe(obs, rew, done)
    assert "status 3" in status(b.host_act)                                   # past T
    b.host_rollout_end()
    a.train_iteration()
    assert_same_state(a, b)
    for c in (a, b, env):
        c.close()


@pytest.mark.parametrize("actions", [2, 4])
def test_host_obs8_reference_network_trains(P, actions):
    """obs 8 with the reference's 2 x 64 network (a LunarLander-like env): the reference-shape rollout kernels, the vector update kernel (the matrix-core
    update is built for 2 and 4 observations).  Two iterations train, the rollout's log-probs and values are ppo_policy_act's / ppo_get_value's on the
    stored observations (a twin context that never trains), and the parameters move."""
    N, T = 32, 16
    base = dict(obs_size=8, head_dims=(actions,), num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2, seed=3, total_timesteps=N * T * 2)
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    twin = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    b.init_orthogonal(5)
    p0 = b.get_params()
    twin.set_params(p0)
    rng = np.random.default_rng(2)
    b.host_env_reset(rng.standard_normal((N, 8)).astype(np.float32))
    for it in range(2):
        b.host_rollout_begin()
        acts = []
        for t in range(T):
            acts.append(b.host_act())
            b.host_observe(rng.standard_normal((N, 8)).astype(np.float32), rng.uniform(-1, 1, N).astype(np.float32),
                           (rng.random(N) < 0.1).astype(np.int32))
        if it == 0:
            b.sync()
            obs = b.read("OBS", (T, N, 8))
            lp = b.read("LOGPROBS", (T, N))
            for t in range(T):
                a_t, lp_t, _, _ = twin.policy_act(obs[t], step_index=t)
                assert np.array_equal(a_t, acts[t]) and np.array_equal(bits(lp_t), bits(lp[t])), t
        b.host_rollout_end()
        if it == 0:
            assert np.array_equal(bits(twin.get_value(obs.reshape(T * N, 8))), bits(b.read("VALUES")))
        st = b.stats()
        assert np.isfinite(st["loss"]) and st["updates"] == it + 1, st
    assert not np.array_equal(p0, b.get_params())
    b.close()
    twin.close()
