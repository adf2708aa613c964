"""Time-limit truncations of the library's own environments (include/ppo_hip.h: ppo_env_truncation_bootstrap / ppo_env_truncations) on the GPU.

The oracle is the merged host path (tests/test_gpu_host_env.py, tests/test_gpu_host_truncation.py).  Context `a` owns the device env with the switch on
and runs ppo_train_iteration.  Context `b` is a PPO_ENV_HOST context with the same parameters and seed whose envs are stepped by the test through a third
device-env context `env`; in front of every env step the test reads `env`'s state, and the stateless transition (ppo_env_transition) of that state under
the action gives the observation the step ends on and the env's own `terminated`: truncated = done & ~terminated, fed to `b` with
host_observe(truncated=, final_obs=).  After every iteration every rollout buffer, the parameters, the AdamW moments and the statistics of `a` are `b`'s
bit for bit, and so are the event lists.
"""
import numpy as np
import pytest

from __graft_entry__ import load_package
from test_gpu_host_env import assert_same_state, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return load_package()


def config(P, env_kind, N, T, limit, vector=False, masked=False, **kw):
    base = dict(num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2, seed=5, total_timesteps=N * T * 5, max_episode_steps=limit,
                kernel_flags=P.KERNEL_ROLLOUT_VECTOR if vector else 0)
    if env_kind == P.ENV_MOUNTAINCAR:
        base.update(obs_size=2, head_dims=(3,), dist_kind=P.DIST_MASKED if masked else P.DIST_CATEGORICAL)
    base.update(kw)
    return base


def inject(P, env_kind, ctx):
    """States that terminate at once, so that a run has episode ends that are no truncations: CartPole, every third env: pole angle 0.2 rad and angular
    velocity 1.0 (over the 12 degree threshold after one step); MountainCar, every fourth env: position 0.49 and velocity 0.06 (the goal).  Returns the
    state = the observation of every env."""
    state = ctx.env_get_state()[0]
    if env_kind == P.ENV_CARTPOLE:
        state[::3, 2], state[::3, 3] = 0.2, 1.0
    else:
        state[::4, 0], state[::4, 1] = 0.49, 0.06
    ctx.env_set_state(state=state)
    return state


def host_iteration_truncated(P, b, env, env_kind, mask=None):
    """One iteration of b on env's steps.  Returns (events, episode ends that are no events)."""
    limit = b.cfg.max_episode_steps
    events = others = 0
    b.host_rollout_begin()
    for _ in range(b.T):
        act = b.host_act(mask)
        state, ep_len, _, _ = env.env_get_state()
        final, _, terminated = P.env_transition(env, env_kind, state, act)
        obs, rew, done = env.env_step(act)
        trunc = ((done != 0) & (terminated == 0)).astype(np.int32)
        assert np.array_equal(done != 0, (terminated != 0) | (ep_len + 1 == limit))   # the env ends an episode for these two reasons only
        b.host_observe(obs, rew, done, truncated=trunc, final_obs=final)
        events += int(trunc.sum())
        others += int((done != 0).sum() - trunc.sum())
    b.host_rollout_end()
    return events, others


def run_against_host_path(P, env_kind, N, T, limit, iters=3, vector=False, masked=False, params_hook=None):
    cfg = config(P, env_kind, N, T, limit, vector, masked)
    a = P.Context(P.make_config(env_kind=env_kind, **cfg))
    env = P.Context(P.make_config(env_kind=env_kind, **cfg))
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, **cfg))
    a.init_orthogonal(11)
    params = a.get_params()
    if params_hook is not None:
        params_hook(params)
    a.set_params(params)
    b.set_params(params)
    a.env_truncation_bootstrap(True)
    a.env_reset()
    env.env_reset()
    inject(P, env_kind, a)
    b.host_env_reset(inject(P, env_kind, env))
    mask = np.ones((N, b.A), np.uint8) if masked else None
    events = others = 0
    for it in range(iters):
        a.train_iteration()
        e, o = host_iteration_truncated(P, b, env, env_kind, mask)
        st = assert_same_state(a, b, tag=it)
        (ia, va), (ib, vb) = a.env_truncations(), b.host_truncations()
        assert ia.dtype == np.int32 and ia.size == e and np.array_equal(ia, ib), (it, ia.size, ib.size, e)
        assert np.array_equal(bits(va), bits(vb)), it
        events += e
        others += o
    assert events > 0 and others > 0, (events, others)   # not vacuous: truncations were folded, and real ends were left alone
    assert st["updates"] == iters
    out = a.profile_read()["vector_fallback_launches"], b.profile_read()["vector_fallback_launches"]
    for c in (a, b, env):
        c.close()
    return out


@pytest.mark.parametrize("vector", [False, True])
@pytest.mark.parametrize("N", [7, 300])
def test_cartpole_equals_the_host_path(P, N, vector):
    """T * N = 168 (one ragged workgroup) and 7200 (29 workgroups of 256 samples, the last one ragged)"""
    fa, fb = run_against_host_path(P, P.ENV_CARTPOLE, N, 24, 12, vector=vector)
    assert fa == fb == 0


@pytest.mark.parametrize("masked", [False, True])
def test_mountaincar_equals_the_host_path(P, masked):
    run_against_host_path(P, P.ENV_MOUNTAINCAR, 96, 24, 10, masked=masked)


def test_weights_outside_the_fp16_range(P):
    """The hook of test_host_cartpole_weights_outside_rollout16_range: the actor's rollout falls back to the vector kernel in both contexts alike, the
    critic of the fold stays the one that fills VALUES."""
    def hook(p):
        p[-130] = 300.0
    fa, fb = run_against_host_path(P, P.ENV_CARTPOLE, 48, 16, 12, params_hook=hook)
    assert fa == fb and fb >= 3


def fold(r, v, gamma):
    return (r + (np.float32(gamma) * v).astype(np.float32)).astype(np.float32)


def test_limit_and_termination_on_the_same_step(P):
    """Envs 0..3 reach the limit on the very step on which the pole falls: FIN_LEN == max_episode_steps, no event, the raw reward.  Envs 4..7 reach the
    limit standing: events."""
    N, T, limit = 8, 8, 6
    a = P.Context(P.make_config(**config(P, P.ENV_CARTPOLE, N, T, limit)))
    a.init_orthogonal(11)
    a.env_truncation_bootstrap(True)
    a.env_reset()
    state = a.env_get_state()[0]
    state[:4, 2], state[:4, 3] = 0.2, 1.0
    a.env_set_state(state=state, ep_len=np.full(N, limit - 1, np.int32))
    a.rollout()
    idx, val = a.env_truncations()
    fin_len, rew = a.read("FIN_LEN", (T, N)), a.read("REWARDS", (T, N))
    assert (fin_len[0] == limit).all()
    assert np.array_equal(idx[idx < N], np.arange(4, 8))
    assert np.array_equal(bits(rew[0, :4]), bits(np.full(4, -1.0, np.float32)))          # CartPole pays -1 where the pole fell
    assert np.array_equal(bits(rew[0, 4:]), bits(fold(np.ones(4, np.float32), val[:4], a.cfg.gamma)))
    assert np.isfinite(val).all() and (bits(rew[0, 4:]) != bits(np.ones(4, np.float32))).any()
    # every event is a sample at the limit whose step did not terminate, and its value is the critic's on the recomputed final observation: within the
    # project's bar for values (3e-6) of ppo_get_value, as tests/test_gpu_host_truncation.py checks the host fold
    assert (fin_len.ravel()[idx] == limit).all()
    obs, act = a.read("OBS", (T * N, 4)), a.read("ACTIONS", (T * N, 1))
    final, _, terminated = P.env_transition(a, P.ENV_CARTPOLE, obs[idx], act[idx].astype(np.int64))
    assert not terminated.any()
    ref = a.get_value(final)   # (ppo_rollout alone does not move the parameters)
    assert np.abs(val - ref).max() <= 3e-6, np.abs(val - ref).max()
    a.close()


def test_off_is_off(P):
    cfg = config(P, P.ENV_CARTPOLE, 33, 24, 12)
    u, v = P.Context(P.make_config(**cfg)), P.Context(P.make_config(**cfg))
    u.init_orthogonal(11)
    v.set_params(u.get_params())
    v.env_truncation_bootstrap(True)
    v.env_truncation_bootstrap(False)
    u.env_reset()
    v.env_reset()
    for it in range(3):
        u.train_iteration()
        v.train_iteration()
        assert_same_state(u, v, tag=it)
        assert (u.read("FIN_LEN") == 12).any()   # there was something to fold
        for c in (u, v):
            idx, val = c.env_truncations()
            assert idx.size == 0 and val.size == 0
    u.close()
    v.close()


def test_stepwise_equals_fused(P):
    cfg = config(P, P.ENV_CARTPOLE, 33, 24, 12, anneal_lr=False)   # (ppo_train_iteration anneals the learning rate itself; the stepwise calls do not)
    f, s = P.Context(P.make_config(**cfg)), P.Context(P.make_config(**cfg))
    f.init_orthogonal(11)
    s.set_params(f.get_params())
    for c in (f, s):
        c.env_truncation_bootstrap(True)
        c.env_reset()
    for it in range(2):
        f.train_iteration()
        s.rollout()
        s.calc_advantage()
        s.update()
        assert_same_state(f, s, tag=it)
        (i_f, v_f), (i_s, v_s) = f.env_truncations(), s.env_truncations()
        assert i_f.size > 0 and np.array_equal(i_f, i_s) and np.array_equal(bits(v_f), bits(v_s))
    f.close()
    s.close()


def test_errors_leave_the_context_unchanged(P):
    N, T = 16, 8
    cfg = config(P, P.ENV_CARTPOLE, N, T, 6)
    a, twin = P.Context(P.make_config(**cfg)), P.Context(P.make_config(**cfg))
    syn = P.Context(P.make_config(env_kind=P.ENV_SYNTHETIC, obs_size=6, head_dims=(3, 2), num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2,
                                  seed=3, total_timesteps=N * T * 4, max_episode_steps=6))
    host = P.Context(P.make_config(env_kind=P.ENV_HOST, **cfg))

    def status(fn, *args):
        with pytest.raises(P.binding.PPOError) as e:
            fn(*args)
        return str(e.value)

    for c in (syn, host):
        for fn, args in ((c.env_truncation_bootstrap, (True,)), (c.env_truncations, ())):
            msg = status(fn, *args)
            assert "status 5" in msg, msg
            assert (c is syn) or "ppo_host_observe_truncated" in msg, msg
    assert "status 1" in status(a.env_truncation_bootstrap, 2)
    assert "status 1" in status(a.env_truncation_bootstrap, -1)
    a.init_orthogonal(3)
    twin.set_params(a.get_params())
    a.env_reset()
    twin.env_reset()
    a.train_iteration()
    twin.train_iteration()
    assert_same_state(a, twin)
    assert (a.read("FIN_LEN") == 6).any() and a.env_truncations()[0].size == 0   # the refused calls did not turn the switch on
    for c in (a, twin, syn, host):
        c.close()
