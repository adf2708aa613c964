"""PPO_ENV_PENDULUM (include/ppo_hip.h; ppo-libtorch_amd/csrc/kernels_gauss_fused.hip: gauss_rollout_kernel) on the GPU through the C-ABI: the env against
float64, the fused rollout against the stepwise API bit for bit, teacher forcing, a device iteration against the host-fed iteration, launch accounting,
episode statistics and every refusal.  Without the env none of these contexts can be created ("unknown env_kind 4").

Common setup: orthogonal init, the actor's output layer scaled by 30 and log_std = 0.3 (samples leave the torque range [-2, 2]), max_episode_steps = 7 and
T = 24: every env resets three times within a rollout, and the resets do not line up with T."""
import importlib.util
import os

import numpy as np
import pytest

from __graft_entry__ import ROOT, load_package

pytestmark = pytest.mark.gpu

T, MAXS = 24, 7
EPS = float(np.finfo(np.float32).eps)
ROLLOUT_BUFS = ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW", "NEXT_OBS", "NEXT_DONE", "VALUES", "NEXT_VALUE")
ALL_BUFS = ROLLOUT_BUFS + ("ADVANTAGES", "RETURNS", "PARAMS", "GRADS", "EXP_AVG", "EXP_AVG_SQ", "ENV_STATE", "EP_LEN", "EP_REW", "RESET_COUNT")


@pytest.fixture(scope="module")
def P():
    return load_package()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def pend_cfg(P, N, **kw):
    d = dict(env_kind=P.ENV_PENDULUM, dist_kind=P.DIST_GAUSSIAN, obs_size=3, head_dims=(1,), num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2,
             max_episode_steps=MAXS, seed=5, total_timesteps=4 * N * T, learning_rate=1e-3, anneal_lr=True, gamma=0.99, gae_lambda=0.95, ent_coef=0.01,
             kernel_flags=P.KERNEL_GAUSS_FUSED)
    d.update(kw)
    return P.make_config(**d)


def common_params(ctx):
    """the common setup's parameters: the flat vector ends with the actor's output layer W3 [1, 64], b3 [1] and log_std [1]"""
    ctx.init_orthogonal(11)
    p = ctx.get_params()
    p[-66:-2] *= 30.0
    p[-1] = 0.3
    return p


def pend_ctx(P, N, params=None, **kw):
    ctx = P.Context(pend_cfg(P, N, **kw))
    ctx.set_params(common_params(ctx) if params is None else params)
    return ctx


def rollout_buffers(ctx):
    return {k: ctx.read(k) for k in ROLLOUT_BUFS}


# ---------------------------------------------------------------------------------------------------------
# 1. the transition against float64
# ---------------------------------------------------------------------------------------------------------
def test_transition_against_float64(P):
    """ppo_env_transition_f32 on 4096 rows against the header's formulas in numpy float64 on the f32 inputs.  Bar per output and row: 8 x f32 epsilon x the
    largest intermediate magnitude of that output's formula (computed here in float64); for the reward that includes (|theta| + pi) 2 |thn|, the first-order
    effect of the rounding of theta + pi on thn^2; for cos / sin the bar of th' plus one ulp of the result.  The cost is continuous across the wrap
    ((-pi)^2 = pi^2) and both clips are continuous, so no row is left out.
    Measured on an MI355X, the largest error as a fraction of its bar: reward 0.136, th' 0.060, td' 0.057, cos 0.056, sin 0.056."""
    rng = np.random.default_rng(3)
    n = 4096
    pi32 = np.float32(np.pi)
    th = rng.uniform(-30, 30, n).astype(np.float32)
    thd = rng.uniform(-8, 8, n).astype(np.float32)
    a = rng.uniform(-3, 3, n).astype(np.float32)
    special = [pi32, -pi32, np.float32(0), np.nextafter(pi32, np.float32(4)), np.nextafter(pi32, np.float32(0)), np.nextafter(-pi32, np.float32(-4)),
               np.nextafter(-pi32, np.float32(0))]
    th[:len(special)] = special
    thd[7:9] = (8.0, -8.0)
    thd[0:2] = (8.0, -8.0)
    a[9:11] = (2.0, -2.0)
    a[2:4] = (2.0, -2.0)
    ctx = pend_ctx(P, 1)
    ns, ob, r, term = P.env_transition_f32(ctx, P.ENV_PENDULUM, np.stack([th, thd], 1), a)
    ns2, none, r2, _ = P.env_transition_f32(ctx, P.ENV_PENDULUM, np.stack([th, thd], 1), a, want_obs=False)
    ctx.close()
    assert none is None and same(ns, ns2) and same(r, r2) and not term.any()

    PI, TWO_PI = float(pi32), float(np.float32(2 * np.pi))
    t, d, act = th.astype(np.float64), thd.astype(np.float64), a.astype(np.float64)
    u = np.minimum(np.maximum(act, -2.0), 2.0)
    x = t + PI
    wrap = TWO_PI * np.floor(x / TWO_PI)
    thn = (x - wrap) - PI
    c0, c1, c2 = thn * thn, float(np.float32(0.1)) * (d * d), float(np.float32(0.001)) * (u * u)
    rew = -((c0 + c1) + c2)
    m_rew = np.max(np.abs([c0, c1, c2, c0 + c1, rew, (np.abs(t) + PI) * 2 * np.abs(thn)]), axis=0)
    g, tq = 15.0 * np.sin(t), 3.0 * u
    acc = (g + tq) * float(np.float32(0.05))
    td_raw = d + acc
    td = np.minimum(np.maximum(td_raw, -8.0), 8.0)
    m_td = np.max(np.abs([d, g, tq, g + tq, acc, td_raw]), axis=0)
    step = td * float(np.float32(0.05))
    th1 = t + step
    m_th = np.maximum(m_td, np.max(np.abs([t, step, th1]), axis=0))
    want = {"reward": (r, rew, 8 * EPS * m_rew), "th'": (ns[:, 0], th1, 8 * EPS * m_th), "td'": (ns[:, 1], td, 8 * EPS * m_td),
            "cos": (ob[:, 0], np.cos(th1), 8 * EPS * m_th + np.spacing(np.abs(np.cos(th1)).astype(np.float32))),
            "sin": (ob[:, 1], np.sin(th1), 8 * EPS * m_th + np.spacing(np.abs(np.sin(th1)).astype(np.float32))),
            "obs td'": (ob[:, 2], td, 8 * EPS * m_td)}
    worst = {k: float((np.abs(got.astype(np.float64) - exp) / bar).max()) for k, (got, exp, bar) in want.items()}
    print("largest error as a fraction of its bar:", {k: round(v, 4) for k, v in worst.items()})
    assert same(ob[:, 2], ns[:, 1])
    for k, v in worst.items():
        assert v <= 1.0, (k, v)


# ---------------------------------------------------------------------------------------------------------
# 2. the fused rollout against the stepwise API, bit for bit
# ---------------------------------------------------------------------------------------------------------
def stepwise_rollout(b, obs, done, step0):
    """T x { policy_act_f32(obs, step_index), env_step_f32 } on context b: the buffers a rollout would fill.  FIN_LEN / FIN_REW from the episode sums the
    context held in front of the step (f32 sum, the kernels' own operation)."""
    N = b.N
    out = {k: [] for k in ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW")}
    for t in range(T):
        act, lp, _, _ = b.policy_act_f32(obs, step_index=step0 + t)
        len0, rew0 = b.read("EP_LEN"), b.read("EP_REW")
        out["OBS"].append(obs)
        out["DONES"].append(done.astype(np.float32))
        obs, r, done = b.env_step_f32(act)
        out["ACTIONS"].append(act)
        out["LOGPROBS"].append(lp)
        out["REWARDS"].append(r)
        out["FIN_LEN"].append(np.where(done != 0, len0 + 1, 0).astype(np.int32))
        out["FIN_REW"].append(np.where(done != 0, rew0 + r, np.float32(0)).astype(np.float32))
        assert obs.shape == (N, 3)
    res = {k: np.stack(v).reshape(-1) for k, v in out.items()}
    res["NEXT_OBS"], res["NEXT_DONE"] = obs.reshape(-1), done
    return res, obs, done


@pytest.mark.parametrize("N", [1, 96, 200])
def test_fused_rollout_equals_stepwise_api(P, N):
    """N = 1: one lane; 96: a tile and a half; 200: three tiles and a bit.  Two rollouts: the second continues with step indices T .. 2 T - 1."""
    a, b = pend_ctx(P, N), pend_ctx(P, N)
    assert same(a.get_params(), b.get_params())
    obs = b.env_reset()
    assert same(a.env_reset(), obs)
    done = np.zeros(N, np.int32)
    n_done, beyond = 0, False
    for k in range(2):
        a.rollout()
        got = rollout_buffers(a)
        want, obs, done = stepwise_rollout(b, obs, done, k * T)
        for name, w in want.items():
            assert same(got[name], w), (k, name, int((bits(got[name]) != bits(w)).sum()))
        for x, y in zip(a.env_get_state(), b.env_get_state()):
            assert same(x, y)
        O = got["OBS"].reshape(T * N, 3)
        assert same(got["VALUES"], a.get_value(O))
        assert same(got["NEXT_VALUE"], a.get_value(got["NEXT_OBS"].reshape(N, 3)))
        # the stored raw sample, forced through the stand-alone policy, gives the stored log-prob's bits
        fa, flp, _, _ = a.policy_act_f32(O, action=got["ACTIONS"].reshape(T * N, 1))
        assert same(fa.reshape(-1), got["ACTIONS"]) and same(flp, got["LOGPROBS"])
        n_done += int(got["DONES"].sum() + got["NEXT_DONE"].sum())
        beyond = beyond or bool((np.abs(got["ACTIONS"]) > 2).any())
        assert set(np.unique(got["FIN_LEN"])) <= {0, MAXS}
    assert n_done > 0 and (beyond or N == 1)
    state, ep_len, _, resets = a.env_get_state()
    assert state.shape == (N, 2) and (resets == 1 + (2 * T) // MAXS + (np.arange(N) == 0)).all() and (ep_len == (2 * T) % MAXS).all()
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------
# 3. a row does not depend on its launch
# ---------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_launch(P):
    big, small = pend_ctx(P, 200), pend_ctx(P, 64)
    small.set_params(big.get_params())
    for ctx in (big, small):
        ctx.env_reset()
        ctx.rollout()
    gb, gs = rollout_buffers(big), rollout_buffers(small)
    for name in ROLLOUT_BUFS:
        per_step = name not in ("NEXT_OBS", "NEXT_DONE", "NEXT_VALUE")
        x = gb[name].reshape((T, 200, -1) if per_step else (200, -1))
        y = gs[name].reshape((T, 64, -1) if per_step else (64, -1))
        assert same(np.ascontiguousarray(x[:, :64] if per_step else x[:64]), y), name
    for x, y in zip(big.env_get_state(), small.env_get_state()):
        assert same(np.ascontiguousarray(x[:64]), y)
    big.close()
    small.close()


def test_injected_state_replays_the_rollout(P):
    """env_set_state / env_get_state carry the state as [N, 2]; NEXT_OBS follows the injected state, and a rollout from it is the original's, bit for bit"""
    N = 70
    a, b = pend_ctx(P, N), pend_ctx(P, N)
    obs0 = a.env_reset()
    s0 = a.env_get_state()
    assert s0[0].shape == (N, 2) and (np.abs(s0[0][:, 0]) <= np.float32(np.pi)).all() and (np.abs(s0[0][:, 1]) <= 1).all()
    b.env_set_state(*s0)
    assert same(b.read("NEXT_OBS", (N, 3)), obs0)
    for x, y in zip(s0, b.env_get_state()):
        assert same(x, y)
    a.rollout()
    b.rollout()
    ga, gb = rollout_buffers(a), rollout_buffers(b)
    assert all(same(ga[k], gb[k]) for k in ROLLOUT_BUFS)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------
# 4. teacher forcing
# ---------------------------------------------------------------------------------------------------------
def test_teacher_forcing(P):
    N = 96
    ctx = pend_ctx(P, N)
    ctx.env_reset()
    forced = np.random.default_rng(4).uniform(-3, 3, (T, N, 1)).astype(np.float32)
    ctx.rollout(forced_actions=forced)
    got = rollout_buffers(ctx)
    assert same(got["ACTIONS"], forced.reshape(-1))
    _, lp, _, v = ctx.policy_act_f32(got["OBS"].reshape(T * N, 3), action=forced.reshape(T * N, 1))
    assert same(lp, got["LOGPROBS"]) and same(v, got["VALUES"])
    # the env saw the clipped copy: replaying the stored states' successors is test 2's business; here the rewards' torque term shows the clip
    assert got["DONES"].sum() > 0 and (np.abs(forced) > 2).any()
    before = {k: ctx.read(k) for k in ALL_BUFS}
    with pytest.raises(P.binding.PPOError, match=r"status 5: .*ppo_rollout_f32"):
        ctx.rollout(forced_actions=np.zeros((T, N, 1), np.int64))
    assert all(same(before[k], ctx.read(k)) for k in ALL_BUFS)
    ctx.close()
    cart = P.Context(P.make_config(num_envs=8, num_steps=4, num_minibatches=1))
    d = cart.dev(np.zeros((4, 8, 1), np.float32))
    assert P.binding.lib().ppo_rollout_f32(cart.h, d.ptr) == 5 and b"ppo_rollout" in P.binding.lib().ppo_last_error(cart.h)
    cart.close()


# ---------------------------------------------------------------------------------------------------------
# 5. an iteration equals the host-fed iteration, bit for bit
# ---------------------------------------------------------------------------------------------------------
def test_iteration_equals_the_host_fed_iteration(P):
    """The new rollout feeds the existing update exactly what the host path feeds it: two train_iterations of a Pendulum context against a PPO_ENV_HOST
    Gaussian context (same config, PPO_KERNEL_GAUSS_FUSED) fed by host_act_f32, a third context's env_step_f32 and host_observe (fin_len / fin_rew NULL)."""
    N = 96
    dev = pend_ctx(P, N)
    host = P.Context(pend_cfg(P, N, env_kind=P.ENV_HOST))
    env = pend_ctx(P, N)
    params = dev.get_params()
    host.set_params(params)
    dev.env_reset()
    host.host_env_reset(env.env_reset())
    for _ in range(2):
        dev.train_iteration()
        host.host_rollout_begin()
        for _t in range(T):
            o, r, d = env.env_step_f32(host.host_act_f32())
            host.host_observe(o, r, d)
        host.host_rollout_end()
    sd, sh = dev.stats(), host.stats()
    for name in ("OBS", "ACTIONS", "LOGPROBS", "REWARDS", "DONES", "VALUES", "ADVANTAGES", "RETURNS", "FIN_LEN", "FIN_REW"):
        assert same(dev.read(name), host.read(name)), name
    assert same(dev.get_params(), host.get_params()) and not same(dev.get_params(), params)
    (m0, v0, k0), (m1, v1, k1) = dev.get_optimizer(), host.get_optimizer()
    assert same(m0, m1) and same(v0, v1) and k0 == k1 == 2 * 2 * 2
    assert sd == sh, (sd, sh)
    assert sd["ep_count"] == 100 and sd["ep_len_mean"] == MAXS and sd["global_step"] == 2 * N * T
    for c in (dev, host, env):
        c.close()


# ---------------------------------------------------------------------------------------------------------
# 6. launch accounting
# ---------------------------------------------------------------------------------------------------------
def test_launch_accounting(P):
    ctx = pend_ctx(P, 96)
    ctx.env_reset()
    a0, v0, u0 = ctx.gauss_fused_launches()
    ctx.rollout()
    a1, v1, u1 = ctx.gauss_fused_launches()
    assert (a1 - a0, v1 - v0, u1 - u0) == (0, 2, 0)   # the rollout kernel is not an act launch; the critic over OBS and over NEXT_OBS
    ctx.calc_advantage()
    a2, v2, u2 = ctx.gauss_fused_launches()
    ctx.update()
    a3, v3, u3 = ctx.gauss_fused_launches()
    assert (a3 - a2, u3 - u2) == (0, ctx.cfg.update_epochs * ctx.cfg.num_minibatches)
    ctx.sync()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 7. episode statistics
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [20, 96])
def test_episode_statistics(P, N):
    """N = 20: 60 episodes, the ring is not full; N = 96: 288 episodes, the ring keeps the last 100 in push order (step, then env).  The ring holds the
    FIN_REW values themselves (f32), so their float64 mean agrees to 1e-6 relative."""
    ctx = pend_ctx(P, N)
    ctx.env_reset()
    ctx.rollout()
    ctx.calc_advantage()
    ctx.update()
    st = ctx.stats()
    fin_len, fin_rew = ctx.read("FIN_LEN"), ctx.read("FIN_REW")
    n_done = int(ctx.read("DONES").sum() + ctx.read("NEXT_DONE").sum())
    assert n_done == int((fin_len > 0).sum()) == N * (T // MAXS)
    assert st["ep_count"] == min(n_done, 100) and st["ep_len_mean"] == MAXS
    last = fin_rew[fin_len > 0][-min(n_done, 100):].astype(np.float64)
    assert abs(st["ep_rew_mean"] - last.mean()) <= 1e-6 * abs(last.mean()), (st["ep_rew_mean"], last.mean())
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,status,word", [
    (dict(obs_size=4), 1, "observation of size 3"),
    (dict(obs_size=2), 1, "observation of size 3"),
    (dict(dist_kind=0), 5, "PPO_DIST_GAUSSIAN"),
    (dict(dist_kind=1), 5, "PPO_DIST_GAUSSIAN"),
    (dict(head_dims=(2,)), 5, "head_dims[0] = 1"),
    (dict(head_dims=(1, 1)), 5, "n_heads = 1"),
    (dict(hidden=32), 5, "hidden = 64"),
    (dict(n_hidden=3), 5, "n_hidden = 2"),
    (dict(compute_dtype=1), 5, "PPO_DTYPE_F32"),
    (dict(kernel_flags=0), 5, "PPO_KERNEL_GAUSS_FUSED"),
    (dict(max_episode_steps=500), 5, "max_episode_steps"),
    (dict(max_episode_steps=0), 5, "max_episode_steps"),
    (dict(env_kind=0, obs_size=4), 5, "PPO_ENV_HOST"),
    (dict(env_kind=1, obs_size=2), 5, "PPO_ENV_HOST"),
    (dict(env_kind=2), 5, "PPO_ENV_HOST"),
])
def test_ctx_create_refusals(P, kw, status, word):
    if "env_kind" in kw:   # Gaussian on CartPole, MountainCar and the synthetic env stays refused
        kw = dict(kw, head_dims=(1,))
    with pytest.raises(P.binding.PPOError) as e:
        P.Context(pend_cfg(P, 8, **kw))
    assert "status %d:" % status in str(e.value) and word in str(e.value), str(e.value)


def test_refused_calls_change_nothing(P):
    N = 40
    ctx = pend_ctx(P, N)
    ctx.env_reset()
    ctx.train_iteration()
    ctx.rollout()
    ctx.sync()
    snap = lambda: ({k: ctx.read(k) for k in ALL_BUFS}, ctx.get_optimizer()[2], ctx.gauss_fused_launches())   # noqa: E731
    before = snap()
    o, r, d, a64 = np.zeros((N, 3), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int32), np.zeros((N, 1), np.int64)
    d_o, d_r, d_d, d_a, d_a64 = ctx.dev(o), ctx.dev(r), ctx.dev(d), ctx.dev(np.zeros((N, 1), np.float32)), ctx.dev(a64)
    calls = [
        # the caller-stepped families: PPO_ERR_STATE, as on any device-env context
        (3, "device environment", lambda: ctx.host_env_reset(o)),
        (3, "device environment", lambda: ctx.host_rollout_begin()),
        (3, "device environment", lambda: ctx.host_rollout_begin(groups=2)),
        (3, "device environment", lambda: ctx.host_act_f32()),
        (3, "device environment", lambda: ctx.host_act()),
        (3, "device environment", lambda: ctx.host_observe(o, r, d)),
        (3, "device environment", lambda: ctx.host_observe(o, r, d, truncated=d, final_obs=o)),
        (3, "device environment", lambda: ctx.host_rollout_end()),
        (3, "device environment", lambda: ctx.host_truncations()),
        (3, "device environment", lambda: ctx.dev_env_reset(d_o)),
        (3, "device environment", lambda: ctx.dev_act_f32(d_a)),
        (3, "device environment", lambda: ctx.dev_act(d_a64)),
        (3, "device environment", lambda: ctx.dev_observe(d_o, d_r, d_d)),
        # not built for this env
        (5, "ppo_env_transition_f32", lambda: ctx.evaluate(4, 1)),
        (5, "theta", lambda: ctx.env_truncation_bootstrap(True)),
        (5, "theta", lambda: ctx.env_truncations()),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_enable(1)),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_get()),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_set(np.zeros(3), np.ones(3), 1.0)),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_apply(o)),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_enable(1)),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_get()),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_set(0.0, 1.0, 1.0)),
        # the integer-action calls name their twins
        (5, "ppo_env_step_f32", lambda: ctx.env_step(a64)),
        (5, "ppo_rollout_f32", lambda: ctx.rollout(forced_actions=np.zeros((T, N, 1), np.int64))),
        (5, "ppo_policy_act_f32", lambda: ctx.policy_act(o)),
    ]
    for status, word, call in calls:
        with pytest.raises(P.binding.PPOError) as e:
            call()
        assert "status %d:" % status in str(e.value) and word in str(e.value), str(e.value)
    ctx.sync()
    after = snap()
    assert before[1:] == after[1:]
    for k in ALL_BUFS:
        assert same(before[0][k], after[0][k]), k
    # and the context still works
    ctx.train_iteration()
    assert np.isfinite(ctx.stats()["loss"])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 9. the Gaussian path learns
# ---------------------------------------------------------------------------------------------------------
def test_pendulum_learns(P):
    """tools/pendulum_curve.py's run, one seed: 1024 envs x 64 steps, its default hyper-parameters, 300 iterations (2.3 s of training on an MI355X).  The
    tool measured, over seeds 1 .. 5, greedy returns on 256 fixed start states of -1240 .. -1266 untrained and -175 .. -188 trained: improvements of
    1061.92, 1067.05, 1068.51, 1091.09 and 1073.08 (profiles/NOTES.md).  The bar is half of the smallest: 530.96."""
    spec = importlib.util.spec_from_file_location("pendulum_curve", os.path.join(ROOT, "tools", "pendulum_curve.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse([])
    assert (args.iters, args.gamma, args.lr, args.epochs, args.minibatches) == (300, 0.95, 3e-4, 10, 8)
    ctx = tool.make_ctx(P, 1, args)
    ctx.init_orthogonal(1)
    ctx.env_reset()
    states = tool.start_states()
    untrained = tool.greedy_return(P, ctx, states)
    for _ in range(args.iters):
        ctx.train_iteration()
    trained = tool.greedy_return(P, ctx, states)
    print("greedy return: untrained %.2f, trained %.2f, improvement %.2f (bar 530.96)" % (untrained, trained, trained - untrained))
    ctx.close()
    assert trained - untrained >= 530.96
