"""PPO_KERNEL_ENV_MATRIX (include/ppo_hip.h, ppo-libtorch_amd/csrc/kernels_env_matrix.hip) on the GPU through the C-ABI: the one-launch rollouts and evaluations
of the seven fused device envs behind the resident f32 matrix-core forward.  The flagged rollout equals a stepwise loop of ppo_policy_act* + ppo_env_step* on
the same flagged context bit for bit; its stored log-probs and values hold the family's forward bar (3e-6 max(1, |x|)) against a plain float64 numpy network,
a minibatch step's gradient the family's gradient bar (5e-6 of each tensor's largest oracle element), ppo_evaluate equals episodes stepped on the host.
Without the flag's bit none of these contexts can be created ("unknown bits in kernel_flags").

Shapes: N = 64 (one exact tile) and 70 (a full tile and a short one of 6); T = 5 with max_episode_steps = 3, so resets fall inside the rollout.  The seven envs
run every layer-1 quarter count: 1 (obs 3, 2, 6, 16), 2 (19), 3 (45), 4 (64)."""
import numpy as np
import pytest
import torch

import cat_fused_shapes as S
import grad_oracle as G
import taxi_model as M
from __graft_entry__ import load_package
from test_evaluate_abi import start_states
from test_gpu_cat_fused import make_ctx as cat_make_ctx, write_batch
from test_gpu_cut_state import bits, envs, same
from test_gpu_fused_wide_obs import check_step
from test_gpu_gauss_fused import FWD_BAR, fill_buffers, rel
from test_gpu_gaussian import HP, ppo_loss, randomised_params, t64, tensor_shapes, unflatten
from test_gpu_mountaincar_continuous import EVAL_MAX, host_episodes as mcc_episodes, pumping_params
from test_gpu_taxi import host_episodes as taxi_episodes, reset_states

pytestmark = pytest.mark.gpu

T, MAXS, SEED = 5, 3, 5
ENVS = ("pendulum", "mcc", "acrobot", "taxi_masked", "frozenlake", "frozenlake8x8", "blackjack")


@pytest.fixture(scope="module")
def P():
    return load_package()


def make_ctx(P, env, n, extra=0, **kw):
    kind, dist, obs, actions, family, gauss = envs(P)[env]
    d = dict(env_kind=kind, dist_kind=dist, obs_size=obs, head_dims=(actions,), num_envs=n, num_steps=T, num_minibatches=1, update_epochs=1,
             max_episode_steps=MAXS, seed=SEED, total_timesteps=1 << 30, learning_rate=1e-3, anneal_lr=False, norm_adv=True, clip_vloss=True,
             kernel_flags=family | P.KERNEL_ENV_MATRIX | extra, **HP)
    d.update(kw)
    ctx = P.Context(P.make_config(**d))
    # the flat vector ends with the actor's output layer W3 [A, 64], b3 [A] (and log_std [1] on a Gaussian policy): scaled, so that every action is drawn
    ctx.init_orthogonal(11)
    p = ctx.get_params()
    if gauss:
        p[-66:-2] *= 30.0
        p[-1] = 0.3
    else:
        p[-(actions * 65):-actions] *= 30.0
    ctx.set_params(p)
    ctx.env_reset()
    return ctx


def stepwise_rollout(P, b, env):
    """T x { policy_act*(obs, the mask of the state, step_index), env_step* } on context b: the buffers a rollout would fill"""
    _, dist, obs_size, actions, _, gauss = envs(P)[env]
    obs, done = b.read("NEXT_OBS", (b.N, obs_size)), b.read("NEXT_DONE")
    out = {k: [] for k in ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW") + (() if gauss else ("MASKS",))}
    for t in range(T):
        state, len0, rew0, _ = b.env_get_state()
        out["OBS"].append(obs)
        out["DONES"].append(done.astype(np.float32))
        if gauss:
            act, lp = b.policy_act_f32(obs, step_index=t)[:2]
            obs, r, done = b.env_step_f32(act)
            out["ACTIONS"].append(act)
        else:
            mask = M.mask(state.astype(np.int64)) if dist == P.DIST_MASKED else None
            act, lp = b.policy_act(obs, mask=mask, step_index=t)[:2]
            obs, r, done = b.env_step(act)
            out["ACTIONS"].append(act.astype(np.int32))
            out["MASKS"].append(np.ones((b.N, actions), np.uint8) if mask is None else mask.astype(np.uint8))
        out["LOGPROBS"].append(lp)
        out["REWARDS"].append(r)
        out["FIN_LEN"].append(np.where(done != 0, len0 + 1, 0).astype(np.int32))
        out["FIN_REW"].append(np.where(done != 0, rew0 + r, np.float32(0)).astype(np.float32))
    res = {k: np.stack(v).reshape(-1) for k, v in out.items()}
    res["NEXT_OBS"], res["NEXT_DONE"] = obs.reshape(-1), done
    return res


def forward64(params, obs_size, actions, x):
    """the plain float64 2 x 64 tanh networks of the flat vector: critic (W1 b1 W2 b2 W3 b3), actor (the same), then log_std -> (value, actor output, the tail)"""
    p, at, outs = params.astype(np.float64), 0, []
    for width in (1, actions):
        h = x.astype(np.float64)
        for i, (r, c) in enumerate(((64, obs_size), (64, 64), (width, 64))):
            W, b = p[at:at + r * c].reshape(r, c), p[at + r * c:at + r * c + r]
            at += r * c + r
            h = h @ W.T + b
            h = np.tanh(h) if i < 2 else h
        outs.append(h)
    return outs[0][:, 0], outs[1], p[at:]


@pytest.mark.parametrize("n", [64, 70])
@pytest.mark.parametrize("env", ENVS)
def test_rollout_equals_the_stepwise_loop_and_holds_float64(P, env, n):
    _, dist, obs_size, actions, _, gauss = envs(P)[env]
    a, b = make_ctx(P, env, n), make_ctx(P, env, n)
    a.rollout()
    got = {k: a.read(k) for k in ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW", "NEXT_OBS", "NEXT_DONE", "VALUES", "MASKS")}
    want = stepwise_rollout(P, b, env)
    for name, w in want.items():
        assert same(got[name], w), (name, int((bits(got[name]) != bits(w)).sum()))
    for x, y in zip(a.env_get_state(), b.env_get_state()):   # ENV_STATE, EP_LEN, EP_REW, RESET_COUNT
        assert same(x, y)
    assert (got["FIN_LEN"] == MAXS).any() and (got["DONES"] == 1).any()   # resets inside the rollout
    if dist == P.DIST_MASKED:
        assert (got["MASKS"] == 0).any() and (got["MASKS"].reshape(-1, actions)[np.arange(T * n), got["ACTIONS"]] == 1).all()
    # the stored log-probs and values against the float64 network, from the stored observations and actions
    x = got["OBS"].reshape(T * n, obs_size)
    v64, out64, tail = forward64(a.get_params(), obs_size, actions, x)
    if gauss:
        z = (got["ACTIONS"].astype(np.float64) - out64[:, 0]) / np.exp(tail[0])
        lp64 = -0.5 * z * z - tail[0] - 0.5 * np.log(2.0 * np.pi)
    else:
        logits = np.where(got["MASKS"].reshape(T * n, actions) != 0, out64, G.MASK_FILL)
        logits = logits - logits.max(axis=1, keepdims=True)
        lp64 = (logits - np.log(np.exp(logits).sum(axis=1, keepdims=True)))[np.arange(T * n), got["ACTIONS"]]
    e_lp, e_v = rel(got["LOGPROBS"], lp64), rel(got["VALUES"], v64)
    print("%s n %d: log-prob %.3g value %.3g of the float64 forward (bar %.3g)" % (env, n, e_lp, e_v, FWD_BAR))
    assert e_lp <= FWD_BAR and e_v <= FWD_BAR
    assert same(got["VALUES"], a.get_value(x))
    a.close()
    b.close()


def test_gaussian_minibatch_step_against_float64(P):
    """MountainCarContinuous; 65 rows: a tile and a ragged one.  The float64 loss is the Gaussian family's own (tests/test_gpu_gaussian.py: ppo_loss)"""
    obs, D, N, M_ = 2, 1, 8, 65
    rng = np.random.default_rng(17)
    shapes = tensor_shapes(obs, 64, 2, D)
    ctx = make_ctx(P, "mcc", N, num_steps=41)
    params = randomised_params(ctx, shapes, rng)
    buf = fill_buffers(ctx, params, shapes, obs, D, N * 41, rng)
    idx = rng.permutation(N * 41)[:M_].astype(np.int32)
    grads = ctx.minibatch_forward_backward(idx)
    st = ctx.stats()
    ts = unflatten(params, shapes, grad=True)
    li = torch.as_tensor(idx.astype(np.int64))
    loss, sc = ppo_loss(ts, *(t64(b)[li] for b in buf), dict(HP, norm_adv=True, clip_vloss=True))
    loss.backward()
    check_step("mcc M %d" % M_, obs, st, sc, grads, np.concatenate([t.grad.numpy().ravel() for t in ts]), shapes)
    ctx.close()


def test_masked_minibatch_step_against_float64(P):
    """Taxi's shape under PPO_DIST_MASKED on the stand-in batch of tests/grad_oracle.py; 65 rows"""
    s = S._cat(19, (6,), True, seed=71)
    b = G.stand_in_batch(s)
    ctx = cat_make_ctx(P, s, P.KERNEL_CAT_FUSED | P.KERNEL_ENV_MATRIX, nmb=1, env_kind=P.ENV_TAXI, max_episode_steps=MAXS)
    write_batch(ctx, s, b)
    idx = np.random.default_rng(65).permutation(b["obs"].shape[0])[:65].astype(np.int32)
    grads = ctx.minibatch_forward_backward(idx)
    st = ctx.stats()
    g64, s64 = G.minibatch_grads(b["shapes"], s["heads"], True, G.shape_hp(s), b["params"], b["obs"], b["actions"], b["logp"], b["adv"], b["ret"], b["values"], idx,
                                 b["masks"])
    check_step("taxi masked M 65", 19, st, s64, grads, g64, [tuple(int(v) for v in r if v) for r in np.asarray(b["shapes"]).reshape(-1, 2)])
    ctx.close()


@pytest.fixture(scope="module")
def O():
    import oracle   # Philox, for the evaluation's start states
    oracle.build()
    return oracle


@pytest.mark.parametrize("env", ["mcc", "taxi_masked"])
def test_evaluate_equals_episodes_stepped_on_the_host(P, O, env):
    """70 episodes (a full tile and a short one), greedy and sampled: every return, length and truncated count is the host loop's on the same context"""
    n, seed, gauss = 70, 9, env == "mcc"
    steps = EVAL_MAX if gauss else 12
    ctx = make_ctx(P, env, 8, max_episode_steps=steps, seed=seed)   # the host loop's draws are keyed by the context's seed
    if gauss:
        ctx.set_params(pumping_params(ctx))
        states = start_states(O, 1, seed, n)
    else:
        states = reset_states(O, seed, np.arange(n), [0] * n)
    for greedy in (True, False):
        st, ret, length = ctx.evaluate(n, seed, greedy=greedy)
        h_ret, h_len, h_trunc = (mcc_episodes(P, ctx, states, greedy) if gauss else taxi_episodes(P, ctx, states, greedy, steps, True))[:3]
        print(env, "greedy" if greedy else "sampled", "lengths %d..%d, truncated %d of %d" % (length.min(), length.max(), st["truncated"], n))
        assert np.array_equal(length, h_len) and same(ret, h_ret) and st["truncated"] == int(h_trunc.sum())
    ctx.close()


def test_what_a_flagged_context_refuses_and_serves(P):
    ctx = make_ctx(P, "mcc", 70, extra=P.KERNEL_ENV_REWARD_NORM)
    with pytest.raises(P.binding.PPOError) as e:
        ctx.env_truncation_bootstrap(True)
    assert "status 5" in str(e.value) and "PPO_KERNEL_ENV_MATRIX" in str(e.value)
    ctx.reward_norm_enable(1)
    ctx.rollout()
    raw = make_ctx(P, "mcc", 70)
    raw.rollout()
    mean, var, count = ctx.reward_norm_get()
    assert count > 0 and var > 0 and np.isfinite(mean)
    assert same(ctx.read("ACTIONS"), raw.read("ACTIONS")) and not same(ctx.read("REWARDS"), raw.read("REWARDS"))
    pend = make_ctx(P, "pendulum", 8)
    with pytest.raises(P.binding.PPOError) as e:
        pend.evaluate(4, 1)
    assert "ppo_evaluate is not built for PPO_ENV_PENDULUM" in str(e.value)
    for c in (ctx, raw, pend):
        c.close()
