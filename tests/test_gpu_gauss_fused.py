"""PPO_KERNEL_GAUSS_FUSED (include/ppo_hip.h, ppo-libtorch_amd/csrc/kernels_gauss_fused.hip): Gaussian policies on a 2 x 64 f32 network through their own
act / value / update kernels, on the GPU through the C-ABI.

The oracle is tests/test_gpu_gaussian.py's float64 torch restatement (imported, never the library), the bars are the project's (3e-6
forward, 1e-5 loss scalars, 5e-6 of the largest gradient element, 2e-5 after a whole update).  Without the flag's support every context here is refused at
creation ("unknown bits in kernel_flags")."""
import numpy as np
import pytest
import torch

from __graft_entry__ import load_package
from test_gpu_gaussian import (HP, LEARN, LEARN_ORACLE_ITERS, Bandit, bits, gauss_entropy, gauss_logprob, host_rollout, make_ctx, mlp, nets, oracle_update,
                               ppo_loss, randomised_params, t64, tensor_shapes, unflatten)

pytestmark = pytest.mark.gpu

FWD_BAR, GRAD_BAR = 3e-6, 5e-6
MAX_BLOCKS = 128   # GAUSS_FUSED_MAX_BLOCKS (csrc/gauss_fused.hpp): the update kernel's workgroups per net


@pytest.fixture(scope="module")
def P():
    return load_package()


def fused_ctx(P, obs, D, **kw):
    return make_ctx(P, obs, D, kernel_flags=P.KERNEL_GAUSS_FUSED, **kw)


def rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


# ---------------------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs,D", [(1, 1), (3, 1), (11, 3), (17, 6), (33, 17), (64, 32)])
def test_forward_against_the_oracle(P, obs, D):
    """policy_act_f32 with forced actions, n = 1 (one lane), 63 / 64 / 65 (around a tile), 300 (several workgroups, a partial last tile): log-prob, entropy
    and value within 3e-6 max(1, |x|) of float64; the greedy action is the mean's bits (the mean whose log-prob at itself is -sum(log_std) - D log(2 pi) / 2)."""
    rng = np.random.default_rng(1000 * obs + D)
    shapes = tensor_shapes(obs, 64, 2, D)
    ctx = fused_ctx(P, obs, D)
    assert ctx.P == sum(int(np.prod(s)) for s in shapes)
    params = randomised_params(ctx, shapes, rng)
    critic, actor, log_std = nets(unflatten(params, shapes))
    for n in (1, 63, 64, 65, 300):
        x = rng.uniform(-1, 1, (n, obs)).astype(np.float32)
        mu = mlp(actor, t64(x))
        a = (mu.numpy() + rng.uniform(-4, 4, (n, D)) * np.exp(log_std.numpy())).astype(np.float32)
        act, lp, en, v = ctx.policy_act_f32(x, action=a, step_index=7)
        lp_o, en_o, v_o = gauss_logprob(mu, log_std, t64(a)).numpy(), gauss_entropy(mu, log_std).numpy(), mlp(critic, t64(x)).squeeze(-1).numpy()
        ag, lpg, _, vg = ctx.policy_act_f32(x, greedy=True)
        err_mu = rel(ag, mu.numpy())
        print("obs %d D %d n %d: log-prob %.3g entropy %.3g value %.3g mean %.3g" % (obs, D, n, rel(lp, lp_o), rel(en, en_o), rel(v, v_o), err_mu))
        assert np.array_equal(bits(act), bits(a))
        assert rel(lp, lp_o) <= FWD_BAR and rel(en, en_o) <= FWD_BAR and rel(v, v_o) <= FWD_BAR
        assert rel(ctx.get_value(x), v_o) <= FWD_BAR
        assert err_mu <= FWD_BAR
        # greedy: action = the mean, bit for bit -- forcing the greedy action gives the greedy log-prob's bits, and the same value
        _, lpf, _, vf = ctx.policy_act_f32(x, action=ag)
        assert np.array_equal(bits(lpf), bits(lpg)) and np.array_equal(bits(vf), bits(vg))
        assert rel(lpg, gauss_logprob(t64(ag), log_std, t64(ag)).numpy()) <= FWD_BAR
    assert ctx.gauss_fused_launches()[2] == 0
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 2. the draw is the generic path's draw
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs,D", [(11, 3), (17, 6), (64, 32)])
def test_draw_equals_the_stateless_gaussian(P, obs, D):
    rng = np.random.default_rng(obs)
    shapes = tensor_shapes(obs, 64, 2, D)
    seed, step = 21, 40
    ctx = fused_ctx(P, obs, D, seed=seed)
    params = randomised_params(ctx, shapes, rng)
    x = rng.uniform(-1, 1, (300, obs)).astype(np.float32)
    mean = ctx.policy_act_f32(x, greedy=True)[0]
    a, lp, _, _ = ctx.policy_act_f32(x, step_index=step)
    want = P.gaussian(ctx, mean, params[-D:], None, seed, 0, step)
    assert np.array_equal(bits(a), bits(want["sample"]))
    assert np.array_equal(bits(lp), bits(want["log_prob"]))
    assert (bits(a) != bits(mean)).mean() > 0.99
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 3. one minibatch step
# ---------------------------------------------------------------------------------------------------------
def fill_buffers(ctx, params, shapes, obs, D, B, rng):
    """test_minibatch_loss_and_gradient's construction: about a third of the rows clip on each side"""
    critic, actor, log_std = nets(unflatten(params, shapes))
    x = rng.uniform(-1, 1, (B, obs)).astype(np.float32)
    with torch.no_grad():
        mu = mlp(actor, t64(x))
        a = (mu.numpy() + rng.normal(0, 1, (B, D)) * np.exp(log_std.numpy())).astype(np.float32)
        lp_now = gauss_logprob(mu, log_std, t64(a)).numpy()
        v_now = mlp(critic, t64(x)).squeeze(-1).numpy()
    shift = np.where(np.arange(B) % 3 == 0, 0.4, np.where(np.arange(B) % 3 == 1, -0.4, 0.02)) * rng.uniform(0.6, 1.0, B)
    oldlp = (lp_now - shift).astype(np.float32)
    adv = rng.normal(0, 1, B).astype(np.float32)
    oldv = (v_now + rng.normal(0, 0.3, B)).astype(np.float32)
    ret = (v_now + rng.normal(0, 0.5, B)).astype(np.float32)
    for name, arr in (("OBS", x), ("ACTIONS", a), ("LOGPROBS", oldlp), ("ADVANTAGES", adv), ("RETURNS", ret), ("VALUES", oldv)):
        ctx.write(name, arr)
    return x, a, oldlp, adv, ret, oldv


# rows of the minibatch: 1 = a single lane of a single tile (norm_adv off: one row has no standard deviation); 82 = a partial tile behind a whole one;
# 128 = whole tiles only; 2624 = 41 workgroups per net, so 41 slabs to add; 8256 = 129 tiles > MAX_BLOCKS workgroups: workgroup 0 walks two tiles
@pytest.mark.parametrize("obs,D,N,T,M,norm_adv,clip_vloss", [(3, 1, 8, 41, 1, False, True), (11, 3, 8, 41, 82, True, True), (17, 6, 8, 41, 128, True, False),
                                                             (33, 17, 8, 328, 2624, False, False), (64, 32, 64, 129, 8256, True, True)])
def test_minibatch_loss_and_gradient(P, obs, D, N, T, M, norm_adv, clip_vloss):
    B = N * T
    assert M <= B and (M != 8256 or (M + 63) // 64 > MAX_BLOCKS)
    rng = np.random.default_rng(7 * D + M)
    shapes = tensor_shapes(obs, 64, 2, D)
    ctx = fused_ctx(P, obs, D, N=N, T=T, nmb=1, norm_adv=norm_adv, clip_vloss=clip_vloss)
    params = randomised_params(ctx, shapes, rng)
    buf = fill_buffers(ctx, params, shapes, obs, D, B, rng)
    idx = rng.permutation(B)[:M].astype(np.int32)
    if M == 1:
        idx = np.array([3 * 17], np.int32)   # a row pushed above the clip range
    grads = ctx.minibatch_forward_backward(idx)
    st = ctx.stats()
    grads2 = ctx.minibatch_forward_backward(idx)
    assert np.array_equal(bits(grads), bits(grads2))
    assert ctx.gauss_fused_launches() == (0, 0, 2)
    ts = unflatten(params, shapes, grad=True)
    li = torch.as_tensor(idx.astype(np.int64))
    loss, sc = ppo_loss(ts, *(t64(b)[li] for b in buf), dict(HP, norm_adv=norm_adv, clip_vloss=clip_vloss))
    loss.backward()
    if M == 1:
        assert sc["clipfrac"] == 1.0   # of one row the clipped share is 0 or 1
    else:
        assert 0.4 < sc["clipfrac"] < 0.9, sc["clipfrac"]
    for key, okey in (("pg_loss", "pg_loss"), ("v_loss", "v_loss"), ("entropy_loss", "entropy_loss"), ("approx_kl", "approx_kl"), ("clipfrac_last", "clipfrac")):
        print("%s %.9g oracle %.9g" % (key, st[key], sc[okey]))
        assert abs(st[key] - sc[okey]) <= 1e-5, (key, st[key], sc[okey])
    g_o = [t.grad.numpy() for t in ts]
    g_max = max(np.abs(g).max() for g in g_o)
    at = 0
    for i, g in enumerate(g_o):
        got = grads[at:at + g.size].reshape(g.shape)
        at += g.size
        err = np.abs(got - g).max() / g_max
        print("M %d tensor %d %s: err %.3g of the largest gradient element (%.3g)" % (M, i, g.shape, err, g_max))
        assert err <= GRAD_BAR, (i, err)
    assert at == ctx.P
    assert np.abs(g_o[-1]).max() > 1e-4 * g_max   # log_std's gradient is not trivially zero
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 4. one whole update
# ---------------------------------------------------------------------------------------------------------
def test_one_whole_update_against_the_oracle(P):
    """8 envs x 41 steps, 2 epochs x 4 minibatches of 82 rows, as tests/test_gpu_gaussian.py::test_one_whole_update_against_the_oracle"""
    N, T, nmb, epochs, obs, D, lr = 8, 41, 4, 2, 2, 2, 1e-3
    shapes = tensor_shapes(obs, 64, 2, D)
    ctx = fused_ctx(P, obs, D, N=N, T=T, nmb=nmb, epochs=epochs, lr=lr)
    ctx.init_orthogonal(4)
    p0 = ctx.get_params()
    env = Bandit(N, 1)
    ctx.host_env_reset(env.reset())
    rec = dict(obs=[], act=[])
    host_rollout(ctx, env, T, rec)
    ctx.sync()
    B, MB = N * T, N * T // nmb
    acts = ctx.read("ACTIONS", (T, N, D))
    assert np.array_equal(bits(acts), bits(np.stack(rec["act"])))
    assert np.array_equal(bits(ctx.read("OBS", (T, N, obs))), bits(np.stack(rec["obs"])))
    buf = [t64(ctx.read("OBS", (B, obs))), t64(acts.reshape(B, D)), t64(ctx.read("LOGPROBS")), t64(ctx.read("ADVANTAGES")), t64(ctx.read("RETURNS")),
           t64(ctx.read("VALUES"))]
    perm = ctx.read("PERM", (epochs, B))
    p_o, m_o, v_o = oracle_update(p0, shapes, buf, perm, MB, dict(HP, norm_adv=True, clip_vloss=True), float(np.float32(lr)))
    p1 = ctx.get_params()
    m1, v1, step = ctx.get_optimizer()
    assert step == epochs * nmb
    err_p = np.abs(p1 - p_o).max()
    err_m, err_v = np.abs(m1 - m_o).max() / np.abs(m_o).max(), np.abs(v1 - v_o).max() / np.abs(v_o).max()
    print("after %d optimizer steps: parameters %.3g, exp_avg %.3g, exp_avg_sq %.3g" % (step, err_p, err_m, err_v))
    assert np.abs(p1 - p0).max() > 1e-3 and np.all(p1[-D:] != 0.0)
    assert err_p <= 2e-5 and err_m <= 2e-5 and err_v <= 2e-5
    assert ctx.gauss_fused_launches() == (T, 2, epochs * nmb)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 5. bit identities
# ---------------------------------------------------------------------------------------------------------
def test_host_act_equals_stepwise_policy_and_device_feed(P):
    N, T, obs, D = 150, 6, 11, 17   # three tiles, the last one partial
    rng = np.random.default_rng(5)
    shapes = tensor_shapes(obs, 64, 2, D)
    feed = [rng.uniform(-1, 1, (N, obs)).astype(np.float32) for _ in range(T + 1)]
    rews = [rng.normal(0, 1, N).astype(np.float32) for _ in range(T)]
    dones = [(rng.uniform(0, 1, N) < 0.2).astype(np.int32) for _ in range(T)]
    host, dev, step = (fused_ctx(P, obs, D, N=N, T=T, seed=21) for _ in range(3))
    params = randomised_params(host, shapes, rng)
    dev.set_params(params)
    step.set_params(params)
    host.host_env_reset(feed[0])
    host.host_rollout_begin()
    got = []
    for t in range(T):
        got.append(host.host_act_f32())
        host.host_observe(feed[t + 1], rews[t], dones[t])
    for t in range(T):
        a, lp, _, _ = step.policy_act_f32(feed[t], step_index=t)
        assert np.array_equal(bits(a), bits(got[t])), t
    host.host_rollout_end()
    host.sync()
    lps = host.read("LOGPROBS", (T, N))
    for t in range(T):
        assert np.array_equal(bits(step.policy_act_f32(feed[t], step_index=t)[1]), bits(lps[t])), t
    assert np.array_equal(bits(host.read("ACTIONS", (T, N, D))), bits(np.stack(got)))
    assert np.array_equal(bits(host.read("OBS", (T, N, obs))), bits(np.stack(feed[:T])))
    assert np.array_equal(host.read("DONES", (T, N))[1:], np.stack(dones[:-1]).astype(np.float32)) and not host.read("DONES", (T, N))[0].any()
    d_act = dev.empty((N, D), np.float32)
    dev.dev_env_reset(dev.dev(feed[0]))
    dev.host_rollout_begin()
    for t in range(T):
        dev.dev_act_f32(d_act)
        dev.sync()
        assert np.array_equal(bits(d_act.download()), bits(got[t])), t
        dev.dev_observe(dev.dev(feed[t + 1]), dev.dev(rews[t]), dev.dev(dones[t], np.int32))
    dev.host_rollout_end()
    dev.sync()
    for name in ("ACTIONS", "LOGPROBS", "OBS", "REWARDS", "DONES", "VALUES", "ADVANTAGES"):
        assert np.array_equal(host.read(name).view(np.uint32), dev.read(name).view(np.uint32)), name
    assert np.array_equal(bits(host.get_params()), bits(dev.get_params()))
    for c in (host, dev, step):
        c.close()


def test_value_identities_under_the_normalisers(P):
    """get_value(obs) == PPO_BUF_VALUES == the V(final obs) ppo_host_truncations reports, on the SAME observation, with observation and reward normalisation
    on.  Learning rate 0 keeps the parameters' bits through the rollout's update (asserted), so get_value afterwards is the critic the rollout's end ran.  The
    second rollout normalises with frozen statistics (mode 2), so a raw observation has one normalised image wherever it enters: raw row F is fed as env 7's
    observation for step 5 and as the final observation of env 5's episode that a time limit cuts at step 3."""
    N, T, obs, D = 70, 8, 5, 3
    rng = np.random.default_rng(6)
    ctx = fused_ctx(P, obs, D, N=N, T=T, nmb=2, epochs=2, lr=0.0)
    randomised_params(ctx, tensor_shapes(obs, 64, 2, D), rng)
    ctx.obs_norm_enable()
    ctx.reward_norm_enable()
    ctx.host_env_reset(3.0 * rng.normal(0, 1, (N, obs)))
    p0 = ctx.get_params()
    F = (3.0 * rng.normal(0, 1, obs)).astype(np.float32)
    for it in range(2):
        if it == 1:
            ctx.obs_norm_enable(2)
        ctx.host_rollout_begin()
        for t in range(T):
            ctx.host_act_f32()
            o = (3.0 * rng.normal(0, 1, (N, obs))).astype(np.float32)
            fin = (3.0 * rng.normal(0, 1, (N, obs))).astype(np.float32)
            done, trunc = np.zeros(N, np.int32), np.zeros(N, np.int32)
            if t == 3:
                done[5] = trunc[5] = 1
                fin[5] = F
            if t == 4:
                o[7] = F
            ctx.host_observe(o, 10.0 * rng.normal(0, 1, N), done, truncated=trunc, final_obs=fin)
        ctx.host_rollout_end()
    ctx.sync()
    assert np.array_equal(bits(ctx.get_params()), bits(p0))
    idx, val = ctx.host_truncations()
    assert list(idx) == [3 * N + 5]
    values, rows = ctx.read("VALUES", (T, N)), ctx.read("OBS", (T, N, obs))
    assert np.array_equal(bits(ctx.get_value(rows.reshape(T * N, obs))), bits(values.ravel()))
    x = ctx.obs_norm_apply(F[None])
    assert np.array_equal(bits(x[0]), bits(rows[5, 7]))
    v = ctx.get_value(x)
    assert np.array_equal(bits(v), bits(values[5, 7:8])) and np.array_equal(bits(v), bits(val))
    # 2 rollouts x (critic batch + NEXT_OBS + the fold), and the two get_value calls above
    assert ctx.gauss_fused_launches() == (2 * T, 2 * 3 + 2, 2 * 4)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 6. flag on against flag off, same data (both are within one bar of float64: a cross-check, not a new tolerance)
# ---------------------------------------------------------------------------------------------------------
def test_fused_against_generic(P):
    obs, D, N, T = 17, 6, 8, 41
    B, M = N * T, 82
    shapes = tensor_shapes(obs, 64, 2, D)
    on, off = fused_ctx(P, obs, D, N=N, T=T, nmb=1), make_ctx(P, obs, D, N=N, T=T, nmb=1)
    params = randomised_params(on, shapes, np.random.default_rng(8))
    off.set_params(params)
    rng = np.random.default_rng(9)
    x = rng.uniform(-1, 1, (300, obs)).astype(np.float32)
    a_on, lp_on, en_on, v_on = on.policy_act_f32(x, step_index=3)
    mu_on, mu_off = on.policy_act_f32(x, greedy=True)[0], off.policy_act_f32(x, greedy=True)[0]
    _, lp_off, en_off, v_off = off.policy_act_f32(x, action=a_on)
    for name, g, w in (("mean", mu_on, mu_off), ("log-prob", lp_on, lp_off), ("entropy", en_on, en_off), ("value", v_on, v_off)):
        print("%s: on against off %.3g" % (name, rel(g, w)))
        assert rel(g, w) <= 2 * FWD_BAR, name
    grads = []
    for ctx in (on, off):
        fill_buffers(ctx, params, shapes, obs, D, B, np.random.default_rng(10))
        grads.append(ctx.minibatch_forward_backward(np.random.default_rng(11).permutation(B)[:M].astype(np.int32)))
    g_max, at = np.abs(grads[1]).max(), 0
    for i, s in enumerate(shapes):
        n = int(np.prod(s))
        err = np.abs(grads[0][at:at + n] - grads[1][at:at + n]).max() / g_max
        at += n
        print("tensor %d %s: on against off %.3g of the largest gradient element" % (i, s, err))
        assert err <= 2 * GRAD_BAR, (i, err)
    assert on.gauss_fused_launches() == (2, 2, 1) and off.gauss_fused_launches() == (0, 0, 0)   # policy_act_f32 returns the value too: a critic launch each
    on.close()
    off.close()


# ---------------------------------------------------------------------------------------------------------
# 7. counters
# ---------------------------------------------------------------------------------------------------------
class Still:
    """an env that never moves and never ends: no truncation, so no fold"""
    def __init__(self, N, O):
        self.N, self.obs = N, np.zeros((N, O), np.float32)

    def step(self, a):
        return self.obs, np.ones(self.N, np.float32), np.zeros(self.N, np.int32)


def test_launch_counters(P):
    """One rollout of T steps and its update of E x MB steps: T act launches, E * MB update launches, and 2 value launches (the [T N] batch and NEXT_OBS; a
    rollout with a truncation event would add 1, the fold's -- test_value_identities_under_the_normalisers counts that).  A context without the flag: 0, 0, 0."""
    N, T, nmb, epochs = 16, 5, 3, 2
    for flagged in (True, False):
        ctx = (fused_ctx if flagged else make_ctx)(P, 4, 2, N=N, T=T, nmb=nmb, epochs=epochs)
        ctx.init_orthogonal(1)
        env = Still(N, 4)
        ctx.host_env_reset(env.obs)
        assert ctx.gauss_fused_launches() == (0, 0, 0)
        host_rollout(ctx, env, T)
        ctx.sync()
        MB = -(-N * T // (N * T // nmb))   # a ragged tail is one more minibatch
        assert ctx.gauss_fused_launches() == ((T, 2, epochs * MB) if flagged else (0, 0, 0))
        assert ctx.stats()["optimizer_steps"] == epochs * MB
        ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------
def test_refusals(P):
    def refused(words, **kw):
        base = dict(env_kind=P.ENV_HOST, dist_kind=P.DIST_GAUSSIAN, obs_size=4, head_dims=(2,), num_envs=4, num_steps=4, num_minibatches=1,
                    kernel_flags=P.KERNEL_GAUSS_FUSED)
        base.update(kw)
        with pytest.raises(P.binding.PPOError) as e:
            P.Context(P.make_config(**base))
        msg = str(e.value)
        assert "status 5" in msg, msg        # PPO_ERR_UNSUPPORTED
        for w in words:
            assert w in msg, (w, msg)
        last = P.binding.lib().ppo_last_error(None)   # a refused create leaves the message with the NULL context
        assert last and last.decode() in msg
    refused(("PPO_KERNEL_GAUSS_FUSED", "hidden = 64", "96"), hidden=96)
    refused(("PPO_KERNEL_GAUSS_FUSED", "n_hidden = 2", "3"), n_hidden=3)
    refused(("PPO_KERNEL_GAUSS_FUSED", "obs_size <= 64", "65"), obs_size=65)
    refused(("PPO_KERNEL_GAUSS_FUSED", "PPO_DIST_GAUSSIAN", "categorical"), dist_kind=P.DIST_CATEGORICAL)
    ctx = P.Context(P.make_config(env_kind=P.ENV_HOST, dist_kind=P.DIST_GAUSSIAN, obs_size=64, head_dims=(32,), num_envs=4, num_steps=4, num_minibatches=1,
                                  kernel_flags=P.KERNEL_GAUSS_FUSED))   # the bounds themselves are served
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 9. learning: tests/test_gpu_gaussian.py::test_bandit_learns's loop and thresholds
# ---------------------------------------------------------------------------------------------------------
def test_bandit_learns(P):
    N, T = LEARN["N"], LEARN["T"]
    ctx = fused_ctx(P, 2, 2, N=N, T=T, nmb=LEARN["nmb"], epochs=LEARN["epochs"], lr=LEARN["lr"], seed=1)
    ctx.init_orthogonal(1)
    env = Bandit(N, 2)
    ctx.host_env_reset(env.reset())
    curve = [host_rollout(ctx, env, T) for _ in range(2 * LEARN_ORACLE_ITERS)]
    log_std = ctx.get_params()[-2:]
    print("mean reward: first %.3f, last 10 %.3f; log_std %s" % (curve[0], np.mean(curve[-10:]), log_std))
    assert -3.2 < curve[0] < -2.2
    assert np.mean(curve[-10:]) > -2.0
    assert np.all(log_std < 0.0)
    ctx.close()
