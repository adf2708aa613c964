"""PPO_KERNEL_FUSED_WIDE_OBS (include/ppo_hip.h, ppo-libtorch_amd/csrc/kernels_fused_wide.hip): the fused 2 x 64 families at observations of 65 .. 384
columns, on the GPU through the C-ABI, against the float64 oracles the families' own tests use (imported, never the library).  Bars: DESIGN section 0 --
3e-6 max(1, |x|) forward, 1e-5 loss scalars, 5e-6 of a gradient tensor's own largest oracle element (W1 per 64-column chunk).  Without the flag every
context here is refused at creation."""
import functools

import numpy as np
import pytest
import torch

import cat_fused_shapes as S
import grad_oracle as G
import oracle as O
from __graft_entry__ import load_package
from test_gpu_gaussian import HP, bits, gauss_entropy, gauss_logprob, make_ctx, mlp, nets, ppo_loss, randomised_params, t64, tensor_shapes, unflatten
from test_gpu_gauss_fused import FWD_BAR, GRAD_BAR, MAX_BLOCKS, fill_buffers, rel

pytestmark = pytest.mark.gpu

STATS = (("pg_loss", "pg_loss"), ("v_loss", "v_loss"), ("entropy_loss", "entropy_loss"), ("approx_kl", "approx_kl"), ("clipfrac_last", "clipfrac"))
CAT = {"obs100 (5,3,4) masked": S._cat(100, (5, 3, 4), True, seed=61), "obs384 eight heads of 4": S._cat(384, (4,) * 8, False, seed=62)}

stand_in = functools.lru_cache(maxsize=None)(lambda name: G.stand_in_batch(CAT[name]))   # made once, shared, never written to


@pytest.fixture(scope="module")
def P():
    return load_package()


def wide_ctx(P, obs, D, **kw):
    return make_ctx(P, obs, D, kernel_flags=P.KERNEL_GAUSS_FUSED | P.KERNEL_FUSED_WIDE_OBS, **kw)


def cat_ctx(P, s, N, T, **kw):
    hp = dict(G.shape_hp(s), **kw)
    return P.Context(P.make_config(env_kind=P.ENV_HOST, dist_kind=P.DIST_MASKED if s["masked"] else P.DIST_CATEGORICAL, obs_size=s["obs"], head_dims=s["heads"],
                                   num_envs=N, num_steps=T, num_minibatches=1, seed=s["seed"], total_timesteps=1 << 30, learning_rate=1e-3, anneal_lr=False,
                                   kernel_flags=P.KERNEL_CAT_FUSED | P.KERNEL_FUSED_WIDE_OBS, **hp))


# (65, 1): one column in the second chunk; (128, 6): two whole chunks; (193, 3): three and a column; (376, 17): the ragged sixth; (384, 32): the cap
@pytest.mark.parametrize("obs,D", [(65, 1), (128, 6), (193, 3), (376, 17), (384, 32)])
def test_gaussian_forward_against_float64(P, obs, D):
    rng = np.random.default_rng(1000 * obs + D)
    shapes = tensor_shapes(obs, 64, 2, D)
    ctx = wide_ctx(P, obs, D)
    critic, actor, log_std = nets(unflatten(randomised_params(ctx, shapes, rng), shapes))
    for n in (1, 63, 64, 65, 300):
        x = rng.uniform(-1, 1, (n, obs)).astype(np.float32)
        mu = mlp(actor, t64(x))
        a = (mu.numpy() + rng.uniform(-4, 4, (n, D)) * np.exp(log_std.numpy())).astype(np.float32)
        act, lp, en, v = ctx.policy_act_f32(x, action=a, step_index=7)
        lp_o, en_o, v_o = gauss_logprob(mu, log_std, t64(a)).numpy(), gauss_entropy(mu, log_std).numpy(), mlp(critic, t64(x)).squeeze(-1).numpy()
        ag, lpg, _, vg = ctx.policy_act_f32(x, greedy=True)
        errs = rel(lp, lp_o), rel(en, en_o), rel(v, v_o), rel(ctx.get_value(x), v_o), rel(ag, mu.numpy())
        print("obs %d D %d n %d: log-prob %.3g entropy %.3g value %.3g get_value %.3g mean %.3g" % ((obs, D, n) + errs))
        assert np.array_equal(bits(act), bits(a)) and max(errs) <= FWD_BAR
        _, lpf, _, vf = ctx.policy_act_f32(x, action=ag)
        assert np.array_equal(bits(lpf), bits(lpg)) and np.array_equal(bits(vf), bits(vg))
    assert ctx.gauss_fused_launches()[2] == 0 and ctx.gauss_fused_launches()[0] > 0
    ctx.close()


@pytest.mark.parametrize("name", list(CAT))
def test_categorical_forward_against_the_oracle(P, name):
    s, b = CAT[name], stand_in(name)
    ctx = cat_ctx(P, s, 8, 4)
    ctx.set_params(b["params"])
    for n in (1, 63, 64, 65, 300):
        obs, acts, mask = b["obs"][:n], b["actions"][:n], (b["masks"][:n] if s["masked"] else None)
        lp_o, en_o, v_o = O.evaluate(b["net"], b["params"], obs, acts, mask)
        a, lp, en, v = ctx.policy_act(obs, mask=mask, action=acts)
        errs = rel(lp, lp_o), rel(en, en_o), rel(v, v_o), rel(ctx.get_value(obs), v_o)
        print("%s n %d: log-prob %.3g entropy %.3g value %.3g get_value %.3g" % ((name, n) + errs))
        assert np.array_equal(a, acts) and max(errs) <= FWD_BAR
        ga, glp, _, gv = ctx.policy_act_greedy(obs, mask=mask)
        _, flp, _, fv = ctx.policy_act(obs, mask=mask, action=ga)
        assert np.array_equal(bits(flp), bits(glp)) and np.array_equal(bits(fv), bits(gv))
    ctx.close()


def test_the_accumulator_crosses_a_chunk_boundary_unchanged(P):
    """columns 64 .. 127 of the input are zero: fmaf(w, 0, acc) is acc, so the wide kernels give the 64-column kernels' bits"""
    rng, D, n = np.random.default_rng(2), 6, 65
    wide, narrow = wide_ctx(P, 128, D), make_ctx(P, 64, D, kernel_flags=P.KERNEL_GAUSS_FUSED)
    sw = tensor_shapes(128, 64, 2, D)
    ts = unflatten(randomised_params(wide, sw, rng), sw)
    narrow.set_params(np.concatenate([(t[:, :64] if t.shape == (64, 128) else t).numpy().ravel() for t in ts]).astype(np.float32))
    x = np.zeros((n, 128), np.float32)
    x[:, :64] = rng.uniform(-1, 1, (n, 64))
    a = rng.uniform(-1, 1, (n, D)).astype(np.float32)
    (_, lp_w, _, v_w), (_, lp_n, _, v_n) = wide.policy_act_f32(x, action=a), narrow.policy_act_f32(x[:, :64], action=a)
    assert np.array_equal(bits(lp_w), bits(lp_n)) and np.array_equal(bits(v_w), bits(v_n))
    assert wide.gauss_fused_launches() == narrow.gauss_fused_launches() == (1, 1, 0)
    wide.close()
    narrow.close()


def check_step(tag, obs, st, sc, grads, g_o, shapes):
    """the five scalars within 1e-5; every tensor within GRAD_BAR of its own largest oracle element, a [64, obs] tensor per 64-column chunk"""
    for key, okey in STATS:
        print("%s %s %.9g oracle %.9g" % (tag, key, st[key], sc[okey]))
        assert abs(st[key] - sc[okey]) <= 1e-5, (tag, key, st[key], sc[okey])
    at = 0
    for i, shp in enumerate(shapes):
        size = int(np.prod(shp))
        got, want = grads[at:at + size].reshape(shp), np.asarray(g_o[at:at + size]).reshape(shp)
        at += size
        for c0 in (range(0, obs, 64) if tuple(shp) == (64, obs) else [None]):
            g, w = (got, want) if c0 is None else (got[:, c0:c0 + 64], want[:, c0:c0 + 64])
            top = np.abs(w).max()   # a tensor the oracle leaves at zero (one row on the clip's dead side: the actor) must be zero here too
            err = np.abs(g - w).max() / top if top > 0 else (0.0 if not g.any() else np.inf)
            print("%s tensor %d %s chunk at %s: err %.3g of its largest element (%.3g)" % (tag, i, tuple(shp), c0, err, top))
            assert err <= GRAD_BAR, (tag, i, c0, err)
    assert at == grads.size


# rows: 1 = one lane (norm_adv off: one row has no standard deviation); 82 = a partial tile behind a whole one; 8256 = 129 tiles > MAX_BLOCKS: a second tile
@pytest.mark.parametrize("M", [1, 82, 8256])
@pytest.mark.parametrize("obs,D", [(65, 1), (193, 3), (376, 17), (384, 32)])
def test_gaussian_minibatch_step_against_float64(P, obs, D, M):
    N, T = (64, 129) if M == 8256 else (8, 41)
    assert M != 8256 or (M + 63) // 64 > MAX_BLOCKS
    rng = np.random.default_rng(7 * D + M)
    shapes = tensor_shapes(obs, 64, 2, D)
    ctx = wide_ctx(P, obs, D, N=N, T=T, nmb=1, norm_adv=M > 1)
    params = randomised_params(ctx, shapes, rng)
    buf = fill_buffers(ctx, params, shapes, obs, D, N * T, rng)
    idx = rng.permutation(N * T)[:M].astype(np.int32) if M > 1 else np.array([3 * 17], np.int32)
    grads = ctx.minibatch_forward_backward(idx)
    st = ctx.stats()
    assert np.array_equal(bits(grads), bits(ctx.minibatch_forward_backward(idx))) and ctx.gauss_fused_launches() == (0, 0, 2)
    ts = unflatten(params, shapes, grad=True)
    li = torch.as_tensor(idx.astype(np.int64))
    loss, sc = ppo_loss(ts, *(t64(b)[li] for b in buf), dict(HP, norm_adv=M > 1, clip_vloss=True))
    loss.backward()
    assert M == 1 or 0.4 < sc["clipfrac"] < 0.9
    check_step("obs %d D %d M %d" % (obs, D, M), obs, st, sc, grads, np.concatenate([t.grad.numpy().ravel() for t in ts]), shapes)
    ctx.close()


@pytest.mark.parametrize("M", [1, 82, 8256])
def test_masked_categorical_minibatch_step_against_float64(P, M):
    """the stand-in batch of tests/grad_oracle.py (1152 rows) eight times over: 9216 rows, so that 8256 distinct rows exist"""
    s, b = CAT["obs100 (5,3,4) masked"], stand_in("obs100 (5,3,4) masked")
    hp = dict(G.shape_hp(s), norm_adv=M > 1)
    rep = {k: np.concatenate([b[k]] * 8) for k in ("obs", "actions", "masks", "logp", "values", "adv", "ret")}
    ctx = cat_ctx(P, s, 8 * G.N_ENVS, G.N_STEPS, norm_adv=M > 1)
    for name, key, dt in (("OBS", "obs", np.float32), ("ACTIONS", "actions", np.int32), ("MASKS", "masks", np.uint8), ("LOGPROBS", "logp", np.float32),
                          ("VALUES", "values", np.float32), ("ADVANTAGES", "adv", np.float32), ("RETURNS", "ret", np.float32)):
        ctx.write(name, rep[key].astype(dt))
    ctx.set_params(b["params"])
    idx = np.random.default_rng(M).permutation(rep["obs"].shape[0])[:M].astype(np.int32) if M > 1 else G.ref_index_lists(dict(s, lists=(2,)), b)[0][:1]   # a row inside both clips
    grads = ctx.minibatch_forward_backward(idx)
    st = ctx.stats()
    assert ctx.gauss_fused_launches() == (0, 0, 1)
    g64, s64 = G.minibatch_grads(b["shapes"], s["heads"], True, hp, b["params"], rep["obs"], rep["actions"], rep["logp"], rep["adv"], rep["ret"], rep["values"], idx,
                                 rep["masks"])
    shapes = [tuple(int(v) for v in r if v) for r in np.asarray(b["shapes"]).reshape(-1, 2)]
    check_step("masked obs 100 M %d" % M, 100, st, s64, grads, g64, shapes)
    ctx.close()


def test_the_truncation_fold(P):
    """ppo_dev_observe with flags on rows of the first, second and last workgroup and tile: r + gamma V(final obs), V = get_value's bits; nothing else moves"""
    obs, D, N = 100, 3, 300
    rng = np.random.default_rng(4)
    ctx = wide_ctx(P, obs, D, N=N, T=1, lr=0.0)
    randomised_params(ctx, tensor_shapes(obs, 64, 2, D), rng)
    x0, x1, fin = (rng.uniform(-1, 1, (N, obs)).astype(np.float32) for _ in range(3))
    rew = rng.normal(0, 1, N).astype(np.float32)
    flagged = np.array([0, 63, 64, 130, 299])
    done, trunc = np.zeros(N, np.int32), np.zeros(N, np.int32)
    done[flagged] = trunc[flagged] = 1
    done[5], trunc[7] = 1, 1   # terminated, not truncated; a flag without a done: neither folds
    ctx.dev_env_reset(ctx.dev(x0))
    ctx.host_rollout_begin()
    ctx.dev_act_f32(ctx.empty((N, D), np.float32))
    ctx.dev_observe(ctx.dev(x1), ctx.dev(rew), ctx.dev(done, np.int32), truncated=ctx.dev(trunc, np.int32), final_obs=ctx.dev(fin))
    ctx.host_rollout_end()
    ctx.sync()
    v = ctx.get_value(fin[flagged])
    want = rew.copy()
    want[flagged] = (rew[flagged] + (np.float32(HP["gamma"]) * v).astype(np.float32)).astype(np.float32)
    assert np.array_equal(bits(ctx.read("REWARDS", (N,))), bits(want))
    idx, val = ctx.host_truncations()
    assert list(idx) == list(flagged) and np.array_equal(bits(val), bits(v))
    ctx.close()


def test_a_flagged_context_at_obs_33_is_its_unflagged_twin(P):
    obs, D, N, T, M = 33, 17, 8, 41, 82
    shapes = tensor_shapes(obs, 64, 2, D)
    got = []
    for ctx in (wide_ctx(P, obs, D, N=N, T=T), make_ctx(P, obs, D, N=N, T=T, kernel_flags=P.KERNEL_GAUSS_FUSED)):
        params = randomised_params(ctx, shapes, np.random.default_rng(8))
        buf = fill_buffers(ctx, params, shapes, obs, D, N * T, np.random.default_rng(10))
        _, lp, _, v = ctx.policy_act_f32(buf[0][:300], action=buf[1][:300])
        grads = ctx.minibatch_forward_backward(np.random.default_rng(11).permutation(N * T)[:M].astype(np.int32))
        got.append((ctx.gauss_fused_launches(), bits(lp), bits(v), bits(grads)))
        ctx.close()
    assert got[0][0] == got[1][0] == (1, 1, 1)
    assert all(np.array_equal(a, b) for a, b in zip(got[0][1:], got[1][1:]))
