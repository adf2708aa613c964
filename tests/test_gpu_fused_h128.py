"""hidden = 128 under PPO_KERNEL_FUSED_MATRIX (ppo-libtorch_amd/csrc/kernels_fused_matrix_h128.hip): the fused families on a 2 x 128 network, on the GPU through
the C-ABI, against the float64 models the families' own tests use (imported, never the library).  Bars: the families' f32 bars, as set for the 64-wide
kernels -- 3e-6 max(1, |x|) forward, 1e-5 loss scalars, 5e-6 of a gradient tensor's own largest oracle element (W1 per 64-column chunk), a whole update 2e-6
on the parameters.  Without the feature every context here is refused at creation (hidden = 128 is "built for hidden = 64")."""
import functools

import numpy as np
import pytest
import torch

import cat_fused_shapes as S
import grad_oracle as G
import oracle as O
from __graft_entry__ import load_package
from test_gpu_cat_fused import make_ctx as cat_make_ctx, write_batch
from test_gpu_fused_matrix import flags, rows_of
from test_gpu_fused_wide_obs import GRAD_BAR, STATS
from test_gpu_gauss_fused import FWD_BAR, MAX_BLOCKS, fill_buffers, rel
from test_gpu_gaussian import HP, bits, gauss_entropy, gauss_logprob, make_ctx, mlp, nets, ppo_loss, randomised_params, t64, tensor_shapes, unflatten

pytestmark = pytest.mark.gpu

H = 128
CAT = {name: dict(S._cat(obs, (5, 3, 4), True, seed=seed), hidden=H) for name, obs, seed in (("obs17 masked", 17, 52), ("obs100 masked", 100, 61))}
stand_in = functools.lru_cache(maxsize=None)(lambda name: G.stand_in_batch(CAT[name]))   # made once, shared, never written to
ROWS = (65, 64 * MAX_BLOCKS + 1)   # a ragged last tile; a workgroup with a second tile (its slab elements are added to, not stored)


@pytest.fixture(scope="module")
def P():
    return load_package()


def gauss_ctx(P, obs, D, **kw):
    return make_ctx(P, obs, D, hidden=H, kernel_flags=flags(P, P.KERNEL_GAUSS_FUSED, obs), **kw)


def cat_ctx(P, s, N, T, **kw):
    return cat_make_ctx(P, s, flags(P, P.KERNEL_CAT_FUSED, s["obs"]), N=N, T=T, hidden=H, **kw)


def check_step(tag, obs, st, sc, grads, g_o, shapes):
    """the five scalars within 1e-5; every tensor within GRAD_BAR of its own largest oracle element, a [128, obs] tensor per 64-column chunk"""
    for key, okey in STATS:
        print("%s %s %.9g oracle %.9g" % (tag, key, st[key], sc[okey]))
        assert abs(st[key] - sc[okey]) <= 1e-5, (tag, key, st[key], sc[okey])
    at = 0
    for i, shp in enumerate(shapes):
        size = int(np.prod(shp))
        got, want = grads[at:at + size].reshape(shp), np.asarray(g_o[at:at + size]).reshape(shp)
        at += size
        for c0 in (range(0, obs, 64) if i in (0, 6) else [None]):   # the two W1
            g, w = (got, want) if c0 is None else (got[:, c0:c0 + 64], want[:, c0:c0 + 64])
            top = np.abs(w).max()   # a tensor the oracle leaves at zero must be zero here too
            err = np.abs(g - w).max() / top if top > 0 else (0.0 if not g.any() else np.inf)
            print("%s tensor %d %s chunk at %s: err %.3g of its largest element (%.3g)" % (tag, i, tuple(shp), c0, err, top))
            assert err <= GRAD_BAR, (tag, i, c0, err)
    assert at == grads.size


# (3, 1): one ragged chunk; (64, 32): a whole one, the widest head; (65, 1): one column into the second chunk; (384, 32): the cap, six chunks
@pytest.mark.parametrize("obs,D", [(3, 1), (64, 32), (65, 1), (384, 32)])
def test_gaussian_forward_against_float64(P, obs, D):
    rng = np.random.default_rng(1000 * obs + D)
    shapes = tensor_shapes(obs, H, 2, D)
    ctx = gauss_ctx(P, obs, D)
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


def test_masked_categorical_forward_against_the_oracle(P):
    s, b = CAT["obs17 masked"], stand_in("obs17 masked")
    ctx = cat_ctx(P, s, 8, 4, nmb=1)
    ctx.set_params(b["params"])
    for n in (1, 63, 64, 65, 300):
        obs, acts, mask = b["obs"][:n], b["actions"][:n], b["masks"][:n]
        lp_o, en_o, v_o = O.evaluate(b["net"], b["params"], obs, acts, mask)
        a, lp, en, v = ctx.policy_act(obs, mask=mask, action=acts)
        errs = rel(lp, lp_o), rel(en, en_o), rel(v, v_o), rel(ctx.get_value(obs), v_o)
        print("masked obs 17 n %d: log-prob %.3g entropy %.3g value %.3g get_value %.3g" % ((n,) + errs))
        assert np.array_equal(a, acts) and max(errs) <= FWD_BAR
        ga, glp, _, gv = ctx.policy_act_greedy(obs, mask=mask)
        _, flp, _, fv = ctx.policy_act(obs, mask=mask, action=ga)
        assert np.array_equal(bits(flp), bits(glp)) and np.array_equal(bits(fv), bits(gv))
    ctx.close()


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("obs,D", [(5, 2), (128, 6), (193, 3)])   # (193, 3): four chunks, the backward fetches chunks 1 and 0 of X again
def test_gaussian_minibatch_step_against_float64(P, obs, D, M):
    N, T = (64, 129) if M > 65 else (8, 41)
    rng = np.random.default_rng(7 * D + M)
    shapes = tensor_shapes(obs, H, 2, D)
    ctx = gauss_ctx(P, obs, D, N=N, T=T, nmb=1)
    params = randomised_params(ctx, shapes, rng)
    buf = fill_buffers(ctx, params, shapes, obs, D, N * T, rng)
    idx = rng.permutation(N * T)[:M].astype(np.int32)
    grads = ctx.minibatch_forward_backward(idx)
    st = ctx.stats()
    assert np.array_equal(bits(grads), bits(ctx.minibatch_forward_backward(idx))) and ctx.gauss_fused_launches() == (0, 0, 2)
    ts = unflatten(params, shapes, grad=True)
    li = torch.as_tensor(idx.astype(np.int64))
    loss, sc = ppo_loss(ts, *(t64(b)[li] for b in buf), dict(HP, norm_adv=True, clip_vloss=True))
    loss.backward()
    assert 0.4 < sc["clipfrac"] < 0.9
    check_step("obs %d D %d M %d" % (obs, D, M), obs, st, sc, grads, np.concatenate([t.grad.numpy().ravel() for t in ts]), shapes)
    ctx.close()


@pytest.mark.parametrize("M", ROWS)
def test_masked_categorical_minibatch_step_against_float64(P, M):
    """the stand-in batch of tests/grad_oracle.py (1152 rows) eight times over: 9216 rows, so that 8193 distinct rows exist"""
    s, b = CAT["obs100 masked"], stand_in("obs100 masked")
    ctx = cat_ctx(P, s, 8 * G.N_ENVS, G.N_STEPS, nmb=1)
    rep = rows_of(b, 8 * G.N_ENVS * G.N_STEPS, reps=8)
    write_batch(ctx, s, rep)
    idx = np.random.default_rng(M).permutation(rep["obs"].shape[0])[:M].astype(np.int32)
    grads = ctx.minibatch_forward_backward(idx)
    st = ctx.stats()
    assert ctx.gauss_fused_launches() == (0, 0, 1)
    g64, s64 = G.minibatch_grads(b["shapes"], s["heads"], True, G.shape_hp(s), b["params"], rep["obs"], rep["actions"], rep["logp"], rep["adv"], rep["ret"],
                                 rep["values"], idx, rep["masks"])
    shapes = [tuple(int(v) for v in r if v) for r in np.asarray(b["shapes"]).reshape(-1, 2)]
    check_step("masked obs 100 M %d" % M, 100, st, s64, grads, g64, shapes)
    ctx.close()


def test_every_entry_point_gives_a_row_the_same_value_bits(P):
    """policy_act_f32, get_value, a ppo_dev_observe fold event and a second identical call, on rows of the first, second and last workgroup and tile"""
    obs, D, N = 100, 3, 300
    rng = np.random.default_rng(obs)
    ctx = gauss_ctx(P, obs, D, N=N, T=1, lr=0.0)
    randomised_params(ctx, tensor_shapes(obs, H, 2, D), rng)
    x0, x1, fin = (rng.uniform(-1, 1, (N, obs)).astype(np.float32) for _ in range(3))
    rew = rng.normal(0, 1, N).astype(np.float32)
    flagged = np.array([0, 63, 64, 130, 299])
    done = np.zeros(N, np.int32)
    done[flagged] = 1
    ctx.dev_env_reset(ctx.dev(x0))
    ctx.host_rollout_begin()
    ctx.dev_act_f32(ctx.empty((N, D), np.float32))
    ctx.dev_observe(ctx.dev(x1), ctx.dev(rew), ctx.dev(done, np.int32), truncated=ctx.dev(done, np.int32), final_obs=ctx.dev(fin))
    ctx.host_rollout_end()
    ctx.sync()
    v = ctx.get_value(fin)
    idx, val = ctx.host_truncations()
    assert list(idx) == list(flagged) and np.array_equal(bits(val), bits(v[flagged]))
    assert np.array_equal(bits(ctx.policy_act_f32(fin, greedy=True)[3]), bits(v)) and np.array_equal(bits(ctx.get_value(fin)), bits(v))
    assert np.array_equal(bits(ctx.get_value(fin[flagged])), bits(v[flagged]))   # the same rows at other places of a tile
    ctx.close()


def test_a_whole_update_tracks_the_float64_replay(P):
    """two epochs x two minibatches of 256 rows on its own permutations; the replay: float64 gradients through the oracle's clip and AdamW"""
    name, E, N, T = "obs17 masked", 2, 8, 64
    s, b = CAT[name], stand_in(name)
    B, MB = N * T, N * T // 2
    ctx = cat_ctx(P, s, N, T, nmb=2, epochs=E)
    rep = rows_of(b, B)
    write_batch(ctx, s, rep)
    ctx.update()
    perm = ctx.read("PERM", (E, B))
    assert ctx.cat_fused_launches() == (0, 0, 2 * E) and ctx.stats()["optimizer_steps"] == 2 * E
    p, step = b["params"].copy(), 0
    m, v = np.zeros_like(p), np.zeros_like(p)
    for e in range(E):
        for k in range(2):
            g, _ = G.minibatch_grads(b["shapes"], s["heads"], True, G.shape_hp(s), p, rep["obs"], rep["actions"], rep["logp"], rep["adv"], rep["ret"], rep["values"],
                                     perm[e, k * MB:(k + 1) * MB], rep["masks"])
            g, _ = O.clip_grad_norm(b["net"], g, G.BASE_HP["max_grad_norm"])
            step += 1
            p, m, v = O.adamw_step(p, g, m, v, 1e-3, step)
    err = np.abs(p - ctx.get_params()).max()
    print("parameters %.3g from the replay's after %d steps" % (err, step))
    assert err <= 2e-6 and not np.array_equal(bits(ctx.get_params()), bits(b["params"]))
    ctx.close()
