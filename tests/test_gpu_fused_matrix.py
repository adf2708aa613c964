"""PPO_KERNEL_FUSED_MATRIX (include/ppo_hip.h, ppo-libtorch_amd/csrc/kernels_fused_matrix.hip): the fused 2 x 64 families with their 64-wide products on the f32
matrix cores, on the GPU through the C-ABI, against the float64 oracles the families' own tests use (imported, never the library).  Bars: the families' f32
bars, unchanged -- 3e-6 max(1, |x|) forward, 1e-5 loss scalars, 5e-6 of a gradient tensor's own largest oracle element (W1 per 64-column chunk), a whole
update 2e-6 on the parameters and 1e-5 on the explained variance.  Without the flag every context here is refused at creation ("unknown bits in
kernel_flags")."""
import functools

import numpy as np
import pytest
import torch

import cat_fused_shapes as S
import grad_oracle as G
import oracle as O
from __graft_entry__ import load_package
from test_gpu_cat_fused import make_ctx as cat_make_ctx, write_batch
from test_gpu_fused_wide_obs import check_step
from test_gpu_gauss_fused import FWD_BAR, MAX_BLOCKS, fill_buffers, rel
from test_gpu_gaussian import HP, bits, gauss_entropy, gauss_logprob, make_ctx, mlp, nets, ppo_loss, randomised_params, t64, tensor_shapes, unflatten

pytestmark = pytest.mark.gpu

CAT = {"obs17 (5,3,4) masked": S._cat(17, (5, 3, 4), True, seed=52), "obs100 (5,3,4) masked": S._cat(100, (5, 3, 4), True, seed=61),
       "obs384 eight heads of 4": S._cat(384, (4,) * 8, False, seed=62)}
stand_in = functools.lru_cache(maxsize=None)(lambda name: G.stand_in_batch(CAT[name]))   # made once, shared, never written to
ROWS = (65, 64 * MAX_BLOCKS + 1)   # a ragged last tile; a workgroup with a second tile


@pytest.fixture(scope="module")
def P():
    return load_package()


def flags(P, family, obs):
    return family | P.KERNEL_FUSED_MATRIX | (P.KERNEL_FUSED_WIDE_OBS if obs > 64 else 0)


def gauss_ctx(P, obs, D, **kw):
    return make_ctx(P, obs, D, kernel_flags=flags(P, P.KERNEL_GAUSS_FUSED, obs), **kw)


def cat_ctx(P, s, N, T, **kw):
    return cat_make_ctx(P, s, flags(P, P.KERNEL_CAT_FUSED, s["obs"]), N=N, T=T, **kw)


def rows_of(b, rows, reps=1):   # the first `rows` rows of the stand-in batch `reps` times over, with its parameters, as write_batch takes them
    return dict({k: np.concatenate([b[k]] * reps)[:rows] for k in ("obs", "actions", "masks", "logp", "values", "adv", "ret")}, params=b["params"])


# (3, 1): one ragged resident chunk; (64, 32): a whole one; (65, 1): one column into the second chunk; (193, 3): three chunks and a column; (384, 32): the cap
@pytest.mark.parametrize("obs,D", [(3, 1), (64, 32), (65, 1), (193, 3), (384, 32)])
def test_gaussian_forward_against_float64(P, obs, D):
    rng = np.random.default_rng(1000 * obs + D)
    shapes = tensor_shapes(obs, 64, 2, D)
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


@pytest.mark.parametrize("name", ["obs17 (5,3,4) masked", "obs384 eight heads of 4"])
def test_categorical_forward_against_the_oracle(P, name):
    s, b = CAT[name], stand_in(name)
    ctx = cat_ctx(P, s, 8, 4, nmb=1)
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


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("obs,D", [(5, 2), (128, 6), (376, 17)])
def test_gaussian_minibatch_step_against_float64(P, obs, D, M):
    N, T = (64, 129) if M > 65 else (8, 41)
    rng = np.random.default_rng(7 * D + M)
    shapes = tensor_shapes(obs, 64, 2, D)
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
    s, b = CAT["obs100 (5,3,4) masked"], stand_in("obs100 (5,3,4) masked")
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


@pytest.mark.parametrize("obs", [33, 100])
def test_every_entry_point_gives_a_row_the_same_value_bits(P, obs):
    """policy_act_f32, get_value, a ppo_dev_observe fold event and a second identical call, on rows of the first, second and last workgroup and tile"""
    D, N = 3, 300
    rng = np.random.default_rng(obs)
    ctx = gauss_ctx(P, obs, D, N=N, T=1, lr=0.0)
    randomised_params(ctx, tensor_shapes(obs, 64, 2, D), rng)
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
    name, E, N, T = "obs17 (5,3,4) masked", 2, 8, 64
    s, b = CAT[name], stand_in(name)
    B, MB = N * T, N * T // 2
    ctx = cat_ctx(P, s, N, T, nmb=2, epochs=E)
    rep = rows_of(b, B)
    write_batch(ctx, s, rep)
    ctx.update()
    perm = ctx.read("PERM", (E, B))
    assert ctx.cat_fused_launches() == (0, 0, 2 * E) and ctx.stats()["optimizer_steps"] == 2 * E
    assert abs(ctx.stats()["explained_variance"] - O.explained_variance(rep["ret"], rep["values"])) <= 1e-5
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
