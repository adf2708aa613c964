"""compute_dtype = PPO_DTYPE_BF16 under PPO_KERNEL_FUSED_MATRIX (ppo-libtorch_amd/csrc/kernels_fused_matrix_bf16.hip) on the GPU through the C-ABI, at hidden 64
and 128, against a float64 model of the arithmetic DESIGN.md states ("Fused matrix families at bf16"): the heads and the loss are the models of
tests/test_gpu_gaussian.py and tests/grad_oracle.py, imported, with their MLP replaced by RoundedMLP below, which rounds x, W1, W2, h1, h2, dz2 and dz1 to
bf16 (tests/bf16_layers.py: bf16_rne) where the kernels do.  The library is never called for an expectation.  Every input is made on the CPU, so the bars
can be measured without a GPU (tools/fused_bf16_bars.py evaluates the model below twice on these very inputs: in float64, and with every product and sum in
float32; the second keeps the rounding points and carries f32 accumulation error only -- both evaluate tanh in float64, so the bars do not model the
error of the kernels' tanh_fast, which can push an activation across a bf16 midpoint just as an accumulation error can).

Measured there (worst case over all parametrised cases, hidden 64 and 128), and the bars = 4 x that, never below the family's f32 bars (3e-6, 1e-5, 5e-6):
    forward outputs (log-prob, entropy, value, mean), |got - want| / max(1, |want|):   1.80e-3    bar 7.2e-3
    the five loss scalars, absolute:                                                    6.29e-7    bar 1e-5 (the floor)
    a gradient tensor, of its own largest element (W1 per 64-column chunk):            5.02e-4    bar 2.0e-3
The seeds are chosen so that every gradient tensor's float64-versus-float32 deviation stays below 1 % of its largest element: a case above that has an
activation on a bf16 midpoint, and gets another seed, not another bar.  What the bars can tell apart: the plain unrounded float64 network is up to 2.0e-2
(forward; 5e-3 typically, so the forward bar sits close to it) and 7e-3 .. 9.9 of a tensor (gradient tensors) away from the rounded model on the same inputs.
Without the feature every context here is refused at creation ("bf16 storage is not")."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import cat_fused_shapes as S
import grad_oracle as G
import test_gpu_gaussian as TG
from __graft_entry__ import load_package
from bf16_layers import bf16_rne
from test_gpu_cat_fused import make_ctx as cat_make_ctx, write_batch
from test_gpu_fused_matrix import flags, rows_of
from test_gpu_fused_wide_obs import STATS
from test_gpu_gauss_fused import MAX_BLOCKS, rel
from test_gpu_gaussian import HP, bits, gauss_entropy, gauss_logprob, make_ctx, nets, t64, tensor_shapes, unflatten

FWD_BAR, LOSS_BAR, GRAD_BAR = 7.2e-3, 1e-5, 2.0e-3
NS = (1, 63, 64, 65, 300)
ROWS = (65, 64 * MAX_BLOCKS + 1)   # a ragged last tile; a workgroup with a second tile (its slab elements are added to, not stored)
FWD_SHAPES = [(3, 1), (64, 32), (65, 1), (384, 32)]   # one ragged chunk; a whole one, the widest head; one column into the second chunk; the cap, six chunks
STEP_SHAPES = [(5, 2), (193, 3)]                      # (193, 3): four chunks, the backward fetches chunks 1 and 0 of X again
# (obs, masked, hidden): the masked policy at both widths; the plain categorical one once per kernel kind, at the width with two row tiles
CAT_KEYS = [(17, True, 64), (17, True, 128), (17, False, 128), (100, True, 64), (100, True, 128), (100, False, 128)]
CAT = {k: dict(S._cat(k[0], (5, 3, 4), k[1], seed=52 if k[0] == 17 else 61), hidden=k[2]) for k in CAT_KEYS}
CAT_STEPS = [(k, M) for k in CAT_KEYS if k[0] == 100 for M in ROWS if k[1] or M == 65]
stand_in = functools.lru_cache(maxsize=None)(lambda key: G.stand_in_batch(CAT[key]))   # made once, shared, never written to


class RoundedMLP(torch.autograd.Function):
    """obs -> H -> H -> out with the kernels' rounding points, forward and backward; prec: the numpy type every product and sum is made in"""
    @staticmethod
    def forward(ctx, prec, x, W1, b1, W2, b2, W3, b3):
        f = lambda t: np.asarray(t.detach().numpy(), prec)   # noqa: E731
        r = lambda a: bf16_rne(a).astype(prec)               # noqa: E731
        xh, w2 = r(f(x)), r(f(W2))
        h1 = r(np.tanh((xh @ r(f(W1)).T + f(b1)).astype(np.float64)))
        h2 = r(np.tanh((h1 @ w2.T + f(b2)).astype(np.float64)))
        ctx.saved = prec, xh, h1, h2, w2, f(W3)
        return torch.as_tensor((h2 @ f(W3).T + f(b3)).astype(np.float64))

    @staticmethod
    def backward(ctx, d_out):
        prec, xh, h1, h2, w2, W3 = ctx.saved
        r = lambda a: bf16_rne(a).astype(prec)               # noqa: E731
        d = np.asarray(d_out.numpy(), prec)
        dz2 = (d @ W3) * (1 - h2 * h2)
        dz1 = (r(dz2) @ w2) * (1 - h1 * h1)
        g = r(dz1).T @ xh, dz1.sum(0), r(dz2).T @ h1, dz2.sum(0), d.T @ h2, d.sum(0)
        return (None, None) + tuple(torch.as_tensor(a.astype(np.float64)) for a in g)


def model(prec, fn):
    """fn() with the imported models' MLP replaced: prec = a numpy type: the rounded network in that precision; None: the plain float64 network"""
    if prec is None:
        return fn()
    def mlp(layers, x):   # noqa: E306
        W1, b1, W2, b2, W3, b3 = layers
        return RoundedMLP.apply(prec, x, W1, b1.reshape(-1), W2, b2.reshape(-1), W3, b3.reshape(-1))
    old = TG.mlp, G._mlp
    TG.mlp = G._mlp = mlp
    try:
        return fn()
    finally:
        TG.mlp, G._mlp = old


def gauss_params(rng, obs, D, H):
    """a 2 x H Gaussian agent made on the CPU: hidden layers of unit gain, means of order 0.3, log_std in [-2, 1]"""
    out = []
    for o, i, gain in ((H, obs, 1.4), (H, H, 1.4), (1, H, 1.0), (H, obs, 1.4), (H, H, 1.4), (D, H, 0.3)):
        out += [rng.normal(0, gain / np.sqrt(i), (o, i)), rng.uniform(-0.3, 0.3, o)]
    return np.concatenate([a.ravel() for a in out] + [rng.uniform(-2.0, 1.0, D)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gauss_forward_case(H, obs, D):
    rng = np.random.default_rng(1000 * obs + D + H)
    params = gauss_params(rng, obs, D, H)
    return params, [(rng.uniform(-1, 1, (n, obs)).astype(np.float32), rng.uniform(-4, 4, (n, D))) for n in NS]


def gauss_forward(prec, H, obs, D, params, x, spread):
    """(mean, forced action, log-prob, entropy, value) of the model; the action is the float64 rounded model's mean + spread x std, in f32"""
    def run():
        critic, actor, log_std = nets(unflatten(params, tensor_shapes(obs, H, 2, D)))
        with torch.no_grad():
            mu, v = TG.mlp(actor, t64(x)), TG.mlp(critic, t64(x)).squeeze(-1)
            return mu, v, log_std
    mu64, _, log_std = model(np.float64, run)
    a = (mu64.numpy() + spread * np.exp(log_std.numpy())).astype(np.float32)
    mu, v, _ = model(prec, run)
    return mu.numpy(), a, gauss_logprob(mu, log_std, t64(a)).numpy(), gauss_entropy(mu, log_std).numpy(), v.numpy()


@functools.lru_cache(maxsize=None)
def gauss_step_case(H, obs, D, M):
    """fill_buffers' construction (tests/test_gpu_gauss_fused.py) on the CPU: about a third of the rows clip on each side"""
    N, T = (64, 129) if M > 65 else (8, 41)
    B = N * T
    rng = np.random.default_rng(7 * D + M + H)
    params = gauss_params(rng, obs, D, H)
    x = rng.uniform(-1, 1, (B, obs)).astype(np.float32)
    mu, a, lp_now, _, v_now = gauss_forward(np.float64, H, obs, D, params, x, rng.normal(0, 1, (B, D)))
    shift = np.where(np.arange(B) % 3 == 0, 0.4, np.where(np.arange(B) % 3 == 1, -0.4, 0.02)) * rng.uniform(0.6, 1.0, B)
    buf = (x, a, (lp_now - shift).astype(np.float32), rng.normal(0, 1, B).astype(np.float32), (v_now + rng.normal(0, 0.5, B)).astype(np.float32),
           (v_now + rng.normal(0, 0.3, B)).astype(np.float32))   # obs, actions, old log-probs, advantages, returns, old values
    return N, T, params, buf, rng.permutation(B)[:M].astype(np.int32)


def gauss_step(prec, H, obs, D, params, buf, idx):
    def run():
        ts = unflatten(params, tensor_shapes(obs, H, 2, D), grad=True)
        li = torch.as_tensor(idx.astype(np.int64))
        loss, sc = TG.ppo_loss(ts, *(t64(b)[li] for b in buf), dict(HP, norm_adv=True, clip_vloss=True))
        loss.backward()
        return np.concatenate([t.grad.numpy().ravel() for t in ts]), sc
    return model(prec, run)


def cat_forward(prec, key, n):
    s, b = CAT[key], stand_in(key)
    def run():   # noqa: E306
        ts = [torch.tensor(np.asarray(v, np.float64)) for _, _, _, _, v in G.split(b["params"], b["shapes"])]
        x = t64(b["obs"][:n])
        with torch.no_grad():
            lp, en = G._heads(G._mlp(ts[6:], x), torch.tensor(b["actions"][:n].astype(np.int64)), torch.tensor(b["masks"][:n] != 0) if s["masked"] else None, s["heads"], s["masked"])
            return lp.numpy(), en.numpy(), G._mlp(ts[:6], x).squeeze(1).numpy()
    return model(prec, run)


@functools.lru_cache(maxsize=None)
def cat_step_case(key, M):
    """the stand-in batch of tests/grad_oracle.py (1152 rows) eight times over: 9216 rows, so that 8193 distinct rows exist"""
    b = stand_in(key)
    rep = rows_of(dict(b, masks=b["masks"] if key[1] else b["actions"]), 8 * G.N_ENVS * G.N_STEPS, reps=8)   # a plain categorical batch has no masks: never read
    return rep, np.random.default_rng(M + key[2]).permutation(rep["obs"].shape[0])[:M].astype(np.int32)


def cat_step(prec, key, M):
    s, b = CAT[key], stand_in(key)
    rep, idx = cat_step_case(key, M)
    return model(prec, lambda: G.minibatch_grads(b["shapes"], s["heads"], s["masked"], G.shape_hp(s), b["params"], rep["obs"], rep["actions"], rep["logp"],
                                                 rep["adv"], rep["ret"], rep["values"], idx, rep["masks"]))


def cat_shapes(key):
    return [tuple(int(v) for v in r if v) for r in np.asarray(stand_in(key)["shapes"]).reshape(-1, 2)]


def tensor_errors(got, want, shapes, obs):
    """(label, error of its own largest reference element) per tensor, the two W1 per 64-column chunk; a tensor the reference leaves at zero must be zero"""
    at, out = 0, []
    for i, shp in enumerate(shapes):
        size = int(np.prod(shp))
        g, w = np.asarray(got[at:at + size]).reshape(shp), np.asarray(want[at:at + size]).reshape(shp)
        at += size
        for c0 in (range(0, obs, 64) if i in (0, 6) else [None]):
            gc, wc = (g, w) if c0 is None else (g[:, c0:c0 + 64], w[:, c0:c0 + 64])
            top = np.abs(wc).max()
            out.append(("tensor %d %s chunk at %s" % (i, tuple(shp), c0), np.abs(gc - wc).max() / top if top > 0 else (0.0 if not gc.any() else np.inf)))
    assert at == len(got)
    return out


def check_step(tag, obs, st, sc, grads, g_o, shapes):
    for key, okey in STATS:
        print("%s %s %.9g model %.9g" % (tag, key, st[key], sc[okey]))
        assert abs(st[key] - sc[okey]) <= LOSS_BAR, (tag, key, st[key], sc[okey])
    for label, err in tensor_errors(grads, g_o, shapes, obs):
        print("%s %s: err %.3g of its largest element" % (tag, label, err))
        assert err <= GRAD_BAR, (tag, label, err)


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return load_package()


def gauss_ctx(P, H, obs, D, **kw):
    return make_ctx(P, obs, D, hidden=H, compute_dtype=P.DTYPE_BF16, kernel_flags=flags(P, P.KERNEL_GAUSS_FUSED, obs), **kw)


def cat_ctx(P, s, N, T, **kw):
    return cat_make_ctx(P, s, flags(P, P.KERNEL_CAT_FUSED, s["obs"]), N=N, T=T, hidden=s["hidden"], compute_dtype=P.DTYPE_BF16, **kw)


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("obs,D", FWD_SHAPES)
def test_gaussian_forward_against_the_rounded_float64_model(P, H, obs, D):
    params, rows = gauss_forward_case(H, obs, D)
    ctx = gauss_ctx(P, H, obs, D)
    ctx.set_params(params)
    for x, spread in rows:
        mu, a, lp_o, en_o, v_o = gauss_forward(np.float64, H, obs, D, params, x, spread)
        act, lp, en, v = ctx.policy_act_f32(x, action=a, step_index=7)
        ag, lpg, _, vg = ctx.policy_act_f32(x, greedy=True)
        errs = rel(lp, lp_o), rel(en, en_o), rel(v, v_o), rel(ctx.get_value(x), v_o), rel(ag, mu)
        print("H %d obs %d D %d n %d: log-prob %.3g entropy %.3g value %.3g get_value %.3g mean %.3g" % ((H, obs, D, len(x)) + errs))
        assert np.array_equal(bits(act), bits(a)) and max(errs) <= FWD_BAR
        _, lpf, _, vf = ctx.policy_act_f32(x, action=ag)
        assert np.array_equal(bits(lpf), bits(lpg)) and np.array_equal(bits(vf), bits(vg))
    assert ctx.gauss_fused_launches()[2] == 0 and ctx.gauss_fused_launches()[0] > 0
    ctx.close()


@pytest.mark.parametrize("key", [k for k in CAT_KEYS if k[0] == 17])
def test_categorical_forward_against_the_rounded_float64_model(P, key):
    s, b = CAT[key], stand_in(key)
    ctx = cat_ctx(P, s, 8, 4, nmb=1)
    ctx.set_params(b["params"])
    for n in NS:
        obs, acts, mask = b["obs"][:n], b["actions"][:n], b["masks"][:n] if s["masked"] else None
        lp_o, en_o, v_o = cat_forward(np.float64, key, n)
        a, lp, en, v = ctx.policy_act(obs, mask=mask, action=acts)
        errs = rel(lp, lp_o), rel(en, en_o), rel(v, v_o), rel(ctx.get_value(obs), v_o)
        print("%s n %d: log-prob %.3g entropy %.3g value %.3g get_value %.3g" % ((key, n) + errs))
        assert np.array_equal(a, acts) and max(errs) <= FWD_BAR
        ga, glp, _, gv = ctx.policy_act_greedy(obs, mask=mask)
        _, flp, _, fv = ctx.policy_act(obs, mask=mask, action=ga)
        assert np.array_equal(bits(flp), bits(glp)) and np.array_equal(bits(fv), bits(gv))
    ctx.close()


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("obs,D", STEP_SHAPES)
def test_gaussian_minibatch_step_against_the_rounded_float64_model(P, H, obs, D, M):
    N, T, params, buf, idx = gauss_step_case(H, obs, D, M)
    ctx = gauss_ctx(P, H, obs, D, N=N, T=T, nmb=1)
    ctx.set_params(params)
    for name, arr in zip(("OBS", "ACTIONS", "LOGPROBS", "ADVANTAGES", "RETURNS", "VALUES"), buf):
        ctx.write(name, arr)
    grads = ctx.minibatch_forward_backward(idx)
    st = ctx.stats()
    assert np.array_equal(bits(grads), bits(ctx.minibatch_forward_backward(idx))) and ctx.gauss_fused_launches() == (0, 0, 2)
    g_o, sc = gauss_step(np.float64, H, obs, D, params, buf, idx)
    assert 0.4 < sc["clipfrac"] < 0.9
    check_step("H %d obs %d D %d M %d" % (H, obs, D, M), obs, st, sc, grads, g_o, tensor_shapes(obs, H, 2, D))
    ctx.close()


@pytest.mark.parametrize("key,M", CAT_STEPS)
def test_categorical_minibatch_step_against_the_rounded_float64_model(P, key, M):
    s = CAT[key]
    rep, idx = cat_step_case(key, M)
    ctx = cat_ctx(P, s, 8 * G.N_ENVS, G.N_STEPS, nmb=1)
    write_batch(ctx, s, rep)
    grads = ctx.minibatch_forward_backward(idx)
    st = ctx.stats()
    assert np.array_equal(bits(grads), bits(ctx.minibatch_forward_backward(idx))) and ctx.gauss_fused_launches() == (0, 0, 2)
    g64, s64 = cat_step(np.float64, key, M)
    check_step("%s M %d" % (key, M), 100, st, s64, grads, g64, cat_shapes(key))
    ctx.close()


@pytest.mark.parametrize("H", [64, 128])
def test_every_entry_point_gives_a_row_the_same_value_bits(P, H):
    """policy_act_f32, get_value, a ppo_dev_observe fold event and a second identical call, on rows of the first, second and last workgroup and tile"""
    obs, D, N = 100, 3, 300
    rng = np.random.default_rng(obs + H)
    ctx = gauss_ctx(P, H, obs, D, N=N, T=1, lr=0.0)
    ctx.set_params(gauss_params(rng, obs, D, H))
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


def test_the_facade_creates_the_bf16_context(tmp_path):
    """host/tests/host_fused_bf16_test in a fresh directory: `bf16 = true` in [network] on PPO_HostEnvBox beside matrix_cores, fused_policy and hidden_size 128"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ppo-libtorch_amd", "host", "host_fused_bf16_test")
    r = subprocess.run([exe], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host_fused_bf16_test ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
