"""A float64 restatement of the generic engine's minibatch step (MLP bodies, categorical / masked categorical heads, PPO loss), written with torch autograd
on the CPU -- TEST INFRASTRUCTURE, NOT PRODUCT CODE, and not a test.  Written from the formulas (PPO_Discrete.cpp:585-631 as oracle/ppo_oracle.c restates
them) and held to the C oracle's f32 arithmetic by tests/test_grad_oracle_cpu.py; the GPU tests (tests/test_gpu_generic_grads.py) compare the HIP kernels'
gradient with it TENSOR BY TENSOR, each against its own largest element.  The same oracle holds the 2 x 64 kernels of caller-stepped contexts
(REF_SHAPES below, tests/test_gpu_ref_shape_grads.py); stand_in_batch makes their batch without the library, since such a context has no env to roll out.

Every input is the f32 number the library sees, widened to float64; nothing is rounded afterwards.  What the C oracle does in f32 and this file in float64:
the layer products, tanh, log-softmax, exp of the log-ratio, the advantage normalisation, the clips.  The branch conditions are the same comparisons
(a row within an f32 rounding of a clip boundary could take the other branch here; make_off_policy's noise makes that a 1e-6 event per row).
"""
import numpy as np
import torch

import oracle as O

F64 = torch.float64
FLT_MIN = float(np.finfo(np.float32).tiny)
MASK_FILL = -1e8          # CategoricalMasked: where(mask, logits, -1e8f)  (oracle/ppo_oracle.c: categorical_row)
STAT_NAMES = ("pg_loss", "v_loss", "entropy_loss", "approx_kl", "clipfrac", "loss")


def _f(x):
    """an f32 hyper-parameter as the library holds it (c_float), widened"""
    return float(np.float32(x))


def split(flat, shapes):
    """(index, net, layer, "w" | "b", view) for every tensor of the library's parameter order: shapes = oracle.param_shapes(net), [out, in] weight then
    [out, 1] bias per layer, critic layers (net 0) first, then the actor's (net 1)"""
    shapes = np.asarray(shapes, np.int64).reshape(-1, 2)
    n_layers = len(shapes) // 4
    at = 0
    for i, (a, b) in enumerate(shapes):
        n = int(a * b)
        yield i, i // (2 * n_layers), (i // 2) % n_layers, "wb"[i & 1], flat[at:at + n].reshape(int(a), int(b))
        at += n
    assert at == len(flat), (at, len(flat))


def tensor_name(net, layer, kind):
    return "%s L%d %s" % (("critic", "actor")[net], layer, kind)


def tensor_distance(g, g_ref, shapes):
    """per tensor: max |g - g_ref| / max |g_ref| over that tensor alone (inf where the reference tensor is all zero and g is not)"""
    g, g_ref = np.asarray(g, np.float64), np.asarray(g_ref, np.float64)
    out = []
    for (_, _, _, _, a), (_, _, _, _, r) in zip(split(g, shapes), split(g_ref, shapes)):
        top, err = np.abs(r).max(), np.abs(a - r).max()
        out.append(err / top if top > 0 else (0.0 if err == 0 else np.inf))
    return np.array(out)


def make_off_policy(rng, logp, values, logp_std=0.3, value_std=0.3):
    """Perturbed f32 copies of the rollout's LOGPROBS and VALUES: normal noise that moves the step away from ratio = 1 and v = v_old.  With clip_coef 0.2 a
    std of 0.3 puts about half the rows outside each clip (P(|exp(n) - 1| > 0.2) = 0.50, P(|n| > 0.2) = 0.50 for n ~ N(0, 0.3^2))."""
    logp, values = np.asarray(logp, np.float32), np.asarray(values, np.float32)
    return ((logp + logp_std * rng.standard_normal(logp.shape)).astype(np.float32),
            (values + value_std * rng.standard_normal(values.shape)).astype(np.float32))


def _mlp(layers, x):
    h = x
    for i in range(0, len(layers) - 2, 2):
        h = torch.tanh(h @ layers[i].T + layers[i + 1].T)
    return h @ layers[-2].T + layers[-1].T


def _heads(logits, actions, masks, heads, masked):
    """log-prob of the taken actions and entropy, summed over heads.  Masked: disabled logits become -1e8 before the log-softmax and their p log p terms
    leave the entropy (a head with one allowed action has p = 1, entropy 0 and no gradient).  Plain: Categorical's entropy clamps the log-probs at
    FLT_MIN from below, so it is -FLT_MIN * sum(p): zero, with a zero gradient."""
    lp = torch.zeros(logits.shape[0], dtype=F64)
    ent = torch.zeros(logits.shape[0], dtype=F64)
    off = 0
    for h, w in enumerate(heads):
        z = logits[:, off:off + w]
        if masked:
            m = masks[:, off:off + w]
            z = torch.where(m, z, torch.full_like(z, MASK_FILL))
        ml = z - torch.logsumexp(z, dim=1, keepdim=True)
        p = ml.exp()
        lp = lp + ml.gather(1, actions[:, h:h + 1]).squeeze(1)
        if masked:
            ent = ent - torch.where(m, ml * p, torch.zeros_like(p)).sum(1)
        else:
            ent = ent - (torch.clamp(ml, min=FLT_MIN) * p).sum(1)
        off += w
    return lp, ent


def minibatch_grads(shapes, heads, masked, hp, params, obs, actions, logp, adv, ret, values, idx, masks=None, rows=None):
    """One minibatch step in float64.  shapes = oracle.param_shapes(net); hp = dict(clip_coef, ent_coef, vf_coef, norm_adv, clip_vloss); the buffers are the
    flat [B, ...] rollout arrays and idx the step's rows.  Returns (flat float64 gradient in the library's order, dict of the six scalars).
    rows (a dict, optional) receives per-row arrays the tests' preconditions and derived bars read: ratio, l1, l2, dv = v - v_old, adv, v_err."""
    shapes = np.asarray(shapes, np.int64).reshape(-1, 2)
    idx = np.asarray(idx, np.int64)
    flat = torch.tensor(np.asarray(params, np.float64))
    ts = [v.clone().requires_grad_(True) for _, _, _, _, v in split(flat, shapes)]
    k = len(ts) // 2
    critic, actor = ts[:k], ts[k:]
    t = lambda a: torch.tensor(np.asarray(a)[idx].astype(np.float64))   # noqa: E731
    x, oldlp, A, R, oldv = t(obs), t(logp).reshape(-1), t(adv).reshape(-1), t(ret).reshape(-1), t(values).reshape(-1)
    act = torch.tensor(np.asarray(actions)[idx].astype(np.int64)).reshape(len(idx), len(heads))
    m = torch.tensor(np.asarray(masks)[idx] != 0) if masked else None
    clip, ent_coef, vf_coef = _f(hp["clip_coef"]), _f(hp["ent_coef"]), _f(hp["vf_coef"])
    lo, hi = float(np.float32(1) - np.float32(clip)), float(np.float32(1) + np.float32(clip))   # int - float -> float (PPO_Discrete.cpp:598)

    v = _mlp(critic, x).squeeze(1)
    newlp, ent = _heads(_mlp(actor, x), act, m, heads, masked)
    logratio = newlp - oldlp
    ratio = logratio.exp()
    if hp["norm_adv"]:
        A = (A - A.mean()) / (A.std() + _f(1e-8))            # Bessel-corrected (torch's default), PPO_Discrete.cpp:591-594
    l1, l2 = -A * ratio, -A * torch.clamp(ratio, lo, hi)
    pg = torch.max(l1, l2).mean()                            # ties split half / half; the clamp passes its gradient on [lo, hi], ends included
    un = (v - R) ** 2
    if hp["clip_vloss"]:
        un = torch.max(un, (oldv + torch.clamp(v - oldv, -clip, clip) - R) ** 2)
    vl = 0.5 * un.mean()
    el = ent.mean()
    loss = pg - ent_coef * el + vf_coef * vl
    loss.backward()
    grad = np.concatenate([(p.grad if p.grad is not None else torch.zeros_like(p)).numpy().ravel() for p in ts])
    with torch.no_grad():
        sc = dict(pg_loss=float(pg), v_loss=float(vl), entropy_loss=float(el), approx_kl=float(((ratio - 1) - logratio).mean()),
                  clipfrac=float(((ratio - 1).abs() > clip).double().mean()), loss=float(loss))
        if rows is not None:
            rows.update(ratio=ratio.numpy().copy(), l1=l1.numpy().copy(), l2=l2.numpy().copy(), dv=(v - oldv).numpy().copy(), adv=A.numpy().copy(),
                        v_err=torch.sqrt(un).numpy().copy())   # adv: as the loss uses it; v_err: the larger of |v - R|, |v_clipped - R|
    return grad, sc


# f32 kernels against float64, per tensor: the bar is min(1e-4, K_F32 max(d_ref, 1e-7)) of the tensor's largest element, d_ref = the C oracle's own distance from
# float64 on the same rows.  K_F32 is K_REF's committed value (below), not a figure taken from the generic engine: the same yardstick d_ref, the same float64
# oracle, and sibling split-operand matrix-core products (f32x3 here, fp16 terms there).  A worst f32 ratio above 8 is a finding to trace to its kernel
# ("Per-tensor gradient checks of the generic engine"), not a reason to move this constant.
K_F32 = 14.6


def f32_tensor_bars(d_ref):
    d_ref = np.asarray(d_ref, np.float64)
    return np.minimum(1e-4, K_F32 * np.maximum(d_ref, 1e-7))


# bf16 kernels, per tensor, against the C oracle's bf16 mode (which rounds where the kernels round).  Two things make a bar from the two references alone:
#
# branch-safe rows.  A bf16 activation that tips across a rounding boundary moves a row's log-prob by about 2e-3 and its value by about 4e-3 (the suite's bf16
#   forward bars, TOL[1] of tests/test_gpu_generic.py).  A row that sits that close to a clip boundary, or to a tie of the value loss's max, then takes the other
#   branch and its whole gradient contribution switches on or off: two correct bf16 implementations differ by percents of a tensor, heavy-tailed (the bf16 oracle
#   against itself after a relative 2e-6 parameter change: up to 2.3e-1 of a tensor at obs376 h256x4; tests/test_grad_oracle_cpu.py).  The bf16 tests therefore
#   step on rows that keep a margin from every such switch.  margin = 0.02 is derived: 10 x the log-prob bar 2e-3, 5 x the value bar 4e-3.
# the unit.  d_b16[t] = the bf16 oracle's own per-tensor distance from float64 on the same rows: what bf16 arithmetic costs tensor t.  A kernel that rounds where
#   the oracle rounds is no farther from the bf16 oracle than bf16 arithmetic itself is from exact arithmetic: bar[t] = max(d_b16[t], median(d_b16)), margin 1 x.
#   The unit is 5e-3 .. 1e-2; a structural error (one of four slabs, a column block, a column-sum tile) moves a tensor by tens of percent.  Nothing measured on a
#   kernel enters the bar.
BRANCH_MARGIN = 0.02
SAFE_SHARE_MIN = 0.75        # the rows that stay are at least this share of the batch (a condition of the tests; 80 - 93 % on stand-in data)
D_B16_MAX = 2e-2             # stand-in data: the bf16 oracle's own distance from float64 on safe rows stays below this per tensor (tests/test_grad_oracle_cpu.py)
D_B16_ROLLED_MAX = 1e-1      # batches rolled out with the actor's head x 30 (a sharp policy: d_b16 of actor tensors is 2e-2 .. 5e-2 there): a bar must stay below the
                             # smallest structural error the lists are built to show, one 64-row column-sum tile of 576 rows = 11 % of a bias gradient


def _branch_state(rows, hp, values_old, returns, margin):
    """(safe, side) per row from one arithmetic's ratio and dv: safe = no switch within margin; side = which branch each switch is on (one bit each)"""
    clip = _f(hp["clip_coef"])
    ratio, dv = np.asarray(rows["ratio"], np.float64), np.asarray(rows["dv"], np.float64)
    safe = np.abs(np.abs(ratio - 1.0) - clip) > margin * np.maximum(ratio, 1.0)
    side = (np.abs(ratio - 1.0) > clip).astype(np.int64)
    if hp["clip_vloss"]:
        v_old, R = np.asarray(values_old, np.float64).reshape(-1), np.asarray(returns, np.float64).reshape(-1)
        v, v_clipped = v_old + dv, v_old + np.clip(dv, -clip, clip)
        safe &= np.abs(np.abs(dv) - clip) > margin
        safe &= (np.abs(dv) < clip) | (np.abs(np.abs(v - R) - np.abs(v_clipped - R)) > margin)
        side += 2 * (np.abs(dv) > clip) + 4 * (np.abs(v - R) >= np.abs(v_clipped - R))
    return safe, side


def branch_safe_rows(rows, hp, values_old, returns, margin=BRANCH_MARGIN, rows_b16=None):
    """Boolean array over the rows minibatch_grads(..., rows=rows) stepped on (float64): True where no PPO branch is within `margin` of switching.
    values_old / returns = VALUES / RETURNS of those rows, in the same order.
      ratio clip:      | |ratio - 1| - clip | > margin max(ratio, 1)      (margin is on the log-prob; d ratio = ratio d logp)
      value clip:      | |dv| - clip | > margin                            (dv = v - v_old; clip_vloss only)
      value loss max:  |dv| < clip (both arms equal), or | |v - R| - |v_clipped - R| | > margin   (clip_vloss only)
    rows_b16 (bf16_forward_rows: the same rows' ratio and dv in the bf16 oracle's arithmetic): the row must hold the three conditions there as well, and lie on
    the same side of every switch in both arithmetics.  The margin covers what separates two bf16 implementations (2e-3, 4e-3), not what separates bf16 from
    float64: with a sharp policy a bf16 log-prob is tenths from the float64 one (0.38 at configs[4]'s shape, tests/test_gpu_generic.py), so a row that float64
    puts well inside a clip can sit on its boundary, or beyond it, in bf16.  Without this the bf16 oracle and float64 step on different branches, d_b16 is tens of
    percent and the bar built from it holds nothing (seen on an MI355X-rolled batch at obs132 h160x3: d_b16 0.3 .. 0.7 on every actor tensor)."""
    safe, side = _branch_state(rows, hp, values_old, returns, margin)
    if rows_b16 is not None:
        safe_b, side_b = _branch_state(rows_b16, hp, values_old, returns, margin)
        safe = safe & safe_b & (side == side_b)
    return safe


def bf16_forward_rows(s, params, obs, actions, masks, logp_old, values_old):
    """ratio and dv = v - v_old of every row as the C oracle's bf16 mode computes them (its forward pass alone), for branch_safe_rows"""
    net = O.Net.make(s["obs"], list(s["heads"]), hidden=s["hidden"], n_hidden=s["n_hidden"], dist_kind=O.DIST_MASKED if s["masked"] else O.DIST_CATEGORICAL, dtype=1)
    lp, _, v = O.evaluate(net, params, obs, actions, masks if s["masked"] else None)
    return dict(ratio=np.exp(lp.astype(np.float64) - np.asarray(logp_old, np.float64).reshape(-1)), dv=v.astype(np.float64) - np.asarray(values_old, np.float64).reshape(-1))


def bf16_tensor_bars(d_b16):
    """per tensor: max(d_b16[t], median(d_b16)), d_b16 = tensor_distance(bf16 oracle, float64 oracle) on the rows of the step"""
    d_b16 = np.asarray(d_b16, np.float64)
    return np.maximum(d_b16, np.median(d_b16))


# The 2 x 64 kernels (tests/test_gpu_ref_shape_grads.py) get a constant of their own: the matrix-core update kernels cut every f32 operand into fp16 terms, so
# their distance from float64 is not the generic engine's.  K_REF = twice the worst d_hip / d_ref measured on an MI355X over REF_SHAPES, their flags and lists
# (table in DESIGN.md, "Per-tensor gradient checks").  None = not measured: the 1e-4 cap alone.
# Measured: worst ratio 7.28 (obs 4 (2,) under PPO_KERNEL_UPDATE_VECTOR, M = 33, the critic's output bias, where d_ref sits on the 1e-7 floor); worst on the
# matrix cores 4.72 (the wave-specialised kernel, same shape).
K_REF = 14.6


def ref_tensor_bars(d_ref):
    d_ref = np.asarray(d_ref, np.float64)
    return np.full(d_ref.shape, 1e-4) if K_REF is None else np.minimum(1e-4, K_REF * np.maximum(d_ref, 1e-7))


def clipped_norm(grad, shapes):
    """clip_grad_norm_'s total norm: the L2 norm of the per-tensor L2 norms (= the L2 norm of the flat gradient), in float64"""
    return float(np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for _, _, _, _, v in split(np.asarray(grad), shapes))))


# -------------------------------------------------------------------------------------------------------------------------------------------------------
# The shapes both new test files walk.  Each is one small context: 48 envs x 24 steps, two minibatches (the workspace holds 576 rows).  `lists` = sizes of
# the random row subsets stepped on; dtype 0 = f32, 1 = bf16 storage.  What each reaches in the library is said in tests/test_gpu_generic_grads.py.
# The bf16 shapes' seeds are the first, counting up from an arbitrary start (13, 17, 3, 21, 5, 7), at which the conditions of tests/test_grad_oracle_cpu.py
# hold on stand-in data: on some batches the critic's output-bias gradient (a signed mean of residuals) nearly cancels on one list, or the one live row of a
# two-row list has a small residual, and the bf16 oracle alone is then 3e-2 .. 7e-2 of that tensor from float64 (traced there).
# -------------------------------------------------------------------------------------------------------------------------------------------------------
N_ENVS, N_STEPS = 48, 24
BASE_HP = dict(gamma=0.99, gae_lambda=0.95, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5)
SHAPES = {
    # name: obs, hidden, n_hidden, heads, masked, dtype, lists, clip_vloss / norm_adv, seed
    "f32 obs5 h30x2 (3,)":            dict(obs=5, hidden=30, n_hidden=2, heads=(3,), masked=False, dtype=0, lists=(576, 225, 200, 2), seed=11),
    "f32 obs20 h160x2 (2,3) masked":  dict(obs=20, hidden=160, n_hidden=2, heads=(2, 3), masked=True, dtype=0, lists=(576, 225, 65, 2), seed=13),
    "f32 obs7 h48x1 (4,)":            dict(obs=7, hidden=48, n_hidden=1, heads=(4,), masked=False, dtype=0, lists=(576, 225, 2), seed=9,
                                           max_grad_norm=0.25),   # its eight steps' norms are 0.32 .. 0.49: 0.5 never clips (tests/test_gpu_generic_update.py)
    "f32 obs24 h64x2 six heads masked, plain value loss, raw advantages":
                                      dict(obs=24, hidden=64, n_hidden=2, heads=(5, 3, 4, 2, 3, 3), masked=True, dtype=0, lists=(576, 225, 2), seed=21,
                                           clip_vloss=False, norm_adv=False),
    "bf16 obs120 h48x2 (2,3) masked": dict(obs=120, hidden=48, n_hidden=2, heads=(2, 3), masked=True, dtype=1, lists=(576, 225, 2), seed=14),
    "bf16 obs132 h160x3 (3,3,3,2) masked":
                                      dict(obs=132, hidden=160, n_hidden=3, heads=(3, 3, 3, 2), masked=True, dtype=1, lists=(576, 225, 65, 40, 2), seed=20),
    "bf16 obs130 h160x3 (3,3,3,2) masked":
                                      dict(obs=130, hidden=160, n_hidden=3, heads=(3, 3, 3, 2), masked=True, dtype=1, lists=(576, 225, 65, 2), seed=17),
    "bf16 obs376 h256x4 (3,3,3,2) masked":
                                      dict(obs=376, hidden=256, n_hidden=4, heads=(3, 3, 3, 2), masked=True, dtype=1, lists=(576,), seed=3),
    "bf16 obs24 h64x2 (5,3,4)":       dict(obs=24, hidden=64, n_hidden=2, heads=(5, 3, 4), masked=False, dtype=1, lists=(576, 225, 2), seed=22),
    "bf16 obs24 h64x2 six heads masked":
                                      dict(obs=24, hidden=64, n_hidden=2, heads=(5, 3, 4, 2, 3, 3), masked=True, dtype=1, lists=(576, 225, 2), seed=22),
    "bf16 obs120 h128x1 (4,) plain value loss":
                                      dict(obs=120, hidden=128, n_hidden=1, heads=(4,), masked=False, dtype=1, lists=(576, 225, 2), seed=7, clip_vloss=False),
    "bf16 obs24 h257x2 (2,3) masked": dict(obs=24, hidden=257, n_hidden=2, heads=(2, 3), masked=True, dtype=1, lists=(576, 225, 2), seed=7),
}


def shape_hp(s):
    return dict(BASE_HP, norm_adv=bool(s.get("norm_adv", True)), clip_vloss=bool(s.get("clip_vloss", True)), max_grad_norm=s.get("max_grad_norm", BASE_HP["max_grad_norm"]))


def context(P, s, flags=0, num_minibatches=2, update_epochs=1, **over):
    """A synthetic-env context of a SHAPES entry (P = the loaded package): 48 envs x 24 steps, the shape's own shape_hp; `over` replaces config fields"""
    kw = dict(env_kind=P.ENV_SYNTHETIC, dist_kind=P.DIST_MASKED if s["masked"] else P.DIST_CATEGORICAL, obs_size=s["obs"], head_dims=tuple(s["heads"]),
              hidden=s["hidden"], n_hidden=s["n_hidden"], num_envs=N_ENVS, num_steps=N_STEPS, num_minibatches=num_minibatches, update_epochs=update_epochs,
              max_episode_steps=30, seed=s["seed"], total_timesteps=8 * N_ENVS * N_STEPS, learning_rate=1e-3, anneal_lr=False,
              compute_dtype=s["dtype"], kernel_flags=flags, **shape_hp(s))
    kw.update(over)
    return P.Context(P.make_config(**kw))


def make_params(P, s):
    """init_orthogonal, 0.02 normal noise on every parameter (biases away from zero), the actor's head x 30 (a policy that is not uniform)"""
    ctx = context(P, s, 0)
    ctx.init_orthogonal(s["seed"])
    params = ctx.get_params()
    ctx.close()
    A = sum(s["heads"])
    params = (params + 0.02 * np.random.default_rng(s["seed"]).standard_normal(params.shape)).astype(np.float32)
    params[-(A * s["hidden"] + A):] *= 30.0
    return params


def clip_scale(grad, total, max_norm):
    """clip_grad_norm_'s scaling given the total norm as an f32 number (the device's published one, or the C oracle's): every step in float32, as
    oracle/ppo_oracle.c:orc_clip_grad_norm and the kernels do it -- c = min(1, max_norm / (total + 1e-6f)), g * c (also when c is 1).
    Returns (the scaled f32 gradient, c)."""
    c = np.float32(max_norm) / (np.float32(total) + np.float32(1e-6))
    c = np.float32(1.0) if c > np.float32(1.0) else np.float32(c)
    return (np.asarray(grad, np.float32) * c).astype(np.float32), c


def index_lists(s, d_logp, d_values):
    """The shape's random row subsets (int32, without repeats).  d_logp / d_values = what make_off_policy added to the flat LOGPROBS / VALUES.  A two-row
    list cannot rely on chance to carry a gradient (both rows on the dead side of both clips: every critic tensor zero), so it is one row well inside both
    clips (|noise| < 0.1) and one well outside both (> 0.3), the first of each kind in the permutation."""
    rng = np.random.default_rng(1000 + s["seed"])
    d_logp, d_values = np.abs(np.asarray(d_logp).reshape(-1)), np.abs(np.asarray(d_values).reshape(-1))
    out = []
    for M in s["lists"]:
        perm = rng.permutation(d_logp.size)
        if M == 2:
            inside = perm[(d_logp[perm] < 0.1) & (d_values[perm] < 0.1)]
            outside = perm[(d_logp[perm] > 0.3) & (d_values[perm] > 0.3)]
            perm = np.array([inside[0], outside[0]])
        out.append(perm[:M].astype(np.int32))
    return out


def safe_index_lists(s, safe, d_logp, d_values):
    """index_lists on branch-safe rows: the same permutations from the same rng stream, restricted to the rows where `safe` (branch_safe_rows over the whole
    batch) holds BEFORE the first M are taken, so every list keeps its exact size (the sizes are there for tile and range edges).  The two-row list keeps its
    inside / outside rule."""
    rng = np.random.default_rng(1000 + s["seed"])
    safe = np.asarray(safe, bool).reshape(-1)
    d_logp, d_values = np.abs(np.asarray(d_logp).reshape(-1)), np.abs(np.asarray(d_values).reshape(-1))
    assert safe.size == d_logp.size
    out = []
    for M in s["lists"]:
        perm = rng.permutation(d_logp.size)
        perm = perm[safe[perm]]
        if M == 2:
            inside = perm[(d_logp[perm] < 0.1) & (d_values[perm] < 0.1)]
            outside = perm[(d_logp[perm] > 0.3) & (d_values[perm] > 0.3)]
            perm = np.array([inside[0], outside[0]])
        assert perm.size >= M, (M, perm.size)
        out.append(perm[:M].astype(np.int32))
    return out


def single_action_rows(masks, heads):
    """share of rows in which some head has exactly one allowed action"""
    masks = np.asarray(masks)
    one = np.zeros(masks.shape[0], bool)
    off = 0
    for w in heads:
        one |= masks[:, off:off + w].sum(1) == 1
        off += w
    return float(one.mean())


# -------------------------------------------------------------------------------------------------------------------------------------------------------
# The 2 x 64 kernels' shapes (tests/test_gpu_ref_shape_grads.py): the reference's network (hidden 64 x 2, f32) on a caller-stepped context, one row per
# dispatch case of api.hip.  flags = the ppo_config.kernel_flags values each shape runs under.  lists: 576 = whole 32-row tiles, 225 = a one-row last tile,
# 33 = one tile plus a row, 2 = fewer rows than a tile.  Each shape has its own seed, chosen so that the conditions tests/test_grad_oracle_cpu.py asserts hold
# (the C oracle alone inside every bar of the GPU test, every tensor's float64 gradient non-zero on every list).
# -------------------------------------------------------------------------------------------------------------------------------------------------------
VECTOR, ONE_WAVE = 2, 4      # PPO_KERNEL_UPDATE_VECTOR, PPO_KERNEL_UPDATE_ONE_WAVE (include/ppo_hip.h)
REF_LISTS = (576, 225, 33, 2)


def _ref(obs, heads, masked, flags, seed, **kw):
    return dict(obs=obs, hidden=64, n_hidden=2, heads=tuple(heads), masked=masked, dtype=0, lists=REF_LISTS, seed=seed, flags=tuple(flags), **kw)


REF_SHAPES = {
    "ref cartpole obs4 (2,)":            _ref(4, (2,), False, (0, ONE_WAVE, VECTOR), seed=31),
    "ref mountaincar obs2 (3,) masked":  _ref(2, (3,), True, (0, ONE_WAVE, VECTOR), seed=32),
    "ref obs4 (4,)":                     _ref(4, (4,), False, (0, VECTOR), seed=33),
    "ref obs4 (2,2) masked":             _ref(4, (2, 2), True, (0, VECTOR), seed=34),
    "ref obs4 (2,) masked":              _ref(4, (2,), True, (0,), seed=35),
    "ref obs2 (3,)":                     _ref(2, (3,), False, (0, VECTOR), seed=36),
    "ref obs2 (2,1,1) masked":           _ref(2, (2, 1, 1), True, (0, VECTOR), seed=37),
    "ref obs4 (3,) plain value loss, raw advantages":
                                         _ref(4, (3,), False, (0, VECTOR), seed=38, clip_vloss=False, norm_adv=False),
    "ref obs4 (3,2)":                    _ref(4, (3, 2), False, (0,), seed=39),
    "ref obs2 (3,3,3,2) masked":         _ref(2, (3, 3, 3, 2), True, (0,), seed=40),
    "ref obs8 (4,)":                     _ref(8, (4,), False, (0,), seed=41),
    "ref obs8 eight heads of 4 masked":  _ref(8, (4,) * 8, True, (0,), seed=42),
    "ref obs8 (2,) masked, plain value loss, raw advantages":
                                         _ref(8, (2,), True, (0,), seed=43, clip_vloss=False, norm_adv=False),
}
ALL_SHAPES = dict(SHAPES, **REF_SHAPES)


def choice_rows(masks, heads):
    """per row: some head of width >= 2 has at least two allowed actions (the row can carry an actor gradient)"""
    masks = np.asarray(masks)
    any_choice = np.zeros(masks.shape[0], bool)
    off = 0
    for w in heads:
        if w >= 2:
            any_choice |= masks[:, off:off + w].sum(1) >= 2
        off += w
    return any_choice


def ref_index_lists(s, b):
    """index_lists for REF_SHAPES (b = stand_in_batch(s)), with two more conditions on a two-row list:
      norm_adv on: the two rows' raw advantages differ by at least 0.5.  (A - mean) / std of two nearly equal advantages is a cancellation: the f32 C oracle
        alone then sits 1e-4 from float64, above the GPU test's bars before any kernel ran.
      masked: the row inside both clips has a head with at least two allowed actions.  At narrow head lists most rows have one allowed action in every
        head; two such rows leave every actor tensor's gradient at zero, and a zero gradient hides any error.
    The pair is the first (inside, outside) in the permutation's order that satisfies them."""
    rng = np.random.default_rng(1000 + s["seed"])
    d_logp, d_values = np.abs(np.asarray(b["d_logp"]).reshape(-1)), np.abs(np.asarray(b["d_values"]).reshape(-1))
    adv = np.asarray(b["adv"], np.float64).reshape(-1)
    can_move = choice_rows(b["masks"], s["heads"]) if s["masked"] else np.ones(adv.size, bool)
    norm_adv = bool(s.get("norm_adv", True))
    out = []
    for M in s["lists"]:
        perm = rng.permutation(d_logp.size)
        if M == 2:
            inside = perm[(d_logp[perm] < 0.1) & (d_values[perm] < 0.1) & can_move[perm]]
            outside = perm[(d_logp[perm] > 0.3) & (d_values[perm] > 0.3)]
            pairs = ((i, o) for i in inside for o in outside if not norm_adv or abs(adv[i] - adv[o]) >= 0.5)
            perm = np.array(next(pairs))
        out.append(perm[:M].astype(np.int32))
    return out


def stand_in_batch(s):
    """Parameters and one rollout's buffers for a shape, made without the library: normal weights at the scale of the orthogonal init (sqrt(2 / in) per element
    in the hidden layers, 1 / sqrt(in) in the critic's head, 0.3 / sqrt(in) in the actor's: its 0.01 gain x 30 as the GPU tests scale it), 0.02 noise on
    every weight and bias."""
    obs_dim, hidden, n_hidden, heads, masked = s["obs"], s["hidden"], s["n_hidden"], s["heads"], s["masked"]
    N, T, seed = N_ENVS, N_STEPS, s["seed"]
    net = O.Net.make(obs_dim, list(heads), hidden=hidden, n_hidden=n_hidden, dist_kind=O.DIST_MASKED if masked else O.DIST_CATEGORICAL, dtype=0)
    shp = O.param_shapes(net)
    rng = np.random.default_rng(seed)
    parts = []
    for i, net_i, layer, kind, v in split(np.zeros(O.param_count(net)), shp):
        if kind == "w":
            gain = np.sqrt(2.0) if layer < n_hidden else (1.0 if net_i == 0 else 0.3)
            parts.append(gain / np.sqrt(v.shape[1]) * rng.standard_normal(v.shape) + 0.02 * rng.standard_normal(v.shape))
        else:
            parts.append(0.02 * rng.standard_normal(v.shape))
    params = np.concatenate([p.ravel() for p in parts]).astype(np.float32)
    envs = np.arange(N)
    obs = np.stack([O.synthetic_obs(seed, envs, t, obs_dim) for t in range(T)])
    masks = np.stack([O.synthetic_mask(seed, envs, t, list(heads)) for t in range(T)]) if masked else None
    actions, logp, values = np.empty((T, N, len(heads)), np.int64), np.empty((T, N), np.float32), np.empty((T, N), np.float32)
    rewards, dones = np.empty((T, N), np.float32), np.zeros((T, N), np.float32)
    for t in range(T):
        actions[t], logp[t], _, values[t] = O.act(net, params, obs[t], seed, t, 0, masks[t] if masked else None)
        rewards[t], d = O.synthetic_transition(seed, envs, t)
        if t + 1 < T:
            dones[t + 1] = d
    next_done = d.astype(np.int32)
    next_value = O.get_value(net, params, O.synthetic_obs(seed, envs, T, obs_dim))
    adv, ret = O.gae(rewards, values, dones, next_value, next_done, BASE_HP["gamma"], BASE_HP["gae_lambda"])
    B = T * N
    # teacher-forced evaluation equals what the sampler reported (the stand-in data is a rollout of these parameters: ratio = 1 before the perturbation)
    lp_e, _, v_e = O.evaluate(net, params, obs.reshape(B, obs_dim), actions.reshape(B, -1), masks.reshape(B, -1) if masked else None)
    assert np.abs(lp_e - logp.reshape(B)).max() <= 1e-5 and np.abs(v_e - values.reshape(B)).max() <= 1e-5
    logp2, values2 = make_off_policy(np.random.default_rng(seed + 1), logp, values)
    return dict(net=net, shapes=shp, params=params, d_logp=(logp2 - logp).reshape(B), d_values=(values2 - values).reshape(B), obs=obs.reshape(B, obs_dim),
                masks=masks.reshape(B, -1) if masked else None,
                actions=actions.reshape(B, -1), logp=logp2.reshape(B), values=values2.reshape(B), adv=adv.reshape(B), ret=ret.reshape(B))
