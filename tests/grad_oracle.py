"""A float64 restatement of the generic engine's minibatch step (MLP bodies, categorical / masked categorical heads, PPO loss), written with torch autograd
on the CPU -- TEST INFRASTRUCTURE, NOT PRODUCT CODE, and not a test.  Written from the formulas (PPO_Discrete.cpp:585-631 as oracle/ppo_oracle.c restates
them) and held to the C oracle's f32 arithmetic by tests/test_grad_oracle_cpu.py; the GPU tests (tests/test_gpu_generic_grads.py) compare the HIP kernels'
gradient with it TENSOR BY TENSOR, each against its own largest element.

Every input is the f32 number the library sees, widened to float64; nothing is rounded afterwards.  What the C oracle does in f32 and this file in float64:
the layer products, tanh, log-softmax, exp of the log-ratio, the advantage normalisation, the clips.  The branch conditions are the same comparisons
(a row within an f32 rounding of a clip boundary could take the other branch here; make_off_policy's noise makes that a 1e-6 event per row).
"""
import numpy as np
import torch

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
# float64 on the same rows.  K_F32 = twice the worst d_hip / d_ref measured on an MI355X (tests/test_gpu_generic_grads.py; table in DESIGN.md).  None = not
# measured: the 1e-4 cap alone.
K_F32 = None


def f32_tensor_bars(d_ref):
    d_ref = np.asarray(d_ref, np.float64)
    return np.full(d_ref.shape, 1e-4) if K_F32 is None else np.minimum(1e-4, K_F32 * np.maximum(d_ref, 1e-7))


def clipped_norm(grad, shapes):
    """clip_grad_norm_'s total norm: the L2 norm of the per-tensor L2 norms (= the L2 norm of the flat gradient), in float64"""
    return float(np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for _, _, _, _, v in split(np.asarray(grad), shapes))))


# -------------------------------------------------------------------------------------------------------------------------------------------------------
# The shapes both new test files walk.  Each is one small context: 48 envs x 24 steps, two minibatches (the workspace holds 576 rows).  `lists` = sizes of
# the random row subsets stepped on; dtype 0 = f32, 1 = bf16 storage.  What each reaches in the library is said in tests/test_gpu_generic_grads.py.
# -------------------------------------------------------------------------------------------------------------------------------------------------------
N_ENVS, N_STEPS = 48, 24
BASE_HP = dict(gamma=0.99, gae_lambda=0.95, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5)
SHAPES = {
    # name: obs, hidden, n_hidden, heads, masked, dtype, lists, clip_vloss / norm_adv, seed
    "f32 obs5 h30x2 (3,)":            dict(obs=5, hidden=30, n_hidden=2, heads=(3,), masked=False, dtype=0, lists=(576, 225, 200, 2), seed=11),
    "f32 obs20 h160x2 (2,3) masked":  dict(obs=20, hidden=160, n_hidden=2, heads=(2, 3), masked=True, dtype=0, lists=(576, 225, 65, 2), seed=13),
    "f32 obs7 h48x1 (4,)":            dict(obs=7, hidden=48, n_hidden=1, heads=(4,), masked=False, dtype=0, lists=(576, 225, 2), seed=9),
    "f32 obs24 h64x2 six heads masked, plain value loss, raw advantages":
                                      dict(obs=24, hidden=64, n_hidden=2, heads=(5, 3, 4, 2, 3, 3), masked=True, dtype=0, lists=(576, 225, 2), seed=21,
                                           clip_vloss=False, norm_adv=False),
    "bf16 obs120 h48x2 (2,3) masked": dict(obs=120, hidden=48, n_hidden=2, heads=(2, 3), masked=True, dtype=1, lists=(576, 225, 2), seed=13),
    "bf16 obs132 h160x3 (3,3,3,2) masked":
                                      dict(obs=132, hidden=160, n_hidden=3, heads=(3, 3, 3, 2), masked=True, dtype=1, lists=(576, 225, 65, 40, 2), seed=17),
    "bf16 obs130 h160x3 (3,3,3,2) masked":
                                      dict(obs=130, hidden=160, n_hidden=3, heads=(3, 3, 3, 2), masked=True, dtype=1, lists=(576, 225, 65, 2), seed=17),
    "bf16 obs376 h256x4 (3,3,3,2) masked":
                                      dict(obs=376, hidden=256, n_hidden=4, heads=(3, 3, 3, 2), masked=True, dtype=1, lists=(576,), seed=3),
    "bf16 obs24 h64x2 (5,3,4)":       dict(obs=24, hidden=64, n_hidden=2, heads=(5, 3, 4), masked=False, dtype=1, lists=(576, 225, 2), seed=21),
    "bf16 obs24 h64x2 six heads masked":
                                      dict(obs=24, hidden=64, n_hidden=2, heads=(5, 3, 4, 2, 3, 3), masked=True, dtype=1, lists=(576, 225, 2), seed=21),
    "bf16 obs120 h128x1 (4,) plain value loss":
                                      dict(obs=120, hidden=128, n_hidden=1, heads=(4,), masked=False, dtype=1, lists=(576, 225, 2), seed=5, clip_vloss=False),
    "bf16 obs24 h257x2 (2,3) masked": dict(obs=24, hidden=257, n_hidden=2, heads=(2, 3), masked=True, dtype=1, lists=(576, 225, 2), seed=7),
}


def shape_hp(s):
    return dict(BASE_HP, norm_adv=bool(s.get("norm_adv", True)), clip_vloss=bool(s.get("clip_vloss", True)))


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


def single_action_rows(masks, heads):
    """share of rows in which some head has exactly one allowed action"""
    masks = np.asarray(masks)
    one = np.zeros(masks.shape[0], bool)
    off = 0
    for w in heads:
        one |= masks[:, off:off + w].sum(1) == 1
        off += w
    return float(one.mean())
