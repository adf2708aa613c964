"""The generic engine's minibatch step, every gradient TENSOR against its own largest element, at a step that is off the ratio = 1 point.

tests/test_gpu_generic.py compares the flat gradient with its largest element, right after the rollout: with the actor's head scaled by 30 the critic's
tensors are 4e-3 .. 5e-2 of that element (a critic layer could be wrong by percents of its own size), and with ratio = 1 and v = v_old the ratio clip, the
max's tie split, the clipped value loss and approx_kl are dead code.  Here LOGPROBS and VALUES of the rollout are perturbed (grad_oracle.make_off_policy:
about half the rows outside each clip) before the step, and the yardstick is per tensor:

  f32   the float64 oracle of tests/grad_oracle.py.  The C oracle's own distance from it on the same rows, d_ref[t] (its f32 rounding noise), scales the bar of
        tensor t: min(1e-4, K max(d_ref[t], 1e-7)) of the tensor's largest element; K = grad_oracle.K_F32 = 14.6, the constant of the 2 x 64 kernels' test
        (same yardstick, same oracle, sibling split-operand products), not a figure of this engine ("Per-tensor gradient checks of the generic
        engine": a worst ratio above 8 is a finding).  The six scalars within 1e-5, total_norm within 2e-6 (the suite's bars).
  bf16  the C oracle's bf16 mode, which rounds where the kernels round, on BRANCH-SAFE rows: one float64 forward over the whole batch marks the rows that keep a
        margin of 0.02 from both clip boundaries and from a tie of the value loss's max (grad_oracle.branch_safe_rows; at least 75 % of the batch must stay),
        in float64 AND in the bf16 oracle's forward, on the same side of each in both, and the shape's lists are drawn from those rows at their full sizes (grad_oracle.safe_index_lists).  On all rows two correct bf16 implementations
        differ by up to 2e-1 of a tensor -- a tipped bf16 activation carries a row across a clip and switches its whole contribution -- so no bar on all rows
        means anything (tests/test_grad_oracle_cpu.py measures this on the two oracles alone).  The bar of tensor t is grad_oracle.bf16_tensor_bars:
        max(d_b16[t], median(d_b16)), d_b16 = the bf16 oracle's own distance from float64 on the same rows, computed here at run time from the two references;
        d_b16 itself must stay within 1e-1 (grad_oracle.D_B16_ROLLED_MAX).  No distance measured on a kernel enters it.  The three forms of the bf16 step (default,
        PPO_KERNEL_GENERIC_SPLIT_HEAD, PPO_KERNEL_GENERIC_CLASSIC) against each other per tensor at 2e-5 (FORMS_BAR), on the same lists.

What each shape of grad_oracle.SHAPES reaches (api.hip: gen_fwd_bwd; pitches: ld_in0 = pad128(obs), ld_h = pad128(hidden)):
  f32, all shapes: gen_forward's tiled f32x3 products, loss_kernel, gen_backward's products with row ranges of 64-row multiples (one partial slab and one
      db_part row per range) and slab_sum_kernel.
    obs 5 / hidden 30 x 2 / (3,)          every tile an edge tile, 4-byte operand loads; M = 200: ranges 64 + 64 + 64 + 8 (ragged last slab)
    obs 20 / hidden 160 x 2 / (2, 3) m.   two n tiles, the second ragged; loss_kernel<MASKED>; M = 65: one row in the second range
    obs 7 / hidden 48 x 1 / (4,)          layer 0 directly under the head (no hidden-to-hidden product)
    obs 24 / hidden 64 x 2 / six heads m. clip_vloss = false, norm_adv = false: loss_kernel's other value-loss and advantage branches
  bf16, fused (obs % 4 == 0, ld_h in {128, 256}): generic_forward_kernel on rows read in place, bwd_layer_kernel<NB, P1, KCB> per layer for both nets,
      slab_sum_layers_kernel.  Layer 0's pitch is a multiple of 128, so gen_bwd_col_blocks always gives it 128-column blocks (KCB = 2); 64-column
      blocks (KCB = 1) are what every layer with a layer below it takes -- a layer 0 in 64-column blocks cannot be reached through a context.
    obs 120 / hidden 48 x 2 / (2, 3) m.          dZ pitch 128, layer 0 one 128-column block; head-fused loss (generic_forward_kernel<true, LOSS>)
    obs 132 / hidden 160 x 3 / (3, 3, 3, 2) m.   dZ pitch 256, layer 0 two 128-column blocks, three hidden layers (top activation in the other LDS tile); head-fused loss;
                                                 M = 65, 40: a one-row last tile, fewer rows than a tile
    obs 376 / hidden 256 x 4 / (3, 3, 3, 2) m.   configs[4]'s network
    obs 24 / hidden 64 x 2 / (5, 3, 4), six heads m.   heads wider than 4: loss_reg_kernel<., 4, 16> and <., 8, 32> as a launch of its own, bwd_layer_kernel for the heads
    obs 120 / hidden 128 x 1 / (4,), clip_vloss = false   one hidden layer; head-fused loss with the plain value loss
  bf16, not fused:
    obs 130 / hidden 160 x 3   obs % 4 != 0: gathered copies, launch_matmul_bf16 forward, loss_reg_kernel, bwd_layer_kernel one net per launch on two streams
    obs 24 / hidden 257 x 2    ld_h = 384, gen_fused_backward_ok false (257 is the smallest such width): the bf16 product-kernel backward, its 128-row column sums
                               (cs_part) and slab_sum_layers_kernel per net
"""
import numpy as np
import pytest

import grad_oracle as G
import oracle as O
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

# f32: the bar min(1e-4, K max(d_ref, 1e-7)) is grad_oracle.f32_tensor_bars (K = grad_oracle.K_F32, shared with tests/test_gpu_generic.py)
# bf16: the bar max(d_b16, median(d_b16)) is grad_oracle.bf16_tensor_bars (shared with tests/test_gpu_generic.py), on grad_oracle.safe_index_lists
# bf16 forms against each other: the suite's 2e-5 (test_fused_head_epilogue_equals_the_split_launches), per tensor
FORMS_BAR = 2e-5

F32_SHAPES = [n for n, s in G.SHAPES.items() if s["dtype"] == 0]
BF16_SHAPES = [n for n, s in G.SHAPES.items() if s["dtype"] == 1]


@pytest.fixture(scope="module")
def P():
    return load_package()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


make_params = G.make_params   # (moved to grad_oracle.py: tests/test_gpu_generic_update.py starts from the same parameters)


def _context(P, s, flags):
    return G.context(P, s, flags)


def rolled_out(P, s, params, flags=0, off_policy=None):
    """A context after env_reset / rollout / calc_advantage on `params`, LOGPROBS and VALUES replaced by their perturbed copies (off_policy: another
    context's, for the form-against-form test), and the flat buffers the oracles need."""
    ctx = _context(P, s, flags)
    ctx.set_params(params)
    ctx.env_reset()
    ctx.rollout()
    ctx.calc_advantage()
    T, N, A, H = G.N_STEPS, G.N_ENVS, sum(s["heads"]), len(s["heads"])
    B = T * N
    logp, values = ctx.read("LOGPROBS", (B,)), ctx.read("VALUES", (B,))
    logp2, values2 = off_policy if off_policy is not None else G.make_off_policy(np.random.default_rng(s["seed"] + 1), logp, values)
    ctx.write("LOGPROBS", logp2)
    ctx.write("VALUES", values2)
    b = dict(obs=ctx.read("OBS", (B, s["obs"])), actions=ctx.read("ACTIONS", (B, H)).astype(np.int64), masks=ctx.read("MASKS", (B, A)) if s["masked"] else None,
             logp=logp2, values=values2, adv=ctx.read("ADVANTAGES", (B,)), ret=ctx.read("RETURNS", (B,)), d_logp=logp2 - logp, d_values=values2 - values)
    return ctx, b


def oracles(s, b, params, idx, dtype):
    """(float64 gradient, scalars, per-row arrays), (C oracle's gradient in the given arithmetic, scalars), the parameter shape list.  dtype None: the float64
    oracle alone"""
    net = O.Net.make(s["obs"], list(s["heads"]), hidden=s["hidden"], n_hidden=s["n_hidden"], dist_kind=O.DIST_MASKED if s["masked"] else O.DIST_CATEGORICAL,
                     dtype=dtype or 0)
    shp = O.param_shapes(net)
    hp = G.shape_hp(s)
    rows = {}
    g64, s64 = G.minibatch_grads(shp, s["heads"], s["masked"], hp, params, b["obs"], b["actions"], b["logp"], b["adv"], b["ret"], b["values"], idx, b["masks"], rows=rows)
    if dtype is None:
        return (g64, s64, rows), None, shp
    hpo = O.HParams(norm_adv=int(hp["norm_adv"]), clip_vloss=int(hp["clip_vloss"]), **G.BASE_HP)
    gc, sc = O.minibatch_grads(net, hpo, params, b["obs"], b["actions"].astype(np.float32), b["logp"], b["adv"], b["ret"], b["values"], idx.astype(np.int64), b["masks"])
    return (g64, s64, rows), (gc, sc), shp


def check_preconditions(name, s, b, idx, g64, s64, rows, shp):
    """the step really exercises PPO's branches and every tensor carries a gradient (the same conditions tests/test_grad_oracle_cpu.py holds on stand-in data)"""
    for _, net_i, layer, kind, v in G.split(g64, shp):
        assert np.abs(v).max() > 0, (name, idx.size, G.tensor_name(net_i, layer, kind))
    if idx.size >= 40:
        assert 0.2 <= s64["clipfrac"] <= 0.8, (name, idx.size, s64["clipfrac"])
        assert 0.2 <= float((np.abs(rows["dv"]) > G.BASE_HP["clip_coef"]).mean()) <= 0.8, (name, idx.size)
        assert (rows["l1"] > rows["l2"]).any() and (rows["l1"] < rows["l2"]).any(), (name, idx.size)
        if s["masked"]:
            assert G.single_action_rows(b["masks"][idx], s["heads"]) >= 0.01, (name, idx.size)


def worst_elements(g, g_ref, shp, t):
    """where a tensor's largest differences sit: (row, column, got, reference) of the five worst elements, and how many exceed 6e-4 of the tensor's maximum"""
    a = [v for *_, v in G.split(np.asarray(g, np.float64), shp)][t]
    r = [v for *_, v in G.split(np.asarray(g_ref, np.float64), shp)][t]
    err = np.abs(a - r) / np.abs(r).max()
    order = np.argsort(err.ravel())[::-1][:5]
    return int((err > 6e-4).sum()), err.size, [(int(k // a.shape[1]), int(k % a.shape[1]), float(a.ravel()[k]), float(r.ravel()[k])) for k in order]


@pytest.mark.parametrize("name", F32_SHAPES)
def test_f32_gradient_per_tensor_against_float64(P, name):
    s = G.SHAPES[name]
    params = make_params(P, s)
    ctx, b = rolled_out(P, s, params)
    bad = []
    lists = G.index_lists(s, b["d_logp"], b["d_values"])
    for idx in lists:
        grads = ctx.minibatch_forward_backward(idx)
        st = ctx.stats()
        (g64, s64, rows), (gc, sc), shp = oracles(s, b, params, idx, 0)
        check_preconditions(name, s, b, idx, g64, s64, rows, shp)
        d_ref, d_hip = G.tensor_distance(gc, g64, shp), G.tensor_distance(grads, g64, shp)
        for (t, net_i, layer, kind, v), dr, dh, bar in zip(G.split(g64, shp), d_ref, d_hip, G.f32_tensor_bars(d_ref)):
            print("F32 %-70s M=%3d %-12s max|g| %.2e d_ref %.2e d_hip %.2e ratio %6.2f bar %.1e" %
                  (name, idx.size, G.tensor_name(net_i, layer, kind), np.abs(v).max(), dr, dh, dh / max(dr, 1e-7), bar))
            if not dh <= bar:
                bad.append((idx.size, G.tensor_name(net_i, layer, kind), float(dh), float(dr), bar))
        for key, okey in (("pg_loss", "pg_loss"), ("v_loss", "v_loss"), ("entropy_loss", "entropy_loss"), ("approx_kl", "approx_kl"), ("clipfrac_last", "clipfrac"),
                          ("loss", "loss")):
            print("F32 %-70s M=%3d %-13s hip %.8e float64 %.8e" % (name, idx.size, okey, st[key], s64[okey]))
            if not abs(st[key] - s64[okey]) <= 1e-5 * max(1.0, abs(s64[okey])):
                bad.append((idx.size, okey, st[key], s64[okey]))
    # the optimizer's norm of the first list's gradient against the float64 gradient's
    idx = lists[0]
    ctx.minibatch_forward_backward(idx)
    ctx.set_learning_rate(1e-3)
    ctx.optimizer_step()
    g64 = oracles(s, b, params, idx, 0)[0][0]
    total = G.clipped_norm(g64, shp)
    print("F32 %-70s total_norm hip %.8e float64 %.8e" % (name, ctx.stats()["total_norm"], total))
    if not abs(ctx.stats()["total_norm"] - total) <= 2e-6 * total:
        bad.append(("total_norm", ctx.stats()["total_norm"], total))
    ctx.close()
    assert not bad, bad


def _bf16_scalar_bars(s, s64, rows, M):
    """bf16 scalars against the C oracle's bf16 mode, bars derived from the suite's own forward bars (TOL of tests/test_gpu_generic.py): a bf16 row's log-prob and
    entropy within 2e-3 of that oracle's, its value within 4e-3.  Carried through each mean with the float64 rows' derivatives: |d pg / d logp| <= |adv| ratio,
    |d kl / d logp| = |ratio - 1|, |d (v_loss term) / d v| <= the larger of |v - R|, |v_clipped - R|; plus the f32 bar 1e-5 for everything else.  A wrong branch
    moves these means by tenths.  clipfrac is a count: rows whose ratio lies within 2e-3 (relative) of a clip boundary may fall on either side -- on a
    branch-safe list there is no such row (asserted), so the count is exact."""
    hp = G.shape_hp(s)
    pg = 2e-3 * float((np.abs(rows["adv"]) * rows["ratio"]).mean())
    vl = 4e-3 * float(rows["v_err"].mean()) + 0.5 * 4e-3 ** 2
    near = int((np.abs(np.abs(rows["ratio"] - 1.0) - hp["clip_coef"]) <= 2e-3 * rows["ratio"] + 1e-6).sum())
    assert near == 0, near
    bars = dict(pg_loss=pg, v_loss=vl, entropy_loss=2e-3, approx_kl=2e-3 * float(np.abs(rows["ratio"] - 1.0).mean()) + 2e-3 ** 2, clipfrac=(near + 0.5) / M,
                loss=pg + hp["ent_coef"] * 2e-3 + hp["vf_coef"] * vl)
    return {k: (v if k == "clipfrac" else v + 1e-5 * max(1.0, abs(s64[k]))) for k, v in bars.items()}


def safe_lists(name, s, b, params):
    """the shape's index lists on branch-safe rows of the rolled-out batch (one float64 and one bf16-oracle forward over all rows), and the share of rows that stayed"""
    B = G.N_ENVS * G.N_STEPS
    (_, _, rows), _, _ = oracles(s, b, params, np.arange(B), None)
    rows_b16 = G.bf16_forward_rows(s, params, b["obs"], b["actions"], b["masks"], b["logp"], b["values"])
    safe = G.branch_safe_rows(rows, G.shape_hp(s), b["values"], b["ret"], rows_b16=rows_b16)
    share = float(safe.mean())
    print("BF16 %-50s branch-safe rows %.1f%%" % (name, 100 * share))
    assert share >= G.SAFE_SHARE_MIN, (name, share)
    return G.safe_index_lists(s, safe, b["d_logp"], b["d_values"]), share


@pytest.mark.parametrize("name", BF16_SHAPES)
def test_bf16_gradient_per_tensor_against_the_bf16_oracle(P, name):
    s = G.SHAPES[name]
    params = make_params(P, s)
    ctx, b = rolled_out(P, s, params)
    lists, share = safe_lists(name, s, b, params)
    bad, worst = [], 0.0
    for idx in lists:
        grads = ctx.minibatch_forward_backward(idx)
        st = ctx.stats()
        (g64, s64, rows), (gb, sb), shp = oracles(s, b, params, idx, 1)
        check_preconditions(name, s, b, idx, g64, s64, rows, shp)
        d_hip, d_b16 = G.tensor_distance(grads, gb, shp), G.tensor_distance(gb, g64, shp)
        bars = G.bf16_tensor_bars(d_b16)
        for (t, net_i, layer, kind, v), dh, db, bar in zip(G.split(gb.astype(np.float64), shp), d_hip, d_b16, bars):
            print("BF16 %-50s M=%3d %-12s max|g| %.2e d_hip %.2e d_b16 %.2e bar %.2e d_hip / bar %5.2f" %
                  (name, idx.size, G.tensor_name(net_i, layer, kind), np.abs(v).max(), dh, db, bar, dh / bar))
            if not db <= G.D_B16_ROLLED_MAX:   # the unit itself: a bar this wide would no longer show a missing column-sum tile
                bad.append((idx.size, G.tensor_name(net_i, layer, kind), "d_b16", float(db)))
            if not dh <= bar:
                print("BF16   above its bar: %d of %d elements above 6e-4; worst (row, col, hip, oracle): %s" % worst_elements(grads, gb, shp, t))
                bad.append((idx.size, G.tensor_name(net_i, layer, kind), float(dh), float(bar)))
        worst = max(worst, float((d_hip / bars).max()))
        sbars = _bf16_scalar_bars(s, s64, rows, idx.size)
        for key, okey in (("pg_loss", "pg_loss"), ("v_loss", "v_loss"), ("entropy_loss", "entropy_loss"), ("approx_kl", "approx_kl"), ("clipfrac_last", "clipfrac"),
                          ("loss", "loss")):
            print("BF16 %-50s M=%3d %-13s hip %.8e bf16 oracle %.8e float64 %.8e" % (name, idx.size, okey, st[key], sb[okey], s64[okey]))
            if not abs(st[key] - sb[okey]) <= sbars[okey]:
                bad.append((idx.size, okey, st[key], sb[okey], sbars[okey]))
    print("BF16 %-50s worst d_hip / bar %.2f, safe share %.1f%%" % (name, worst, 100 * share))
    ctx.close()
    assert not bad, bad


@pytest.mark.parametrize("name", BF16_SHAPES)
def test_bf16_forms_agree_per_tensor(P, name):
    """default, PPO_KERNEL_GENERIC_SPLIT_HEAD and PPO_KERNEL_GENERIC_CLASSIC on the same batch, parameters and perturbed LOGPROBS / VALUES: the same roundings,
    another f32 summation order -- every tensor within 2e-5 of its own largest element.  The lists are the branch-safe ones of the test above (the forms round
    identically, so branch flips were never between them: this only keeps one set of lists for the file)."""
    s = G.SHAPES[name]
    params = make_params(P, s)
    ctx0, b = rolled_out(P, s, params)
    others = {}
    for form, flags in (("split head", P.KERNEL_GENERIC_SPLIT_HEAD), ("classic", P.KERNEL_GENERIC_CLASSIC)):
        c, b1 = rolled_out(P, s, params, flags, off_policy=(b["logp"], b["values"]))
        assert np.array_equal(bits(b1["adv"]), bits(b["adv"])) and np.array_equal(bits(b1["ret"]), bits(b["ret"])) and np.array_equal(b1["actions"], b["actions"]), form
        others[form] = c
    shp = O.param_shapes(O.Net.make(s["obs"], list(s["heads"]), hidden=s["hidden"], n_hidden=s["n_hidden"]))
    bad = []
    for idx in safe_lists(name, s, b, params)[0]:
        g0 = ctx0.minibatch_forward_backward(idx)
        assert np.isfinite(g0).all()
        for form, c in others.items():
            d = G.tensor_distance(c.minibatch_forward_backward(idx), g0, shp)
            for (t, net_i, layer, kind, v), dt in zip(G.split(g0, shp), d):
                print("FORMS %-50s M=%3d %-10s %-12s %.2e" % (name, idx.size, form, G.tensor_name(net_i, layer, kind), dt))
                if not dt <= FORMS_BAR:
                    bad.append((idx.size, form, G.tensor_name(net_i, layer, kind), float(dt)))
    for c in [ctx0] + list(others.values()):
        c.close()
    assert not bad, bad
