"""The float64 oracle of tests/grad_oracle.py against the project's C oracle (oracle/ppo_oracle.c, f32 arithmetic), and the preconditions that keep the GPU
tests of tests/test_gpu_generic_grads.py and tests/test_gpu_ref_shape_grads.py honest -- no kernel involved, no GPU needed.

Per shape of grad_oracle.SHAPES (the generic engine's) and grad_oracle.REF_SHAPES (the 2 x 64 kernels'): stand-in rollout data from the C oracle's synthetic env and forward (observations, masks, sampled actions, log-probs,
values, rewards, done flags, GAE), LOGPROBS and VALUES perturbed by make_off_policy, then one minibatch step per index list in both oracles.  They must
agree per tensor (each tensor against ITS OWN largest element) and on the six scalars; the distances are the C oracle's f32 rounding noise, which is what
the GPU test's f32 bars are multiples of.

Measured (worst per-tensor distance of each shape over its index lists and tensors, C oracle f32 against float64; the test prints every tensor):

    f32 obs5 h30x2 (3,)                                                      5.2e-07
    f32 obs20 h160x2 (2,3) masked                                            5.5e-07
    f32 obs7 h48x1 (4,)                                                      1.1e-06
    f32 obs24 h64x2 six heads masked, plain value loss, raw advantages       5.1e-07
    bf16 obs120 h48x2 (2,3) masked                                           7.9e-07
    bf16 obs132 h160x3 (3,3,3,2) masked                                      1.1e-06
    bf16 obs130 h160x3 (3,3,3,2) masked                                      9.3e-07
    bf16 obs376 h256x4 (3,3,3,2) masked                                      8.7e-07
    bf16 obs24 h64x2 (5,3,4)                                                 4.2e-07
    bf16 obs24 h64x2 six heads masked                                        4.2e-07
    bf16 obs120 h128x1 (4,) plain value loss                                 7.1e-07
    bf16 obs24 h257x2 (2,3) masked                                           9.6e-07
    ref cartpole obs4 (2,)                                                   1.4e-06
    ref mountaincar obs2 (3,) masked                                         6.1e-07
    ref obs4 (4,)                                                            4.3e-07
    ref obs4 (2,2) masked                                                    1.1e-06
    ref obs4 (2,) masked                                                     1.9e-06
    ref obs2 (3,)                                                            7.2e-07
    ref obs2 (2,1,1) masked                                                  1.3e-06
    ref obs4 (3,) plain value loss, raw advantages                           5.6e-07
    ref obs4 (3,2)                                                           4.4e-07
    ref obs2 (3,3,3,2) masked                                                5.0e-07
    ref obs8 (4,)                                                            2.8e-06
    ref obs8 eight heads of 4 masked                                         1.8e-06
    ref obs8 (2,) masked, plain value loss, raw advantages                   4.3e-07

A distance above 1e-4 would be a disagreement about the formula, not noise.  The fence below is 3 x the measured worst of each shape.

The bf16 shapes are walked a second time (test_bf16_oracle_stays_within_its_own_bar_on_branch_safe_rows): the per-tensor bar the GPU test puts on the bf16
kernels -- branch-safe rows, max(d_b16, median(d_b16)) -- is asserted of the bf16 oracle itself against eight twins of it, so that the bar is known to be sound
before a kernel meets it.  Its docstring has the measured table and the trace of the obs24 h257x2 outlier.

REF_SHAPES, measured with the committed seeds (31 .. 43): the six scalars of the two oracles differ by at most 2.3e-7 (relative to max(1, |value|)); clipfrac and
the value-clip share lie between 0.45 and 0.54 on the 576- and 225-row lists; ties of max(l1, l2) are present on both.  Rows with a head of width >= 2 that has
>= 2 allowed actions: 22.0 % at obs4 (2,) masked, 23.4 % at obs2 (2,1,1) masked, 24.3 % at obs8 (2,) masked, 45 % and more elsewhere (asserted >= 10 %).
Two input conditions hold on their two-row lists (grad_oracle.ref_index_lists, asserted below): with norm_adv on the two rows' raw advantages differ by >= 0.5
(two nearly equal advantages make (A - mean) / std a cancellation, and the f32 oracle alone then sits 1e-4 from float64), and at a masked shape the row
inside both clips has a head with >= 2 allowed actions (else every actor tensor's gradient is zero).
"""
import numpy as np
import pytest

import grad_oracle as G
import oracle as O

# worst per-tensor distance measured per shape (see the docstring); the test asserts 3 x this
MEASURED = {
    'f32 obs5 h30x2 (3,)': 5.2e-07,
    'f32 obs20 h160x2 (2,3) masked': 5.5e-07,
    'f32 obs7 h48x1 (4,)': 1.1e-06,
    'f32 obs24 h64x2 six heads masked, plain value loss, raw advantages': 5.1e-07,
    'bf16 obs120 h48x2 (2,3) masked': 7.9e-07,
    'bf16 obs132 h160x3 (3,3,3,2) masked': 1.1e-06,
    'bf16 obs130 h160x3 (3,3,3,2) masked': 9.3e-07,
    'bf16 obs376 h256x4 (3,3,3,2) masked': 8.7e-07,
    'bf16 obs24 h64x2 (5,3,4)': 4.2e-07,
    'bf16 obs24 h64x2 six heads masked': 4.2e-07,
    'bf16 obs120 h128x1 (4,) plain value loss': 7.1e-07,
    'bf16 obs24 h257x2 (2,3) masked': 9.6e-07,
    # grad_oracle.REF_SHAPES (the 2 x 64 kernels' shapes), with the seeds committed there
    'ref cartpole obs4 (2,)': 1.4e-06,
    'ref mountaincar obs2 (3,) masked': 6.1e-07,
    'ref obs4 (4,)': 4.3e-07,
    'ref obs4 (2,2) masked': 1.1e-06,
    'ref obs4 (2,) masked': 1.9e-06,
    'ref obs2 (3,)': 7.2e-07,
    'ref obs2 (2,1,1) masked': 1.3e-06,
    'ref obs4 (3,) plain value loss, raw advantages': 5.6e-07,
    'ref obs4 (3,2)': 4.4e-07,
    'ref obs2 (3,3,3,2) masked': 5.0e-07,
    'ref obs8 (4,)': 2.8e-06,
    'ref obs8 eight heads of 4 masked': 1.8e-06,
    'ref obs8 (2,) masked, plain value loss, raw advantages': 4.3e-07,
}


stand_in_batch = G.stand_in_batch


def both_oracles(s, b, idx, dtype=0):
    """(float64 gradient, its scalars, per-row arrays), (C oracle's gradient, its scalars) of one step"""
    hp = G.shape_hp(s)
    rows = {}
    g64, s64 = G.minibatch_grads(b["shapes"], s["heads"], s["masked"], hp, b["params"], b["obs"], b["actions"], b["logp"], b["adv"], b["ret"], b["values"], idx,
                                 b["masks"], rows=rows)
    gc, sc = O.minibatch_grads(*_oracle_args(s, b, idx, dtype))
    return (g64, s64, rows), (gc, sc)


def _oracle_args(s, b, idx, dtype):
    """the C oracle's minibatch_grads arguments for a shape, a batch and a list (dtype 0: f32 arithmetic, 1: bf16 storage)"""
    hp = G.shape_hp(s)
    net = O.Net.make(s["obs"], list(s["heads"]), hidden=s["hidden"], n_hidden=s["n_hidden"], dist_kind=O.DIST_MASKED if s["masked"] else O.DIST_CATEGORICAL,
                     dtype=dtype)
    hpo = O.HParams(norm_adv=int(hp["norm_adv"]), clip_vloss=int(hp["clip_vloss"]), **G.BASE_HP)
    return (net, hpo, b["params"], b["obs"], b["actions"].astype(np.float32), b["logp"], b["adv"], b["ret"], b["values"], idx.astype(np.int64), b["masks"])


@pytest.mark.parametrize("name", list(G.ALL_SHAPES))
def test_float64_oracle_agrees_with_the_c_oracle_per_tensor(name):
    s = G.ALL_SHAPES[name]
    ref = name in G.REF_SHAPES
    b = stand_in_batch(s)
    if s["masked"]:   # rows in which a head has exactly one allowed action: p = 1, no entropy and no gradient through that head
        share = G.single_action_rows(b["masks"], s["heads"])
        print("%s: %.1f%% of rows have a head with one allowed action" % (name, 100 * share))
        assert share >= 0.01
    if s["masked"] and ref:   # ... and at the 2 x 64 shapes' narrow head lists, enough rows in which the actor has a choice at all
        choice = float(G.choice_rows(b["masks"], s["heads"]).mean())
        print("%s: %.1f%% of rows have a head of width >= 2 with >= 2 allowed actions" % (name, 100 * choice))
        assert choice >= 0.10
    worst = 0.0
    lists = G.ref_index_lists(s, b) if ref else G.index_lists(s, b["d_logp"], b["d_values"])
    if ref:   # what ref_index_lists promises of a two-row list
        two = lists[s["lists"].index(2)]
        assert abs(b["d_logp"][two[0]]) < 0.1 and abs(b["d_values"][two[0]]) < 0.1 and abs(b["d_logp"][two[1]]) > 0.3 and abs(b["d_values"][two[1]]) > 0.3
        assert not G.shape_hp(s)["norm_adv"] or abs(float(b["adv"][two[0]]) - float(b["adv"][two[1]])) >= 0.5, (name, b["adv"][two])
        assert not s["masked"] or G.choice_rows(b["masks"][two[:1]], s["heads"])[0], name
    for idx in lists:
        (g64, s64, rows), (gc, sc) = both_oracles(s, b, idx)
        d = G.tensor_distance(gc, g64, b["shapes"])
        for (i, net_i, layer, kind, v), di in zip(G.split(g64, b["shapes"]), d):
            print("%-70s M=%3d  %-14s max|g| %.3e  C oracle f32 vs float64 %.2e" % (name, idx.size, G.tensor_name(net_i, layer, kind), np.abs(v).max(), di))
            assert np.abs(v).max() > 0, (name, idx.size, G.tensor_name(net_i, layer, kind))          # every tensor carries a gradient
        for key in G.STAT_NAMES:
            assert abs(s64[key] - sc[key]) <= 1e-5 * max(1.0, abs(s64[key])), (name, idx.size, key, s64[key], sc[key])
        worst = max(worst, float(d.max()))
        assert d.max() <= 1e-4, (name, idx.size, d)                        # above this the two oracles disagree about the formula
        if name in MEASURED:
            assert d.max() <= 3 * MEASURED[name], (name, idx.size, d.max(), MEASURED[name])
        if idx.size >= 40:   # the conditions that make the step exercise PPO's branches (two rows cannot hold shares)
            clip = G.BASE_HP["clip_coef"]
            assert 0.2 <= s64["clipfrac"] <= 0.8, (name, idx.size, s64["clipfrac"])
            v_share = float((np.abs(rows["dv"]) > clip).mean())
            assert 0.2 <= v_share <= 0.8, (name, idx.size, v_share)
            assert (rows["l1"] > rows["l2"]).any() and (rows["l1"] < rows["l2"]).any() and (rows["l1"] == rows["l2"]).any(), (name, idx.size)
    print("MEASURED %r: %.1e," % (name, worst))
    assert name in MEASURED, "no measured distance recorded for this shape"


# -------------------------------------------------------------------------------------------------------------------------------------------------------
# The bf16 bars of tests/test_gpu_generic_grads.py, held on the two references alone
# -------------------------------------------------------------------------------------------------------------------------------------------------------
BF16_SHAPES = [n for n, s in G.SHAPES.items() if s["dtype"] == 1]
N_TWINS = 8


def twin_params(params, k):
    """twin k of a parameter vector: every parameter moved by a relative 2e-6 at most -- far below bf16 resolution (4e-3), so all it can do to the bf16 oracle
    is tip values that sit on a rounding boundary, which is what another correct bf16 implementation (another summation order, another tanh) does as well"""
    return (np.asarray(params, np.float64) * (1 + 2e-6 * np.random.default_rng(1000 + k).uniform(-1, 1, np.shape(params)))).astype(np.float32)


def whole_batch_safe_rows(s, b):
    B = b["adv"].size
    rows = {}
    G.minibatch_grads(b["shapes"], s["heads"], s["masked"], G.shape_hp(s), b["params"], b["obs"], b["actions"], b["logp"], b["adv"], b["ret"], b["values"],
                      np.arange(B), b["masks"], rows=rows)
    rows_b16 = G.bf16_forward_rows(s, b["params"], b["obs"], b["actions"], b["masks"], b["logp"], b["values"])
    return G.branch_safe_rows(rows, G.shape_hp(s), b["values"], b["ret"], rows_b16=rows_b16)


@pytest.mark.parametrize("name", BF16_SHAPES)
def test_bf16_oracle_stays_within_its_own_bar_on_branch_safe_rows(name):
    """What tests/test_gpu_generic_grads.py asserts of the bf16 kernels, asserted here of the bf16 oracle itself: twin 0 (the committed parameters) stands in for
    the HIP kernel, twins 1 .. 8 (twin_params) for the oracle it is compared with.  If the reference alone left its bar, the bar would be unsound.

    Why branch-safe rows.  On ALL rows the worst per-tensor twin distance is 7.0e-2 at obs132 h160x3 and 2.3e-1 at obs376 h256x4 (M = 576; seeds 17 and 3),
    heavy-tailed (obs132: six twins at 3e-3, two at 7e-2), and the bf16 oracle is up to 3.1e-1 of a tensor from float64: a tipped bf16 activation moves a row's
    log-prob by about 2e-3 and its value by about 4e-3, a row near a clip boundary crosses it, and its whole gradient contribution switches on or off.  No
    multiple of a once-measured distance is a bar there.  With the rows within grad_oracle.BRANCH_MARGIN of a switch removed, the same figures are regular.

    Conditions (asserted): safe rows (in float64 and in the bf16 oracle's forward, same side in both) >= 75 % of the batch; on safe lists of 40 rows or more the preconditions of the test above (clipfrac and the value-clip share
    in 0.2 .. 0.8, both sides and ties of max(l1, l2), single-action rows >= 1 %); every tensor non-zero on every list; the worst twin distance per tensor within
    bf16_tensor_bars(d_b16); d_b16 (bf16 oracle to float64, same rows) within 2e-2 per tensor.

    Measured with the committed seeds (safe share of the 1152 rows; then over the shape's safe lists and tensors: worst twin distance, worst twin distance / bar,
    d_b16 smallest median .. worst tensor):

        bf16 obs120 h48x2 (2,3) masked                 80.6 %   1.9e-03   0.35   4.9e-03 .. 8.4e-03
        bf16 obs132 h160x3 (3,3,3,2) masked            80.6 %   7.4e-03   0.89   4.4e-03 .. 1.3e-02
        bf16 obs130 h160x3 (3,3,3,2) masked            80.8 %   8.0e-03   0.79   5.2e-03 .. 1.4e-02
        bf16 obs376 h256x4 (3,3,3,2) masked            79.9 %   5.8e-03   0.68   6.4e-03 .. 9.4e-03
        bf16 obs24 h64x2 (5,3,4)                       83.4 %   4.5e-03   0.71   4.3e-03 .. 1.0e-02
        bf16 obs24 h64x2 six heads masked              83.7 %   4.7e-03   0.60   4.4e-03 .. 1.0e-02
        bf16 obs120 h128x1 (4,) plain value loss       91.0 %   3.2e-03   0.62   3.6e-03 .. 6.6e-03
        bf16 obs24 h257x2 (2,3) masked                 82.8 %   3.3e-03   0.61   4.6e-03 .. 1.3e-02

    The outlier, traced.  obs24 h257x2 at M = 225 (seed 7, rows safe in float64 alone): d_b16 4.5e-2 on ONE tensor, against 7e-3 on its other tensors and lists.
    The tensor is the critic's output bias -- one element, vf_coef x the mean over the rows of each row's value residual (v - R, or v_clipped - R, or zero where
    the clipped arm wins outside the clip).  The residuals carry both signs, and on that list their mean is a near-cancellation: sum |terms| / |sum of terms| is
    308 (the gradient is 1.6e-3) against 4 .. 15 (3e-2 .. 1.2e-1) on the lists that behave, so the rows' bf16 value errors are divided by a largest element that
    happens to be tiny.  obs120 h48x2, seed 13, M = 225 is the same (ratio 316, d_b16 6.8e-2).  The two-row lists show the same thing without a sum: one row
    lies outside the value clip and carries no critic gradient, so every critic tensor is the other row's residual times a Jacobian; at obs132 h160x3, seed 17,
    that residual is 0.146 and the value's bf16 error (4e-3, absolute) is 3e-2 of every critic tensor at once; at obs120 h128x1, seed 5, the two residuals
    cancel 6.6-fold.  None of this is a branch -- no row changes side -- so the safe-row rule has nothing to add for it; they are properties of the seed's
    batch, and those shapes got other seeds (grad_oracle.SHAPES; REF_SHAPES chose its seeds the same way): the first seed counting up from the old one at which
    every condition of this file holds.  With the bf16 side of the safe-row rule the h257 lists changed and seed 7 holds every condition, so it stayed.
    No bar was widened.

    What WAS one more switch: float64 and bf16 disagreeing about a row's branch.  The margin covers two bf16 implementations (2e-3 apart), not bf16 against
    float64.  On stand-in data (actor head gain 0.3) the two arithmetics' log-probs are close and it hardly matters; on a batch rolled out with the actor's
    head x 30 a bf16 log-prob is tenths from the float64 one, rows that float64 calls safe sit on the other side of the clip in bf16, and d_b16 was 0.3 .. 0.7
    on every actor tensor of obs132 h160x3 (M = 576) -- a bar that holds nothing.  branch_safe_rows therefore takes the bf16 oracle's forward as well
    (rows_b16): safe in both arithmetics and on the same side of every switch in both."""
    s = G.SHAPES[name]
    b = stand_in_batch(s)
    hp = G.shape_hp(s)
    safe = whole_batch_safe_rows(s, b)
    share = float(safe.mean())
    print("%s: %.1f%% of rows are branch-safe" % (name, 100 * share))
    assert share >= G.SAFE_SHARE_MIN, (name, share)
    twins = [dict(b, params=twin_params(b["params"], k)) for k in range(1, N_TWINS + 1)]
    worst_noise, worst_ratio, med, top = 0.0, 0.0, [], 0.0
    for idx in G.safe_index_lists(s, safe, b["d_logp"], b["d_values"]):
        assert safe[idx].all() and np.unique(idx).size == idx.size == s["lists"][len(med)]
        (g64, s64, rows), (gb, sb) = both_oracles(s, b, idx, dtype=1)
        assert G.branch_safe_rows(rows, hp, b["values"][idx], b["ret"][idx]).all()   # safety does not depend on which rows share the step
        for (_, net_i, layer, kind, v) in G.split(g64, b["shapes"]):
            assert np.abs(v).max() > 0, (name, idx.size, G.tensor_name(net_i, layer, kind))
        if idx.size >= 40:
            clip = G.BASE_HP["clip_coef"]
            assert 0.2 <= s64["clipfrac"] <= 0.8, (name, idx.size, s64["clipfrac"])
            v_share = float((np.abs(rows["dv"]) > clip).mean())
            assert 0.2 <= v_share <= 0.8, (name, idx.size, v_share)
            assert (rows["l1"] > rows["l2"]).any() and (rows["l1"] < rows["l2"]).any() and (rows["l1"] == rows["l2"]).any(), (name, idx.size)
            if s["masked"]:
                assert G.single_action_rows(b["masks"][idx], s["heads"]) >= 0.01, (name, idx.size)
        d_b16 = G.tensor_distance(gb, g64, b["shapes"])
        bars = G.bf16_tensor_bars(d_b16)
        noise = np.zeros_like(d_b16)
        for bk in twins:
            gk = O.minibatch_grads(*_oracle_args(s, bk, idx, 1))[0]
            noise = np.maximum(noise, G.tensor_distance(gb, gk, b["shapes"]))     # twin 0 in the kernel's place, twin k in the oracle's
        for (_, net_i, layer, kind, v), n_, d_, bar in zip(G.split(g64, b["shapes"]), noise, d_b16, bars):
            print("%-50s M=%3d %-12s max|g| %.2e twin noise %.2e d_b16 %.2e bar %.2e noise / bar %.2f" %
                  (name, idx.size, G.tensor_name(net_i, layer, kind), np.abs(v).max(), n_, d_, bar, n_ / bar))
        assert (d_b16 <= G.D_B16_MAX).all(), (name, idx.size, d_b16)
        assert (noise <= bars).all(), (name, idx.size, noise, bars)
        worst_noise, worst_ratio, top = max(worst_noise, float(noise.max())), max(worst_ratio, float((noise / bars).max())), max(top, float(d_b16.max()))
        med.append(float(np.median(d_b16)))
    print("BF16_TABLE %-45s %5.1f %%   %.1e   %.2f   %.1e .. %.1e" % (name, 100 * share, worst_noise, worst_ratio, min(med), top))


# -------------------------------------------------------------------------------------------------------------------------------------------------------
# The clip arithmetic of tests/test_gpu_generic_update.py, held on the C oracle alone
# -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_grad_norm", [None, 1e30], ids=["the shape's max_grad_norm", "1e30"])
@pytest.mark.parametrize("name", list(G.SHAPES))
def test_clip_scale_reproduces_the_c_oracles_clipped_gradient(name, max_grad_norm):
    """grad_oracle.clip_scale, fed the C oracle's own total norm as an f32 number, gives orc_clip_grad_norm's scaled gradient bit for bit: the GPU test feeds it
    the device's published norm instead and hands the result to the C oracle's AdamW, so its arithmetic is pinned here before any kernel runs.  Also at a
    max_grad_norm below the total (0.37 of it), so that every shape walks the c < 1 side whatever its gradient's size."""
    s = G.SHAPES[name]
    max_grad_norm = G.shape_hp(s)["max_grad_norm"] if max_grad_norm is None else max_grad_norm
    b = stand_in_batch(s)
    idx = G.index_lists(s, b["d_logp"], b["d_values"])[0]
    g = O.minibatch_grads(*_oracle_args(s, b, idx, s["dtype"]))[0]
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    _, total = O.clip_grad_norm(b["net"], g, 1.0)
    assert float(np.float32(total)) == total           # the oracle returns its f32 total, widened
    assert abs(total - G.clipped_norm(g, b["shapes"])) <= 2e-6 * total
    for mgn in (max_grad_norm, float(np.float32(0.37) * np.float32(total))):
        gc, total_again = O.clip_grad_norm(b["net"], g, mgn)
        mine, c = G.clip_scale(g, np.float32(total), mgn)
        print("%-70s max_grad_norm %-12g total %.6f c %.8f" % (name, mgn, total, c))
        assert total_again == total and mine.dtype == np.float32 and c.dtype == np.float32
        assert (c == 1.0) == (mgn >= total + 1e-6), (name, mgn, total, c)
        assert np.array_equal(mine.view(np.uint32), gc.view(np.uint32)), (name, mgn, int((mine.view(np.uint32) != gc.view(np.uint32)).sum()))
    assert G.clip_scale(g, np.float32(total), 1e30)[1] == 1.0
