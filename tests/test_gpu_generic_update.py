"""The generic engine inside ppo_update: a whole update against its own step-by-step replay, bit for bit, and every optimizer step against the C oracle.

Inside ppo_update the generic engine runs on state that is derived once and then kept up incrementally ("Derived state of the generic engine"):
the bf16 weight planes and their fragment-order copy (rewritten element by element behind every optimizer step by gen_opt_fused_kernel), the update's rounded
observations and packed rows (obs_bf / row_rec, made once per update), the next step's rows gathered ahead on the second stream, the gradient norm taken from
the slab sums' partial sums of squares.  A step driven from Python never reads any of it: every ppo_memcpy_h2d -- the upload of the step's index list is one --
marks the planes dirty and drops the partial sums, a stand-alone step rounds and packs its own rows, and nothing is gathered ahead outside ppo_update.  So the
stepwise path is the yardstick here: the same kernels, fed by state that was just built whole.  DO NOT "optimise" the replay loops below (one upload per step,
get_params between steps): the blanket invalidation by the upload is what makes them a reference.

Shapes: the twelve of grad_oracle.SHAPES (what each reaches in the forward and backward passes: tests/test_gpu_generic_grads.py), on 48 envs x 24 steps, four
minibatches of 288 rows (four 64-row tiles and a 32-row one), two epochs: eight optimizer steps per update.  LOGPROBS and VALUES are perturbed
(grad_oracle.make_off_policy) before the first update, so step 1 is already off ratio = 1.

Which optimizer kernels a context runs (api.hip: gen_fwd_bwd sets gen_opt_fused_ok = not CLASSIC and both nets' backward passes left sq_part, i.e.
gen_fused_backward_ok; clip_adamw_any dispatches on it), and which step form (in place on obs_bf / row_rec, or gathered copies with gather-ahead on stream2):

  f32, all four shapes                                  gen_norm_kernel + gen_adamw_kernel; one stream, gathered rows, planes (three bf16 terms) rebuilt whole
  bf16 obs120 h48x2, obs132 h160x3, obs376 h256x4,
       obs24 h64x2 (both), obs120 h128x1                gen_opt_fused_kernel (norm from sq_part, planes and frags rewritten per element); in place, no gather
  bf16 obs130 h160x3 (obs % 4 != 0)                     gen_opt_fused_kernel (fused backward, one net per launch); gathered rows, GATHER-AHEAD
  bf16 obs24 h257x2 (ld_h = 384)                        gen_norm_kernel + gen_adamw_kernel (product-kernel backward leaves no sq_part); gathered rows, GATHER-AHEAD
  any bf16 shape under PPO_KERNEL_GENERIC_CLASSIC       gen_norm_kernel + gen_adamw_kernel; gathered rows, GATHER-AHEAD, planes rebuilt whole after every step

Bars.  Test 1: bit equality -- both sides run the same kernels on the same operand values with the same partition of every partial sum.  Test 2: moments
bit-identical (exactly rounded multiplications and fused multiply-adds only); parameters bit-identical expected (-ffp-contract=off, -fno-fast-math, HIP's f32
divide and sqrt correctly rounded), and never beyond the suite's bar for AdamW against a reference (test_adamw_bit_exact_given_reference_gradient: 4 ULP, on
at most 2e-3 of the elements); total_norm within 2e-6 of the float64 norm of the returned gradient (the suite's bar).  Measured: DESIGN.md, same section.
"""
import numpy as np
import pytest

import grad_oracle as G
import oracle as O
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

E, NMB = 2, 4
STEPS = E * NMB
B = G.N_ENVS * G.N_STEPS
MB = B // NMB
LR = 1e-3
NO_CLIP = 1e30
ROLLOUT_BUFS = ("OBS", "ACTIONS", "MASKS", "LOGPROBS", "VALUES", "ADVANTAGES", "RETURNS", "REWARDS", "DONES")
STAT_KEYS = ("pg_loss", "v_loss", "entropy_loss", "approx_kl", "clipfrac_last", "loss", "total_norm")
CLASSIC = 16   # PPO_KERNEL_GENERIC_CLASSIC (include/ppo_hip.h), asserted against the binding's constant in the fixture

CASES = [(n, 0) for n in G.SHAPES] + [(n, CLASSIC) for n, s in G.SHAPES.items() if s["dtype"] == 1]
CASE_IDS = ["%s%s" % (n, " [classic]" if f else "") for n, f in CASES]


@pytest.fixture(scope="module")
def P():
    pkg = load_package()
    assert pkg.KERNEL_GENERIC_CLASSIC == CLASSIC
    return pkg


_params = {}


def start_params(P, name):
    """grad_oracle.make_params of the shape, made once for the file and never written to"""
    if name not in _params:
        _params[name] = G.make_params(P, G.SHAPES[name])
        _params[name].setflags(write=False)
    return _params[name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def ulp_distance(a, b):
    """per element: how many f32 numbers lie between a and b (0 = the same bits, up to the sign of zero)"""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def where_they_differ(tag, a, b, shp):
    """per tensor: how many elements differ and by how much (printed when a bit comparison fails, for the trace)"""
    for (_, net_i, layer, kind, va), (_, _, _, _, vb) in zip(G.split(np.asarray(a), shp), G.split(np.asarray(b), shp)):
        n = int((va.view(np.uint32) != vb.view(np.uint32)).sum())
        if n:
            print("DIFF %s %-12s %d of %d elements, max |a - b| %.3e (max |b| %.3e), max ULP %d" %
                  (tag, G.tensor_name(net_i, layer, kind), n, va.size, np.abs(va.astype(np.float64) - vb).max(), np.abs(vb).max(), ulp_distance(va, vb).max()))


def context(P, name, flags, max_grad_norm=None):
    s = G.SHAPES[name]
    over = {} if max_grad_norm is None else dict(max_grad_norm=max_grad_norm)
    ctx = G.context(P, s, flags, num_minibatches=NMB, update_epochs=E, **over)
    assert ctx.B == B and ctx.P == start_params(P, name).size
    return ctx


def rolled_out(P, name, flags, max_grad_norm=None):
    """a context after set_params / env_reset / rollout / calc_advantage: (context, its rollout buffers as read back)"""
    ctx = context(P, name, flags, max_grad_norm)
    ctx.set_params(start_params(P, name))
    ctx.env_reset()
    ctx.rollout()
    ctx.calc_advantage()
    return ctx, {n: ctx.read(n) for n in ROLLOUT_BUFS}


def go_off_policy(ctx, bufs, seed):
    """LOGPROBS / VALUES replaced by their perturbed copies, in the context and in bufs"""
    bufs["LOGPROBS"], bufs["VALUES"] = G.make_off_policy(np.random.default_rng(seed + 1), bufs["LOGPROBS"], bufs["VALUES"])
    ctx.write("LOGPROBS", bufs["LOGPROBS"])
    ctx.write("VALUES", bufs["VALUES"])


def state(ctx):
    m, v, step = ctx.get_optimizer()
    return dict(params=ctx.get_params(), exp_avg=m, exp_avg_sq=v, step=step)


def replay(ctx, perm):
    """the update's steps one at a time on its permutations.  Every step uploads its index list: the planes are rebuilt whole, the step's rows are rounded and
    packed again, nothing is gathered ahead -- that is the point (module docstring)."""
    for e in range(E):
        for k in range(NMB):
            ctx.minibatch_forward_backward(perm[e, k * MB:(k + 1) * MB])
            ctx.optimizer_step()


def check_perm(perm):
    for e in range(E):
        assert np.array_equal(np.sort(perm[e]), np.arange(B)), e
    assert not np.array_equal(perm[0], perm[1]) and not np.array_equal(perm[0], np.arange(B))


@pytest.mark.parametrize("name,flags", CASES, ids=CASE_IDS)
def test_whole_update_equals_its_stepwise_replay(P, name, flags):
    """ppo_update (context X: planes and fragments kept up per element behind each step, obs_bf / row_rec made once, rows gathered ahead) == the same eight
    steps one at a time on X's permutations (context Y: everything derived is rebuilt whole before each step, see replay), bit for bit: parameters, both
    moments, the last step's scalars.  Then the rollout that follows (X reads the planes and fragments its update left, Y freshly built ones), and a second
    update (a stale obs_bf / row_rec or a gather claim that survived the first one shows here)."""
    s = G.SHAPES[name]
    shp = O.param_shapes(O.Net.make(s["obs"], list(s["heads"]), hidden=s["hidden"], n_hidden=s["n_hidden"]))
    p0 = start_params(P, name)
    # 1. X: the whole update
    X, bufs = rolled_out(P, name, flags)
    own = dict(bufs)
    go_off_policy(X, bufs, s["seed"])
    X.set_learning_rate(LR)
    X.update()
    perm = X.read("PERM", (E, B))
    sx, stx = state(X), X.stats()
    check_perm(perm)
    assert stx["optimizer_steps"] == STEPS == sx["step"]
    assert np.isfinite(sx["params"]).all() and not same_bits(sx["params"], p0)
    moved = float(np.abs(sx["params"].astype(np.float64) - p0).max())
    print("UPD %-55s flags %2d parameters moved by up to %.2e in %d steps, last total_norm %.4f" % (name, flags, moved, STEPS, stx["total_norm"]))
    # 2. Y: at the same point with X's buffers verbatim, then the replay
    Y, bufs_y = rolled_out(P, name, flags)
    for n in ROLLOUT_BUFS:
        assert same_bits(bufs_y[n], own[n]), n
        if bufs[n].size:
            Y.write(n, bufs[n])
    Y.set_learning_rate(LR)
    replay(Y, perm)
    sy, sty = state(Y), Y.stats()
    # 3. bit equality
    bad = []
    for key in ("params", "exp_avg", "exp_avg_sq"):
        if not same_bits(sx[key], sy[key]):
            where_they_differ("%s update 1 %s" % (name, key), sx[key], sy[key], shp)
            bad.append(("update 1", key, int((sx[key].view(np.uint32) != sy[key].view(np.uint32)).sum())))
    assert sy["step"] == STEPS
    for key in STAT_KEYS:
        if not stx[key] == sty[key]:
            bad.append(("update 1", key, stx[key], sty[key]))
    assert not bad, bad
    # 4. the planes and fragments the rollout reads: X's were written element by element over eight steps, Y's are rebuilt whole
    Y.set_params(Y.get_params())
    for c in (X, Y):
        c.rollout()
        c.calc_advantage()
    for n in ("OBS", "MASKS", "ACTIONS", "LOGPROBS", "VALUES", "NEXT_VALUE", "ADVANTAGES", "RETURNS"):
        a, b = X.read(n), Y.read(n)
        if not same_bits(a, b):
            bad.append(("rollout after update 1", n, int((a != b).sum()), a.size))
    assert not bad, bad
    # 5. the second update
    X.update()
    perm2 = X.read("PERM", (E, B))
    check_perm(perm2)
    assert not np.array_equal(perm2, perm)
    replay(Y, perm2)
    sx, sy = state(X), state(Y)
    assert sx["step"] == sy["step"] == 2 * STEPS
    for key in ("params", "exp_avg", "exp_avg_sq"):
        if not same_bits(sx[key], sy[key]):
            where_they_differ("%s update 2 %s" % (name, key), sx[key], sy[key], shp)
            bad.append(("update 2", key, int((sx[key].view(np.uint32) != sy[key].view(np.uint32)).sum())))
    X.close()
    Y.close()
    assert not bad, bad


@pytest.mark.parametrize("max_grad_norm", [None, NO_CLIP], ids=["clip at the shape's max_grad_norm", "clip coefficient 1"])
@pytest.mark.parametrize("name,flags", CASES, ids=CASE_IDS)
def test_each_optimizer_step_against_the_c_oracle(P, name, flags, max_grad_norm):
    """Eight stand-alone steps (two epochs of four 288-row minibatches).  Each step alone: the library's own gradient, scaled by the clip coefficient formed in
    float32 from the library's own published norm (grad_oracle.clip_scale), through the C oracle's AdamW from the library's own parameters and moments before
    the step.  Steps 2 .. 8 carry non-zero moments and bias corrections of k > 1."""
    s = G.SHAPES[name]
    mgn = G.shape_hp(s)["max_grad_norm"] if max_grad_norm is None else max_grad_norm
    shp = O.param_shapes(O.Net.make(s["obs"], list(s["heads"]), hidden=s["hidden"], n_hidden=s["n_hidden"]))
    ctx, bufs = rolled_out(P, name, flags, max_grad_norm)
    go_off_policy(ctx, bufs, s["seed"])
    ctx.set_learning_rate(LR)
    rng = np.random.default_rng(2000 + s["seed"])
    bad, hist, totals, coefs = [], np.zeros(6, np.int64), [], []
    k = 0
    for e in range(E):
        perm = rng.permutation(B).astype(np.int32)
        for mb in range(NMB):
            k += 1
            before = state(ctx)
            g = ctx.minibatch_forward_backward(perm[mb * MB:(mb + 1) * MB])
            total = ctx.stats()["total_norm"]
            held = state(ctx)
            ctx.optimizer_step()
            after = state(ctx)
            assert before["step"] == held["step"] == k - 1 and after["step"] == k
            assert all(same_bits(before[key], held[key]) for key in ("params", "exp_avg", "exp_avg_sq")), (name, k)   # the backward pass touches none of them
            assert ctx.stats()["total_norm"] == total and float(np.float32(total)) == total    # one f32 number, published twice
            assert np.isfinite(g).all() and np.isfinite(total)
            total64 = G.clipped_norm(g, shp)
            if not abs(total - total64) <= 2e-6 * total64:
                bad.append((k, "total_norm", total, total64))
            g_c, c = G.clip_scale(g, total, mgn)
            totals.append(total)
            coefs.append(float(c))
            p1, m1, v1 = O.adamw_step(before["params"], g_c, before["exp_avg"], before["exp_avg_sq"], LR, k)
            for key, ref in (("exp_avg", m1), ("exp_avg_sq", v1)):
                if not same_bits(after[key], ref):
                    where_they_differ("%s step %d %s" % (name, k, key), after[key], ref, shp)
                    bad.append((k, key, int((after[key].view(np.uint32) != ref.view(np.uint32)).sum())))
            ulp = ulp_distance(after["params"], p1)
            hist += np.bincount(np.minimum(ulp, 5), minlength=6)
            print("OPT %-55s flags %2d max_grad_norm %-7g step %d total_norm %.6f c %.6f  parameters: %d of %d differ, max %d ULP" %
                  (name, flags, mgn, k, total, c, int((ulp != 0).sum()), ulp.size, int(ulp.max())))
            if not (ulp.max() <= 4 and (ulp != 0).mean() <= 2e-3):
                where_they_differ("%s step %d params" % (name, k), after["params"], p1, shp)
                bad.append((k, "params", int(ulp.max()), float((ulp != 0).mean())))
            assert (after["exp_avg"] != 0).any() and bool((before["exp_avg"] != 0).any()) == (k > 1)   # steps 2 .. 8 start from non-zero moments
    print("ULP %-55s flags %2d max_grad_norm %-7g parameters over %d steps, elements at 0 / 1 / 2 / 3 / 4 / 5+ ULP: %s" % (name, flags, mgn, STEPS, " / ".join(map(str, hist))))
    ctx.close()
    if max_grad_norm is None:
        if not max(totals) > mgn:
            bad.append(("no step clips: the largest total_norm is %.4f against max_grad_norm %g" % (max(totals), mgn),))
    elif not all(c == 1.0 for c in coefs):
        bad.append(("a coefficient below 1 under max_grad_norm 1e30", coefs))
    assert not bad, bad


@pytest.mark.parametrize("name", ["bf16 obs132 h160x3 (3,3,3,2) masked", "f32 obs20 h160x2 (2,3) masked"])
def test_a_backward_pass_without_a_step_leaves_everything_alone(P, name):
    """ppo_minibatch_forward_backward runs the optimizer launch with do_step = false (loss scalars and the norm only).  Twice on the same list: the same
    gradient bits, parameters, moments and the step count untouched; the optimizer step that follows equals that of a context that ran the pass once."""
    s = G.SHAPES[name]
    idx = np.random.default_rng(3000 + s["seed"]).permutation(B)[:MB].astype(np.int32)
    got = []
    for passes in (1, 2):
        ctx, bufs = rolled_out(P, name, 0)
        go_off_policy(ctx, bufs, s["seed"])
        ctx.set_learning_rate(LR)
        s0 = state(ctx)
        grads = [ctx.minibatch_forward_backward(idx).copy() for _ in range(passes)]
        stats = ctx.stats()
        s1 = state(ctx)
        assert s1["step"] == s0["step"] == 0 and stats["optimizer_steps"] == 0
        for key in ("params", "exp_avg", "exp_avg_sq"):
            assert same_bits(s0[key], s1[key]), (name, passes, key)
        assert np.abs(grads[0]).max() > 0 and all(same_bits(grads[0], g) for g in grads), (name, passes)
        ctx.optimizer_step()
        s2 = state(ctx)
        assert s2["step"] == 1 and not same_bits(s2["params"], s1["params"])
        got.append((grads[0], s2, stats))
        ctx.close()
    (g1, a, st1), (g2, b, st2) = got
    assert same_bits(g1, g2)
    for key in STAT_KEYS:
        assert st1[key] == st2[key], key
    for key in ("params", "exp_avg", "exp_avg_sq"):
        assert same_bits(a[key], b[key]), (name, key)
