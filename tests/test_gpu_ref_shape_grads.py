"""The 2 x 64 kernels (fwd_bwd_kernel, fwd_bwd_mfma_kernel, fwd_bwd_mfma_ws_kernel, pack_records_kernel, policy_act_kernel, values_kernel) at every kind of
head list a caller-stepped context accepts, against float64 -- tensor by tensor, at a step that is off the ratio = 1 point.

The reference fixtures hold these kernels at (2,) plain and (3,) masked only, by the flat gradient and next to ratio = 1.  grad_oracle.REF_SHAPES has one row
per dispatch case of api.hip (fwd_bwd, launch_minibatch_fwd_bwd_mfma, launch_minibatch_fwd_bwd, launch_policy_act):

  obs 4 (2,) / obs 2 (3,) masked               flags 0: fwd_bwd_mfma_ws_kernel; ONE_WAVE: fwd_bwd_mfma_kernel<.., EXACT = true>; VECTOR: fwd_bwd_kernel
  obs 4 (4,), (3,) / obs 2 (3,)                fwd_bwd_mfma_kernel<CAT, 4 or 2, 4, false>; the (3,) at obs 4 with clip_vloss and norm_adv off
  obs 4 (2,2) m., (2,) m. / obs 2 (2,1,1) m.   fwd_bwd_mfma_kernel<MASKED, 4 or 2, 4, false>; several heads' action and mask bits in pack_records_kernel; heads of width 1
  obs 4 (3,2) / obs 2 (3,3,3,2) m.             more than 4 logits: fwd_bwd_kernel<DIST, OBS> with several heads
  obs 8 (4,), eight heads of 4 m., (2,) m.     fwd_bwd_kernel<DIST, 8>, values_kernel<8>, policy_act_kernel<.., 8, 4 or 32>; 8 heads / 32 logits is the ABI's maximum

Every context is a PPO_ENV_HOST one (it has no env of its own): the batch is grad_oracle.stand_in_batch, written with ctx.write.  Lists of 576, 225, 33 and 2
rows: whole 32-row tiles, a one-row last tile, a tile plus a row, fewer rows than a tile.

Which kernel ran: the binding reports ppo_profile.vector_fallback_launches (asserted 0: no launch left the matrix cores for the fp16 range) and nothing else
about the choice, so where the matrix-core kernel is expected its gradient is also required to differ in some bit from the same step under
PPO_KERNEL_UPDATE_VECTOR (two-term fp16 products against plain f32 multiply-adds cannot agree on ~9 000 sums; a silent vector launch would be bit-identical).

Bars (the suite's, none of them from these kernels' own output): forward rtol 1e-5 / atol 3e-6 and 99.5 % sampled actions (test_multihead_masked_agent, TOL f32);
scalars 1e-5, total_norm 1e-5, flat gradient 5e-6 of its largest element (test_minibatch_step_matches_reference); per tensor min(1e-4, K_REF max(d_ref, 1e-7))
(grad_oracle.ref_tensor_bars; K_REF and the measured table: DESIGN.md, "Per-tensor gradient checks"); flags against each other 5e-6 per tensor
(test_update_kernels_agree_on_awkward_minibatch_sizes' bar, per tensor); AdamW moments rtol 1e-5 / 2e-5 and parameters 1e-6 given the library's own gradient
(_check_shape), parameters of the oracle's own chain 1e-6 after step 1 and 2e-6 after step 3, a whole update 2e-6 (test_full_update_tracks_reference).
"""
import functools

import numpy as np
import pytest

import grad_oracle as G
import oracle as O
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

FWD = dict(rtol=1e-5, atol=3e-6)
AGREE = 0.995
FLAT_BAR = 5e-6
FLAGS_BAR = 5e-6
FLAG_NAME = {0: "default", G.ONE_WAVE: "one wave", G.VECTOR: "vector"}
STAT_KEYS = (("pg_loss", "pg_loss"), ("v_loss", "v_loss"), ("entropy_loss", "entropy_loss"), ("approx_kl", "approx_kl"), ("clipfrac_last", "clipfrac"), ("loss", "loss"))
UPDATE_SHAPES = ["ref obs4 (2,2) masked", "ref obs4 (3,2)", "ref obs8 eight heads of 4 masked"]


@pytest.fixture(scope="module")
def P():
    return load_package()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def batch(name):
    """the shape's stand-in batch and index lists, made once and shared (nothing writes to them)"""
    s = G.REF_SHAPES[name]
    b = G.stand_in_batch(s)
    b["lists"] = G.ref_index_lists(s, b)
    for v in b.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def oracle_step(name, k):
    """list k of the shape in both oracles: (float64 gradient, its scalars, per-row arrays), (C oracle's f32 gradient, its scalars)"""
    s, b = G.REF_SHAPES[name], batch(name)
    hp = G.shape_hp(s)
    rows = {}
    idx = b["lists"][k]
    g64, s64 = G.minibatch_grads(b["shapes"], s["heads"], s["masked"], hp, b["params"], b["obs"], b["actions"], b["logp"], b["adv"], b["ret"], b["values"], idx, b["masks"],
                                 rows=rows)
    gc, sc = O.minibatch_grads(b["net"], _hparams(s), b["params"], b["obs"], b["actions"].astype(np.float32), b["logp"], b["adv"], b["ret"], b["values"],
                               idx.astype(np.int64), b["masks"])
    return (g64, s64, rows), (gc, sc)


def _hparams(s):
    hp = G.shape_hp(s)
    return O.HParams(norm_adv=int(hp["norm_adv"]), clip_vloss=int(hp["clip_vloss"]), **G.BASE_HP)


def expects_matrix_cores(s, flags):
    """api.hip, ppo_ctx_create: the matrix-core update kernels take up to 4 logits at observation widths 2 and 4, unless PPO_KERNEL_UPDATE_VECTOR"""
    return sum(s["heads"]) <= 4 and s["obs"] in (2, 4) and not flags & G.VECTOR


def context(P, name, flags=0, epochs=1):
    """a caller-stepped context of the shape with the stand-in batch in its rollout buffers and the stand-in parameters"""
    s, b = G.REF_SHAPES[name], batch(name)
    ctx = P.Context(P.make_config(env_kind=P.ENV_HOST, dist_kind=P.DIST_MASKED if s["masked"] else P.DIST_CATEGORICAL, obs_size=s["obs"], head_dims=tuple(s["heads"]),
                                  hidden=s["hidden"], n_hidden=s["n_hidden"], num_envs=G.N_ENVS, num_steps=G.N_STEPS, num_minibatches=2, update_epochs=epochs,
                                  seed=s["seed"], total_timesteps=8 * G.N_ENVS * G.N_STEPS, learning_rate=1e-3, anneal_lr=False, compute_dtype=0, kernel_flags=flags,
                                  **G.shape_hp(s)))
    assert ctx.P == b["params"].size == O.param_count(b["net"])
    ctx.write("OBS", b["obs"])
    ctx.write("ACTIONS", b["actions"].astype(np.int32))
    if s["masked"]:
        ctx.write("MASKS", b["masks"].astype(np.uint8))
    ctx.write("LOGPROBS", b["logp"])
    ctx.write("VALUES", b["values"])
    ctx.write("ADVANTAGES", b["adv"])
    ctx.write("RETURNS", b["ret"])
    ctx.set_params(b["params"])
    ctx.set_learning_rate(1e-3)
    return ctx


def worst_elements(g, g_ref, shp, t):
    """where a tensor's largest differences sit: (row, column, got, reference) of the five worst elements"""
    a = [v for *_, v in G.split(np.asarray(g, np.float64), shp)][t]
    r = [v for *_, v in G.split(np.asarray(g_ref, np.float64), shp)][t]
    err = np.abs(a - r) / np.abs(r).max()
    order = np.argsort(err.ravel())[::-1][:5]
    return [(int(k // a.shape[1]), int(k % a.shape[1]), float(a.ravel()[k]), float(r.ravel()[k])) for k in order]


def head_offsets(heads):
    return np.concatenate([[0], np.cumsum(heads)[:-1]]).astype(np.int64)


@pytest.mark.parametrize("name", list(G.REF_SHAPES))
def test_forward_against_the_oracle(P, name):
    """ppo_policy_act teacher-forced and sampling, ppo_get_value: 256 rows against the C oracle's forward"""
    s, b = G.REF_SHAPES[name], batch(name)
    ctx = context(P, name)
    n = 256
    obs, acts, mask = b["obs"][:n], b["actions"][:n], (b["masks"][:n] if s["masked"] else None)
    lp_o, en_o, v_o = O.evaluate(b["net"], b["params"], obs, acts, mask)
    a, lp, en, v = ctx.policy_act(obs, mask=mask, action=acts)
    print("FWD %-55s logp %.2e entropy %.2e value %.2e" % (name, np.abs(lp - lp_o).max(), np.abs(en - en_o).max(), np.abs(v - v_o).max()))
    assert np.array_equal(a, acts)
    np.testing.assert_allclose(lp, lp_o, **FWD)
    np.testing.assert_allclose(en, en_o, **FWD)
    np.testing.assert_allclose(v, v_o, **FWD)
    np.testing.assert_allclose(ctx.get_value(obs), O.get_value(b["net"], b["params"], obs), **FWD)
    sa, slp, _, _ = ctx.policy_act(obs, mask=mask, step_index=3)
    oa, _, _, _ = O.act(b["net"], b["params"], obs, s["seed"], 3, 0, mask)
    agree = float((sa == oa).all(axis=1).mean())
    print("FWD %-55s sampled actions agree on %.4f of rows" % (name, agree))
    assert agree >= AGREE
    assert np.isfinite(slp).all()
    assert (sa >= 0).all() and (sa < np.asarray(s["heads"])[None, :]).all()
    if s["masked"]:
        assert np.take_along_axis(mask, sa + head_offsets(s["heads"])[None, :], axis=1).all()
    assert ctx.profile_read()["vector_fallback_launches"] == 0
    ctx.close()


@pytest.mark.parametrize("name", list(G.REF_SHAPES))
def test_minibatch_step_per_tensor_against_float64(P, name):
    s, b = G.REF_SHAPES[name], batch(name)
    shp = b["shapes"]
    bad, got = [], {}
    for flags in s["flags"]:
        ctx = context(P, name, flags)
        tag = "%s [%s]" % (name, FLAG_NAME[flags])
        worst_d, worst_ratio = 0.0, 0.0
        for k, idx in enumerate(b["lists"]):
            M = idx.size
            grads = ctx.minibatch_forward_backward(idx)
            st = ctx.stats()
            got[flags, k] = grads
            (g64, s64, rows), (gc, sc) = oracle_step(name, k)
            # the preconditions of tests/test_gpu_generic_grads.py: every tensor carries a gradient, both sides of both clips are populated
            for _, net_i, layer, kind, v in G.split(g64, shp):
                assert np.abs(v).max() > 0, (name, M, G.tensor_name(net_i, layer, kind))
            if M >= 40:
                assert 0.2 <= s64["clipfrac"] <= 0.8, (name, M, s64["clipfrac"])
                assert 0.2 <= float((np.abs(rows["dv"]) > G.BASE_HP["clip_coef"]).mean()) <= 0.8, (name, M)
                assert (rows["l1"] > rows["l2"]).any() and (rows["l1"] < rows["l2"]).any(), (name, M)
                if s["masked"]:
                    assert G.single_action_rows(b["masks"][idx], s["heads"]) >= 0.01, (name, M)
            assert np.isfinite(grads).all(), (tag, M)
            d_ref, d_hip = G.tensor_distance(gc, g64, shp), G.tensor_distance(grads, g64, shp)
            for (t, net_i, layer, kind, v), dr, dh, bar in zip(G.split(g64, shp), d_ref, d_hip, G.ref_tensor_bars(d_ref)):
                print("REF %-68s M=%3d %-12s max|g| %.2e d_ref %.2e d_hip %.2e ratio %6.2f bar %.1e" %
                      (tag, M, G.tensor_name(net_i, layer, kind), np.abs(v).max(), dr, dh, dh / max(dr, 1e-7), bar))
                worst_d, worst_ratio = max(worst_d, float(dh)), max(worst_ratio, float(dh / max(dr, 1e-7)))
                if not dh <= bar:
                    bad.append((tag, M, G.tensor_name(net_i, layer, kind), float(dh), float(dr), float(bar)))
                    print("REF   worst (row, col, hip, float64):", worst_elements(grads, g64, shp, t))
            flat = float(np.abs(grads - g64).max() / np.abs(g64).max())
            print("REF %-68s M=%3d flat gradient %.2e of its largest element" % (tag, M, flat))
            if not flat <= FLAT_BAR:
                bad.append((tag, M, "flat gradient", flat))
            for key, okey in STAT_KEYS:
                print("REF %-68s M=%3d %-13s hip %.8e float64 %.8e" % (tag, M, okey, st[key], s64[okey]))
                bar = 1e-5 * max(1.0, abs(s64[okey])) + (1.0 / M if okey == "clipfrac" else 0.0)   # clipfrac is a count: one row on a clip's edge may fall either way
                if not abs(st[key] - s64[okey]) <= bar:
                    bad.append((tag, M, okey, st[key], s64[okey]))
            total = G.clipped_norm(g64, shp)
            print("REF %-68s M=%3d total_norm    hip %.8e float64 %.8e" % (tag, M, st["total_norm"], total))
            if not abs(st["total_norm"] - total) <= 1e-5 * total:
                bad.append((tag, M, "total_norm", st["total_norm"], total))
        print("REF_MEASURED %-68s worst d_hip %.1e worst d_hip / d_ref %.2f" % (tag, worst_d, worst_ratio))
        if ctx.profile_read()["vector_fallback_launches"] != 0:
            bad.append((tag, "a launch fell back to the vector kernel for the fp16 range"))
        ctx.close()
    # the flags against each other, per tensor; the plain-f32 vector kernel is the yardstick
    if len(s["flags"]) > 1:
        for k, idx in enumerate(b["lists"]):
            for flags in s["flags"]:
                if flags == G.VECTOR:
                    continue
                d = G.tensor_distance(got[flags, k], got[G.VECTOR, k], shp)
                print("REF %-55s M=%3d %-8s against vector, per tensor: %s" % (name, idx.size, FLAG_NAME[flags], " ".join("%.1e" % x for x in d)))
                if not (d <= FLAGS_BAR).all():
                    bad.append((name, idx.size, FLAG_NAME[flags], "against vector", [float(x) for x in d]))
    # which kernel ran: a matrix-core step cannot be the vector kernel's bits
    if expects_matrix_cores(s, 0):
        if G.VECTOR in s["flags"]:
            g_vec = got[G.VECTOR, 0]
        else:
            ctx = context(P, name, G.VECTOR)
            g_vec = ctx.minibatch_forward_backward(b["lists"][0])
            ctx.close()
        for flags in s["flags"]:
            if expects_matrix_cores(s, flags) and np.array_equal(bits(got[flags, 0]), bits(g_vec)):
                bad.append((name, FLAG_NAME[flags], "bit-identical to the vector kernel's gradient: the matrix-core kernel did not run"))
    assert not bad, bad


@pytest.mark.parametrize("name", list(G.REF_SHAPES))
def test_three_optimizer_steps_on_these_parameter_counts(P, name):
    """P differs per head list (the tails of grad_norm_kernel and clip_adamw_kernel).  Three ppo_minibatch_forward_backward + ppo_optimizer_step rounds on the
    576-row list.  Each step alone: the C oracle's clip_grad_norm + AdamW applied to the library's own gradient and state (moments rtol 1e-5 / 2e-5, parameters
    1e-6, total_norm 2e-6: _check_shape's bars).  And the oracle's own chain from its own gradients: parameters within 1e-6 after step 1 and 2e-6 after step 3,
    moments within 5e-6 / 1e-5 of their largest element (test_minibatch_step_matches_reference's bars for moments that inherit another gradient's rounding:
    element by element, a small element carries the absolute error of the gradient's largest terms -- the two CPU oracles miss rtol 1e-5 against each other)."""
    s, b = G.REF_SHAPES[name], batch(name)
    idx = b["lists"][0]
    assert idx.size == 576
    ctx = context(P, name)
    net, hpo = b["net"], _hparams(s)
    act_f = b["actions"].astype(np.float32)
    p_o, m_o, v_o = b["params"].copy(), np.zeros_like(b["params"]), np.zeros_like(b["params"])
    for k in (1, 2, 3):
        p_l, (m_l, v_l, _) = ctx.get_params(), ctx.get_optimizer()
        grads = ctx.minibatch_forward_backward(idx)
        ctx.optimizer_step()
        m, v, step = ctx.get_optimizer()
        p = ctx.get_params()
        assert step == k
        # the step alone
        gc, total = O.clip_grad_norm(net, grads, G.BASE_HP["max_grad_norm"])
        assert abs(ctx.stats()["total_norm"] - float(total)) <= 2e-6 * float(total), (name, k)
        p1, m1, v1 = O.adamw_step(p_l, gc, m_l, v_l, 1e-3, k)
        np.testing.assert_allclose(m, m1, rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(v, v1, rtol=2e-5, atol=1e-18)
        np.testing.assert_allclose(p, p1, rtol=0, atol=1e-6)
        # the oracle's own chain
        g_o, _ = O.minibatch_grads(net, hpo, p_o, b["obs"], act_f, b["logp"], b["adv"], b["ret"], b["values"], idx.astype(np.int64), b["masks"])
        g_o, _ = O.clip_grad_norm(net, g_o, G.BASE_HP["max_grad_norm"])
        p_o, m_o, v_o = O.adamw_step(p_o, g_o, m_o, v_o, 1e-3, k)
        dm, dv, dp = np.abs(m - m_o).max() / np.abs(m_o).max(), np.abs(v - v_o).max() / np.abs(v_o).max(), np.abs(p - p_o).max()
        print("OPT %-55s step %d  m %.2e v %.2e of their largest element, parameters %.2e" % (name, k, dm, dv, dp))
        assert dm <= 5e-6 and dv <= 1e-5, (name, k, dm, dv)
        assert dp <= (1e-6 if k == 1 else 2e-6), (name, k, dp)
    assert ctx.profile_read()["vector_fallback_launches"] == 0
    ctx.close()


@pytest.mark.parametrize("name", UPDATE_SHAPES)
def test_whole_update_equals_the_stepwise_path_and_tracks_the_oracle(P, name):
    """ppo_update on a caller-stepped context whose buffers hold the stand-in batch (two epochs x two minibatches, its own permutations) == a second context
    stepped one minibatch at a time on those permutations, bit for bit; the C oracle driven on them ends within 2e-6."""
    s, b = G.REF_SHAPES[name], batch(name)
    E, B = 2, G.N_ENVS * G.N_STEPS
    MB = B // 2
    ctx = context(P, name, epochs=E)
    ctx.update()
    p_fused = ctx.get_params()
    perm = ctx.read("PERM", (E, B))
    for e in range(E):
        assert np.array_equal(np.sort(perm[e]), np.arange(B))
    assert not np.array_equal(perm[0], perm[1]) and not np.array_equal(perm[0], np.arange(B))
    st = ctx.stats()
    assert st["optimizer_steps"] == 2 * E and np.isfinite(st["loss"])
    assert abs(st["explained_variance"] - O.explained_variance(b["ret"], b["values"])) <= 1e-5
    ctx2 = context(P, name, epochs=E)
    for e in range(E):
        for k in range(2):
            ctx2.minibatch_forward_backward(perm[e, k * MB:(k + 1) * MB])
            ctx2.optimizer_step()
    assert np.array_equal(bits(p_fused), bits(ctx2.get_params()))
    net, hpo = b["net"], _hparams(s)
    p, step = b["params"].copy(), 0
    m, v = np.zeros_like(p), np.zeros_like(p)
    for e in range(E):
        for k in range(2):
            g, _ = O.minibatch_grads(net, hpo, p, b["obs"], b["actions"].astype(np.float32), b["logp"], b["adv"], b["ret"], b["values"],
                                     perm[e, k * MB:(k + 1) * MB].astype(np.int64), b["masks"])
            g, _ = O.clip_grad_norm(net, g, G.BASE_HP["max_grad_norm"])
            step += 1
            p, m, v = O.adamw_step(p, g, m, v, 1e-3, step)
    print("UPD %-55s parameters %.2e from the oracle's after %d steps" % (name, np.abs(p - p_fused).max(), step))
    assert np.abs(p - p_fused).max() <= 2e-6
    assert not np.array_equal(bits(p_fused), bits(b["params"]))
    for c in (ctx, ctx2):
        assert c.profile_read()["vector_fallback_launches"] == 0
        c.close()
