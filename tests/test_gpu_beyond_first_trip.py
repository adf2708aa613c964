"""The forward kernels past their grid caps: every launcher caps its grid, so above a row count a workgroup walks a second tile (and a third), through the
barrier that ends a trip, the rebuilt row list and the next tile's origin.  The rest of the suite stays under those caps.

Launcher (file)                                                        cap           rows per workgroup and trip
  gauss_fused_act / cat_fused_act / gauss_fused_values (kernels_gauss_fused.hip)   1024          64
  launch_policy_act, matrix-core form: policy_act16_kernel (kernels_rollout.hip)   4096          16
  launch_policy_act / launch_values, vector form (kernels_rollout.hip)             8192          1
  gen_fused_forward, bf16 storage (kernels_generic_fused.hip)                      256           64

Row counts: n = C R + R + 5 (workgroup 0 walks a whole second tile, workgroup 1 one of 5 rows; 8197 in the vector form, whose "tile" is one row) and, once per
family, n = 2 C R + 5 (a third trip that ends ragged).  Every test asserts from the cap that its n reaches the second trip.

No tolerance is new here.  Every comparison is either bit equality with launches that stay on the first trip (the same rows sent in pieces of at most C R
rows, which the files named below hold to the oracles), or the oracle at the bar the neighbouring test asserts: tests/test_gpu_cat_fused.py's FWD,
tests/test_gpu_gauss_fused.py's FWD_BAR, atol 3e-6 of tests/test_gpu_parity.py, TOL[1] of tests/test_gpu_generic.py.  The measured maximum is printed before
each such assertion."""
import functools

import numpy as np
import pytest

import cat_fused_shapes as S
import grad_oracle as G
import oracle as O
from __graft_entry__ import load_package
from test_gpu_cat_fused import FWD
from test_gpu_cat_fused import make_ctx as cat_ctx
from test_gpu_gauss_fused import FWD_BAR, fused_ctx, rel
from test_gpu_gaussian import gauss_entropy, gauss_logprob, mlp, nets, randomised_params, t64, tensor_shapes, unflatten
from test_gpu_generic import TOL

pytestmark = pytest.mark.gpu

# (workgroups at most, rows per workgroup and trip) as the launchers have them
FUSED_CAP = (1024, 64)      # kernels_gauss_fused.hip: std::min<int64_t>(tiles, 1024), tiles = ceil(n / 64)
ACT16_CAP = (4096, 16)      # kernels_rollout.hip, launch_policy_act: tiles < 4096 ? tiles : 4096, tiles = ceil(n / 16)
VECTOR_CAP = (8192, 1)      # kernels_rollout.hip, launch_policy_act / launch_values: n < 8192 ? n : 8192, one row per wave
GENERIC_CAP = (256, 64)     # kernels_generic_fused.hip, gen_fused_forward: n_tiles < 256 ? n_tiles : 256, n_tiles = ceil(rows / 64)
PARITY_ATOL = 3e-6          # tests/test_gpu_parity.py::test_policy_forward_teacher_forced


@pytest.fixture(scope="module")
def P():
    return load_package()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def pieces(n, cap):
    """[lo, hi) ranges of at most C R rows: each is a launch whose workgroups serve one tile"""
    first = cap[0] * cap[1]
    return [(lo, min(lo + first, n)) for lo in range(0, n, first)]


def assert_past_the_cap(n, cap):
    """n is one of the two row counts of this file for the launcher's cap, and workgroup 0 gets a second (third) tile"""
    C, R = cap
    tiles = (n + R - 1) // R
    assert tiles > C, (n, cap)                                  # more tiles than workgroups: workgroup 0 walks tile C after tile 0
    if n > 2 * C * R:
        assert n == 2 * C * R + 5 and tiles > 2 * C             # ... and tile 2 C: a third trip that ends ragged (5 rows)
    elif R > 1:
        assert n == C * R + R + 5 and tiles == C + 2            # tile C is whole, tile C + 1 (workgroup 1's second) has 5 rows
    else:
        assert n == C + 5
    assert all(hi - lo <= C * R for lo, hi in pieces(n, cap)) and len(pieces(n, cap)) >= 2


def in_pieces(call, n, cap, *arrays):
    """call(rows of every array) per piece; the outputs concatenated"""
    outs = [call(*(None if a is None else a[lo:hi] for a in arrays)) for lo, hi in pieces(n, cap)]
    if isinstance(outs[0], tuple):
        return tuple(np.concatenate([o[k] for o in outs]) for k in range(len(outs[0])))
    return np.concatenate(outs)


def assert_same_bits(tag, whole, parts, names):
    for name, w, p in zip(names, whole, parts):
        assert w.shape == p.shape, (tag, name)
        differ = bits(w) != bits(p)
        assert not differ.any(), (tag, name, int(differ.sum()), "first differing row %d" % int(np.argwhere(differ)[0][0]))


@functools.lru_cache(maxsize=None)
def _synthetic_rows(seed, obs_size, heads, n):
    envs = np.arange(n)
    obs = O.synthetic_obs(seed, envs, 0, obs_size)
    mask = O.synthetic_mask(seed, envs, 0, list(heads)) if heads else None
    for a in (obs, mask):
        if a is not None:
            a.setflags(write=False)
    return obs, mask


def synthetic_rows(seed, obs_size, heads, n, n_made=None):
    """O.synthetic_obs / O.synthetic_mask (heads given) of envs 0 .. n - 1 at step 0 -- tests/test_gpu_cat_fused.py::big_batch's recipe -- made once per shape
    for its largest n (n_made) and read-only"""
    obs, mask = _synthetic_rows(seed, obs_size, heads, max(n, n_made or n))
    return obs[:n], (None if mask is None else mask[:n])


def allowed_actions(rng, heads, mask, n):
    """an action per row and head to force, uniform over the head's allowed ones"""
    out, off = np.empty((n, len(heads)), np.int64), 0
    for h, w in enumerate(heads):
        score = rng.random((n, w))
        if mask is not None:
            assert mask[:, off:off + w].any(axis=1).all()
            score = np.where(mask[:, off:off + w] != 0, score, -1.0)
        out[:, h] = score.argmax(axis=1)
        off += w
    return out


# ---------------------------------------------------------------------------------------------------------
# 1. the fused 2 x 64 family: cat_act_kernel, gauss_act_kernel, gauss_values_kernel
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("obs17 (5,3,4) masked", 65605), ("obs17 (5,3,4) masked", 131077), ("obs64 (32,)", 65605)])
def test_cat_fused_act_and_values(P, name, n):
    """PPO_KERNEL_CAT_FUSED in a 4 x 4 caller-stepped context; the stand-alone calls take any n in one launch (asserted on the launch counters)"""
    assert_past_the_cap(n, FUSED_CAP)
    s, b = S.CAT_SHAPES[name], S.batch(name)
    net, params = b["net"], b["params"]
    obs, mask = synthetic_rows(s["seed"], s["obs"], tuple(s["heads"]) if s["masked"] else None, n, 131077 if s["obs"] == 17 else None)
    acts = allowed_actions(np.random.default_rng(n), s["heads"], mask, n)
    ctx = cat_ctx(P, s, N=4, T=4, nmb=1)
    ctx.set_params(params)
    tag = "CAT %s n=%d" % (name, n)

    def counted(call, want):
        before = ctx.cat_fused_launches()
        out = call()
        assert tuple(x - y for x, y in zip(ctx.cat_fused_launches(), before)) == want, tag   # one launch per kernel and call
        return out

    a, lp, en, v = counted(lambda: ctx.policy_act(obs, mask=mask, action=acts), (1, 1, 0))
    gv = counted(lambda: ctx.get_value(obs), (0, 1, 0))
    ga, glp, gen, gvv = counted(lambda: ctx.policy_act_greedy(obs, mask=mask), (1, 1, 0))
    # against the oracle, every row
    lp_o, en_o, v_o = O.evaluate(net, params, obs, acts, mask)
    print("%s against the C oracle: logp %.2e entropy %.2e value %.2e get_value %.2e (max abs)" %
          (tag, np.abs(lp - lp_o).max(), np.abs(en - en_o).max(), np.abs(v - v_o).max(), np.abs(gv - v_o).max()))
    assert np.array_equal(a, acts)
    np.testing.assert_allclose(lp, lp_o, **FWD)
    np.testing.assert_allclose(en, en_o, **FWD)
    np.testing.assert_allclose(v, v_o, **FWD)
    np.testing.assert_allclose(gv, v_o, **FWD)
    # the whole call against first-trip pieces, bit for bit
    names = ("action", "logp", "entropy", "value")
    assert_same_bits(tag + " forced", (a, lp, en, v), in_pieces(lambda o, m, f: ctx.policy_act(o, mask=m, action=f), n, FUSED_CAP, obs, mask, acts), names)
    assert_same_bits(tag + " get_value", (gv,), (in_pieces(ctx.get_value, n, FUSED_CAP, obs),), ("value",))
    assert_same_bits(tag + " greedy", (ga, glp, gen, gvv), in_pieces(lambda o, m: ctx.policy_act_greedy(o, mask=m), n, FUSED_CAP, obs, mask), names)
    assert not np.array_equal(ga, acts)   # the greedy call is a second set of outputs, not the forced one again
    ctx.close()


@pytest.mark.parametrize("obs_size,D,n", [(17, 6, 65605), (17, 6, 131077), (64, 32, 65605)])
def test_gauss_fused_act_and_values(P, obs_size, D, n):
    """PPO_KERNEL_GAUSS_FUSED in a 4 x 4 caller-stepped context: forced, greedy and sampled calls of n rows, each one launch"""
    assert_past_the_cap(n, FUSED_CAP)
    seed, step = 21, 40
    rng = np.random.default_rng(1000 * obs_size + D)
    shapes = tensor_shapes(obs_size, 64, 2, D)
    ctx = fused_ctx(P, obs_size, D, N=4, T=4, seed=seed)
    params = randomised_params(ctx, shapes, rng)
    critic, actor, log_std = nets(unflatten(params, shapes))
    x, _ = synthetic_rows(seed, obs_size, None, n, 131077 if obs_size == 17 else None)
    mu = mlp(actor, t64(x))
    forced = (mu.numpy() + rng.uniform(-4, 4, (n, D)) * np.exp(log_std.numpy())).astype(np.float32)
    tag = "GAUSS obs %d D %d n=%d" % (obs_size, D, n)

    def counted(call, want):
        before = ctx.gauss_fused_launches()
        out = call()
        assert tuple(p - q for p, q in zip(ctx.gauss_fused_launches(), before)) == want, tag
        return out

    a, lp, en, v = counted(lambda: ctx.policy_act_f32(x, action=forced, step_index=7), (1, 1, 0))
    gv = counted(lambda: ctx.get_value(x), (0, 1, 0))
    ga, glp, gen, gvv = counted(lambda: ctx.policy_act_f32(x, greedy=True), (1, 1, 0))
    sa, slp, _, _ = counted(lambda: ctx.policy_act_f32(x, step_index=step), (1, 1, 0))
    # against float64, every row (tests/test_gpu_gauss_fused.py::test_forward_against_the_oracle's quantities and bar)
    lp_o, en_o, v_o = gauss_logprob(mu, log_std, t64(forced)).numpy(), gauss_entropy(mu, log_std).numpy(), mlp(critic, t64(x)).squeeze(-1).numpy()
    err = dict(logp=rel(lp, lp_o), entropy=rel(en, en_o), value=rel(v, v_o), get_value=rel(gv, v_o), mean=rel(ga, mu.numpy()),
               greedy_logp=rel(glp, gauss_logprob(t64(ga), log_std, t64(ga)).numpy()))
    print("%s against float64: %s (max |d| / max(1, |x|))" % (tag, " ".join("%s %.2e" % kv for kv in err.items())))
    assert np.array_equal(bits(a), bits(forced))
    for name, e in err.items():
        assert e <= FWD_BAR, (tag, name, e)
    # the whole call against first-trip pieces, bit for bit
    names = ("action", "logp", "entropy", "value")
    assert_same_bits(tag + " forced", (a, lp, en, v), in_pieces(lambda o, f: ctx.policy_act_f32(o, action=f, step_index=7), n, FUSED_CAP, x, forced), names)
    assert_same_bits(tag + " get_value", (gv,), (in_pieces(ctx.get_value, n, FUSED_CAP, x),), ("value",))
    assert_same_bits(tag + " greedy", (ga, glp, gen, gvv), in_pieces(lambda o: ctx.policy_act_f32(o, greedy=True), n, FUSED_CAP, x), names)
    # the draw: tests/test_gpu_gauss_fused.py::test_draw_equals_the_stateless_gaussian's recipe over all n rows -- the greedy action is the mean's bits, and the
    # sampled call is the stateless Gaussian on those means, keyed by the row's own index
    want = P.gaussian(ctx, ga, params[-D:], None, seed, 0, step)
    assert_same_bits(tag + " draw", (sa, slp), (want["sample"], want["log_prob"]), ("action", "logp"))
    assert (bits(sa) != bits(ga)).mean() > 0.99
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 2. the reference-shape act kernels: policy_act16_kernel (default), policy_act_kernel and values_kernel (the vector form)
# ---------------------------------------------------------------------------------------------------------
def ref_case(P, case, vector):
    flags = P.KERNEL_ROLLOUT_VECTOR if vector else 0
    if case == "cartpole":
        return "ref cartpole obs4 (2,)", dict(env_kind=P.ENV_CARTPOLE, kernel_flags=flags)
    if case == "mountaincar masked":
        return "ref mountaincar obs2 (3,) masked", dict(env_kind=P.ENV_MOUNTAINCAR, obs_size=2, head_dims=(3,), dist_kind=P.DIST_MASKED, kernel_flags=flags)
    assert case == "obs8 (4,)" and vector   # obs 8 has no matrix-core form: the vector kernels without a flag
    return "ref obs8 (4,)", dict(env_kind=P.ENV_HOST, obs_size=8, head_dims=(4,))


@functools.lru_cache(maxsize=None)
def ref_params(shape_name):
    b = G.stand_in_batch(G.REF_SHAPES[shape_name])
    b["params"].setflags(write=False)
    return b["net"], b["params"]


@pytest.mark.parametrize("case,vector,n", [("cartpole", False, 65557), ("mountaincar masked", False, 65557), ("cartpole", False, 131077),
                                           ("cartpole", True, 8197), ("mountaincar masked", True, 8197), ("obs8 (4,)", True, 8197), ("cartpole", True, 16389)])
def test_reference_shape_act_and_values(P, case, vector, n):
    """ppo_policy_act teacher-forced, ppo_policy_act_greedy and ppo_get_value on device-env contexts of the reference's shapes (stand-in parameters of
    tests/grad_oracle.py, synthetic observations and masks)"""
    cap = VECTOR_CAP if vector else ACT16_CAP
    assert_past_the_cap(n, cap)
    shape_name, cfg = ref_case(P, case, vector)
    s = G.REF_SHAPES[shape_name]
    net, params = ref_params(shape_name)
    ctx = P.Context(P.make_config(num_envs=8, num_steps=8, seed=s["seed"], **cfg))
    assert ctx.P == params.size
    ctx.set_params(params)
    obs, mask = synthetic_rows(s["seed"], s["obs"], tuple(s["heads"]) if s["masked"] else None, n, 131077 if case == "cartpole" and not vector else None)
    acts = allowed_actions(np.random.default_rng(n), s["heads"], mask, n)
    tag = "REF %s%s n=%d" % (case, " vector" if vector else "", n)
    a, lp, en, v = ctx.policy_act(obs, mask=mask, action=acts)
    gv = ctx.get_value(obs)
    ga, glp, gen, gvv = ctx.policy_act_greedy(obs, mask=mask)
    lp_o, en_o, v_o = O.evaluate(net, params, obs, acts, mask)
    print("%s against the C oracle: logp %.2e entropy %.2e value %.2e get_value %.2e (max abs)" %
          (tag, np.abs(lp - lp_o).max(), np.abs(en - en_o).max(), np.abs(v - v_o).max(), np.abs(gv - v_o).max()))
    assert np.array_equal(a, acts)
    np.testing.assert_allclose(lp, lp_o, rtol=0, atol=PARITY_ATOL)
    np.testing.assert_allclose(en, en_o, rtol=0, atol=PARITY_ATOL)
    np.testing.assert_allclose(v, v_o, rtol=0, atol=PARITY_ATOL)
    np.testing.assert_allclose(gv, v_o, rtol=0, atol=PARITY_ATOL)
    names = ("action", "logp", "entropy", "value")
    assert_same_bits(tag + " forced", (a, lp, en, v), in_pieces(lambda o, m, f: ctx.policy_act(o, mask=m, action=f), n, cap, obs, mask, acts), names)
    assert_same_bits(tag + " get_value", (gv,), (in_pieces(ctx.get_value, n, cap, obs),), ("value",))
    assert_same_bits(tag + " greedy", (ga, glp, gen, gvv), in_pieces(lambda o, m: ctx.policy_act_greedy(o, mask=m), n, cap, obs, mask), names)
    if not vector:
        assert ctx.profile_read()["vector_fallback_launches"] == 0   # the default path stayed on the matrix-core kernel
    ctx.close()


# ---------------------------------------------------------------------------------------------------------
# 3. the generic engine's fused bf16 forward: generic_forward_kernel
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16453, 32773])
def test_generic_bf16_fused_forward(P, n):
    """"bf16 obs120 h48x2 (2,3) masked" of grad_oracle.SHAPES in a context of n envs x 1 step, one minibatch: the workspaces hold max(minibatch, num_envs)
    = n rows, so ppo_policy_act over n rows is ONE chunk and one launch of 256 workgroups (a smaller context would cut the call into first-trip chunks).

    Parameters: _check_shape's recipe (orthogonal init, the actor's head x 30), because the bar is _check_shape's: TOL[1] is a fence measured under that
    recipe, where one bf16 ulp of one activation (2^-8) moves a logit by at most 2^-8 x 0.14.  grad_oracle.make_params also adds 0.02 noise before the
    x 30, which puts head weights up to 2.1: there a single activation that rounds the other way moves a logit by 8e-3, four times the log-prob bar, in
    any implementation -- the C oracle's bf16 mode against itself after a relative 1e-6 change of the parameters is above 2e-3 on 120 of these 16 453 rows
    (max 5.1e-3), and the library measured 5 rows above it (max 1.7e-2, all in first-trip rows, the whole call and its pieces equal bit for bit)."""
    assert_past_the_cap(n, GENERIC_CAP)
    s = G.SHAPES["bf16 obs120 h48x2 (2,3) masked"]
    assert s["dtype"] == 1 and s["masked"]
    A = sum(s["heads"])
    ctx = G.context(P, s, num_envs=n, num_steps=1, num_minibatches=1, total_timesteps=8 * n)
    assert ctx.N * ctx.T >= n and ctx.N >= n   # rows_max >= n: one chunk
    ctx.init_orthogonal(s["seed"])
    params = ctx.get_params()
    params[-(A * s["hidden"] + A):] *= 30.0    # a policy that is not uniform (tests/test_gpu_generic.py::_check_shape)
    ctx.set_params(params)
    net = O.Net.make(s["obs"], list(s["heads"]), hidden=s["hidden"], n_hidden=s["n_hidden"], dist_kind=O.DIST_MASKED, dtype=1)
    obs, mask = synthetic_rows(s["seed"], s["obs"], tuple(s["heads"]), n, 32773)
    acts = allowed_actions(np.random.default_rng(n), s["heads"], mask, n)
    tag = "GENERIC bf16 n=%d" % n
    a, lp, en, v = ctx.policy_act(obs, mask=mask, action=acts)
    gv = ctx.get_value(obs)
    names = ("action", "logp", "entropy", "value")
    assert_same_bits(tag + " forced", (a, lp, en, v), in_pieces(lambda o, m, f: ctx.policy_act(o, mask=m, action=f), n, GENERIC_CAP, obs, mask, acts), names)
    assert_same_bits(tag + " get_value", (gv,), (in_pieces(ctx.get_value, n, GENERIC_CAP, obs),), ("value",))
    # the C oracle's bf16 forward at the bars tests/test_gpu_generic.py::_check_shape asserts for it (TOL[1]: log-prob, value; entropy with rtol 1e-5)
    tol = TOL[1]
    lp_o, en_o, v_o = O.evaluate(net, params, obs, acts, mask)
    print("%s against the C oracle's bf16 mode: logp %.2e entropy %.2e value %.2e get_value %.2e (max abs)" %
          (tag, np.abs(lp - lp_o).max(), np.abs(en - en_o).max(), np.abs(v - v_o).max(), np.abs(gv - v_o).max()))
    assert np.array_equal(a, acts)
    np.testing.assert_allclose(lp, lp_o, rtol=0, atol=tol["fwd"])
    np.testing.assert_allclose(v, v_o, rtol=0, atol=tol["fwd_v"])
    np.testing.assert_allclose(gv, v_o, rtol=0, atol=tol["fwd_v"])
    np.testing.assert_allclose(en, en_o, rtol=1e-5, atol=tol["fwd"])
    ctx.close()
