"""Networks other than the reference's 2 x 64 and the synthetic env of BASELINE configs[4] (obs 376, heads [3, 3, 3, 2], 4 x 256 MLP),
through the same C-ABI, against the oracle -- which is generic in width, depth and head list (oracle/ppo_oracle.c:mlp_forward1 /
mlp_backward1) and restates the synthetic env with integer arithmetic (orc_synthetic_*).

Per shape: the env's observations / masks / rewards / done flags in the rollout buffers bit-exact; log-probs, values and the sampler
against the oracle's forward; advantages / returns bit-exact; one minibatch step (losses 1e-5, gradient 1e-4 of max) and the
optimizer step; then whole updates run.  The gradient is held twice: as one flat vector within 1e-4 (f32) / 6e-4 (bf16) of its largest element, and tensor by
tensor, each against its OWN largest element (f32: the float64 oracle of tests/grad_oracle.py and the bar of tests/test_gpu_generic_grads.py; bf16: the bf16
oracle, tensor t within grad_oracle.bf16_tensor_bars = max(d_b16[t], median(d_b16)), d_b16 = that oracle's own distance from float64 on the same rows).  That step
is at ratio = 1 and v = v_old, so no row is near a branch and the rows need no filtering; the step off it is tests/test_gpu_generic_grads.py's.
"""
import numpy as np
import pytest

import grad_oracle as GO
import oracle as O
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def P():
    return load_package()


# tolerances per compute dtype: (log-prob / value / entropy abs, sampler agreement, loss scalars rel, gradient of max, stand-alone vs rollout abs)
# bf16: HIP and oracle round at the same points (operands and stored activations, nearest even); what differs is the f32 summation order and
# tanh (hardware exp2 against tanhf), which now and then tips a value across a bf16 rounding boundary (one part in 256 of that activation).
# Measured at configs[4]'s shape (tools/bf16_dev_report.py): log-prob 6e-4 max / 4e-6 mean, value 2e-3 max / 2e-5 mean, losses 2e-6, gradient 2e-4
# of its largest element -- against 0.38 / 1e-2 / 1e-2 between the bf16 and the f32 arithmetic themselves.
# What pins what: the yardstick of _check_shape is the oracle's generic / bf16 mode (ORC_DTYPE_BF16).  The oracle's f32 arithmetic is held to the compiled reference at the
# reference's own 2 x 64 shape AND at configs[4]'s shape (obs 376, 4 x 256, heads [3, 3, 3, 2]: tests/test_oracle_vs_golden.py against tests/golden/config4_*.pgld), and the
# build's f32 generic path is held to the same fixtures directly (tests/test_gpu_config4_ref.py; the tests at the end of this file for 2 x 64).  bf16 arithmetic has no
# counterpart in the reference: its bars are distances (measured, x 3), not parity.
# bf16 bars = REGRESSION FENCES at ~3x the measured values above (log-prob 6e-4 -> 2e-3, value 2e-3 -> 4e-3 (2x), losses 2e-6 -> 6e-6, gradient 2e-4 -> 6e-4 of max): they
# say "the bf16 kernels have not moved away from the bf16 oracle", not "the bf16 kernels are within a derived bound of the reference" (DESIGN.md section 0, row x1).
# The fences remain the END-TO-END check of the bf16 forward (a row's log-prob, value and entropy through all layers and the heads).  The DERIVED check is
# tests/test_gpu_bf16_layers.py: every hidden layer element by element against float64 on the layer's own inputs (tests/bf16_layers.py), which sees what the
# fences absorb -- a store that truncates, a tanh 1e-4 off, a lost k chunk, a few rows off by less than the fence.
TOL = {0: dict(fwd=5e-6, fwd_v=5e-6, agree=0.995, loss=1e-5, grad=1e-4, same=1e-6), 1: dict(fwd=2e-3, fwd_v=4e-3, agree=0.98, loss=6e-6, grad=6e-4, same=1e-6)}


def _check_shape(P, obs_dim, hidden, n_hidden, heads, N, T, nmb, masked, seed, max_steps=40, dtype=0):
    A, H = sum(heads), len(heads)
    tol = TOL[dtype]
    hp = dict(gamma=0.99, gae_lambda=0.95, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5)
    dist = P.DIST_MASKED if masked else P.DIST_CATEGORICAL
    ctx = P.Context(P.make_config(env_kind=P.ENV_SYNTHETIC, dist_kind=dist, obs_size=obs_dim, head_dims=tuple(heads), hidden=hidden, n_hidden=n_hidden,
                                  num_envs=N, num_steps=T, num_minibatches=nmb, update_epochs=2, max_episode_steps=max_steps, seed=seed,
                                  total_timesteps=8 * N * T, learning_rate=1e-3, anneal_lr=False, compute_dtype=dtype, **hp))
    net = O.Net.make(obs_dim, list(heads), hidden=hidden, n_hidden=n_hidden, dist_kind=O.DIST_MASKED if masked else O.DIST_CATEGORICAL, dtype=dtype)
    assert ctx.P == O.param_count(net)
    ctx.init_orthogonal(seed)
    params = ctx.get_params()
    # every parameter tensor of the oracle's shape list, in order (critic layers then actor layers)
    shp = O.param_shapes(net)
    assert int(sum(a * b for a, b in shp)) == params.size
    params[-(A * hidden + A):] *= 30.0    # a policy that is not uniform
    ctx.set_params(params)

    obs0 = ctx.env_reset()
    envs = np.arange(N)
    assert np.array_equal(bits(obs0), bits(O.synthetic_obs(seed, envs, 0, obs_dim)))
    ctx.rollout()
    obs = ctx.read("OBS", (T, N, obs_dim))
    masks = ctx.read("MASKS", (T, N, A))
    actions = ctx.read("ACTIONS", (T, N, H)).astype(np.int64)
    logp, values = ctx.read("LOGPROBS", (T, N)), ctx.read("VALUES", (T, N))
    rewards, dones = ctx.read("REWARDS", (T, N)), ctx.read("DONES", (T, N))
    next_obs, next_done, next_value = ctx.read("NEXT_OBS", (N, obs_dim)), ctx.read("NEXT_DONE", (N,)), ctx.read("NEXT_VALUE", (N,))
    # ---- the env, bit for bit ----
    ep_len = np.zeros(N, np.int64)
    for t in range(T):
        assert np.array_equal(bits(obs[t]), bits(O.synthetic_obs(seed, envs, t, obs_dim))), t
        assert np.array_equal(masks[t], O.synthetic_mask(seed, envs, t, list(heads)) if masked else np.ones((N, A), np.uint8)), t
        r, d = O.synthetic_transition(seed, envs, t)
        ep_len += 1
        d = np.where(ep_len == max_steps, 1, d)          # time-limit truncation counts as done (PPO_Discrete.cpp:443-445)
        ep_len[d != 0] = 0
        assert np.array_equal(rewards[t], r), t
        assert np.array_equal(dones[t + 1] if t + 1 < T else next_done.astype(np.float32), d.astype(np.float32)), t
    assert np.array_equal(bits(next_obs), bits(O.synthetic_obs(seed, envs, T, obs_dim)))
    assert dones.sum() > 0
    if masked:   # sampled actions respect the masks
        off = 0
        for h, w in enumerate(heads):
            picked = np.take_along_axis(masks[:, :, off:off + w], actions[:, :, h:h + 1], axis=2)
            assert picked.all()
            off += w
    # ---- policy and critic against the oracle's forward ----
    flat_obs, flat_act, flat_mask = obs.reshape(T * N, obs_dim), actions.reshape(T * N, H), masks.reshape(T * N, A)
    rows = np.random.default_rng(0).choice(T * N, min(T * N, 1024), replace=False)
    lp_o, en_o, v_o = O.evaluate(net, params, flat_obs[rows], flat_act[rows], flat_mask[rows] if masked else None)
    np.testing.assert_allclose(logp.reshape(-1)[rows], lp_o, rtol=0, atol=tol["fwd"])
    np.testing.assert_allclose(values.reshape(-1)[rows], v_o, rtol=0, atol=tol["fwd_v"])
    np.testing.assert_allclose(next_value[:64], O.get_value(net, params, next_obs[:64]), rtol=0, atol=tol["fwd_v"])
    a_o, _, _, _ = O.act(net, params, obs[3], seed, 3, 0, masks[3] if masked else None)
    assert (a_o == actions[3]).mean() >= tol["agree"]
    # stand-alone entry points agree with the rollout's stores
    a2, lp2, en2, v2 = ctx.policy_act(obs[3], mask=masks[3] if masked else None, action=actions[3], step_index=3)
    np.testing.assert_allclose(lp2, logp[3], rtol=0, atol=tol["same"])
    np.testing.assert_allclose(v2, values[3], rtol=0, atol=tol["same"])
    np.testing.assert_allclose(en2[:256], O.evaluate(net, params, obs[3][:256], actions[3][:256], masks[3][:256] if masked else None)[1], rtol=1e-5, atol=tol["fwd"])
    # ---- advantages / returns, bit for bit ----
    adv, ret = ctx.calc_advantage()
    adv_o, ret_o = O.gae(rewards, values, dones, next_value, next_done, hp["gamma"], hp["gae_lambda"])
    assert np.array_equal(bits(adv), bits(adv_o)) and np.array_equal(bits(ret), bits(ret_o))
    # ---- one minibatch step ----
    B = T * N
    MB = B // nmb
    idx = np.random.default_rng(1).permutation(B)[:MB].astype(np.int32)
    grads = ctx.minibatch_forward_backward(idx)
    st = ctx.stats()
    hpo = O.HParams(norm_adv=1, clip_vloss=1, **hp)
    g_o, s_o = O.minibatch_grads(net, hpo, params, flat_obs, flat_act.astype(np.float32), logp.reshape(B), adv.reshape(B), ret.reshape(B), values.reshape(B),
                                 idx.astype(np.int64), flat_mask if masked else None)[:2]
    for key, okey in (("pg_loss", "pg_loss"), ("v_loss", "v_loss"), ("entropy_loss", "entropy_loss"), ("approx_kl", "approx_kl"),
                      ("clipfrac_last", "clipfrac"), ("loss", "loss")):
        assert abs(st[key] - s_o[okey]) <= tol["loss"] * max(1.0, abs(s_o[okey])), (key, st[key], s_o[okey])
    assert np.abs(grads - g_o).max() <= 1e-6 + tol["grad"] * np.abs(g_o).max(), np.abs(grads - g_o).max() / np.abs(g_o).max()
    # ... and tensor by tensor, each against its own largest element (the actor's x 30 head dominates the flat vector)
    names = [GO.tensor_name(n_, l_, k_) for _, n_, l_, k_, _ in GO.split(g_o, shp)]
    g64 = GO.minibatch_grads(shp, heads, masked, dict(hp, norm_adv=True, clip_vloss=True), params, flat_obs, flat_act, logp.reshape(B), adv.reshape(B), ret.reshape(B),
                             values.reshape(B), idx, flat_mask if masked else None)[0]
    d_ref = GO.tensor_distance(g_o, g64, shp)          # the oracle's own distance from float64 in this arithmetic: the unit of either bar
    if dtype == 0:
        d_t, bars = GO.tensor_distance(grads, g64, shp), GO.f32_tensor_bars(d_ref)
    else:
        d_t, bars = GO.tensor_distance(grads, g_o, shp), GO.bf16_tensor_bars(d_ref)
    print("per tensor:", ", ".join("%s %.1e (bar %.1e)" % (n_, x, b_) for n_, x, b_ in zip(names, d_t, bars)), "| worst %.1e, worst of bar %.2f" % (d_t.max(), (d_t / bars).max()))
    assert (d_t <= bars).all(), [(n_, float(x), float(b_)) for n_, x, b_ in zip(names, d_t, bars) if not x <= b_]
    ctx.set_learning_rate(1e-3)
    ctx.optimizer_step()
    m, v, step = ctx.get_optimizer()
    gc, total = O.clip_grad_norm(net, grads, 0.5)
    assert abs(ctx.stats()["total_norm"] - float(total)) <= 2e-6 * float(total)
    p_o, m_o, v_o2 = O.adamw_step(params, gc, np.zeros_like(params), np.zeros_like(params), 1e-3, 1)
    np.testing.assert_allclose(m, m_o, rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(v, v_o2, rtol=2e-5, atol=1e-18)
    np.testing.assert_allclose(ctx.get_params(), p_o, rtol=0, atol=1e-6)
    # ---- whole iterations ----
    ctx.update()
    for _ in range(2):
        ctx.train_iteration()
    st = ctx.stats()
    assert np.isfinite(st["loss"]) and st["optimizer_steps"] == 1 + 3 * 2 * nmb and st["ep_count"] > 0
    ctx.close()


def test_small_multihead_masked_three_layers(P):
    _check_shape(P, obs_dim=12, hidden=32, n_hidden=3, heads=(3, 2), N=64, T=16, nmb=2, masked=True, seed=5)


def test_plain_categorical_one_layer(P):
    _check_shape(P, obs_dim=7, hidden=48, n_hidden=1, heads=(4,), N=32, T=12, nmb=3, masked=False, seed=9)


def test_widths_that_are_not_multiples_of_four(P):
    """hidden 30, obs 5, 40 envs x 10 steps: every operand of every layer product has a ragged contiguous extent (4-byte loads, zero-filled
    tails), every tile is an edge tile, the weight planes are mostly padding, and the minibatch (200 rows) is not a multiple of a chunk."""
    _check_shape(P, obs_dim=5, hidden=30, n_hidden=2, heads=(3,), N=40, T=10, nmb=2, masked=False, seed=11)


def test_hidden_wider_than_one_tile(P):
    """hidden 160: two n tiles of which the second is ragged (XCD-aware tile order with an odd tile count, plane rows beyond the width)."""
    _check_shape(P, obs_dim=20, hidden=160, n_hidden=2, heads=(2, 3), N=48, T=12, nmb=2, masked=True, seed=13)


def test_config4_shape_obs376_4x256_heads_3332(P):
    """BASELINE configs[4]'s network and head list on a batch the scalar oracle can still check (256 envs x 32 steps)."""
    _check_shape(P, obs_dim=376, hidden=256, n_hidden=4, heads=(3, 3, 3, 2), N=256, T=32, nmb=4, masked=True, seed=3, max_steps=25)


def test_config4_shape_in_bf16(P):
    """BASELINE configs[4] in the arithmetic it names -- "4x256 MLP bf16 with MFMA GEMMs" (compute_dtype = PPO_DTYPE_BF16: bf16 operands and
    stored activations, f32 accumulation, f32 master weights) -- end to end against the oracle's bf16 mode (oracle/ppo_oracle.h: ORC_DTYPE_BF16),
    which rounds at the same points: rollout log-probs / values, the sampler, one minibatch step's losses and gradient, the optimizer step.  The bars are regression fences
    (TOL above), not parity with the reference: the f32 path carries that (tests/test_gpu_config4_ref.py)."""
    _check_shape(P, obs_dim=376, hidden=256, n_hidden=4, heads=(3, 3, 3, 2), N=256, T=32, nmb=4, masked=True, seed=3, max_steps=25, dtype=1)


def test_bf16_ragged_shapes(P):
    """bf16 storage with widths that fill neither a tile nor a chunk (hidden 48 in a 128-wide pitch, obs 20, 5 logits) and a minibatch that is
    not a multiple of the 64-row contraction step (48 envs x 10 steps / 2 = 240 rows): the zero padding of every buffer is what the
    unguarded staging relies on."""
    _check_shape(P, obs_dim=20, hidden=48, n_hidden=2, heads=(2, 3), N=48, T=10, nmb=2, masked=True, seed=13, dtype=1)


@pytest.mark.parametrize("masked", [True, False])
def test_bf16_many_heads(P, masked):
    """bf16 storage beyond four heads / sixteen logits: the loss kernel's second register layout (eight heads, 32 logits -- the ABI's maximum)."""
    _check_shape(P, obs_dim=24, hidden=64, n_hidden=2, heads=(5, 3, 4, 2, 3, 3), N=64, T=12, nmb=2, masked=masked, seed=21, dtype=1)


@pytest.mark.parametrize("dtype", [0, 1])
def test_config4_per_gpu_size_runs(P, dtype):
    """configs[4] per-GPU share (16 384 envs / 8 GPUs = 2048 envs x 128 steps, 4 minibatches): two whole iterations, f32 and bf16."""
    ctx = P.Context(P.make_config(env_kind=P.ENV_SYNTHETIC, dist_kind=P.DIST_MASKED, obs_size=376, head_dims=(3, 3, 3, 2), hidden=256, n_hidden=4,
                                  num_envs=2048, num_steps=128, num_minibatches=4, update_epochs=2, max_episode_steps=200, seed=1,
                                  total_timesteps=4 * 2048 * 128, ent_coef=0.01, compute_dtype=dtype))
    ctx.init_orthogonal(1)
    ctx.env_reset()
    for _ in range(2):
        ctx.train_iteration()
    st = ctx.stats()
    assert np.isfinite(st["loss"]) and st["optimizer_steps"] == 16 and st["global_step"] == 2 * 2048 * 128
    assert 0.0 < st["entropy_loss"] <= 3 * np.log(3) + np.log(2) + 1e-3
    ctx.close()


@pytest.mark.parametrize("dtype", [0, 1])
def test_config4_runs_are_bit_reproducible(P, dtype):
    """The same configs[4] share twice from the same seed: parameters, log-probs and actions bit-identical (weight-gradient slabs, bias column
    sums and loss partials are all added in a fixed order; sampling is counter-based)."""
    outs = []
    for _ in range(2):
        ctx = P.Context(P.make_config(env_kind=P.ENV_SYNTHETIC, dist_kind=P.DIST_MASKED, obs_size=376, head_dims=(3, 3, 3, 2), hidden=256, n_hidden=4,
                                      num_envs=2048, num_steps=32, num_minibatches=4, update_epochs=2, max_episode_steps=200, seed=4,
                                      total_timesteps=4 * 2048 * 32, ent_coef=0.01, compute_dtype=dtype))
        ctx.init_orthogonal(2)
        ctx.env_reset()
        for _ in range(2):
            ctx.train_iteration()
        outs.append((ctx.get_params(), ctx.read("LOGPROBS"), ctx.read("ACTIONS"), ctx.stats()["loss"]))
        ctx.close()
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0]))
    assert np.array_equal(bits(outs[0][1]), bits(outs[1][1])) and np.array_equal(outs[0][2], outs[1][2]) and outs[0][3] == outs[1][3]


@pytest.mark.parametrize("shape", ["f32 small", "bf16 configs[4] widths"])
def test_generic_two_rank_shards_equal_single_context(P, shape):
    """Data parallelism on the generic path: two shards (env_offset / global_num_envs) reproduce their columns of the single-context rollout
    -- env buffers and actions bit for bit, network outputs to float noise (the library GEMM picks its kernel, and with it the order of
    the K-sum, by batch size) -- and one optimizer step over the in-process communicator (same protocol as RCCL: global advantage sums, then ONE
    all-reduce of the 1/M_global-scaled gradient) equals the single-context step on the concatenated minibatch."""
    import threading
    # the second shape takes the fused bf16 kernels (rows read in place, both nets per launch) on every rank, and the multi-rank optimizer path behind them
    bf16 = shape != "f32 small"
    N, T = 64, 16
    heads, obs_dim, hidden, n_hidden = ((3, 3, 3, 2), 376, 256, 4) if bf16 else ((3, 2), 20, 32, 2)
    A = sum(heads)
    kw = dict(env_kind=P.ENV_SYNTHETIC, dist_kind=P.DIST_MASKED, obs_size=obs_dim, head_dims=heads, hidden=hidden, n_hidden=n_hidden, num_steps=T, num_minibatches=2,
              update_epochs=1, max_episode_steps=30, seed=11, total_timesteps=4 * N * T, ent_coef=0.01, anneal_lr=False,
              compute_dtype=P.DTYPE_BF16 if bf16 else P.DTYPE_F32)
    whole = P.Context(P.make_config(num_envs=N, **kw))
    whole.init_orthogonal(4)
    params = whole.get_params()
    whole.env_reset(); whole.rollout(); whole.calc_advantage()
    rows_t = np.random.default_rng(2).choice(T, 8, replace=False)
    rows = np.array([t * N + e for t in rows_t for e in range(N)], np.int32)       # whole time rows: both shards hold half of each
    g_ref = whole.minibatch_forward_backward(rows)
    st_ref = whole.stats()
    whole.set_learning_rate(1e-3); whole.optimizer_step()
    p_ref = whole.get_params()
    out, errors = [None, None], []

    def run(rank):
        try:
            n, off = P.dist.shard_envs(N, rank, 2)
            ctx = P.Context(P.make_config(num_envs=n, env_offset=off, global_num_envs=N, **kw))
            ctx.comm_init_local(4321, rank, 2)
            ctx.set_params(params)
            ctx.env_reset(); ctx.rollout(); ctx.calc_advantage()
            sl = slice(off, off + n)
            for name, shape in (("OBS", (T, N, obs_dim)), ("MASKS", (T, N, A)), ("ACTIONS", (T, N, len(heads))), ("LOGPROBS", (T, N)), ("REWARDS", (T, N)),
                                ("VALUES", (T, N)), ("ADVANTAGES", (T, N))):
                full, part = whole.read(name, shape), ctx.read(name, (T, n) + shape[2:])
                if name in ("LOGPROBS", "VALUES", "ADVANTAGES"):
                    np.testing.assert_allclose(part, full[:, sl], rtol=0, atol=2e-5, err_msg=name)
                else:
                    assert np.array_equal(full[:, sl].view(np.uint8), part.view(np.uint8)), (rank, name)
            local = np.array(P.dist.local_rows_of_global_rows(rows, T, N, rank, 2), np.int32)
            d = ctx.dev(local, np.int32)
            P.binding._check(P.binding.lib().ppo_minibatch_forward_backward(ctx.h, d.ptr, __import__("ctypes").c_int64(local.size)), ctx.h)
            P.binding._check(P.binding.lib().ppo_allreduce_grads(ctx.h), ctx.h)
            grads = ctx.read("GRADS")
            ctx.set_learning_rate(1e-3); ctx.optimizer_step()
            out[rank] = (grads, ctx.stats(), ctx.get_params())
            ctx.close()
        except Exception as ex:
            errors.append(ex)

    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errors, errors
    for r in range(2):
        g2, st2, p2 = out[r]
        assert np.abs(g2 - g_ref).max() <= 2e-5 * max(1.0, np.abs(g_ref).max()), r
        for key in ("pg_loss", "v_loss", "entropy_loss", "approx_kl", "loss", "total_norm"):
            assert abs(st2[key] - st_ref[key]) <= 2e-5 * max(1.0, abs(st_ref[key])), (r, key, st2[key], st_ref[key])
        assert np.abs(p2 - p_ref).max() <= 2e-5, r
    assert np.array_equal(bits(out[0][2]), bits(out[1][2]))   # replicas stay bit-identical
    whole.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# The generic kernels AT THE REFERENCE'S OWN SHAPE, against the compiled reference: what pins this file's CODE (not its shapes).
# The reference cannot build a 4 x 256 network, but the generic path can build the reference's 2 x 64 one: env_kind SYNTHETIC selects the GEMM-based
# kernels (kernels_gemm.hip, kernels_generic*.hip) whatever the widths; the reference's rollout batch is written into the context's buffers and the
# 40 optimizer steps of its first update are driven with its own permutations -- the fixtures, loop and bars of
# tests/test_gpu_parity.py::test_full_update_tracks_reference (losses 1e-5: north_star; parameters after the update 2e-6), on the other kernels.
# ---------------------------------------------------------------------------------------------------------------------------------------
import os  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REFERENCE_UPDATES = ["discrete_t32_n8_seed2", "discrete_t64_n16_seed3_trunc", "discrete_t128_n64_seed1", "discrete_shipped_toml_t32_n8_act1",
                     "discrete_config0_t128_n8_seed2", "multidiscrete_mountaincar_t32_n16"]


def _load_reference_update(name):
    g = O.read_pgld(os.path.join(G, name + ".pgld"))
    m, h = g["meta"], g["hparams"]
    meta = dict(T=int(m[0]), N=int(m[1]), obs=int(m[2]), act=int(m[3]), nmb=int(m[4]), epochs=int(m[5]), max_steps=int(m[6]), seed=int(m[7]), updates=int(m[8]),
                anneal=int(m[9]), norm_adv=int(m[11]), clip_vloss=int(m[12]), masked=int(m[13]),
                lr=float(h[0]), gamma=float(h[1]), lam=float(h[2]), clip=float(h[3]), ent=float(h[4]), vf=float(h[5]), mgn=float(h[6]))
    return g, meta


def _generic_ctx_at_reference_shape(P, meta, dtype):
    return P.Context(P.make_config(env_kind=P.ENV_SYNTHETIC, dist_kind=P.DIST_MASKED if meta["masked"] else P.DIST_CATEGORICAL, obs_size=meta["obs"],
                                   head_dims=(meta["act"],), hidden=64, n_hidden=2, num_envs=meta["N"], num_steps=meta["T"], num_minibatches=meta["nmb"],
                                   update_epochs=meta["epochs"], max_episode_steps=meta["max_steps"], use_gae=True, norm_adv=bool(meta["norm_adv"]),
                                   clip_vloss=bool(meta["clip_vloss"]), anneal_lr=bool(meta["anneal"]), seed=meta["seed"],
                                   total_timesteps=meta["updates"] * meta["T"] * meta["N"], learning_rate=meta["lr"], gamma=meta["gamma"], gae_lambda=meta["lam"],
                                   clip_coef=meta["clip"], ent_coef=meta["ent"], vf_coef=meta["vf"], max_grad_norm=meta["mgn"], compute_dtype=dtype))


def _write_reference_batch(ctx, g, U, meta):
    T, N = meta["T"], meta["N"]
    ctx.write("OBS", g[U + "obs"])
    ctx.write("ACTIONS", g[U + "actions"].reshape(T, N, -1)[:, :, :1].astype(np.int32))
    for buf, key in (("LOGPROBS", "logprobs"), ("REWARDS", "rewards"), ("DONES", "dones"), ("VALUES", "values"), ("ADVANTAGES", "gae_advantages"), ("RETURNS", "gae_returns")):
        ctx.write(buf, g[U + key])
    if meta["masked"]:
        ctx.write("MASKS", g[U + "action_masks"].astype(np.uint8))


@pytest.mark.parametrize("name", REFERENCE_UPDATES)
def test_generic_kernels_track_the_reference_update_at_its_own_shape(P, name):
    g, meta = _load_reference_update(name)
    ctx = _generic_ctx_at_reference_shape(P, meta, 0)
    assert ctx.P == g["u1/params_before"].size
    U = "u1/"
    MB = meta["T"] * meta["N"] // meta["nmb"]
    _write_reference_batch(ctx, g, U, meta)
    ctx.set_params(g[U + "params_before"])
    ctx.set_learning_rate(float(g[U + "lr"][0]))
    scal = g[U + "step_scalars"]
    k = 0
    for e in range(meta["epochs"]):
        for s in range(meta["nmb"]):
            ctx.minibatch_forward_backward(g[U + "perms"][e, s * MB:(s + 1) * MB])
            st = ctx.stats()
            for i, key in enumerate(("pg_loss", "v_loss", "entropy_loss", "approx_kl", "clipfrac_last", "loss")):
                assert abs(st[key] - scal[k, i]) <= 1e-5 * max(1.0, abs(scal[k, i])), (name, k, key, st[key], scal[k, i])
            ctx.optimizer_step()
            k += 1
    assert np.abs(ctx.get_params() - g[U + "params_after"]).max() <= 2e-6
    ctx.close()


@pytest.mark.parametrize("name", REFERENCE_UPDATES)
def test_generic_forward_kernels_against_the_reference_at_its_own_shape(P, name):
    """tests/test_gpu_parity.py::test_policy_forward_teacher_forced on the generic forward kernels: the reference's own log-probs, entropies and values of its
    rollout, and its bootstrap value, within 3e-6; then the generic scan on the reference's rewards / values / dones bit for bit."""
    g, meta = _load_reference_update(name)
    ctx = _generic_ctx_at_reference_shape(P, meta, 0)
    U = "u1/"
    T, N = meta["T"], meta["N"]
    B = T * N
    ctx.set_params(g[U + "params_before"])
    obs = g[U + "obs"].reshape(B, meta["obs"])
    acts = g[U + "actions"].reshape(B, -1)[:, :1].astype(np.int64)
    mask = g[U + "action_masks"].reshape(B, -1).astype(np.uint8) if meta["masked"] else None
    a, lp, en, v = ctx.policy_act(obs, mask=mask, action=acts)
    assert np.array_equal(a, acts)
    np.testing.assert_allclose(lp, g[U + "logprobs"].ravel(), rtol=0, atol=3e-6)
    np.testing.assert_allclose(v, g[U + "values"].ravel(), rtol=0, atol=3e-6)
    np.testing.assert_allclose(en, g[U + "rollout_entropy"].ravel(), rtol=0, atol=3e-6)
    np.testing.assert_allclose(ctx.get_value(g[U + "next_obs"]), g[U + "next_value"].ravel(), rtol=0, atol=3e-6)
    ctx.close()


@pytest.mark.parametrize("name", ["discrete_t128_n64_seed1", "multidiscrete_mountaincar_t32_n16"])
def test_generic_bf16_arithmetic_against_the_reference_update(P, name):
    """The bf16 mode (BASELINE configs[4]'s arithmetic) on the reference's own batch: how far bf16 operands and activations move the reference's fp32
    scalars over the 40 steps of an update.  Not a parity claim (the reference has no bf16 mode) -- a measured distance with a bar at ~3x of it (2e-4)."""
    g, meta = _load_reference_update(name)
    ctx = _generic_ctx_at_reference_shape(P, meta, 1)
    U = "u1/"
    MB = meta["T"] * meta["N"] // meta["nmb"]
    _write_reference_batch(ctx, g, U, meta)
    ctx.set_params(g[U + "params_before"])
    ctx.set_learning_rate(float(g[U + "lr"][0]))
    scal = g[U + "step_scalars"]
    worst = {}
    k = 0
    for e in range(meta["epochs"]):
        for s in range(meta["nmb"]):
            ctx.minibatch_forward_backward(g[U + "perms"][e, s * MB:(s + 1) * MB])
            st = ctx.stats()
            for i, key in enumerate(("pg_loss", "v_loss", "entropy_loss", "approx_kl", "loss")):
                d = abs(st[key] - scal[k, [0, 1, 2, 3, 5][i]]) / max(1.0, abs(scal[k, [0, 1, 2, 3, 5][i]]))
                worst[key] = max(worst.get(key, 0.0), d)
            ctx.optimizer_step()
            k += 1
    print(name, "bf16 against the reference's fp32 scalars, worst relative distance over", k, "steps:", {a: "%.2e" % b for a, b in worst.items()})
    assert all(np.isfinite(v) for v in worst.values())
    assert max(worst.values()) <= 2e-4, worst    # measured 5.5e-5 (v_loss, MountainCar fixture), 3.7e-5 (CartPole)
    ctx.close()


def test_generic_forward_kernels_on_the_reference_multihead_agent(P):
    """configs[4]'s head list [3, 3, 3, 2] is the one head list the reference was ALSO run with (Agent::getActionAndValueMasked with m_actionSpace = {3,3,3,2},
    tests/golden/multihead_agent.pgld: Agent.cpp:137-170 with its 2 x 64 bodies): the generic forward kernels against that fixture -- log-probs and entropies
    summed over heads, masks with disabled actions, teacher-forced actions (the bars of tests/test_gpu_parity.py::test_multihead_masked_agent)."""
    g = O.read_pgld(os.path.join(G, "multihead_agent.pgld"))
    heads = tuple(int(h) for h in g["heads"])
    obs_dim = g["x"].shape[1]
    for dtype, tol in ((0, 3e-6), (1, 2e-2)):
        ctx = P.Context(P.make_config(env_kind=P.ENV_SYNTHETIC, dist_kind=P.DIST_MASKED, obs_size=obs_dim, head_dims=heads, hidden=64, n_hidden=2, num_envs=8, num_steps=4,
                                      num_minibatches=1, update_epochs=1, compute_dtype=dtype))
        assert ctx.P == g["params"].size
        ctx.set_params(g["params"])
        a, lp, en, v = ctx.policy_act(g["x"], mask=g["mask"].astype(np.uint8), action=g["action_hn"].T)
        assert np.array_equal(a, g["action_out"])
        np.testing.assert_allclose(lp, g["logprob"], rtol=1e-5 if dtype == 0 else 0, atol=tol)
        np.testing.assert_allclose(en, g["entropy"], rtol=1e-5 if dtype == 0 else 0, atol=tol)
        np.testing.assert_allclose(v, g["value"].ravel(), rtol=1e-5 if dtype == 0 else 0, atol=tol)
        if dtype == 1:
            print("bf16 against the reference's multi-head agent: log-prob %.1e, entropy %.1e, value %.1e (max abs)" %
                  (np.abs(lp - g["logprob"]).max(), np.abs(en - g["entropy"]).max(), np.abs(v - g["value"].ravel()).max()))
        ctx.close()


@pytest.mark.parametrize("envs,steps", [(64, 32), (50, 18)])   # 512-row minibatches (whole 64-row tiles) and 225-row ones (a partial tile at the end of every pass)
def test_generic_bf16_step_forms_agree(P, envs, steps):
    """The bf16-storage minibatch step exists in three forms that must compute the same update: the default (rows read in place through the permutation, both
    nets in every launch on one stream, ONE optimizer launch that takes the gradient norm from the slab sums' partial sums of squares and refreshes the bf16
    weight planes itself; heads, loss and the head layers' backward in the forward launch's epilogue), PPO_KERNEL_GENERIC_SPLIT_HEAD (the same with the loss and the
    head layers' backward as launches of their own), PPO_KERNEL_GENERIC_CLASSIC (gathered copies, one net per launch on two streams, loss sums / norm / AdamW / planes as four launches)
    and the multi-rank form driven on one GPU by PPO_KERNEL_COMM_SELFTEST (paired launches, the loss sums riding the gradient's all-reduce, norm kernel).
    Same product kernels and the same partition of every partial sum: after a whole iteration (eight optimizer steps) at a shape the fused kernels take (hidden 256, obs padded
    to 128-column blocks) the parameters agree to float rounding -- the one thing that differs is the ORDER in which the norm's partial sums are added."""
    kw = dict(env_kind=P.ENV_SYNTHETIC, dist_kind=P.DIST_MASKED, obs_size=376, head_dims=(3, 3, 3, 2), hidden=256, n_hidden=4, num_envs=envs, num_steps=steps,
              num_minibatches=4, update_epochs=2, max_episode_steps=50, seed=21, total_timesteps=envs * steps * 4, learning_rate=3e-4, ent_coef=0.01,
              compute_dtype=P.DTYPE_BF16)
    got = {}
    for name, flags, comm in (("default", 0, False), ("classic", P.KERNEL_GENERIC_CLASSIC, False), ("multi-rank path", P.KERNEL_COMM_SELFTEST, True),
                              ("split head", P.KERNEL_GENERIC_SPLIT_HEAD, False)):
        ctx = P.Context(P.make_config(kernel_flags=flags, **kw))
        if comm:
            ctx.comm_init(P.comm_unique_id(), 0, 1)
        ctx.init_orthogonal(5)
        ctx.env_reset()
        ctx.train_iteration()   # ONE iteration: the rollout is the same kernel on the same parameters in all three; a second one would sample from parameters a rounding apart
        st = ctx.stats()
        got[name] = (ctx.get_params(), st["loss"], st["approx_kl"], ctx.read("LOGPROBS"))
        assert np.isfinite(got[name][0]).all() and st["optimizer_steps"] == 8, name
        ctx.close()
    p0 = got["default"][0]
    scale = np.abs(p0).max()
    for name in ("classic", "multi-rank path", "split head"):
        p1 = got[name][0]
        assert np.abs(p1 - p0).max() <= 2e-6 * scale, (name, np.abs(p1 - p0).max(), scale)
        assert abs(got[name][1] - got["default"][1]) <= 1e-5 * max(1.0, abs(got["default"][1])), name
        assert np.array_equal(bits(got[name][3]), bits(got["default"][3])), name   # the rollout's log-probs: the same launch



@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("heads,hidden,n_hidden", [((3, 3, 3, 2), 256, 4), ((4,), 128, 1), ((2, 4, 1), 256, 3)])
def test_fused_head_epilogue_equals_the_split_launches(P, masked, heads, hidden, n_hidden):
    """Heads + masked categorical + PPO loss + the head layers' backward run in the forward launch's epilogue on the tile still in LDS (kernels_generic_fused.hip:
    FusedLossArgs; the default where the shape allows) or as launches of their own behind a forward pass that writes logits, values and the top activation to memory
    (PPO_KERNEL_GENERIC_SPLIT_HEAD: loss_lanes_kernel + bwd_layer_kernel<1, ...>).  Same arithmetic -- the same bf16 roundings of d logits, h and W_head, f32
    accumulation -- and different partitions of the partial sums (per forward workgroup / per row range): on the SAME batch and parameters the whole gradient, the loss
    scalars and the gradient norm agree to f32 summation order.  Index lists: whole tiles, a ragged last tile, fewer rows than one tile, two rows; depths with the top
    activation in either LDS tile (n_hidden odd / even)."""
    kw = dict(env_kind=P.ENV_SYNTHETIC, dist_kind=P.DIST_MASKED if masked else P.DIST_CATEGORICAL, obs_size=120, head_dims=heads, hidden=hidden, n_hidden=n_hidden,
              num_envs=48, num_steps=24, num_minibatches=2, update_epochs=1, max_episode_steps=30, seed=13, learning_rate=3e-4, ent_coef=0.01, compute_dtype=P.DTYPE_BF16)
    ctxs = [P.Context(P.make_config(kernel_flags=f, **kw)) for f in (0, P.KERNEL_GENERIC_SPLIT_HEAD)]
    ctxs[0].init_orthogonal(4)
    params = ctxs[0].get_params()
    rng = np.random.default_rng(3)
    params = (params + 0.02 * rng.standard_normal(params.shape)).astype(np.float32)   # biases away from zero
    for c in ctxs:
        c.set_params(params)
        c.env_reset()
        c.rollout()
        c.calc_advantage()
    B = 48 * 24
    assert np.array_equal(bits(ctxs[0].read("ADVANTAGES")), bits(ctxs[1].read("ADVANTAGES")))
    for M in (576, 512, 225, 40, 2):   # (the workspace holds one minibatch: B / 2 rows)
        idx = rng.permutation(B)[:M].astype(np.int32)
        g = [c.minibatch_forward_backward(idx) for c in ctxs]
        st = [c.stats() for c in ctxs]
        scale = np.abs(g[1]).max()
        assert scale > 0 and np.isfinite(g[0]).all()
        assert np.abs(g[0] - g[1]).max() <= 2e-5 * scale, (M, float(np.abs(g[0] - g[1]).max()), float(scale))
        for key in ("pg_loss", "v_loss", "entropy_loss", "approx_kl", "clipfrac_last", "total_norm"):
            assert abs(st[0][key] - st[1][key]) <= 2e-6 * max(1.0, abs(st[1][key])), (M, key, st[0][key], st[1][key])
    for c in ctxs:
        c.close()
