"""Plumbing of the kernels whose leading parameters are preloaded into SGPRs (csrc/Makefile: kernel-argument preloading; tests/test_kernarg_preload.py
holds the descriptors): the same values now reach the kernels as leading scalars in front of the argument struct, so a swapped or truncated leading
argument must fail HERE.  Smallest shapes that reach every instantiation and ragged edge: 33 envs x 5 steps (a ragged 16-env rollout tile), 3 minibatches of
55 rows (a ragged 32-row update tile) x 2 epochs, CartPole and masked MountainCar, the matrix-core and the vector kernels (kernel_flags), two iterations.
Checked against the C oracle (oracle/) at tests/test_gpu_parity.py's tolerances, never against the library's own other path; plus the existing contract
fused iteration == stepwise C-ABI sequence, bit for bit, and a clean error word (ppo_read_stats fails with PPO_ERR_STATE on a raised one).
reduce_grads_sumsq_kernel<true> (the direct exchange folded into the slab reduction) needs IPC handles of separate processes: tests/test_gpu_exchange.py
runs it; the two in-process ranks here run the all-reduce path beside the preloaded update kernel."""
import threading

import numpy as np
import pytest

import oracle as O
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

T, N, NMB, EPOCHS, LR = 5, 33, 3, 2, 1e-3
B, MB = T * N, T * N // NMB


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def P():
    return load_package()


def config(P, env, flags, **over):
    kw = dict(num_envs=N, num_steps=T, num_minibatches=NMB, update_epochs=EPOCHS, seed=5, total_timesteps=T * N * 8, anneal_lr=False,
              learning_rate=LR, max_episode_steps=4, kernel_flags=flags)   # 4-step episodes: resets and finished episodes inside 5 steps
    if env == "mountaincar":
        kw.update(env_kind=P.ENV_MOUNTAINCAR, dist_kind=P.DIST_MASKED, obs_size=2, head_dims=(3,))
    kw.update(over)
    return P.make_config(**kw)


def oracle_update(P, env, c, p, m, v, k):
    """The oracle's update on the batch and the permutations context c holds: (params, moments, optimizer step count, last step's scalars, the
    largest clipped gradient element of these steps)."""
    obs_n, act_n = (2, 3) if env == "mountaincar" else (4, 2)
    net = O.Net.make(obs_n, [act_n], dist_kind=O.DIST_MASKED if env == "mountaincar" else O.DIST_CATEGORICAL)
    hp = O.HParams(gamma=0.98, gae_lambda=0.95, clip_coef=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, norm_adv=1, clip_vloss=1)
    perm = c.read("PERM", (EPOCHS, B))
    mask = c.read("MASKS", (B, act_n)) if env == "mountaincar" else None
    batch = (c.read("OBS", (B, obs_n)), c.read("ACTIONS", (B,)).astype(np.float32), c.read("LOGPROBS"), c.read("ADVANTAGES"), c.read("RETURNS"),
             c.read("VALUES"))
    st, gmax = None, 0.0
    for e in range(EPOCHS):
        assert np.array_equal(np.sort(perm[e]), np.arange(B))
        for s in range(NMB):
            g, st = O.minibatch_grads(net, hp, p, *batch, perm[e, s * MB:(s + 1) * MB], b_mask=mask)
            g, total = O.clip_grad_norm(net, g, hp.max_grad_norm)
            st["total_norm"] = total
            gmax = max(gmax, float(np.abs(g).max()))
            k += 1
            p, m, v = O.adamw_step(p, g, m, v, LR, k)
    return p, m, v, k, st, gmax


@pytest.mark.parametrize("flags", ["0", "UPDATE_VECTOR", "UPDATE_ONE_WAVE", "ROLLOUT_VECTOR"])
@pytest.mark.parametrize("env", ["cartpole", "mountaincar"])
def test_two_iterations_match_the_oracle_and_the_stepwise_path(P, env, flags):
    kf = 0 if flags == "0" else getattr(P, "KERNEL_" + flags)
    a, b = P.Context(config(P, env, kf)), P.Context(config(P, env, kf))
    for c in (a, b):
        c.init_orthogonal(4)
        c.env_reset()
    p = b.get_params()
    m, v, k, gmax = np.zeros_like(p), np.zeros_like(p), 0, 0.0
    for it in range(2):
        a.train_iteration()
        b.rollout()
        adv, ret = b.calc_advantage()
        # GAE: bit-exact against the oracle on the rollout's own buffers (north_star; as smoke() and test_gpu_parity do)
        o_adv, o_ret = O.gae(b.read("REWARDS", (T, N)), b.read("VALUES", (T, N)), b.read("DONES", (T, N)), b.read("NEXT_VALUE"), b.read("NEXT_DONE"),
                             0.98, 0.95)
        assert np.array_equal(bits(adv), bits(o_adv)) and np.array_equal(bits(ret), bits(o_ret)), it
        b.update()
        p, m, v, k, st_ref, gm = oracle_update(P, env, b, p, m, v, k)
        gmax = max(gmax, gm)
        # fused iteration == stepwise sequence, bit for bit
        for name in ("ADVANTAGES", "RETURNS", "VALUES", "LOGPROBS", "EXP_AVG", "EXP_AVG_SQ"):
            assert np.array_equal(bits(a.read(name)), bits(b.read(name))), (it, name)
        assert np.array_equal(bits(a.get_params()), bits(b.get_params())), it
        # parameters and both moments against the oracle carried through the same steps.  test_gpu_parity: 2e-6 on the parameters of an update at
        # lr 1e-3; a gradient of an 85-row minibatch within 1e-6 + 1e-4 max|g| of the oracle's (test_ragged_minibatches).  exp_avg is a convex
        # combination of the gradients, so it carries at most that; exp_avg_sq of their squares, so at most 2 max|g| times that.
        dg = 1e-6 + 1e-4 * gmax
        assert np.abs(b.get_params() - p).max() <= 2e-6, it
        assert np.abs(b.read("EXP_AVG") - m).max() <= dg, it
        assert np.abs(b.read("EXP_AVG_SQ") - v).max() <= 2 * gmax * dg, it
        sa, sb = a.stats(), b.stats()   # a raised error word makes this read fail
        for key, n in (("pg_loss", "pg_loss"), ("v_loss", "v_loss"), ("entropy_loss", "entropy_loss"), ("approx_kl", "approx_kl"),
                       ("clipfrac_last", "clipfrac"), ("loss", "loss")):
            assert abs(sb[key] - st_ref[n]) <= 1e-5 * max(1.0, abs(st_ref[n])), (it, key, sb[key], st_ref[n])
            assert sa[key] == sb[key], (it, key)
        assert abs(sb["total_norm"] - st_ref["total_norm"]) <= 1e-5 * max(1.0, st_ref["total_norm"]), it
        assert sb["optimizer_steps"] == (it + 1) * EPOCHS * NMB
    a.close()
    b.close()


def test_two_in_process_ranks_match_the_oracle(P):
    """Two contexts on this device joined by ppo_comm_init_local, twice: one pair runs train_iteration(), its twin the stepwise sequence.  Each rank's update
    kernel gets the leading scalars (M, n_blocks, idx) of ITS shard; 16 envs x 5 steps in 3 minibatches leave a ragged 26-row update tile and a 2-row tail
    per rank.  Two iterations; per rank the advantages and returns bit-exact against the oracle's scan; parameters, both moments and the step scalars against
    the oracle's update on the CONCATENATED minibatches, at the single-rank case's tolerances; fused == stepwise and rank 0 == rank 1 bit for bit."""
    world, n, iters = 2, 16, 2
    bl, mb = T * n, T * n // NMB
    names = ("OBS", "ACTIONS", "LOGPROBS", "ADVANTAGES", "RETURNS", "VALUES")
    out, errors = {}, []

    def run(rank, fused):
        try:
            c = P.Context(P.dist.shard_config(P.make_config, rank, world, world * n, num_steps=T, num_minibatches=NMB, update_epochs=EPOCHS, seed=5,
                                              total_timesteps=T * world * n * 8, anneal_lr=False, learning_rate=LR, max_episode_steps=4))
            c.comm_init_local(4321 + int(fused), rank, world)
            c.init_orthogonal(4)
            c.env_reset()
            rec = [dict(params=c.get_params())]
            for _ in range(iters):
                if fused:
                    c.train_iteration()
                else:
                    c.rollout()
                    c.calc_advantage()
                    scan = {k: c.read(k, (T, n)) for k in ("REWARDS", "VALUES", "DONES", "ADVANTAGES", "RETURNS")}
                    scan.update(NEXT_VALUE=c.read("NEXT_VALUE"), NEXT_DONE=c.read("NEXT_DONE"))
                    c.update()
                st = c.stats()   # a raised error word makes this read fail
                rec.append(dict(params=c.get_params(), m=c.read("EXP_AVG"), v=c.read("EXP_AVG_SQ"), stats=st, perm=c.read("PERM", (EPOCHS, bl)),
                                batch={k: c.read(k) for k in names}, scan=None if fused else scan))
            out[(rank, fused)] = rec
            c.close()
        except Exception as ex:  # surface failures of the worker threads
            errors.append(ex)

    for f in (True, False):   # one pair after the other
        th = [threading.Thread(target=run, args=(r, f)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
    assert not errors, errors
    assert len(out) == 2 * world
    net = O.Net.make(4, [2])
    hp = O.HParams(gamma=0.98, gae_lambda=0.95, clip_coef=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, norm_adv=1, clip_vloss=1)
    step = out[(0, False)]
    p = step[0]["params"].copy()
    m, v, k, gmax = np.zeros_like(p), np.zeros_like(p), 0, 0.0
    for it in range(1, iters + 1):
        for r in range(world):
            # the scan of each rank's own shard: bit-exact against the oracle
            sc = out[(r, False)][it]["scan"]
            o_adv, o_ret = O.gae(sc["REWARDS"], sc["VALUES"], sc["DONES"], sc["NEXT_VALUE"], sc["NEXT_DONE"], 0.98, 0.95)
            assert np.array_equal(bits(sc["ADVANTAGES"]), bits(o_adv)) and np.array_equal(bits(sc["RETURNS"]), bits(o_ret)), (it, r)
            # fused == stepwise, and the replicas agree, bit for bit
            fu, sw = out[(r, True)][it], out[(r, False)][it]
            for key in ("params", "m", "v"):
                assert np.array_equal(bits(fu[key]), bits(sw[key])), (it, r, key)
                assert np.array_equal(bits(sw[key]), bits(step[it][key])), (it, r, key)
            for key in ("ADVANTAGES", "RETURNS", "VALUES", "LOGPROBS"):
                assert np.array_equal(bits(fu["batch"][key]), bits(sw["batch"][key])), (it, r, key)
        # the oracle on the global minibatches: rank r's rows perm_r[e, s * mb : (s + 1) * mb] of ITS batch, concatenated over the ranks
        cat = {key: np.concatenate([out[(r, False)][it]["batch"][key].reshape(bl, -1) for r in range(world)]) for key in names}
        st_ref = None
        for e in range(EPOCHS):
            for s in range(bl // mb + (1 if bl % mb else 0)):
                idx = np.concatenate([out[(r, False)][it]["perm"][e, s * mb:min((s + 1) * mb, bl)] + r * bl for r in range(world)])
                g, st_ref = O.minibatch_grads(net, hp, p, cat["OBS"], cat["ACTIONS"].ravel().astype(np.float32), cat["LOGPROBS"].ravel(),
                                              cat["ADVANTAGES"].ravel(), cat["RETURNS"].ravel(), cat["VALUES"].ravel(), idx)
                g, total = O.clip_grad_norm(net, g, hp.max_grad_norm)
                st_ref["total_norm"] = total
                gmax = max(gmax, float(np.abs(g).max()))
                k += 1
                p, m, v = O.adamw_step(p, g, m, v, LR, k)
        dg = 1e-6 + 1e-4 * gmax   # as in the single-rank case above
        assert np.abs(step[it]["params"] - p).max() <= 2e-6, it
        assert np.abs(step[it]["m"] - m).max() <= dg, it
        assert np.abs(step[it]["v"] - v).max() <= 2 * gmax * dg, it
        for r in range(world):
            sb, sa = out[(r, False)][it]["stats"], out[(r, True)][it]["stats"]
            for key, nm in (("pg_loss", "pg_loss"), ("v_loss", "v_loss"), ("entropy_loss", "entropy_loss"), ("approx_kl", "approx_kl"),
                            ("clipfrac_last", "clipfrac"), ("loss", "loss"), ("total_norm", "total_norm")):
                assert abs(sb[key] - st_ref[nm]) <= 1e-5 * max(1.0, abs(st_ref[nm])), (it, r, key, sb[key], st_ref[nm])
                assert sa[key] == sb[key], (it, r, key)
            assert sb["optimizer_steps"] == k
