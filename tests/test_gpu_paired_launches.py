"""The paired once-per-iteration launches (include/ppo_hip.h: PPO_KERNEL_SEPARATE_LAUNCHES; kernels_update_mfma.hip: values_ring_mfma_kernel = critic batch +
episode ring, pack_perm_stats_kernel = record pack + permutations / advantage sums + the normalisations) against the eight stand-alone launches the flag
selects, on ONE library: two contexts with the same config and seed, one with the flag, and everything an iteration leaves must be equal bit for bit --
parameters, both AdamW moments, PERM, VALUES, ADVANTAGES, RETURNS and every field of stats().

Shapes at which the new code can go wrong, not the workload's: 7 / 33 / 96 / 200 envs (a partial ballot group, one, several), 5 and 16 steps, 4-step episodes
(200 x 16 finishes far more than 100 episodes per rollout, so the ring's window wraps; 7 x 5 fewer than 100), num_minibatches 4 (33 x 5 = 165 rows: the
library cuts 165 // 4 = 41 rows four times and a tail of ONE row; 7 x 5: 8, 8, 8, 8, 3; every part shorter than one eight-deep loop, so only the tail loop
runs), a finite ragged case of its own (165 rows in 7), 2 epochs, CartPole and masked MountainCar, norm_adv off once (the update pair is not taken)."""
import threading

import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

BUFFERS = ("PERM", "VALUES", "ADVANTAGES", "RETURNS", "EXP_AVG", "EXP_AVG_SQ", "LOGPROBS", "NEXT_VALUE")


@pytest.fixture(scope="module")
def P():
    return load_package()


def config(P, env, n, t, flags, **over):
    kw = dict(num_envs=n, num_steps=t, num_minibatches=4, update_epochs=2, seed=11, total_timesteps=n * t * 64, anneal_lr=False, learning_rate=1e-3,
              max_episode_steps=4, kernel_flags=flags)
    if env == "mountaincar":
        kw.update(env_kind=P.ENV_MOUNTAINCAR, dist_kind=P.DIST_MASKED, obs_size=2, head_dims=(3,))
    kw.update(over)
    return P.make_config(**kw)


def context(P, env, n, t, flags, **over):
    c = P.Context(config(P, env, n, t, flags, **over))
    c.init_orthogonal(4)
    c.env_reset()
    return c


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def state(c):
    """Everything an iteration leaves, as bytes (a NaN equals itself); stats() last: it fails on a raised error word."""
    out = {"params": raw(c.get_params())}
    for name in BUFFERS:
        out[name] = raw(c.read(name))
    st = c.stats()
    for k, v in st.items():
        out["stats." + k] = raw(np.array([v]))
    return out, st


def assert_same(a, b, where):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (where, k)


@pytest.mark.parametrize("t", [5, 16])
@pytest.mark.parametrize("n", [7, 33, 96, 200])
@pytest.mark.parametrize("env", ["cartpole", "mountaincar"])
def test_three_iterations_equal_the_stand_alone_launches(P, env, n, t):
    a, b = context(P, env, n, t, 0), context(P, env, n, t, P.KERNEL_SEPARATE_LAUNCHES)
    count = 0
    for it in range(3):
        a.train_iteration()
        b.train_iteration()
        sa, st = state(a)
        sb, _ = state(b)
        assert_same(sa, sb, (env, n, t, it))
        count = st["ep_count"]
    # 4-step episodes: every env finishes one every 4 steps; ep_count is the ring's fill (at most 100)
    assert count == min(100, n * (3 * t // 4)), count
    a.close()
    b.close()


@pytest.mark.parametrize("env", ["cartpole", "mountaincar"])
def test_ragged_minibatches_with_a_short_tail_stay_finite_and_equal(P, env):
    """165 rows in 7 minibatches: the library cuts 165 // 7 = 23 rows each and a tail of 4, eight slots per epoch (165 in 4 gives 41-row minibatches and a tail of
    ONE row, whose Bessel variance is 0 / 0 as in the reference: equal above, but not finite)."""
    a, b = context(P, env, 33, 5, 0, num_minibatches=7), context(P, env, 33, 5, P.KERNEL_SEPARATE_LAUNCHES, num_minibatches=7)
    for it in range(3):
        a.train_iteration()
        b.train_iteration()
        assert_same(state(a)[0], state(b)[0], (env, it))
        assert np.isfinite(a.get_params()).all() and a.stats()["optimizer_steps"] == (it + 1) * 16
    a.close()
    b.close()


def test_without_norm_adv_the_update_pair_is_not_taken_and_results_are_equal(P):
    a, b = context(P, "cartpole", 33, 5, 0, norm_adv=False), context(P, "cartpole", 33, 5, P.KERNEL_SEPARATE_LAUNCHES, norm_adv=False)
    for it in range(3):
        a.train_iteration()
        b.train_iteration()
        assert_same(state(a)[0], state(b)[0], it)
    a.close()
    b.close()


@pytest.mark.parametrize("env,n,t", [("cartpole", 200, 16), ("mountaincar", 33, 5)])
def test_the_last_arriver_epilogues_are_deterministic(P, env, n, t):
    """Which workgroup draws the last ticket differs from run to run; what it leaves must not."""
    runs = []
    for _ in range(2):
        c = context(P, env, n, t, 0)
        rec = []
        for it in range(3):
            c.train_iteration()
            rec.append(state(c)[0])
        runs.append(rec)
        c.close()
    for it in range(3):
        assert_same(runs[0][it], runs[1][it], (env, it))


@pytest.mark.parametrize("env,n,t", [("cartpole", 200, 16), ("cartpole", 7, 5), ("mountaincar", 96, 16)])
def test_two_rollouts_with_no_statistics_read_in_between(P, env, n, t):
    """Stepwise use: the paired context pushes each rollout's episodes behind that rollout, the flagged one in front of the next rollout and of stats()."""
    a, b = context(P, env, n, t, 0), context(P, env, n, t, P.KERNEL_SEPARATE_LAUNCHES)
    for c in (a, b):
        c.rollout()
        c.rollout()
    sa, sb = a.stats(), b.stats()
    assert sa == sb, (sa, sb)
    assert sa["ep_count"] == min(100, n * (2 * t // 4))
    for name in ("VALUES", "NEXT_VALUE", "FIN_LEN", "FIN_REW"):
        assert np.array_equal(raw(a.read(name)), raw(b.read(name))), name
    for c in (a, b):   # ... and the update behind them
        c.calc_advantage()
        c.update()
    assert_same(state(a)[0], state(b)[0], "update")
    a.close()
    b.close()


def test_both_tickets_are_back_at_zero_after_an_iteration(P):
    """The binding reads no raw device word, so indirectly: a ticket left at k != 0 would make a later launch's last arriver come k workgroups early (or
    never), and the ring or the normalisations would differ from the stand-alone launches' within these ten further iterations."""
    a, b = context(P, "cartpole", 96, 16, 0), context(P, "cartpole", 96, 16, P.KERNEL_SEPARATE_LAUNCHES)
    for it in range(13):
        a.train_iteration()
        b.train_iteration()
        if it >= 3:
            assert_same(state(a)[0], state(b)[0], it)
    a.close()
    b.close()


def test_two_in_process_ranks_keep_the_all_reduce_and_the_separate_normalisation(P):
    """A sharded context takes the update pair without the folded normalisations (the sums are all-reduced first): equal to the flagged ranks bit for bit."""
    world, n, t = 2, 16, 5
    out, errors = {}, []

    def run(rank, flags):
        try:
            c = P.Context(P.dist.shard_config(P.make_config, rank, world, world * n, num_steps=t, num_minibatches=3, update_epochs=2, seed=5,
                                              total_timesteps=t * world * n * 8, anneal_lr=False, learning_rate=1e-3, max_episode_steps=4, kernel_flags=flags))
            c.comm_init_local(5321 + flags, rank, world)
            c.init_orthogonal(4)
            c.env_reset()
            rec = []
            for _ in range(2):
                c.train_iteration()
                rec.append(state(c)[0])
            out[(rank, flags)] = rec
            c.close()
        except Exception as ex:  # surface failures of the worker threads
            errors.append(ex)

    for f in (0, P.KERNEL_SEPARATE_LAUNCHES):
        th = [threading.Thread(target=run, args=(r, f)) for r in range(world)]
        for x in th:
            x.start()
        for x in th:
            x.join(timeout=120)
    assert not errors, errors
    assert len(out) == 2 * world
    for r in range(world):
        for it in range(2):
            assert_same(out[(r, 0)][it], out[(r, P.KERNEL_SEPARATE_LAUNCHES)][it], (r, it))
