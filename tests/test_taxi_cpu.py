"""The yardstick of tests/test_gpu_taxi.py, checked on the CPU: the numpy model of the header's Taxi table (tests/taxi_model.py) against what gymnasium
documents for Taxi-v3 and what follows from the table by search.  Integers throughout: nothing here has a tolerance except the two simulated baselines,
whose bars are their own standard errors.

The learning test of tests/test_gpu_taxi.py takes its bar from here: the masked random policy's mean return and the optimum."""
import numpy as np
import pytest

import taxi_model as M


@pytest.fixture(scope="module")
def S():
    return M.all_states()


def test_a_mask_bit_is_set_exactly_when_the_action_changes_the_state(S):
    assert S.shape == (500, 4) and len(set(M.key(S).tolist())) == 500
    m = M.mask(S)
    assert m.shape == (500, 6) and m.dtype == np.uint8 and set(np.unique(m)) == {0, 1}
    for a in range(6):
        ns, rew, term = M.step(S, np.full(500, a))
        changed = (ns != S).any(axis=1)
        assert np.array_equal(changed, m[:, a] == 1), a
        assert ((ns >= 0) & (ns <= M.HI)).all()
        assert set(np.unique(rew)) <= {-1, -10, 20} and np.array_equal(rew == 20, term == 1)
        assert (rew[m[:, a] == 1] != -10).all()            # an allowed action is never an illegal pickup / dropoff
    assert (m.sum(axis=1) >= 1).all()                      # no mask is empty
    assert (m[:, 0] | m[:, 1]).all()                       # ... because south or north is always allowed
    assert m.sum(axis=0).tolist() == [400, 400, 280, 280, 16, 16] and m.sum() == 1392


def test_actions_outside_the_range_are_clamped(S):
    for bad, a in ((-3, 0), (6, 5), (1 << 40, 5)):
        for x, y in zip(M.step(S, np.full(500, bad)), M.step(S, np.full(500, a))):
            assert np.array_equal(x, y)


def test_walls_are_symmetric():
    r, c = np.divmod(np.arange(25), 5)
    east, west = M.east_blocked(r, c), M.west_blocked(r, c)
    assert east.sum() == west.sum() == 5 + 2 + 4           # the border column, the wall of rows 0..1, the two walls of rows 3..4
    inner = c < 4
    assert np.array_equal(east[inner], west[np.flatnonzero(inner) + 1])


def test_reachable_states_and_shortest_episodes():
    starts = M.start_states()
    assert starts.shape == (300, 4)
    seen, terminal, dist = M.bfs(starts)
    assert len(seen) == 400 and len(terminal) == 4 and len(seen | terminal) == 404   # gymnasium's documented 404
    assert dist.min() == 6 and dist.max() == 18 and abs(dist.mean() - 13.07) < 1e-9
    # an optimal episode of k steps returns 20 - (k - 1)
    assert int((21 - dist).sum()) == 2379
    print("optimal mean return", 2379 / 300)


def test_the_observation_holds_the_state(S):
    ob = M.obs(S)
    assert ob.shape == (500, 19) and ob.dtype == np.float32 and set(np.unique(ob)) == {0.0, 1.0} and (ob.sum(axis=1) == 4).all()
    assert np.array_equal(M.state_of(ob), S)
    assert np.array_equal(M.state_of(np.zeros((1, 19), np.float32)), [[0, 0, 0, 0]])   # ties: the first index


def test_the_reset_map_reaches_the_300_start_states_and_no_other():
    import oracle
    oracle.build()
    w = np.array([oracle.philox4x32(5, 0, 3, k, 0, 1) for k in range(1 << 16)], np.uint64)
    got = M.reset(w)
    assert set(M.key(got).tolist()) == set(M.key(M.start_states()).tolist())
    counts = np.bincount(M.key(got), minlength=500)[M.key(M.start_states())]
    print("visits per start state: %d .. %d of %.1f expected" % (counts.min(), counts.max(), (1 << 16) / 300))
    # the ends of the word range
    assert np.array_equal(M.reset([[0, 0, 0, 0]]), [[0, 0, 0, 1]]) and np.array_equal(M.reset([[0xFFFFFFFF] * 4]), [[4, 4, 3, 2]])


def test_random_policy_baselines():
    """4000 episodes each with a seeded generator.  The issue's figures (another generator): -186.7 (standard deviation 38.2, 86.5 % cut at 200) masked, -769.8
    unmasked.  Two samples of 4000 of the same distribution differ by less than 4 sqrt(2) standard errors."""
    ret, trunc = M.random_policy_returns(4000, True, 1)
    se = ret.std() / np.sqrt(4000)
    print("masked random policy: mean %.2f, std %.2f, truncated %.3f" % (ret.mean(), ret.std(), trunc.mean()))
    assert abs(ret.mean() - (-186.7)) <= 4 * np.sqrt(2) * se and abs(trunc.mean() - 0.865) <= 4 * np.sqrt(2) * np.sqrt(0.865 * 0.135 / 4000)
    ret_u, _ = M.random_policy_returns(4000, False, 1)
    se_u = ret_u.std() / np.sqrt(4000)
    print("unmasked random policy: mean %.2f, std %.2f" % (ret_u.mean(), ret_u.std()))
    assert abs(ret_u.mean() - (-769.8)) <= 4 * np.sqrt(2) * se_u
    # the bars of the learning test: the midpoint between the masked random policy and the optimum, and the random policy plus four standard errors at 512
    assert abs((-186.7 + 2379 / 300) / 2 - (-89.4)) < 0.05
    assert abs(-186.7 + 4 * 38.2 / np.sqrt(512) - (-179.9)) < 0.1
