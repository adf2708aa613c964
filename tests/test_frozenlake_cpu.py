"""The yardstick of tests/test_gpu_frozenlake.py, checked on the CPU: the numpy model of the header's FrozenLake statement (tests/frozenlake_model.py)
against what gymnasium documents for FrozenLake-v1 / FrozenLake8x8-v1 with is_slippery = True, and against numbers that follow from the maps by dynamic
programming.  The tolerances are those of the numbers quoted (1e-6; 1e-9 where the value is 1), the statistical bar is 5 sigma of a fair three-way draw.

The learning test of tests/test_gpu_frozenlake.py quotes its ceiling and its floor from here: the limit-100 optimum 0.7442 and the random policy's 0.0139."""
import numpy as np
import pytest

import frozenlake_model as M


@pytest.fixture(scope="module")
def O():
    import oracle   # Philox
    oracle.build()
    return oracle


def test_holes_and_goal_are_gymnasiums():
    assert M.holes(4) == [5, 7, 11, 12] and M.hole_mask(4) == 0x18a0 and M.goal(4) == 15
    assert M.holes(8) == [19, 29, 35, 41, 42, 46, 49, 52, 54, 59] and M.hole_mask(8) == 0x0852460820080000 and M.goal(8) == 63
    for side in (4, 8):
        flat = "".join(M.MAPS[side])
        assert len(flat) == side * side and flat[0] == "S" and flat.count("S") == 1 and flat.count("G") == 1 and set(flat) == {"S", "F", "H", "G"}
        assert M.terminal(side, np.arange(side * side)).sum() == len(M.holes(side)) + 1


@pytest.mark.parametrize("side", [4, 8])
def test_enumerating_the_slip_gives_gymnasiums_transition_matrix(side):
    """gym: under action a the agent moves in direction (a-1)%4, a or (a+1)%4, one third each; a move off the grid stays; entering the goal pays 1; holes and
    the goal end the episode.  Built here from gym's own increments (LEFT 0: col-1, DOWN 1: row+1, RIGHT 2: col+1, UP 3: row-1), not from the model's move."""
    S = side * side
    P, R = M.transition_matrix(side)
    assert np.allclose(P.sum(axis=2), 1.0, atol=1e-15)
    inc = {0: (0, -1), 1: (1, 0), 2: (0, 1), 3: (-1, 0)}
    flat = "".join(M.MAPS[side])
    for c in range(S):
        for a in range(4):
            want, rew = np.zeros(S), 0.0
            if flat[c] in "HG":
                want[c] = 1.0
            else:
                for b in ((a - 1) % 4, a, (a + 1) % 4):
                    row, col = divmod(c, side)
                    row, col = min(max(row + inc[b][0], 0), side - 1), min(max(col + inc[b][1], 0), side - 1)
                    want[row * side + col] += 1.0 / 3.0
                    rew += (flat[row * side + col] == "G") / 3.0
            assert np.allclose(P[c, a], want, atol=1e-15) and abs(R[c, a] - rew) < 1e-15, (c, a)
            assert set(np.round(P[c, a][P[c, a] > 0] * 3).astype(int).tolist()) <= {1, 2, 3}
    # d = 0, 1, 2 are (a-1)%4, a, (a+1)%4 in this order
    st = np.zeros((1, 4), np.int64)
    st[0, 0] = 2 * side + 1                               # (row 2, col 1): frozen on both maps, and every neighbour is inside the grid
    for a in range(4):
        for d in range(3):
            ns, _, _ = M.step_d(side, st, [a], [d])
            b = (a - 1 + d) % 4
            assert ns[0, 0] == (2 + inc[b][0]) * side + 1 + inc[b][1] and ns[0, 1] == 1


def test_the_dynamic_programme_reproduces_the_quoted_values():
    """From the maps alone: the optimal success probability from the start without and within the time limit (gym: 100 and 200 steps), and a uniformly random
    policy's success probability and mean episode length within it."""
    v4, v8 = M.optimal_success(4), M.optimal_success(8)
    assert abs(v4[0] - 14.0 / 17.0) < 1e-6 and abs(v4[0] - 0.8235294) < 1e-6
    assert abs(v8[0] - 1.0) < 1e-9
    assert abs(M.optimal_success(4, 100)[0] - 0.7441903) < 1e-6
    assert abs(M.optimal_success(8, 200)[0] - 0.9132202) < 1e-6
    s4, l4 = M.uniform_policy(4, 100)
    s8, l8 = M.uniform_policy(8, 200)
    assert abs(s4 - 0.0139398) < 1e-6 and abs(s8 - 0.0019014) < 1e-6
    assert abs(l4 - 7.6726) < 1e-4 and abs(l8 - 32.0720) < 1e-4          # quoted to four decimals


def test_slip_directions_are_fair(O):
    """65 536 distinct keys, j = 0 .. 3 (the four words of one Philox call per key): per j, each of the three directions is drawn within 5 sigma of one third
    of the time -- sigma = sqrt(n * 2 / 9) = 121 counts of 65 536 draws."""
    n = 65536
    sigma = np.sqrt(n * 2.0 / 9.0)
    assert 120 < sigma < 122
    k = np.arange(n, dtype=np.int64)
    keys = np.stack([(k * 255 + 17) & M.WORD_MAX, (k * 40503 + 5) & M.WORD_MAX], 1)      # odd multipliers mod 2^24: 65 536 distinct pairs
    assert len(set(map(tuple, keys.tolist()))) == n
    words = np.array([O.philox4x32(int(a), int(b), 0, 0, 0, M.SLIP_TAG) for a, b in keys], np.uint64)
    # slip_words picks the same words
    probe = np.array([[0, j, keys[i, 0], keys[i, 1]] for i in (0, 1, 4097) for j in range(4)], np.int64)
    assert np.array_equal(M.slip_words(O, probe), words[[0, 1, 4097]].reshape(-1))
    for j in range(4):
        counts = np.bincount(M.slip(words[:, j]), minlength=3)
        print("j = %d: %s (n / 3 = %.1f, 5 sigma = %.0f)" % (j, counts.tolist(), n / 3.0, 5 * sigma))
        assert counts.sum() == n and (np.abs(counts - n / 3.0) <= 5 * sigma).all(), (j, counts)
    # j >> 2 is the counter: j = 4 draws from another call than j = 0
    a = M.slip_words(O, np.array([[0, 0, 1, 2], [0, 4, 1, 2], [0, 3, 1, 2], [0, 7, 1, 2]], np.int64))
    assert a[0] == O.philox4x32(1, 2, 0, 0, 0, 0x20)[0] and a[1] == O.philox4x32(1, 2, 1, 0, 0, 0x20)[0]
    assert a[2] == O.philox4x32(1, 2, 0, 0, 0, 0x20)[3] and a[3] == O.philox4x32(1, 2, 1, 0, 0, 0x20)[3]


def test_slip_map_edges():
    assert M.slip(np.array([0, 0x55555555, 0x55555556, 0xAAAAAAAA, 0xAAAAAAAB, 0xFFFFFFFF], np.uint64)).tolist() == [0, 0, 1, 1, 2, 2]


@pytest.mark.parametrize("side", [4, 8])
def test_step_bookkeeping_clamps_and_terminal_cells(O, side):
    S = side * side
    st = np.array([[c, j, 77, 99] for c in range(S) for j in (0, 5, M.WORD_MAX)], np.int64)
    for a in range(4):
        ns, r, t = M.step(O, side, st, np.full(len(st), a))
        dead = M.terminal(side, st[:, 0])
        assert np.array_equal(ns[:, 2:], st[:, 2:])                                       # the key stays
        assert np.array_equal(ns[:, 1], np.minimum(st[:, 1] + 1, M.WORD_MAX))             # j counts, held at 2^24 - 1
        assert np.array_equal(ns[dead, 0], st[dead, 0]) and (r[dead] == 0).all() and (t[dead] == 1).all()
        assert np.array_equal(t[~dead] == 1, M.terminal(side, ns[~dead, 0])) and np.array_equal(r[~dead] == 1, ns[~dead, 0] == M.goal(side))
        assert ((ns[:, 0] >= 0) & (ns[:, 0] < S)).all()
    for bad, a in ((-1, 0), (7, 3), (1 << 40, 3)):                                        # actions outside 0..3 are clamped
        for x, y in zip(M.step(O, side, st, np.full(len(st), bad)), M.step(O, side, st, np.full(len(st), a))):
            assert np.array_equal(x, y)
    foreign = M.clamp(np.array([[np.nan, -3.0, S + 5.0, 2.0 ** 25], [2.0 ** 25, np.nan, -3.0, S + 5.0], [2.9, 1.5, 3.99, 0.0]]), side)
    assert foreign.tolist() == [[0, 0, S + 5, M.WORD_MAX], [S - 1, 0, 0, S + 5], [2, 1, 3, 0]]
    ob = M.obs(side, st)
    assert ob.shape == (len(st), S) and ob.dtype == np.float32 and (ob.sum(axis=1) == 1).all() and np.array_equal(ob.argmax(axis=1), st[:, 0])


def test_the_reset_map_on_the_oracles_words(O):
    seed = (7 << 32) | 5
    envs, ks = [0, 1, 2, 69, 1000], [1, 0, 3, 0, 2]
    got = M.reset_states(O, seed, envs, ks)
    for row, e, k in zip(got.tolist(), envs, ks):
        w = O.philox4x32(5, 7, e, k, 0, 1)
        assert row == [0, 0, w[0] >> 8, w[1] >> 8]
    assert ((got[:, 2:] >= 0) & (got[:, 2:] <= M.WORD_MAX)).all() and len(set(map(tuple, got[:, 2:].tolist()))) == len(envs)
    assert M.reset(np.array([[0xFFFFFFFF, 0x100, 1, 2]], np.uint64)).tolist() == [[0, 0, M.WORD_MAX, 1]]
