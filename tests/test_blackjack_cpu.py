"""The yardstick of tests/test_gpu_blackjack.py, checked on the CPU: the numpy model of the header's Blackjack statement (tests/blackjack_model.py) against
facts that follow from the rules of gymnasium's Blackjack-v1 (natural = False, sab = False, the infinite deck [1..10, 10, 10, 10]) alone.  The quoted values
were computed with exact rational arithmetic and are quoted to seven decimals; the model's dynamic programme, rational too, must reproduce them to 1e-9
beyond the rounding of the quotation -- half a unit of the seventh decimal, 5e-8: the exact values are -0.046555977067, -0.395895992849, 1.375574980722 and
-0.186367666215, which round to the quoted digits and lie 2.3e-8, 7.2e-9, 1.9e-8 and 3.4e-8 from them, so 1e-9 alone against seven decimals cannot be met by
any correct programme.  The statistical bar is 5 standard errors of the sampled mean.

The learning test of tests/test_gpu_blackjack.py quotes its ceiling and its floor from here: the optimum -0.0465560 and the random policy's -0.3958960."""
from fractions import Fraction

import numpy as np
import pytest

import blackjack_model as M

QUOTED = 5e-8 + 1e-9   # a value quoted to seven decimals


@pytest.fixture(scope="module")
def O():
    import oracle   # Philox
    oracle.build()
    return oracle


def test_card_buckets_at_their_exact_word_boundaries():
    """thirteen equal buckets of a 32-bit word: bucket b starts at ceil(b * 2^32 / 13); buckets 0..8 are 1..9 (once each), 9..12 are tens (four)"""
    starts = [-((-b << 32) // 13) for b in range(14)]
    assert starts[0] == 0 and starts[13] == 1 << 32
    want = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10, 10, 10]
    assert tuple(want) == M.DECK
    for b in range(13):
        lo, hi = starts[b], starts[b + 1] - 1
        assert M.card(np.array([lo, hi], np.uint64)).tolist() == [want[b], want[b]]
        if b:
            assert M.card(np.array([lo - 1], np.uint64))[0] == want[b - 1]
        assert (int(lo) * 13) >> 32 == b and (int(hi) * 13) >> 32 == b
    c = M.card(np.array([s for s in starts[:13]], np.uint64))
    assert np.bincount(c, minlength=11).tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 4]
    assert M.card(np.array([0xFFFFFFFF], np.uint64))[0] == 10


def test_pack_unpack_and_clamp():
    for t in (2, 11, 21, 31):
        for ace in (0, 1):
            for show in (1, 5, 10):
                h = int(M.pack(t, ace, show))
                assert 0 <= h <= M.HAND_MAX and tuple(int(x) for x in M.unpack(h)) == (t, ace, show)
    assert int(M.pack(31, 1, 10)) == M.HAND_MAX == 703
    assert int(M.hand_sum(11, 1)) == 21 and int(M.hand_sum(12, 1)) == 12 and int(M.hand_sum(11, 0)) == 11 and int(M.usable(11, 1)) == 1
    foreign = M.clamp(np.array([[np.nan, -3.0, 708.0, 2.0 ** 25], [2.0 ** 25, np.nan, -3.0, 708.0], [0.0, 1.5, 3.99, 0.0], [65.9, 4.0, 1.0, 2.0], [33.0, 0, 0, 0]]))
    assert foreign.tolist() == [[int(M.pack(2, 0, 1)), 0, 708, M.WORD_MAX], [703, 0, 0, 708], [int(M.pack(2, 0, 1)), 1, 3, 0], [int(M.pack(2, 0, 1)), 4, 1, 2],
                                [int(M.pack(2, 1, 1)), 0, 0, 0]]


def test_the_dynamic_programme_reproduces_the_quoted_values():
    opt = M.from_the_deal(lambda t, ace, show: M.optimal(t, ace, show)[0])
    assert abs(float(opt) - (-0.0465560)) < QUOTED, float(opt)
    v_rand, l_rand = M.policy_value(lambda t, ace, show: Fraction(1, 2))
    assert abs(float(M.from_the_deal(v_rand)) - (-0.3958960)) < QUOTED, float(M.from_the_deal(v_rand))
    assert abs(float(M.from_the_deal(l_rand)) - 1.3755750) < QUOTED, float(M.from_the_deal(l_rand))
    v_stick, l_stick = M.policy_value(lambda t, ace, show: 0)
    assert abs(float(M.from_the_deal(v_stick)) - (-0.1863677)) < QUOTED, float(M.from_the_deal(v_stick))
    assert M.from_the_deal(l_stick) == 1
    # the optimum is one: no policy beats it, and the greedy policy of `optimal` attains it
    v_greedy, _ = M.policy_value(lambda t, ace, show: M.optimal(t, ace, show)[1])
    assert M.from_the_deal(v_greedy) == opt and opt > M.from_the_deal(v_stick) > M.from_the_deal(v_rand)


def test_dealer_and_episode_bounds():
    """the dealer draws at most 10 cards from any of the 100 two-card starts (and 10 is met); an episode takes at most 20 steps"""
    most = max(M.dealer_max_draws(s + h, s == 1 or h == 1) for s in range(1, 11) for h in range(1, 11))
    assert most == 10 == M.DEALER_DRAWS
    assert M.dealer_max_draws(2, True) == 10                      # A, A, then 1 1 1 1 6 1 1 1 1 1
    assert M.dealer_play(1, 1, [1, 1, 1, 1, 6, 1, 1, 1, 1, 1]) == (17, 10)
    assert M.dealer_play(10, 7, []) == (17, 0) and M.dealer_play(1, 6, []) == (17, 0) and M.dealer_play(10, 6, [10]) == (0, 1)
    for s in range(1, 11):
        for h in range(1, 11):
            d = M.dealer_scores(s + h, s == 1 or h == 1)
            assert sum(d.values()) == 1 and set(d) <= {0, 17, 18, 19, 20, 21}
    assert M.longest_episode() == 20


def test_the_optimal_policy_is_the_known_basic_strategy():
    act = lambda t, ace, show: M.optimal(t, ace, show)[1]   # noqa: E731
    # no usable ace: 12 sticks against 4, 5, 6 and hits against 2, 3
    assert [act(12, 0, s) for s in (4, 5, 6)] == [0, 0, 0] and [act(12, 0, s) for s in (2, 3)] == [1, 1]
    # a usable ace (t = 8 with an ace is a soft 18): hits against 9, 10, A and sticks against 2..8
    assert [act(8, 1, s) for s in (9, 10, 1)] == [1, 1, 1] and [act(8, 1, s) for s in range(2, 9)] == [0] * 7
    # and the obvious: 11 and less always hits, hard 17 and more always sticks
    assert all(act(t, 0, s) == 1 for t in range(4, 12) for s in range(1, 11))
    assert all(act(t, 0, s) == 0 for t in range(17, 22) for s in range(1, 11))


def test_step_equals_step_c_under_the_keys_cards_and_bookkeeping(O):
    keys = ((0, 0), (123456, 654321))
    rows = np.array([(int(M.pack(t, ace, show)), n, k0, k1) for (k0, k1) in keys for n in (4, 6, 7, 9) for t in (2, 12, 16, 21, 25) for ace in (0, 1)
                     for show in (1, 6, 10)], np.int64)
    for a in (0, 1):
        act = np.full(len(rows), a)
        ns, r, term, drew = M.step(O, rows, act, with_draws=True)
        cards = np.array([[int(M.card(M.deck_words(O, k0, k1, 3, 1))[0])] + M.card(M.deck_words(O, k0, k1, n, 10)).tolist() for (_, n, k0, k1) in rows.tolist()])
        for x, y in zip((ns, r, term, drew), M.step_c(rows, act, cards)):
            assert np.array_equal(x, y)
        t, ace, show = M.unpack(rows[:, 0])
        nt, nace, nshow = M.unpack(ns[:, 0])
        bust = t > 21
        assert np.array_equal(ns[:, 2:], rows[:, 2:]) and np.array_equal(nshow, show)              # the key and the showing card stay
        assert np.array_equal(ns[bust], rows[bust]) and (r[bust] == -1).all() and (term[bust] == 1).all()
        assert np.isin(r, (-1, 0, 1)).all()
        if a == 1:
            c = cards[:, 1]
            assert np.array_equal(nt[~bust], (t + c)[~bust]) and np.array_equal(nace[~bust], (ace | (c == 1))[~bust])
            assert np.array_equal(ns[~bust, 1], rows[~bust, 1] + 1) and np.array_equal(term[~bust], (nt[~bust] > 21).astype(np.int64))
            assert np.array_equal(r[~bust], -(nt[~bust] > 21).astype(np.int64))
        else:
            assert (term == 1).all() and np.array_equal(ns[:, 0], rows[:, 0]) and np.array_equal(ns[:, 1], rows[:, 1] + drew) and (drew[bust] == 0).all()
            assert (drew <= 10).all()
    # card i is word i & 3 of the call with counter i >> 2
    w0, w1 = O.philox4x32(123456, 654321, 0, 0, 0, 0x21), O.philox4x32(123456, 654321, 1, 0, 0, 0x21)
    assert M.deck_words(O, 123456, 654321, 2, 4).tolist() == [w0[2], w0[3], w1[0], w1[1]]
    # n is held at 2^24 - 1; actions outside 0..1 are clamped
    top = np.array([[int(M.pack(12, 0, 2)), M.WORD_MAX, 5, 6], [int(M.pack(12, 0, 2)), M.WORD_MAX - 1, 5, 6]], np.int64)
    ns, _, _, drew = M.step(O, top, [0, 0], with_draws=True)
    assert (ns[:, 1] == np.minimum(top[:, 1] + drew, M.WORD_MAX)).all() and (ns[:, 1] <= M.WORD_MAX).all()
    assert (M.step(O, top, [1, 1])[0][:, 1] == M.WORD_MAX).all()
    for bad, a in ((-1, 0), (7, 1), (1 << 40, 1)):
        for x, y in zip(M.step(O, rows, np.full(len(rows), bad)), M.step(O, rows, np.full(len(rows), a))):
            assert np.array_equal(x, y)
    ob = M.obs(rows)
    t, ace, show = M.unpack(rows[:, 0])
    assert ob.shape == (len(rows), 45) and ob.dtype == np.float32 and (ob.sum(axis=1) == 3).all()
    assert np.array_equal(ob[:, :32].argmax(axis=1), M.hand_sum(t, ace)) and np.array_equal(ob[:, 32:43].argmax(axis=1), show)
    assert np.array_equal(ob[:, 43:].argmax(axis=1), M.usable(t, ace)) and (ob[:, 32] == 0).all()


def test_the_reset_map_on_the_oracles_words(O):
    seed = (7 << 32) | 5
    envs, ks = [0, 1, 2, 69, 1000], [1, 0, 3, 0, 2]
    got = M.reset_states(O, seed, envs, ks)
    for row, e, k in zip(got.tolist(), envs, ks):
        w = O.philox4x32(5, 7, e, k, 0, 1)
        c = M.card(np.array(O.philox4x32(w[0] >> 8, w[1] >> 8, 0, 0, 0, 0x21), np.uint64)).tolist()
        assert row == [c[0] + c[1] + 32 * (1 in c[:2]) + 64 * c[2], 4, w[0] >> 8, w[1] >> 8]
    assert M.deal(1, 2, np.array([0, 0, 0xFFFFFFFF, 7], np.uint64)) == [2 + 32 + 640, 4, 1, 2]


def test_random_play_on_philox_cards_meets_the_dynamic_programme(O):
    """20 000 episodes dealt and played by the model's step on Philox cards, a fair coin per step: the mean return within 5 standard errors of the DP's
    -0.3958960, and the mean length of 1.3755750"""
    n = 20000
    rng = np.random.default_rng(3)
    k = np.arange(n, dtype=np.int64)
    keys = np.stack([(k * 255 + 17) & M.WORD_MAX, (k * 40503 + 5) & M.WORD_MAX], 1)
    calls = {}

    def card_at(e, i):
        if (e, i >> 2) not in calls:
            calls[(e, i >> 2)] = M.card(np.array(O.philox4x32(int(keys[e, 0]), int(keys[e, 1]), i >> 2, 0, 0, M.CARD_TAG), np.uint64))
        return int(calls[(e, i >> 2)][i & 3])
    st = np.array([M.deal(keys[e, 0], keys[e, 1], O.philox4x32(int(keys[e, 0]), int(keys[e, 1]), 0, 0, 0, M.CARD_TAG)) for e in range(n)], np.int64)
    ret, length, alive = np.zeros(n), np.zeros(n), np.ones(n, bool)
    probe = None
    for _ in range(20):
        idx = np.flatnonzero(alive)
        if idx.size == 0:
            break
        act = rng.integers(0, 2, idx.size)
        cards = np.array([[card_at(e, 3)] + [card_at(e, int(st[e, 1]) + d) for d in range(10)] for e in idx])
        ns, r, term, _ = M.step_c(st[idx], act, cards)
        if probe is None:   # step draws the same cards itself
            probe = M.step(O, st[idx[:200]], act[:200])
            assert np.array_equal(probe[0], ns[:200]) and np.array_equal(probe[1], r[:200])
        st[idx] = ns
        ret[idx] += r
        length[idx] += 1
        alive[idx] = term == 0
    assert not alive.any()
    se = ret.std(ddof=1) / np.sqrt(n)
    print("random play: mean return %.4f (DP -0.3958960, 5 s.e. = %.4f), mean length %.4f (DP 1.3755750)" % (ret.mean(), 5 * se, length.mean()))
    assert abs(ret.mean() - (-0.3958960)) <= 5 * se
    assert abs(length.mean() - 1.3755750) <= 5 * length.std(ddof=1) / np.sqrt(n)
