"""The Blackjack env of include/ppo_hip.h (PPO_ENV_BLACKJACK: gymnasium's Blackjack-v1, natural = False, sab = False, the infinite deck), once, in numpy: the
header's statement, integers throughout.  The yardstick of tests/test_gpu_blackjack.py; tests/test_blackjack_cpu.py holds it to facts that follow from the
rules alone.  The Philox words come from oracle.philox4x32 (the caller passes the oracle module: it is built on first use).

State rows are (hand, n, k0, k1): hand = t + 32 * ace + 64 * show (t in 2..31 the player's total with aces as 1, ace in 0..1, show in 1..10), n the index of
the next card, (k0, k1) the episode's key, each of the three in 0..2^24-1.  Card i of an episode is card(w[i & 3]) of philox4x32_10(key = (k0, k1); counter =
(i >> 2, 0, 0, 0x21)): cards 0, 1 the player's, 2 the dealer's showing card, 3 the hidden one, 4.. whoever draws next."""
from fractions import Fraction
from functools import lru_cache

import numpy as np

N_ACTIONS = 2            # 0 stick, 1 hit
WORD_MAX = (1 << 24) - 1
HAND_MAX = 31 + 32 + 64 * 10
CARD_TAG = 0x21
DEALER_DRAWS = 10        # the most cards a dealer draws (dealer_max_draws())
OBS = 45
DECK = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10, 10, 10)   # gym's


def card(words):
    """min(1 + ((uint64(word) * 13) >> 32), 10)"""
    w = np.asarray(words, np.uint64)
    return np.minimum(1 + ((w * np.uint64(13)) >> np.uint64(32)).astype(np.int64), 10)


def pack(t, ace, show):
    return np.asarray(t, np.int64) + 32 * np.asarray(ace, np.int64) + 64 * np.asarray(show, np.int64)


def unpack(hand):
    h = np.asarray(hand, np.int64)
    return h & 31, (h >> 5) & 1, h >> 6


def usable(t, ace):
    return ((np.asarray(ace) == 1) & (np.asarray(t) + 10 <= 21)).astype(np.int64)


def hand_sum(t, ace):
    return np.asarray(t, np.int64) + 10 * usable(t, ace)


def clamp(state):
    """what every device function does first: each component converted (truncated towards zero) and clamped -- a NaN becomes 0; hand into 0..703, then t into
    2..31 and show into 1..10; n, k0, k1 into 0..2^24-1"""
    s = np.array(state, np.float64).reshape(-1, 4)
    s = np.where(np.isnan(s), 0.0, s)
    hi = np.array([HAND_MAX, WORD_MAX, WORD_MAX, WORD_MAX], np.float64)
    s = np.trunc(np.clip(s, 0.0, hi)).astype(np.int64)
    t, ace, show = unpack(s[:, 0])
    s[:, 0] = pack(np.maximum(t, 2), ace, np.maximum(show, 1))
    return s


def deck_words(O, k0, k1, first, count):
    """the words of cards first .. first + count - 1 of the episode with key (k0, k1): one Philox call per index >> 2"""
    out = []
    for b in range(first >> 2, ((first + count - 1) >> 2) + 1):
        out.extend(O.philox4x32(int(k0), int(k1), b, 0, 0, CARD_TAG))
    lo = first - ((first >> 2) << 2)
    return np.array(out[lo:lo + count], np.uint64)


def dealer_play(show, hidden, cards):
    """the dealer's play-out from (show, hidden) on the given cards, in order: (score -- 0 for a bust -- , cards drawn)"""
    dt, dace, k = show + hidden, show == 1 or hidden == 1, 0
    while dt + (10 if dace and dt + 10 <= 21 else 0) < 17:
        c = int(cards[k])
        k += 1
        dt += c
        dace = dace or c == 1
    return (0 if dt > 21 else dt + (10 if dace and dt + 10 <= 21 else 0)), k


def step_c(state, action, cards):
    """the step under GIVEN cards: cards [n, 1 + DEALER_DRAWS] -- column 0 is card 3 (the dealer's hidden card), columns 1.. are cards n, n + 1, ..  state
    i [n,4] in range, action clamped into 0..1 -> (next state [n,4], reward [n], terminated [n], cards the dealer drew [n])"""
    s = np.array(state, np.int64).reshape(-1, 4)
    a = np.clip(np.asarray(action, np.int64).reshape(-1), 0, 1)
    cards = np.asarray(cards, np.int64).reshape(s.shape[0], -1)
    ns, rew, term, drew = s.copy(), np.zeros(len(s), np.int64), np.ones(len(s), np.int64), np.zeros(len(s), np.int64)
    for i in range(len(s)):
        t, ace, show = (int(x) for x in unpack(s[i, 0]))
        n = int(s[i, 1])
        if t > 21:                                  # reachable through an injected state only: nothing is drawn, nothing changes
            rew[i] = -1
        elif a[i] == 1:
            c = int(cards[i, 1])
            t, ace = t + c, int(ace or c == 1)
            ns[i, 0], ns[i, 1] = pack(t, ace, show), min(n + 1, WORD_MAX)
            rew[i], term[i] = (-1, 1) if t > 21 else (0, 0)
        else:
            dealer, k = dealer_play(show, int(cards[i, 0]), cards[i, 1:])
            player = int(hand_sum(t, ace))
            rew[i] = (player > dealer) - (player < dealer)
            ns[i, 1], drew[i] = min(n + k, WORD_MAX), k
    return ns, rew, term, drew


def step_cards(O, state):
    """the cards each row's step may read: card 3 and cards n .. n + DEALER_DRAWS - 1 of the row's key"""
    s = np.asarray(state, np.int64).reshape(-1, 4)
    out = np.zeros((len(s), 1 + DEALER_DRAWS), np.int64)
    cache = {}
    for i, (_, n, k0, k1) in enumerate(s.tolist()):
        key = (n, k0, k1)
        if key not in cache:
            cache[key] = np.concatenate([card(deck_words(O, k0, k1, 3, 1)), card(deck_words(O, k0, k1, n, DEALER_DRAWS))])
        out[i] = cache[key]
    return out


def step(O, state, action, with_draws=False):
    """the env's step: the cards drawn from the state's own key at the state's own card index"""
    s = np.array(state, np.int64).reshape(-1, 4)
    ns, r, t, drew = step_c(s, action, step_cards(O, s))
    return (ns, r, t, drew) if with_draws else (ns, r, t)


def obs(state):
    """f32 [n, 45]: sum at [0..31], 32 + show at [32..42], 43 + usable at [43..44]"""
    s = np.asarray(state, np.int64).reshape(-1, 4)
    t, ace, show = unpack(s[:, 0])
    out = np.zeros((len(s), OBS), np.float32)
    r = np.arange(len(s))
    out[r, hand_sum(t, ace)] = 1.0
    out[r, 32 + show] = 1.0
    out[r, 43 + usable(t, ace)] = 1.0
    return out


def deal(k0, k1, words):
    """the start state of the episode with key (k0, k1) whose first Philox call gave `words` [4]"""
    c = card(words)
    return [int(pack(c[0] + c[1], int(c[0] == 1 or c[1] == 1), c[2])), 4, int(k0), int(k1)]


def reset(O, words):
    """Philox words u32 [n,4] (x, y, z, w) of philox4x32_10(seed; e, k, 0, 1) -> start states [n,4]: k0 = x >> 8, k1 = y >> 8, the deal from the key's call 0"""
    w = np.asarray(words, np.uint64).reshape(-1, 4)
    out = []
    for x, y in zip((w[:, 0] >> np.uint64(8)).tolist(), (w[:, 1] >> np.uint64(8)).tolist()):
        out.append(deal(x, y, np.array(O.philox4x32(int(x), int(y), 0, 0, 0, CARD_TAG), np.uint64)))
    return np.array(out, np.int64).reshape(-1, 4)


def reset_states(O, seed, envs, k):
    """reset number k[i] of global env envs[i] under `seed`"""
    w = [O.philox4x32(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, int(e), int(kk), 0, 1) for e, kk in zip(envs, k)]
    return reset(O, np.array(w, np.uint64))


# ---- the exact dynamic programme over (t, ace, show): rational arithmetic, the infinite deck ----
P_CARD = {c: Fraction(DECK.count(c), 13) for c in range(1, 11)}


@lru_cache(maxsize=None)
def dealer_scores(dt, dace):
    """the distribution {score: probability} of the dealer's final score from hard total dt with / without an ace"""
    if dt + (10 if dace and dt + 10 <= 21 else 0) >= 17:
        return {0 if dt > 21 else dt + (10 if dace and dt + 10 <= 21 else 0): Fraction(1)}
    out = {}
    for c, p in P_CARD.items():
        for sc, q in dealer_scores(dt + c, bool(dace or c == 1)).items():
            out[sc] = out.get(sc, Fraction(0)) + p * q
    return out


@lru_cache(maxsize=None)
def dealer_max_draws(dt, dace):
    if dt + (10 if dace and dt + 10 <= 21 else 0) >= 17:
        return 0
    return 1 + max(dealer_max_draws(dt + c, bool(dace or c == 1)) for c in range(1, 11))


@lru_cache(maxsize=None)
def stick_value(t, ace, show):
    """the expected reward of sticking: the hidden card, then the play-out"""
    player = t + (10 if ace and t + 10 <= 21 else 0)
    v = Fraction(0)
    for hid, p in P_CARD.items():
        for sc, q in dealer_scores(show + hid, show == 1 or hid == 1).items():
            v += p * q * ((player > sc) - (player < sc))
    return v


def policy_value(policy):
    """policy(t, ace, show) -> probability of hitting (a Fraction).  Returns (value(t, ace, show), length(t, ace, show)) as cached functions on live hands
    (t <= 21): the expected return and the expected number of steps from there."""
    @lru_cache(maxsize=None)
    def value(t, ace, show):
        ph = Fraction(policy(t, ace, show))
        hit = Fraction(0)
        if ph:
            for c, p in P_CARD.items():
                hit += p * (-1 if t + c > 21 else value(t + c, int(ace or c == 1), show))
        return (1 - ph) * stick_value(t, ace, show) + ph * hit

    @lru_cache(maxsize=None)
    def length(t, ace, show):
        ph = Fraction(policy(t, ace, show))
        more = Fraction(0)
        if ph:
            for c, p in P_CARD.items():
                more += p * (0 if t + c > 21 else length(t + c, int(ace or c == 1), show))
        return 1 + ph * more
    return value, length


@lru_cache(maxsize=None)
def optimal(t, ace, show):
    """(optimal value, optimal action -- 1 hit, 0 stick; a tie sticks) of a live hand"""
    hit = Fraction(0)
    for c, p in P_CARD.items():
        hit += p * (-1 if t + c > 21 else optimal(t + c, int(ace or c == 1), show)[0])
    st = stick_value(t, ace, show)
    return (hit, 1) if hit > st else (st, 0)


def from_the_deal(f):
    """the expectation of f(t, ace, show) over the deal: two cards for the player, one showing"""
    v = Fraction(0)
    for c0, p0 in P_CARD.items():
        for c1, p1 in P_CARD.items():
            for sh, p2 in P_CARD.items():
                v += p0 * p1 * p2 * f(c0 + c1, int(c0 == 1 or c1 == 1), sh)
    return v


def longest_episode():
    """the most steps an episode can take: hits that do not bust, then one last step"""
    @lru_cache(maxsize=None)
    def longest(t):
        return 1 + max((longest(t + c) for c in range(1, 11) if t + c <= 21), default=0)
    return max(longest(t) for t in range(2, 21))
