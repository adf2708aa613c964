"""The Taxi env of include/ppo_hip.h (PPO_ENV_TAXI), once, in numpy: the header's table, integers throughout.  The yardstick of tests/test_gpu_taxi.py;
tests/test_taxi_cpu.py checks it against the facts gymnasium documents for Taxi-v3.

State rows are (row, col, pass, dest): row, col in 0..4, pass in 0..4 (0..3 waiting at R, G, Y, B; 4 in the taxi), dest in 0..3."""
from collections import deque

import numpy as np

STANDS = ((0, 0), (0, 4), (4, 0), (4, 3))   # R, G, Y, B as (row, col)
N_ACTIONS, OBS = 6, 19
HI = np.array([4, 4, 4, 3])


def all_states():
    """the 500 states, dest fastest"""
    return np.array([(r, c, p, d) for r in range(5) for c in range(5) for p in range(5) for d in range(4)], np.int64)


def east_blocked(r, c):
    r, c = np.asarray(r), np.asarray(c)
    return (c == 4) | ((r <= 1) & (c == 1)) | ((r >= 3) & ((c == 0) | (c == 2)))


def west_blocked(r, c):
    r, c = np.asarray(r), np.asarray(c)
    return (c == 0) | east_blocked(r, c - 1)


def stand_at(r, c):
    """the stand the taxi is on, or -1"""
    r, c = np.asarray(r), np.asarray(c)
    out = np.full(r.shape, -1, np.int64)
    for s, (sr, sc) in enumerate(STANDS):
        out[(r == sr) & (c == sc)] = s
    return out


def step(state, action):
    """state i [n,4], action i [n] (clamped into 0..5) -> (next state [n,4], reward [n], terminated [n])"""
    s = np.array(state, np.int64).reshape(-1, 4)
    a = np.clip(np.asarray(action, np.int64).reshape(-1), 0, 5)
    r, c, p, d = (s[:, k].copy() for k in range(4))
    on = stand_at(r, c)
    rew = np.full(r.shape, -1, np.int64)
    term = np.zeros(r.shape, np.int64)
    m = a == 0
    r[m] = np.minimum(r[m] + 1, 4)
    m = a == 1
    r[m] = np.maximum(r[m] - 1, 0)
    m = (a == 2) & ~east_blocked(s[:, 0], s[:, 1])
    c[m] += 1
    m = (a == 3) & ~west_blocked(s[:, 0], s[:, 1])
    c[m] -= 1
    pick = (a == 4) & (p < 4) & (on == p)
    rew[(a == 4) & ~pick] = -10
    deliver = (a == 5) & (p == 4) & (on == d)
    put = (a == 5) & (p == 4) & (on >= 0) & ~deliver
    rew[(a == 5) & ~deliver & ~put] = -10
    p[pick] = 4
    p[deliver] = d[deliver]
    term[deliver] = 1
    rew[deliver] = 20
    p[put] = on[put]
    return np.stack([r, c, p, d], 1), rew, term


def mask(state):
    """u8 [n,6]: [row < 4, row > 0, !east_blocked, !west_blocked, pass < 4 and on stand pass, pass == 4 and on a stand]"""
    s = np.asarray(state, np.int64).reshape(-1, 4)
    r, c, p = s[:, 0], s[:, 1], s[:, 2]
    on = stand_at(r, c)
    return np.stack([r < 4, r > 0, ~east_blocked(r, c), ~west_blocked(r, c), (p < 4) & (on == p), (p == 4) & (on >= 0)], 1).astype(np.uint8)


def obs(state):
    """f32 [n,19]: four one-hot groups -- row [0..4], col [5..9], pass [10..14], dest [15..18]"""
    s = np.asarray(state, np.int64).reshape(-1, 4)
    out = np.zeros((s.shape[0], OBS), np.float32)
    n = np.arange(s.shape[0])
    for g, lo in enumerate((0, 5, 10, 15)):
        out[n, lo + s[:, g]] = 1.0
    return out


def state_of(ob):
    """the state behind an observation: the index of the largest entry of each group, the first on ties"""
    ob = np.asarray(ob).reshape(-1, OBS)
    return np.stack([np.argmax(ob[:, lo:hi], axis=1) for lo, hi in ((0, 5), (5, 10), (10, 15), (15, 19))], 1).astype(np.int64)


def reset(words):
    """Philox words u32 [n,4] (x, y, z, w) -> start states [n,4]: cell = (x * 25) >> 32, pass = (y * 4) >> 32, d = (z * 3) >> 32, dest = d + (d >= pass)"""
    w = np.asarray(words, np.uint64).reshape(-1, 4)
    cell = (w[:, 0] * np.uint64(25)) >> np.uint64(32)
    p = (w[:, 1] * np.uint64(4)) >> np.uint64(32)
    d = (w[:, 2] * np.uint64(3)) >> np.uint64(32)
    return np.stack([cell // np.uint64(5), cell % np.uint64(5), p, d + (d >= p).astype(np.uint64)], 1).astype(np.int64)


def start_states():
    """gymnasium's 300: the passenger waits, and not at the destination"""
    s = all_states()
    return s[(s[:, 2] < 4) & (s[:, 2] != s[:, 3])]


def key(s):
    s = np.asarray(s, np.int64)
    return ((s[..., 0] * 5 + s[..., 1]) * 5 + s[..., 2]) * 4 + s[..., 3]


def bfs(starts):
    """Breadth-first search over the model from `starts`: (set of reachable non-terminal keys, set of terminal keys entered, distance to delivery per start).
    A terminal state is one entered by a delivering dropoff; it is not expanded."""
    S = all_states()
    nxt = np.zeros((500, 6), np.int64)
    trm = np.zeros((500, 6), np.int64)
    for a in range(6):
        ns, _, t = step(S, np.full(500, a))
        nxt[:, a], trm[:, a] = key(ns), t
    seen, terminal = set(), set()
    q = deque()
    for k in key(starts).tolist():
        if k not in seen:
            seen.add(k)
            q.append(k)
    while q:
        k = q.popleft()
        for a in range(6):
            if trm[k, a]:
                terminal.add(int(nxt[k, a]))
            elif int(nxt[k, a]) not in seen:
                seen.add(int(nxt[k, a]))
                q.append(int(nxt[k, a]))
    # steps to delivery from every state: backwards relaxation (500 states: a few sweeps)
    dist = np.full(500, 10 ** 6, np.int64)
    changed = True
    while changed:
        changed = False
        for a in range(6):
            cand = np.where(trm[:, a] == 1, 1, dist[nxt[:, a]] + 1)
            better = cand < dist
            if better.any():
                dist[better] = cand[better]
                changed = True
    return seen, terminal, dist[key(starts)]


def random_policy_returns(n_episodes, masked, seed, max_steps=200):
    """Returns of a uniformly random policy (over the allowed actions, or over all six) from uniformly drawn start states: (returns, truncated flags)."""
    rng = np.random.default_rng(seed)
    starts = start_states()
    s = starts[rng.integers(0, len(starts), n_episodes)]
    ret = np.zeros(n_episodes, np.int64)
    alive = np.ones(n_episodes, bool)
    trunc = np.zeros(n_episodes, bool)
    for t in range(max_steps):
        if masked:
            m = mask(s).astype(np.float64)
            cdf = np.cumsum(m / m.sum(1, keepdims=True), axis=1)
            a = (rng.random(n_episodes)[:, None] >= cdf).sum(1)
        else:
            a = rng.integers(0, 6, n_episodes)
        ns, r, term = step(s, a)
        ret[alive] += r[alive]
        s = np.where(alive[:, None], ns, s)
        alive &= term == 0
        if t == max_steps - 1:
            trunc = alive.copy()
    return ret, trunc
