"""The FrozenLake env of include/ppo_hip.h (PPO_ENV_FROZENLAKE, PPO_ENV_FROZENLAKE8X8: gymnasium's FrozenLake-v1 / FrozenLake8x8-v1, is_slippery = True),
once, in numpy: the header's statement, integers throughout.  The yardstick of tests/test_gpu_frozenlake.py; tests/test_frozenlake_cpu.py checks it against
the facts gymnasium documents.  The Philox words come from oracle.philox4x32 (the caller passes the oracle module: it is built on first use).

State rows are (cell, j, k0, k1): cell in 0..S-1 (row-major, S = side * side), j the steps taken in this episode, (k0, k1) the episode's key, each in
0..2^24-1.  The env's randomness rides in the state: a step's slip is a word of philox4x32_10(key = (k0, k1); counter = (j >> 2, 0, 0, 0x20))."""
import numpy as np

MAPS = {4: ("SFFF", "FHFH", "FFFH", "HFFG"),
        8: ("SFFFFFFF", "FFFFFFFF", "FFFHFFFF", "FFFFFHFF", "FFFHFFFF", "FHHFFFHF", "FHFFHFHF", "FFFHFFFG")}
N_ACTIONS = 4
WORD_MAX = (1 << 24) - 1
SLIP_TAG = 0x20


def cells(side):
    return side * side


def holes(side):
    return [i for i, ch in enumerate("".join(MAPS[side])) if ch == "H"]


def hole_mask(side):
    return sum(1 << c for c in holes(side))


def goal(side):
    return "".join(MAPS[side]).index("G")


def terminal(side, cell):
    cell = np.asarray(cell, np.int64)
    return np.isin(cell, holes(side)) | (cell == goal(side))


def clamp(state, side):
    """what every device function does first: each component converted (truncated towards zero) and clamped into its range; a NaN becomes 0"""
    s = np.array(state, np.float64).reshape(-1, 4)
    s = np.where(np.isnan(s), 0.0, s)
    hi = np.array([cells(side) - 1, WORD_MAX, WORD_MAX, WORD_MAX], np.float64)
    return np.trunc(np.clip(s, 0.0, hi)).astype(np.int64)


def move(side, cell, eff):
    """one cell in direction eff (0 left, 1 down, 2 right, 3 up), clamped at the border"""
    cell, eff = np.asarray(cell, np.int64), np.asarray(eff, np.int64)
    row, col = cell // side, cell % side
    col = np.where(eff == 0, np.maximum(col - 1, 0), np.where(eff == 2, np.minimum(col + 1, side - 1), col))
    row = np.where(eff == 1, np.minimum(row + 1, side - 1), np.where(eff == 3, np.maximum(row - 1, 0), row))
    return row * side + col


def slip_words(O, state):
    """the 32-bit word each row's step draws: w[j & 3] of philox4x32_10(key = (k0, k1); counter = (j >> 2, 0, 0, 0x20)); one Philox call per distinct
    (k0, k1, j >> 2)"""
    s = np.asarray(state, np.int64).reshape(-1, 4)
    cache, out = {}, np.zeros(s.shape[0], np.uint64)
    for i, (_, j, k0, k1) in enumerate(s.tolist()):
        key = (k0, k1, j >> 2)
        if key not in cache:
            cache[key] = O.philox4x32(k0, k1, j >> 2, 0, 0, SLIP_TAG)
        out[i] = cache[key][j & 3]
    return out


def slip(words):
    """d in {0, 1, 2}: (uint64(word) * 3) >> 32"""
    return ((np.asarray(words, np.uint64) * np.uint64(3)) >> np.uint64(32)).astype(np.int64)


def step_d(side, state, action, d):
    """the step under a GIVEN slip d [n] (0, 1, 2): eff = (a + d + 3) & 3 -- gym's [(a-1)%4, a, (a+1)%4].  state i [n,4] in range, action clamped into 0..3
    -> (next state [n,4], reward [n], terminated [n])"""
    s = np.array(state, np.int64).reshape(-1, 4)
    a = np.clip(np.asarray(action, np.int64).reshape(-1), 0, 3)
    cell, j = s[:, 0], s[:, 1]
    dead = terminal(side, cell)                       # a hole or the goal: reachable through an injected state only; nothing moves
    eff = (a + np.asarray(d, np.int64) + 3) & 3
    nc = np.where(dead, cell, move(side, cell, eff))
    term = np.where(dead, 1, terminal(side, nc).astype(np.int64))
    rew = np.where(~dead & (nc == goal(side)), 1, 0)
    return np.stack([nc, np.minimum(j + 1, WORD_MAX), s[:, 2], s[:, 3]], 1), rew, term


def step(O, side, state, action):
    """the env's step: the slip drawn from the state's own key and step count"""
    s = np.array(state, np.int64).reshape(-1, 4)
    return step_d(side, s, action, slip(slip_words(O, s)))


def obs(side, state):
    """f32 [n, S]: the one-hot of the cell"""
    s = np.asarray(state, np.int64).reshape(-1, 4)
    out = np.zeros((s.shape[0], cells(side)), np.float32)
    out[np.arange(s.shape[0]), s[:, 0]] = 1.0
    return out


def reset(words):
    """Philox words u32 [n,4] (x, y, z, w) of philox4x32_10(seed; e, k, 0, 1) -> start states [n,4]: cell 0, j 0, k0 = x >> 8, k1 = y >> 8"""
    w = np.asarray(words, np.uint64).reshape(-1, 4)
    z = np.zeros(w.shape[0], np.int64)
    return np.stack([z, z, (w[:, 0] >> np.uint64(8)).astype(np.int64), (w[:, 1] >> np.uint64(8)).astype(np.int64)], 1)


def reset_states(O, seed, envs, k):
    """reset number k[i] of global env envs[i] under `seed`"""
    w = [O.philox4x32(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, int(e), int(kk), 0, 1) for e, kk in zip(envs, k)]
    return reset(np.array(w, np.uint64))


def transition_matrix(side):
    """P [S, 4, S] (float64) and R [S, 4]: enumerating d in {0, 1, 2}, one third each.  Terminal cells absorb with reward 0."""
    S = cells(side)
    P, R = np.zeros((S, N_ACTIONS, S)), np.zeros((S, N_ACTIONS))
    st = np.zeros((S, 4), np.int64)
    st[:, 0] = np.arange(S)
    for a in range(N_ACTIONS):
        for d in range(3):
            ns, r, _ = step_d(side, st, np.full(S, a), np.full(S, d))
            P[np.arange(S), a, ns[:, 0]] += 1.0 / 3.0
            R[:, a] += r / 3.0
    return P, R


def optimal_success(side, horizon=None, tol=1e-13):
    """the optimal probability of reaching the goal from every cell: within `horizon` steps (finite-horizon dynamic programme), or without a limit (value
    iteration to `tol`).  Undiscounted; the only reward is 1 on entering the goal, so the value IS the success probability."""
    P, R = transition_matrix(side)
    live = ~terminal(side, np.arange(cells(side)))
    v = np.zeros(cells(side))
    k = 0
    while True:
        nv = np.where(live, (R + P @ v).max(axis=1), 0.0)
        k += 1
        if horizon is not None:
            v = nv
            if k == horizon:
                return v
        else:
            done = np.abs(nv - v).max() < tol
            v = nv
            if done:
                return v


def uniform_policy(side, horizon):
    """a uniformly random policy from the start, within `horizon` steps: (success probability, mean episode length -- a cut-off episode counts `horizon`)"""
    P, R = transition_matrix(side)
    Pu, Ru = P.mean(axis=1), R.mean(axis=1)
    live = ~terminal(side, np.arange(cells(side)))
    dist = np.zeros(cells(side))
    dist[0] = 1.0
    success = length = 0.0
    for _ in range(horizon):
        alive = dist * live
        length += alive.sum()               # every episode still running takes this step
        success += alive @ Ru
        dist = alive @ Pu + dist * ~live    # terminal mass stays where it is
    return success, length
