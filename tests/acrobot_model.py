"""The Acrobot step of include/ppo_hip.h (PPO_ENV_ACROBOT), once, in numpy: the header's formulas in the header's association, parameterised by the dtype
(float32 = the library's arithmetic up to the last bit of sin / cos; float64 = the yardstick) and by the constants.  A helper, not a test module."""
import numpy as np

PI = np.pi
MAX_W1, MAX_W2 = 4 * np.pi, 9 * np.pi
CONSTANTS = dict(g=9.8, dt=0.2)     # the masses, lengths and inertias are 1 / 0.5 as the header folds them


def _reduce(x, dt):
    """The header's large-argument rule: |x| >= 64 is reduced in binary64 and rounded to the dtype."""
    x = np.asarray(x, dt)
    xd = x.astype(np.float64)
    red = (xd - (2 * np.pi) * np.rint(xd / (2 * np.pi))).astype(dt)
    return np.where(np.abs(x) < dt(64.0), x, red)


def sinr(x, dt):
    return np.sin(_reduce(x, dt)).astype(dt)


def cosr(x, dt):
    return np.cos(_reduce(x, dt)).astype(dt)


def dsdt(s, tau, dt, g):
    th1, th2, w1, w2 = s
    f = dt
    half_pi = f(np.pi / 2)
    c_phi2, c_phi1 = f(0.5 * g), f(1.5 * g)      # m2 lc2 g, (m1 lc1 + m2 l1) g
    c2, s2 = cosr(th2, dt), sinr(th2, dt)
    d1 = (f(0.25) + (f(1.25) + c2)) + f(2.0)
    d2 = (f(0.25) + f(0.5) * c2) + f(1.0)
    phi2 = c_phi2 * cosr((th1 + th2) - half_pi, dt)
    phi1 = (((f(-0.5) * (w2 * w2)) * s2 - (w2 * w1) * s2) + c_phi1 * cosr(th1 - half_pi, dt)) + phi2
    dw2 = (((tau + (d2 / d1) * phi1) - (f(0.5) * (w1 * w1)) * s2) - phi2) / (f(1.25) - (d2 * d2) / d1)
    dw1 = -(d2 * dw2 + phi1) / d1
    return [w1, w2, dw1, dw2]


def wrap(x, dt):
    x = x.copy()
    pi, two_pi = dt(np.pi), dt(2 * np.pi)
    for _ in range(1024):
        m = x > pi
        if not m.any():
            break
        x[m] = x[m] - two_pi
    for _ in range(1024):
        m = x < -pi
        if not m.any():
            break
        x[m] = x[m] + two_pi
    return x


def step(state, action, dtype=np.float32, g=CONSTANTS["g"], h=CONSTANTS["dt"], full=False):
    """state [n, 4], action int [n] -> (next_state [n, 4], reward [n], terminated [n]); full: also the pre-wrap angles [n, 2] and the termination margin
    -cos th1' - cos(th1' + th2') - 1 [n]."""
    dt = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        s = [np.asarray(state, np.float64)[:, i].astype(dt) for i in range(4)]
        tau = (np.asarray(action).astype(dt) - dt(1.0)).astype(dt)
        h2, h1, h6 = dt(0.5 * h), dt(h), dt(h / 6.0)
        k1 = dsdt(s, tau, dt, g)
        k2 = dsdt([s[i] + h2 * k1[i] for i in range(4)], tau, dt, g)
        k3 = dsdt([s[i] + h2 * k2[i] for i in range(4)], tau, dt, g)
        k4 = dsdt([s[i] + h1 * k3[i] for i in range(4)], tau, dt, g)
        y = [s[i] + h6 * (((k1[i] + dt(2.0) * k2[i]) + dt(2.0) * k3[i]) + k4[i]) for i in range(4)]
        th1, th2 = wrap(y[0], dt), wrap(y[1], dt)
        w1 = np.clip(y[2], -dt(MAX_W1), dt(MAX_W1))
        w2 = np.clip(y[3], -dt(MAX_W2), dt(MAX_W2))
        margin = ((-cosr(th1, dt)) - cosr(th2 + th1, dt)) - dt(1.0)
        term = ((-cosr(th1, dt)) - cosr(th2 + th1, dt) > dt(1.0))
    ns = np.stack([th1, th2, w1, w2], axis=1).astype(dt)
    rew = np.where(term, dt(0.0), dt(-1.0)).astype(dt)
    if full:
        return ns, rew, term.astype(np.int32), np.stack([y[0], y[1]], axis=1), margin
    return ns, rew, term.astype(np.int32)


def observation(state, dtype=np.float32):
    dt = np.dtype(dtype).type
    s = np.asarray(state, np.float64).astype(dt)
    return np.stack([cosr(s[:, 0], dt), sinr(s[:, 0], dt), cosr(s[:, 1], dt), sinr(s[:, 1], dt), s[:, 2], s[:, 3]], axis=1).astype(dt)


def set_a(n=4096, seed=20261020):
    """Set A: angles uniform in [-pi, pi], |w1| <= 2 pi, |w2| <= 4 pi, actions uniform; float32 states (what the device is given)."""
    rng = np.random.default_rng(seed)
    st = np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-2 * np.pi, 2 * np.pi, n),
                   rng.uniform(-4 * np.pi, 4 * np.pi, n)], axis=1).astype(np.float32)
    return st, rng.integers(0, 3, n).astype(np.int64)


def set_b(n_random=256, seed=7):
    """Set B: the 16 corners of the box [-pi, pi]^2 x [-4 pi, 4 pi] x [-9 pi, 9 pi] (in float32) times the 3 actions, plus random rows at the full velocity range."""
    f = np.float32
    lim = [f(np.pi), f(np.pi), f(MAX_W1), f(MAX_W2)]
    rows, acts = [], []
    for c in range(16):
        for a in range(3):
            rows.append([lim[i] if (c >> i) & 1 else -lim[i] for i in range(4)])
            acts.append(a)
    rng = np.random.default_rng(seed)
    rnd = np.stack([rng.uniform(-lim[i], lim[i], n_random) for i in range(4)], axis=1)
    st = np.concatenate([np.asarray(rows, np.float64), rnd]).astype(np.float32)
    return st, np.concatenate([np.asarray(acts), rng.integers(0, 3, n_random)]).astype(np.int64)


def ang_diff(a, b):
    """|a - b| modulo 2 pi."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


def yardstick(seed=20261020):
    """Set A through the model in both precisions, once: what test_acrobot_cpu.py checks and test_gpu_acrobot.py compares against.
    Returns a dict: st, act, ref (f64 next state), rew, term, keep (rows kept in the GPU comparison), e_out [4], excluded fractions."""
    st, act = set_a(seed=seed)
    ns64, rew64, term64, pre64, margin64 = step(st, act, np.float64, full=True)
    ns32, _, _ = step(st, act, np.float32)
    # within 1e-3 of +- pi, or of any other odd multiple of pi where the wrap loops turn once more (set A never gets that far)
    by_wrap = (np.abs(np.abs(((pre64 + np.pi) % (2 * np.pi)) - np.pi) - np.pi) < 1e-3).any(axis=1)
    by_margin = np.abs(margin64) < 1e-3
    keep = ~(by_wrap | by_margin)
    return dict(st=st, act=act, ref=ns64, rew=rew64.astype(np.float32), term=term64, keep=keep, e_out=state_error(ns32, ns64).max(axis=0),
                frac_wrap_each=by_wrap_each(pre64), frac_wrap=float(by_wrap.mean()), frac_margin=float(by_margin.mean()), ns32=ns32)


def by_wrap_each(pre64):
    return (np.abs(np.abs(((pre64 + np.pi) % (2 * np.pi)) - np.pi) - np.pi) < 1e-3).mean(axis=0)


def state_error(ns, ref64):
    """|ns - ref| per output [n, 4]: the angles modulo 2 pi."""
    ns = np.asarray(ns, np.float64)
    return np.stack([ang_diff(ns[:, 0], ref64[:, 0]), ang_diff(ns[:, 1], ref64[:, 1]), np.abs(ns[:, 2] - ref64[:, 2]), np.abs(ns[:, 3] - ref64[:, 3])], axis=1)
