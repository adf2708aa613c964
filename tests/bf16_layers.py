"""One hidden layer of the generic engine's bf16 arithmetic, held ELEMENT BY ELEMENT from float64 alone -- TEST INFRASTRUCTURE, NOT PRODUCT CODE, and not a
test.  numpy float64, no GPU, no library.  tests/test_bf16_layers_cpu.py holds the rule itself; tests/test_gpu_bf16_layers.py applies it to the kernels.

The layer: inputs H_in [n, K] that are bf16 values, weights rounded to bf16 (nearest even, as weight_planes_kernel<1> does), an f32 bias (as
oracle/ppo_oracle.c:mlp_forward1 keeps it), f32 accumulation in any order, tanh, and the activation stored as bf16, nearest even.

The rule.  z = H_in W^T + b and S = |H_in| |W|^T + |b| in float64, a = tanh(z), expected = bf16_rne(a).  A correct implementation computes some z' with
|z' - z| <= dz and stores bf16_rne(t) for some t with |t - tanh(z')| <= E_TANH.  So |t - a| <= max over the interval of tanh' times dz, plus E_TANH; tanh' =
1 - tanh^2 falls with |z|, so its largest value on [|z| - dz, |z| + dz] is at max(|z| - dz, 0).  An element whose a lies FARTHER than that from both
midpoints between expected and its bf16 neighbours is SAFE: every correct implementation stores the same 16 bits.  Any other element comes out as a bf16
value between bf16_rne(a - margin) and bf16_rne(a + margin): expected or the ONE neighbour on the side of the midpoint it is near, wherever the margin is
below a bf16 spacing.  It is not below it at small |a| (the margin is absolute and bf16 spacings shrink with |a|: at K = 376 the margin is 8e-4, the spacing of
|a| < 0.12 or so; at any K a unit at 1.5e-6 has neighbours 6e-9 away, and the oracle's own arithmetic lands several steps off), so "expected or a neighbour"
cannot be asked there of anyone; the interval is what the derivation gives, and it is the same rule everywhere else, one-sided and so a little tighter.

dz = (K + 2) U S (+ |W| applied to the uncertainty of the inputs, when the caller has one), U = 2^-23:
  bf16 x bf16 products are exact in f32 (8 x 8 significant bits).  The K + 1 additions (K products and the bias) are charged one FULL ulp each, relative to the
  running sum, which S bounds: twice the nearest-even bound, so an adder that truncates (a matrix core's) is covered; the + 2 absorbs the second-order terms
  ((1 + U)^(K + 1) - 1 <= (K + 2) U for K <= 10^4).  Nothing is assumed about the order of the sum or about where the bias enters it.

E_TANH = 2e-6 bounds the kernels' tanh, tanh_mufu of ppo_internal.hpp, against the exact one, in absolute terms.  Derived, not measured.  tanh_mufu(y):
      t = fl(y c), c = fl(2 / ln 2);   e = v_exp_f32(t);   s = fl(1 + e);   r = v_rcp_f32(s);   result = fma(-2, r, 1)
  With E = exp(2 y): tanh y = 1 - 2 / (1 + E), d tanh / d ln E = 2 E / (1 + E)^2 = (1 - tanh^2) / 2, and 2 / (1 + E) = 1 - tanh y <= 2.  To first order, with
  u = 2^-24 (half an ulp, relative) and the ISA's 1-ulp v_exp_f32 and v_rcp_f32 (relative 2 u each):
      the argument: c carries u, the product another u, so ln E moves by 2 |y| 2 u and tanh by |y| (1 - tanh^2) 2 u <= 0.448 x 2 u      0.9 u
      v_exp_f32:    ln E moves by 2 u, tanh by (1 - tanh^2) / 2 x 2 u                                                                      1.0 u
      fl(1 + e):    s moves by u relative, 2 / s by (1 - tanh) u                                                                           2.0 u
      v_rcp_f32:    r moves by 2 u relative, 2 r by (1 - tanh) 2 u                                                                         4.0 u
      the fma:      one rounding of a result of magnitude <= 1                                                                             1.0 u
  8.9 u = 5.3e-7 if every term were at its maximum at once (they are not: the first two peak near y = 0.77 and y = 0, the next two as tanh -> -1).
  E_TANH is 3 x that, rounded up.  The formula's own share (exact exp2 and reciprocal, each rounded to nearest: 0.9 + 0.5 + 2 + 2 + 1 = 6.4 u = 3.8e-7) is
  asserted to stay within E_TANH / 2 by tests/test_bf16_layers_cpu.py; the other half is the hardware's second half-ulp in v_exp_f32 and v_rcp_f32
  (0.5 u + 2 u = 1.5e-7).  The C library's tanhf (the oracle's) is within a few ulp of the result, 3e-7 at most, inside the same bound.
"""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -23
E_TANH = 2e-6
SAFE_SHARE_MIN = 0.60        # a condition of the tests, not a measurement: the reference alone gives 0.66 (K = 376) .. 0.98 (K = 24) on stand-in data
TANH_C = np.float32(2.885390081777927)   # tanh_mufu's constant, fl(2 / ln 2)
_BF16_TINY = 2.0 ** -133     # the smallest bf16 subnormal: the spacing of bf16 below its smallest normal 2^-126


def _spacing(mag):
    """the distance from the bf16 value mag >= 0 to the next bf16 value above it (8 significant bits; 2^-133 throughout the subnormal range and at zero)"""
    _, e = np.frexp(mag)                       # mag = m 2^e, 0.5 <= m < 1
    e = np.where(mag == 0, -125, np.maximum(e, -125))
    return np.ldexp(1.0, e - 8)


def bf16_rne(x):
    """x (finite, below bf16's largest value) rounded to the nearest bf16 value, ties to the even significand, as float64.  Straight from float64: going
    through float32 first would round twice."""
    x = np.asarray(x, np.float64)
    ulp = _spacing(np.abs(x))                  # the spacing of the binade x lies in; x / ulp is exact (a power of two)
    return np.rint(x / ulp) * ulp              # np.rint: halves to even, and an even quotient is an even significand


def bf16_trunc(x):
    """x cut to bf16 toward zero: what a store that drops the low 16 bits of an f32 does (the sensitivity tests' wrong kernel)"""
    x = np.asarray(x, np.float64)
    ulp = _spacing(np.abs(x))
    return np.trunc(x / ulp) * ulp


def bf16_neighbours(v):
    """(lo, hi): the bf16 values next to the bf16 value v on either side.  Below a power of two the spacing halves (the neighbour of 1.0 below is 1 - 2^-8,
    above 1 + 2^-7); the neighbours of zero are the smallest subnormals, -2^-133 and 2^-133 (and -0 counts as zero)."""
    v = np.asarray(v, np.float64)
    mag = np.abs(v)
    ulp = _spacing(mag)
    m, _ = np.frexp(mag)
    away = mag + ulp
    toward = mag - np.where((m == 0.5) & (mag > 2.0 ** -126), ulp / 2, ulp)
    lo = np.where(v > 0, toward, np.where(v < 0, -away, -_BF16_TINY))
    hi = np.where(v > 0, away, np.where(v < 0, -toward, _BF16_TINY))
    return lo, hi


def layer_expectation(H_in, W_f32, b_f32, H_err=None):
    """The rule of the module docstring for one layer.  H_in [n, K]: the bf16-exact inputs as floats; W_f32 [J, K], b_f32 [J] (or [J, 1]): the f32 parameters.
    H_err [n, K] (optional, >= 0): how far each input may be from the number the implementation really held (the GPU test's actor inputs are decoded from
    log-probs, and a small unit cannot be told from its neighbours that way); |H_err| |W|^T is added to dz.
    Returns a namespace of [n, J] float64 arrays: z, a, expected, lo, hi (expected's neighbours), dist, margin, the boolean safe, and allowed_lo / allowed_hi =
    bf16_rne(a -+ margin), the bf16 values an element that is not safe may take (both equal expected on a safe one)."""
    H = np.asarray(H_in, np.float64)
    assert np.array_equal(H, bf16_rne(H)), "the inputs of a layer must be bf16 values"
    W = bf16_rne(np.asarray(W_f32, np.float32).astype(np.float64))
    b = np.asarray(b_f32, np.float32).astype(np.float64).reshape(-1)
    K = H.shape[1]
    assert W.shape == (b.size, K), (W.shape, b.size, K)
    z = H @ W.T + b
    S = np.abs(H) @ np.abs(W).T + np.abs(b)
    dz = (K + 2) * U * S
    if H_err is not None:
        dz = dz + np.asarray(H_err, np.float64) @ np.abs(W).T
    a = np.tanh(z)
    expected = bf16_rne(a)
    lo, hi = bf16_neighbours(expected)
    dist = np.minimum(np.abs(a - 0.5 * (expected + lo)), np.abs(a - 0.5 * (expected + hi)))
    margin = (1.0 - np.tanh(np.maximum(np.abs(z) - dz, 0.0)) ** 2) * dz + E_TANH
    return SimpleNamespace(z=z, a=a, expected=expected, lo=lo, hi=hi, dist=dist, margin=margin, safe=dist > margin, W=W, b=b,
                           allowed_lo=bf16_rne(a - margin), allowed_hi=bf16_rne(a + margin))


class LayerMismatch(AssertionError):
    pass


def count_layer(observed, exp):
    """counts of one layer's observed activations [n, J] against layer_expectation's namespace; values are compared, so -0 equals +0 (and a NaN equals nothing).
    safe_mismatch: safe elements that are not expected.  unsafe_flips: other elements that are not expected but a bf16 value inside [allowed_lo, allowed_hi]
    (informational).  unsafe_bad: other elements outside it."""
    obs = np.asarray(observed, np.float64)
    assert obs.shape == exp.expected.shape, (obs.shape, exp.expected.shape)
    same = obs == exp.expected
    near = (obs == bf16_rne(obs)) & (obs >= exp.allowed_lo) & (obs <= exp.allowed_hi) & ~same
    return dict(n=int(obs.size), safe=int(exp.safe.sum()), safe_share=float(exp.safe.mean()), safe_mismatch=int((exp.safe & ~same).sum()),
                unsafe_flips=int((~exp.safe & near).sum()), unsafe_bad=int((~exp.safe & ~same & ~near).sum()))


def offenders(observed, exp, limit=5):
    """(row, column, observed, expected, exact tanh, dist, margin, safe) of the first few elements that break the rule"""
    obs = np.asarray(observed, np.float64)
    same = obs == exp.expected
    near = (obs == bf16_rne(obs)) & (obs >= exp.allowed_lo) & (obs <= exp.allowed_hi)
    bad = np.argwhere(~same & (exp.safe | ~near))[:limit]
    return [(int(r), int(c), float(obs[r, c]), float(exp.expected[r, c]), float(exp.a[r, c]), float(exp.dist[r, c]), float(exp.margin[r, c]), bool(exp.safe[r, c]))
            for r, c in bad]


def check_layer(observed, H_in, W_f32, b_f32, H_err=None):
    """count_layer of observed against layer_expectation(H_in, W_f32, b_f32).  Raises LayerMismatch if a safe element differs from expected, or if any other
    element is no bf16 value of [allowed_lo, allowed_hi] (expected or the neighbour beyond the near midpoint, except at small |a|); returns the counts otherwise."""
    exp = layer_expectation(H_in, W_f32, b_f32, H_err)
    counts = count_layer(observed, exp)
    if counts["safe_mismatch"] or counts["unsafe_bad"]:
        raise LayerMismatch("%s; (row, col, observed, expected, tanh, dist, margin, safe): %s" % (counts, offenders(observed, exp)))
    return counts


def tanh_mufu_f32(x):
    """tanh_mufu's formula in numpy float32 with an exact exp2 and an exact reciprocal, each rounded to nearest once: t = fl(x c), e = fl(exp2(t)),
    s = fl(1 + e), r = fl(1 / s), fl(1 - 2 r).  (1 - 2 r is exact in float64 for r >= 2^-28, so the last step rounds once, as the fma does.)"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        t = (x * TANH_C).astype(np.float32)
        e = np.exp2(t.astype(np.float64)).astype(np.float32)
        s = (np.float32(1.0) + e).astype(np.float32)
        r = (1.0 / s.astype(np.float64)).astype(np.float32)
    return (1.0 - 2.0 * r.astype(np.float64)).astype(np.float32)
