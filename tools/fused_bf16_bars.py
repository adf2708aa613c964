#!/usr/bin/env python3
"""Where the bars of tests/test_gpu_fused_bf16.py come from; no GPU, no library.  Evaluates that file's own model on that file's own inputs three times:
in float64, with every product and sum of the network in float32 (the same rounding points, f32 accumulation error only), and as the plain unrounded
float64 network.  Prints the worst float64-versus-float32 deviation per quantity over all parametrised cases -- the bars are 4 x that, never below the
family's f32 bars -- each gradient tensor's own deviation (a seed is fit if all stay below 1 % of the tensor's largest element), and, for the reader, how
far the unrounded network is from the rounded model.

    python tools/fused_bf16_bars.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_fused_bf16 as T   # noqa: E402

worst = dict(fwd=0.0, loss=0.0, grad=0.0, plain_fwd=0.0, plain_grad=0.0)


def forward(tag, run):
    a, b, p = run(np.float64), run(np.float32), run(None)
    d, dp = max(T.rel(y, x) for x, y in zip(a, b)), max(T.rel(y, x) for x, y in zip(a, p))
    print("%-44s f32 %.3g   unrounded %.3g" % (tag, d, dp))
    worst.update(fwd=max(worst["fwd"], d), plain_fwd=max(worst["plain_fwd"], dp))


def step(tag, run, shapes, obs):
    (g, sc), (g32, sc32), (gp, _) = run(np.float64), run(np.float32), run(None)
    dl = max(abs(sc[k] - sc32[k]) for _, k in T.STATS)
    errs, errs_p = T.tensor_errors(g32, g, shapes, obs), T.tensor_errors(gp, g, shapes, obs)
    dg, dgp = max(e for _, e in errs), max(e for _, e in errs_p)
    print("%-44s loss %.3g   gradient f32 %.3g (%s)   unrounded %.3g" % (tag, dl, dg, max(errs, key=lambda t: t[1])[0], dgp))
    assert dg < 0.01, "a gradient tensor moves by more than 1 %% of its largest element between float64 and float32: another seed (%s)" % tag
    worst.update(loss=max(worst["loss"], dl), grad=max(worst["grad"], dg), plain_grad=max(worst["plain_grad"], dgp))


for H in (64, 128):
    for obs, D in T.FWD_SHAPES:
        params, rows = T.gauss_forward_case(H, obs, D)
        for x, spread in rows:
            forward("H %d Gaussian forward obs %d D %d n %d" % (H, obs, D, len(x)),
                    lambda prec: [v for i, v in enumerate(T.gauss_forward(prec, H, obs, D, params, x, spread)) if i != 1])
    for M in T.ROWS:
        for obs, D in T.STEP_SHAPES:
            N, Tn, params, buf, idx = T.gauss_step_case(H, obs, D, M)
            step("H %d Gaussian step obs %d D %d M %d" % (H, obs, D, M), lambda prec: T.gauss_step(prec, H, obs, D, params, buf, idx),
                 T.tensor_shapes(obs, H, 2, D), obs)
for key in T.CAT_KEYS:
    for n in T.NS if key[0] == 17 else ():
        forward("categorical forward %s n %d" % (key, n), lambda prec: T.cat_forward(prec, key, n))
for key, M in T.CAT_STEPS:
    step("categorical step %s M %d" % (key, M), lambda prec: T.cat_step(prec, key, M), T.cat_shapes(key), 100)

print("\nworst float64-versus-float32 deviation: forward %.3g, loss scalars %.3g, gradient tensors %.3g" % (worst["fwd"], worst["loss"], worst["grad"]))
print("bars (4 x, floors 3e-6 / 1e-5 / 5e-6):   forward %.3g, loss scalars %.3g, gradient tensors %.3g"
      % (max(4 * worst["fwd"], 3e-6), max(4 * worst["loss"], 1e-5), max(4 * worst["grad"], 5e-6)))
print("the unrounded float64 network against the rounded model: forward %.3g, gradient tensors %.3g" % (worst["plain_fwd"], worst["plain_grad"]))
