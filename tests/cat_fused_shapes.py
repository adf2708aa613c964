"""The shapes tests/test_cat_fused_cpu.py and tests/test_gpu_cat_fused.py walk (PPO_KERNEL_CAT_FUSED: categorical policies of a 2 x 64 f32 caller-stepped
context at any observation width up to 64) -- TEST INFRASTRUCTURE, not a test.  Dicts in the form grad_oracle._ref makes, fed to grad_oracle.stand_in_batch /
ref_index_lists; the batch and both oracles' steps are made once and shared (nothing writes to them).

Lists of 576, 225, 65 and 2 rows: nine whole 64-row tiles, three tiles plus 33 rows, a tile plus a row, fewer rows than a tile.  The seeds were chosen on
the CPU with the two oracles alone so that every condition tests/test_grad_oracle_cpu.py puts on a shape holds at every list (asserted again by
tests/test_cat_fused_cpu.py)."""
import functools

import numpy as np

import grad_oracle as G
import oracle as O

CAT_FUSED = 256                   # PPO_KERNEL_CAT_FUSED (include/ppo_hip.h)
CAT_LISTS = (576, 225, 65, 2)


def _cat(obs, heads, masked, seed, **kw):
    return dict(obs=obs, hidden=64, n_hidden=2, heads=tuple(heads), masked=masked, dtype=0, lists=CAT_LISTS, seed=seed, flags=(CAT_FUSED,), **kw)


CAT_SHAPES = {
    "obs1 (2,) masked":               _cat(1, (2,), True, seed=55),
    "obs6 (3,)":                      _cat(6, (3,), False, seed=51),
    "obs17 (5,3,4) masked":           _cat(17, (5, 3, 4), True, seed=52),
    "obs33 eight heads of 4 masked":  _cat(33, (4,) * 8, True, seed=53),   # 32 logits, 8 heads: the ABI's maximum
    "obs64 (32,)":                    _cat(64, (32,), False, seed=54, clip_vloss=False, norm_adv=False),
}


def hparams(s):
    hp = G.shape_hp(s)
    return O.HParams(norm_adv=int(hp["norm_adv"]), clip_vloss=int(hp["clip_vloss"]), **G.BASE_HP)


@functools.lru_cache(maxsize=None)
def batch(name):
    """the shape's stand-in batch and index lists"""
    s = CAT_SHAPES[name]
    b = G.stand_in_batch(s)
    b["lists"] = G.ref_index_lists(s, b)
    for v in b.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def oracle_step(name, k):
    """list k of the shape in both oracles: (float64 gradient, its scalars, per-row arrays), (C oracle's f32 gradient, its scalars)"""
    s, b = CAT_SHAPES[name], batch(name)
    rows = {}
    idx = b["lists"][k]
    g64, s64 = G.minibatch_grads(b["shapes"], s["heads"], s["masked"], G.shape_hp(s), b["params"], b["obs"], b["actions"], b["logp"], b["adv"], b["ret"], b["values"], idx,
                                 b["masks"], rows=rows)
    gc, sc = O.minibatch_grads(b["net"], hparams(s), b["params"], b["obs"], b["actions"].astype(np.float32), b["logp"], b["adv"], b["ret"], b["values"],
                               idx.astype(np.int64), b["masks"])
    return (g64, s64, rows), (gc, sc)
