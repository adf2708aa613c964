"""What PPO_KERNEL_FUSED_MATRIX buys: a 2 x 64 policy on the fused family's kernels with the 64-wide products on the f32 matrix cores (kernels_fused_matrix.hip),
on the same context without the new flag (the family's vector kernels: kernels_gauss_fused.hip at obs <= 64, kernels_fused_wide.hip above) and with no flag at
all (the generic engine), alternated in one process on one GPU.  Shapes: obs 17 / D 6, obs 105 / D 8 and obs 376 / D 17 Gaussian (HalfCheetah, Ant, Humanoid),
obs 100 / heads (5, 3, 4) masked -- tools/wide_obs_cost.py's, and one resident shape.

    python tools/fused_matrix_cost.py [--repeats 7] [--warmup 2]

Per shape and path, over the timed repeats, median and range of
  act_ms           one ppo_dev_act / ppo_dev_act_f32 step at N = 4096: enqueue to completion (a synchronisation in front and behind), mean over 8 steps
  step_2048_ms     one minibatch step of 2048 rows: a whole ppo_update (1 epoch x 16 minibatches of the 32 768-row rollout) / 16
  step_32768_ms    one minibatch step of 32 768 rows: a whole ppo_update (1 epoch x 1 minibatch)
There is no threshold: the flag is opt-in either way.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402
from tools.wide_obs_cost import N, T, SHAPES, make, rollout, update_ms  # noqa: E402

SHAPES = (("obs 17, D 6 Gaussian", 17, (6,), "gauss"),) + SHAPES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    P = load_package()
    out = {"envs": N, "steps": T, "repeats": args.repeats, "shapes": []}
    for label, obs, heads, kind in SHAPES:
        family = (P.KERNEL_GAUSS_FUSED if kind == "gauss" else P.KERNEL_CAT_FUSED) | (P.KERNEL_FUSED_WIDE_OBS if obs > 64 else 0)
        paths = {"generic": 0, "fused": family, "matrix": family | P.KERNEL_FUSED_MATRIX}
        ctxs = {name: [make(P, obs, heads, kind, flags, nmb) for nmb in (16, 1)] for name, flags in paths.items()}
        times = {name: [] for name in paths}
        for rep in range(args.warmup + args.repeats):
            for name in paths:
                (c16, d16), (c1, d1) = ctxs[name]
                act = rollout(c16, d16)
                rollout(c1, d1)
                if rep >= args.warmup:
                    times[name].append((act, update_ms(c16) / 16, update_ms(c1)))
        row = {"shape": label}
        for k, key in enumerate(("act_ms", "step_2048_ms", "step_32768_ms")):
            row[key] = {}
            for name in paths:
                v = [t[k] for t in times[name]]
                row[key].update({name + "_median": statistics.median(v), name + "_min": min(v), name + "_max": max(v)})
        assert ctxs["generic"][0][0].gauss_fused_launches() == (0, 0, 0)
        assert ctxs["fused"][0][0].gauss_fused_launches()[2] > 0 and ctxs["matrix"][0][0].gauss_fused_launches()[2] > 0
        out["shapes"].append(row)
        for name in paths:
            for ctx, _ in ctxs[name]:
                ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
