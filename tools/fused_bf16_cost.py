"""What compute_dtype = PPO_DTYPE_BF16 under PPO_KERNEL_FUSED_MATRIX costs or buys (kernels_fused_matrix_bf16.hip), at hidden 128 and 64: three paths alternated in
one process on one GPU -- the generic engine at PPO_DTYPE_BF16 (no flag; it refuses a Gaussian policy at that dtype, and such a cell is null), the flagged
context at PPO_DTYPE_F32 (kernels_fused_matrix_h128.hip / kernels_fused_matrix.hip) and the flagged context at PPO_DTYPE_BF16.  Shapes and the three
figures per cell (act_ms, step_2048_ms, step_32768_ms) are tools/fused_h128_cost.py's.

    python tools/fused_bf16_cost.py [--repeats 7] [--warmup 2] [--parent-lib PATH [--bench-steps 20] [--bench-warmup 5]]

--parent-lib: as in tools/fused_h128_cost.py, `bench.py --gpus 1` alternated between the parent commit's library and this tree's, in fresh child processes,
before this process makes its first HIP call.  There is no threshold: the dtype is opt-in.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
from tools.fused_h128_cost import bench_against, spread  # noqa: E402
from tools.fused_matrix_cost import SHAPES  # noqa: E402
from tools.wide_obs_cost import N, T, make, rollout, update_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    args = ap.parse_args()
    out = {"envs": N, "steps": T, "repeats": args.repeats, "cells": []}
    if args.parent_lib:
        out["bench_env_steps_per_s"] = bench_against(args.parent_lib, args)
    P = load_package()
    for hidden in (128, 64):
        for label, obs, heads, kind in SHAPES:
            flagged = (P.KERNEL_GAUSS_FUSED if kind == "gauss" else P.KERNEL_CAT_FUSED) | (P.KERNEL_FUSED_WIDE_OBS if obs > 64 else 0) | P.KERNEL_FUSED_MATRIX
            paths = {"generic_bf16": (0, P.DTYPE_BF16), "flagged_f32": (flagged, P.DTYPE_F32), "flagged_bf16": (flagged, P.DTYPE_BF16)}
            if kind == "gauss":   # ppo_ctx_create: "dist_kind = PPO_DIST_GAUSSIAN is built for compute_dtype = PPO_DTYPE_F32"
                del paths["generic_bf16"]
            ctxs = {name: [make(P, obs, heads, kind, fl, nmb, hidden=hidden, compute_dtype=dt) for nmb in (16, 1)] for name, (fl, dt) in paths.items()}
            times = {name: [] for name in paths}
            for rep in range(args.warmup + args.repeats):
                for name in paths:
                    (c16, d16), (c1, d1) = ctxs[name]
                    act = rollout(c16, d16)
                    rollout(c1, d1)
                    if rep >= args.warmup:
                        times[name].append((act, update_ms(c16) / 16, update_ms(c1)))
            row = {"hidden": hidden, "shape": label}
            for k, key in enumerate(("act_ms", "step_2048_ms", "step_32768_ms")):
                row[key] = {name: spread([t[k] for t in times[name]]) for name in paths}
                row[key].setdefault("generic_bf16", None)
            assert all(ctxs[name][0][0].gauss_fused_launches()[2] > 0 for name in ("flagged_f32", "flagged_bf16"))
            out["cells"].append(row)
            print("hidden %d %s done" % (hidden, label), file=sys.stderr, flush=True)
            for name in paths:
                for ctx, _ in ctxs[name]:
                    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
