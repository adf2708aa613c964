"""What hidden = 128 under PPO_KERNEL_FUSED_MATRIX costs or buys: a 2 x 128 policy on kernels_fused_matrix_h128.hip (the family flag, the wide flag above 64
observation columns, the matrix flag) and with no flag at all (the generic engine, the route the shape takes otherwise), alternated in one process on one GPU.
Shapes: tools/fused_matrix_cost.py's -- obs 17 / D 6, obs 105 / D 8 and obs 376 / D 17 Gaussian, obs 100 / heads (5, 3, 4) masked.

    python tools/fused_h128_cost.py [--repeats 7] [--warmup 2] [--parent-lib PATH [--bench-steps 20] [--bench-warmup 5]]

Per shape and path, over the timed repeats, median and range of
  act_ms           one ppo_dev_act / ppo_dev_act_f32 step at N = 4096: enqueue to completion (a synchronisation in front and behind), mean over 8 steps
  step_2048_ms     one minibatch step of 2048 rows: a whole ppo_update (1 epoch x 16 minibatches of the 32 768-row rollout) / 16
  step_32768_ms    one minibatch step of 32 768 rows: a whole ppo_update (1 epoch x 1 minibatch)
--parent-lib: a libppo_hip.so built from the parent commit.  `bench.py --gpus 1` (the CartPole path, which this width does not touch) then runs in fresh child
processes, alternated between that library and this tree's (PPO_HIP_LIBRARY), the same warm-up and repeats, before this process makes its first HIP call.
There is no threshold: the width is opt-in either way.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
from tools.fused_matrix_cost import SHAPES  # noqa: E402
from tools.wide_obs_cost import N, T, make, rollout, update_ms  # noqa: E402

HIDDEN = 128


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def bench_against(parent_lib, args):
    """env-steps/s of bench.py --gpus 1 under either library, one child process per run"""
    libs = {"parent": os.path.abspath(parent_lib), "this": os.path.join(ROOT, "ppo-libtorch_amd", "libppo_hip.so")}
    got = {name: [] for name in libs}
    for rep in range(args.warmup + args.repeats):
        for name, lib in libs.items():
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)],
                               env=dict(os.environ, PPO_HIP_LIBRARY=lib), capture_output=True, text=True, timeout=300, check=True)
            if rep >= args.warmup:
                got[name].append(json.loads(r.stdout.strip().splitlines()[-1])["value"])
    return {name: spread(v) for name, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    args = ap.parse_args()
    out = {"hidden": HIDDEN, "envs": N, "steps": T, "repeats": args.repeats, "shapes": []}
    if args.parent_lib:
        out["bench_env_steps_per_s"] = bench_against(args.parent_lib, args)
    P = load_package()
    for label, obs, heads, kind in SHAPES:
        family = (P.KERNEL_GAUSS_FUSED if kind == "gauss" else P.KERNEL_CAT_FUSED) | (P.KERNEL_FUSED_WIDE_OBS if obs > 64 else 0)
        paths = {"generic": 0, "h128": family | P.KERNEL_FUSED_MATRIX}
        ctxs = {name: [make(P, obs, heads, kind, flags, nmb, hidden=HIDDEN) for nmb in (16, 1)] for name, flags in paths.items()}
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
            row[key] = {name: spread([t[k] for t in times[name]]) for name in paths}
        assert ctxs["generic"][0][0].gauss_fused_launches() == (0, 0, 0) and ctxs["h128"][0][0].gauss_fused_launches()[2] > 0
        out["shapes"].append(row)
        for name in paths:
            for ctx, _ in ctxs[name]:
                ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
