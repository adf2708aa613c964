"""What PPO_KERNEL_FUSED_WIDE_OBS buys: a 2 x 64 policy over more than 64 observation columns with the family flag and the wide flag (kernels_fused_wide.hip:
layer 1 streamed in chunks of 64 columns) and with no flag at all (the generic engine, the route such a shape takes without the flag), alternated in one
process on one GPU.  Shapes: obs 105 / D 8 and obs 376 / D 17 Gaussian (Ant, Humanoid), obs 100 / heads (5, 3, 4) masked.

    python tools/wide_obs_cost.py [--repeats 7] [--warmup 2]

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
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

N, T = 4096, 8
SHAPES = (("obs 105, D 8 Gaussian", 105, (8,), "gauss"), ("obs 376, D 17 Gaussian", 376, (17,), "gauss"), ("obs 100, heads (5, 3, 4) masked", 100, (5, 3, 4), "masked"))


def make(P, obs, heads, kind, flags, nmb, hidden=64, compute_dtype=0):
    gauss = kind == "gauss"
    ctx = P.Context(P.make_config(env_kind=P.ENV_HOST, dist_kind=P.DIST_GAUSSIAN if gauss else P.DIST_MASKED, obs_size=obs, head_dims=heads, hidden=hidden, n_hidden=2,
                                  num_envs=N, num_steps=T, num_minibatches=nmb, update_epochs=1, seed=3, total_timesteps=1 << 40, learning_rate=1e-4,
                                  anneal_lr=False, max_episode_steps=1000, kernel_flags=flags, compute_dtype=compute_dtype))
    ctx.init_orthogonal(3)
    rng = np.random.default_rng(obs)
    dev = dict(act=ctx.empty((N, heads[0]), np.float32) if gauss else ctx.empty((N, len(heads)), np.int64),
               obs=[ctx.dev(rng.uniform(-1, 1, (N, obs)).astype(np.float32)) for _ in range(2)],
               mask=None if gauss else ctx.dev(np.ones((N, sum(heads)), np.uint8), np.uint8), rew=ctx.dev(rng.normal(0, 1, N).astype(np.float32)),
               done=ctx.dev((rng.uniform(0, 1, N) < 0.01).astype(np.int32), np.int32), gauss=gauss)
    ctx.dev_env_reset(dev["obs"][0])
    return ctx, dev


def rollout(ctx, dev):
    """a device-fed rollout on fixed arrays and its end; returns the mean act step in ms"""
    ctx.host_rollout_begin()
    act = 0.0
    for t in range(T):
        ctx.sync()
        t0 = time.perf_counter()
        if dev["gauss"]:
            ctx.dev_act_f32(dev["act"])
        else:
            ctx.dev_act(dev["act"], mask=dev["mask"])
        ctx.sync()
        act += time.perf_counter() - t0
        ctx.dev_observe(dev["obs"][t & 1], dev["rew"], dev["done"])
    ctx.host_rollout_end()
    ctx.sync()
    return 1e3 * act / T


def update_ms(ctx):
    ctx.sync()
    t0 = time.perf_counter()
    ctx.update()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    P = load_package()
    out = {"envs": N, "steps": T, "repeats": args.repeats, "shapes": []}
    for label, obs, heads, kind in SHAPES:
        family = P.KERNEL_GAUSS_FUSED if kind == "gauss" else P.KERNEL_CAT_FUSED
        paths = {"generic": 0, "wide": family | P.KERNEL_FUSED_WIDE_OBS}
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
        assert ctxs["generic"][0][0].gauss_fused_launches() == (0, 0, 0) and ctxs["wide"][0][0].gauss_fused_launches()[2] > 0
        out["shapes"].append(row)
        for name in paths:
            for ctx, _ in ctxs[name]:
                ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
