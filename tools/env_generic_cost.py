"""What PPO_KERNEL_ENV_GENERIC costs and buys on CartPole, in one process on one GPU, at 4096 envs x 128 steps (4 minibatches x 4 epochs, max_episode_steps 500).

    python tools/env_generic_cost.py [--repeats 7] [--warmup 2] [--envs 4096] [--steps 128]

Four contexts, each timed for
  rollout    ppo_rollout alone
  iteration  ppo_train_iteration: the rollout, the scan, the update
    unflagged 2 x 64      the reference-shape kernels (rollout16_kernel, one launch): the A/B partner
    flagged 2 x 64 f32    the generic engine at the same network: T x { layer products, heads, stores, env step }
    flagged 2 x 256 f32   the same plan at a width the reference-shape kernels do not have
    flagged 4 x 256 bf16  generic_env_rollout_kernel: all T steps in one launch
and, for the bf16 context,
  stepwise   the same T steps as a loop of ppo_policy_act(step_index = rollout_steps + t) and ppo_env_step on device arrays of the same context: nothing copied
             to the host, no host wait inside the loop (the rollout's stores and its critic are not in it: the loop does less).
Every timing is a host clock around work that ends in a synchronisation; median and range over the repeats after the warm-up, the contexts taking turns
inside every repeat.  One condition: the one-launch bf16 rollout is not slower than the stepwise loop of the same context (exit status 1 otherwise).
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

NMB, EPOCHS = 4, 4


def timed(fn, ctx):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    args = ap.parse_args()
    P = load_package()
    L = P.binding.lib()
    N, T = args.envs, args.steps
    common = dict(env_kind=P.ENV_CARTPOLE, dist_kind=P.DIST_CATEGORICAL, obs_size=4, head_dims=(2,), num_envs=N, num_steps=T, num_minibatches=NMB, update_epochs=EPOCHS,
                  seed=3, total_timesteps=200 * N * T, learning_rate=1e-4, anneal_lr=False, max_episode_steps=500)
    F = P.KERNEL_ENV_GENERIC
    ctxs = {"unflagged_2x64": P.Context(P.make_config(**common)),
            "flagged_2x64_f32": P.Context(P.make_config(kernel_flags=F, **common)),
            "flagged_2x256_f32": P.Context(P.make_config(kernel_flags=F, hidden=256, **common)),
            "flagged_4x256_bf16": P.Context(P.make_config(kernel_flags=F, hidden=256, n_hidden=4, compute_dtype=P.DTYPE_BF16, **common))}
    for c in ctxs.values():
        c.init_orthogonal(3)
        c.env_reset()
    bf = ctxs["flagged_4x256_bf16"]
    d_obs, d_act = bf.empty((N, 4), np.float32), bf.empty((N, 1), np.int64)
    d_lp, d_rew, d_done = bf.empty(N, np.float32), bf.empty(N, np.float32), bf.empty(N, np.int32)
    next_obs = bf.buffer_ptr("NEXT_OBS")[0]
    chk = P.binding._check

    def stepwise():
        obs = next_obs
        for t in range(T):
            chk(L.ppo_policy_act(bf.h, obs, None, None, C.c_int64(N), C.c_int64(t), d_act.ptr, d_lp.ptr, None, None), bf.h)
            chk(L.ppo_env_step(bf.h, d_act.ptr, d_obs.ptr, d_rew.ptr, d_done.ptr), bf.h)
            obs = d_obs.ptr

    runs = {}
    for name, c in ctxs.items():
        runs[name + "_rollout"] = (c.rollout, c)
        runs[name + "_iteration"] = (c.train_iteration, c)
    runs["flagged_4x256_bf16_stepwise"] = (stepwise, bf)
    times = {k: [] for k in runs}
    for r in range(args.warmup + args.repeats):
        for k, (fn, c) in runs.items():
            t = timed(fn, c)
            if r >= args.warmup:
                times[k].append(t)
    out = {"shape": "CartPole, obs 4, 2 actions, %d minibatches x %d epochs" % (NMB, EPOCHS), "envs": N, "steps": T, "repeats": args.repeats}
    for k, ts in times.items():
        rate = sorted(N * T / t for t in ts)
        out["%s_ms" % k] = round(1e3 * statistics.median(ts), 4)
        out["%s_Msteps_per_s" % k] = {"median": round(statistics.median(rate) / 1e6, 2), "min": round(rate[0] / 1e6, 2), "max": round(rate[-1] / 1e6, 2)}
    out["flagged_2x64_rollout_over_unflagged"] = round(out["flagged_2x64_f32_rollout_ms"] / out["unflagged_2x64_rollout_ms"], 2)
    out["flagged_2x64_iteration_over_unflagged"] = round(out["flagged_2x64_f32_iteration_ms"] / out["unflagged_2x64_iteration_ms"], 2)
    ok = out["flagged_4x256_bf16_rollout_ms"] <= out["flagged_4x256_bf16_stepwise_ms"]
    out["one_launch_not_slower_than_stepwise"] = ok
    print(json.dumps(out))
    for c in ctxs.values():
        c.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
