"""What the fused masked rollout (PPO_ENV_TAXI: cat_rollout_kernel, one launch for all T steps, the mask formed on the chip) buys over stepping the same env
on the same context through the stand-alone calls, in one process on one GPU, at 4096 envs x 128 steps (4 minibatches x 4 epochs, max_episode_steps 200).

    python tools/taxi_cost.py [--repeats 7] [--warmup 2] [--envs 4096] [--steps 128]

rollout    ppo_rollout alone: cat_rollout_kernel<PPO_DIST_MASKED> and the two critic launches
iteration  ppo_train_iteration: the rollout, the scan, the update
stepwise   the same T steps as a loop of ppo_policy_act(mask, step_index = rollout_steps + t) and ppo_env_step on device arrays of the same context: 2 T
           launches, nothing copied to the host, no host wait inside the loop.  The loop does less: the rollout's stores and its critic are not in it, and the
           mask it passes is a fixed array of ones -- the caller of a real loop would need a third launch per step to form it
fold       ppo_rollout with ppo_env_truncation_bootstrap on, minus the rollout without: the cost of cat_trunc_fold_kernel (the switch is turned off again)
acrobot    ppo_rollout of a PPO_ENV_ACROBOT context of the same size (the same kernel on gf_carve(8, 4), an env step of four RK4 stages), for the difference
Every timing is a host clock around work that ends in a synchronisation; median and range over the repeats after the warm-up.  No bar is set.  Prints one
JSON line."""
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


def timed(fn, *ctxs):
    for c in ctxs:
        c.sync()
    t0 = time.perf_counter()
    fn()
    for c in ctxs:
        c.sync()
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
    common = dict(num_envs=N, num_steps=T, num_minibatches=NMB, update_epochs=EPOCHS, seed=3, total_timesteps=1 << 40, learning_rate=1e-4, anneal_lr=False,
                  kernel_flags=P.KERNEL_CAT_FUSED)
    ctx = P.Context(P.make_config(env_kind=P.ENV_TAXI, dist_kind=P.DIST_MASKED, obs_size=19, head_dims=(6,), max_episode_steps=200, **common))
    boot = P.Context(P.make_config(env_kind=P.ENV_TAXI, dist_kind=P.DIST_MASKED, obs_size=19, head_dims=(6,), max_episode_steps=200, **common))
    acro = P.Context(P.make_config(env_kind=P.ENV_ACROBOT, dist_kind=P.DIST_CATEGORICAL, obs_size=6, head_dims=(3,), max_episode_steps=500, **common))
    for c in (ctx, boot, acro):
        c.init_orthogonal(3)
        c.env_reset()
    boot.env_truncation_bootstrap(True)
    d_obs, d_act = ctx.empty((N, 19), np.float32), ctx.empty((N, 1), np.int64)
    d_lp, d_rew, d_done = ctx.empty(N, np.float32), ctx.empty(N, np.float32), ctx.empty(N, np.int32)
    d_mask = ctx.dev(np.ones((N, 6), np.uint8))
    next_obs = ctx.buffer_ptr("NEXT_OBS")[0]
    chk = P.binding._check

    def stepwise():
        obs = next_obs
        for t in range(T):
            chk(L.ppo_policy_act(ctx.h, obs, d_mask.ptr, None, C.c_int64(N), C.c_int64(t), d_act.ptr, d_lp.ptr, None, None), ctx.h)
            chk(L.ppo_env_step(ctx.h, d_act.ptr, d_obs.ptr, d_rew.ptr, d_done.ptr), ctx.h)
            obs = d_obs.ptr

    runs = {"rollout": (ctx.rollout, ctx), "iteration": (ctx.train_iteration, ctx), "stepwise": (stepwise, ctx), "rollout_with_fold": (boot.rollout, boot),
            "acrobot": (acro.rollout, acro)}
    times = {k: [] for k in runs}
    events = []
    for r in range(args.warmup + args.repeats):
        for k, (fn, c) in runs.items():
            t = timed(fn, c)
            if r >= args.warmup:
                times[k].append(t)
        events.append(len(boot.env_truncations()[0]))
    out = {"shape": "Taxi-v3, obs 19, 6 actions, masked, 2 x 64, %d minibatches x %d epochs" % (NMB, EPOCHS), "envs": N, "steps": T, "repeats": args.repeats,
           "rollout_workgroups": (N + 63) // 64}
    for k, ts in times.items():
        rate = sorted(N * T / t for t in ts)
        out["%s_ms" % k] = round(1e3 * statistics.median(ts), 4)
        out["%s_Msteps_per_s" % k] = {"median": round(statistics.median(rate) / 1e6, 2), "min": round(rate[0] / 1e6, 2), "max": round(rate[-1] / 1e6, 2)}
    out["fold_ms"] = round(out["rollout_with_fold_ms"] - out["rollout_ms"], 4)
    out["fold_events_per_rollout"] = {"min": min(events), "max": max(events)}
    out["one_launch_beats_2T_launches"] = out["rollout_ms"] < out["stepwise_ms"]
    print(json.dumps(out))
    boot.env_truncation_bootstrap(False)
    for c in (ctx, boot, acro):
        c.close()


if __name__ == "__main__":
    main()
