"""What the fused rollout of the slippery FrozenLake (PPO_ENV_FROZENLAKE, PPO_ENV_FROZENLAKE8X8: cat_rollout_kernel, one launch for all T steps, the env's slip
drawn on the chip from a key the state carries) buys over stepping the same env on the same context through the stand-alone calls, in one process on one GPU,
at 4096 envs x 128 steps (4 minibatches x 4 epochs; max_episode_steps 100 resp. 200).

    python tools/frozenlake_cost.py [--repeats 7] [--warmup 2] [--envs 4096] [--steps 128]

Per map (lake4: the 4x4 map, obs 16; lake8: the 8x8 map, obs 64):
rollout    ppo_rollout alone: cat_rollout_kernel and the two critic launches
iteration  ppo_train_iteration: the rollout, the scan, the update
stepwise   the same T steps as a loop of ppo_policy_act(step_index = rollout_steps + t) and ppo_env_step on device arrays of the same context: 2 T launches,
           nothing copied to the host, no host wait inside the loop.  The loop does less: the rollout's stores and its critic are not in it
and, in the same run,
taxi       ppo_rollout of a PPO_ENV_TAXI context of the same size (the same kernel on gf_carve(20, 8), masked), for the difference: the 8x8 map pays a 64-wide
           first layer and 64-float observation rows
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
    lakes = {"lake4": P.Context(P.make_config(env_kind=P.ENV_FROZENLAKE, dist_kind=P.DIST_CATEGORICAL, obs_size=16, head_dims=(4,), max_episode_steps=100, **common)),
             "lake8": P.Context(P.make_config(env_kind=P.ENV_FROZENLAKE8X8, dist_kind=P.DIST_CATEGORICAL, obs_size=64, head_dims=(4,), max_episode_steps=200, **common))}
    taxi = P.Context(P.make_config(env_kind=P.ENV_TAXI, dist_kind=P.DIST_MASKED, obs_size=19, head_dims=(6,), max_episode_steps=200, **common))
    for c in list(lakes.values()) + [taxi]:
        c.init_orthogonal(3)
        c.env_reset()
    chk = P.binding._check
    keep = []   # the loops' device arrays, alive for the whole run

    def stepwise_of(ctx):
        d_obs, d_act = ctx.empty((N, ctx.O), np.float32), ctx.empty((N, 1), np.int64)
        d_lp, d_rew, d_done = ctx.empty(N, np.float32), ctx.empty(N, np.float32), ctx.empty(N, np.int32)
        keep.extend([d_obs, d_act, d_lp, d_rew, d_done])
        next_obs = ctx.buffer_ptr("NEXT_OBS")[0]

        def stepwise():
            obs = next_obs
            for t in range(T):
                chk(L.ppo_policy_act(ctx.h, obs, None, None, C.c_int64(N), C.c_int64(t), d_act.ptr, d_lp.ptr, None, None), ctx.h)
                chk(L.ppo_env_step(ctx.h, d_act.ptr, d_obs.ptr, d_rew.ptr, d_done.ptr), ctx.h)
                obs = d_obs.ptr
        return stepwise

    runs = {}
    for name, c in lakes.items():
        runs["%s_rollout" % name] = (c.rollout, c)
        runs["%s_iteration" % name] = (c.train_iteration, c)
        runs["%s_stepwise" % name] = (stepwise_of(c), c)
    runs["taxi_rollout"] = (taxi.rollout, taxi)
    times = {k: [] for k in runs}
    for r in range(args.warmup + args.repeats):
        for k, (fn, c) in runs.items():
            t = timed(fn, c)
            if r >= args.warmup:
                times[k].append(t)
    out = {"shape": "FrozenLake-v1 (obs 16) and FrozenLake8x8-v1 (obs 64), slippery, 4 actions, 2 x 64, %d minibatches x %d epochs" % (NMB, EPOCHS), "envs": N,
           "steps": T, "repeats": args.repeats, "rollout_workgroups": (N + 63) // 64}
    for k, ts in times.items():
        rate = sorted(N * T / t for t in ts)
        ms = sorted(1e3 * t for t in ts)
        out["%s_ms" % k] = {"median": round(statistics.median(ms), 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}
        out["%s_Msteps_per_s" % k] = {"median": round(statistics.median(rate) / 1e6, 2), "min": round(rate[0] / 1e6, 2), "max": round(rate[-1] / 1e6, 2)}
    for name in lakes:
        out["%s_one_launch_beats_2T_launches" % name] = out["%s_rollout_ms" % name]["median"] < out["%s_stepwise_ms" % name]["median"]
        out["%s_rollout_over_taxi" % name] = round(out["%s_rollout_ms" % name]["median"] / out["taxi_rollout_ms"]["median"], 3)
    print(json.dumps(out))
    for c in list(lakes.values()) + [taxi]:
        c.close()


if __name__ == "__main__":
    main()
