"""What the fused categorical rollout (PPO_ENV_ACROBOT: cat_rollout_kernel, one launch for all T steps) buys over stepping the same env on the same context
through the stand-alone calls, in one process on one GPU, at 4096 envs x 128 steps (4 minibatches x 4 epochs, max_episode_steps 500).

    python tools/acrobot_cost.py [--repeats 7] [--warmup 2] [--envs 4096] [--steps 128]

rollout    ppo_rollout alone: cat_rollout_kernel and the two critic launches
iteration  ppo_train_iteration: the rollout, the scan, the update
stepwise   the same T steps as a loop of ppo_policy_act(step_index = rollout_steps + t) and ppo_env_step on device arrays of the same context: 2 T launches,
           nothing copied to the host, no host wait inside the loop (the rollout's stores and its critic are not in it: the loop does less)
env_only   T ppo_env_step launches under a fixed action (one thread per env, the whole device): what the RK4 step costs when it is not confined to wave 0 of
           one workgroup per 64 envs
pendulum   ppo_rollout of a PPO_ENV_PENDULUM context of the same size (gauss_rollout_kernel: the same plan, an env step of one sine), for the difference
Every timing is a host clock around work that ends in a synchronisation; median and range over the repeats after the warm-up.  No bar is set: the
expectation is only that one launch beats 2 T.  Prints one JSON line."""
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
    common = dict(num_envs=N, num_steps=T, num_minibatches=NMB, update_epochs=EPOCHS, seed=3, total_timesteps=1 << 40, learning_rate=1e-4, anneal_lr=False)
    ctx = P.Context(P.make_config(env_kind=P.ENV_ACROBOT, dist_kind=P.DIST_CATEGORICAL, obs_size=6, head_dims=(3,), max_episode_steps=500,
                                  kernel_flags=P.KERNEL_CAT_FUSED, **common))
    pend = P.Context(P.make_config(env_kind=P.ENV_PENDULUM, dist_kind=P.DIST_GAUSSIAN, obs_size=3, head_dims=(1,), max_episode_steps=200,
                                   kernel_flags=P.KERNEL_GAUSS_FUSED, **common))
    for c in (ctx, pend):
        c.init_orthogonal(3)
        c.env_reset()
    d_obs, d_act = ctx.empty((N, 6), np.float32), ctx.empty((N, 1), np.int64)
    d_lp, d_rew, d_done = ctx.empty(N, np.float32), ctx.empty(N, np.float32), ctx.empty(N, np.int32)
    d_fixed = ctx.dev(np.full((N, 1), 2, np.int64))
    next_obs = ctx.buffer_ptr("NEXT_OBS")[0]
    chk = P.binding._check

    def stepwise():
        obs = next_obs
        for t in range(T):
            chk(L.ppo_policy_act(ctx.h, obs, None, None, C.c_int64(N), C.c_int64(t), d_act.ptr, d_lp.ptr, None, None), ctx.h)
            chk(L.ppo_env_step(ctx.h, d_act.ptr, d_obs.ptr, d_rew.ptr, d_done.ptr), ctx.h)
            obs = d_obs.ptr

    def env_only():
        for _ in range(T):
            chk(L.ppo_env_step(ctx.h, d_fixed.ptr, d_obs.ptr, d_rew.ptr, d_done.ptr), ctx.h)

    runs = {"rollout": (ctx.rollout, ctx), "iteration": (ctx.train_iteration, ctx), "stepwise": (stepwise, ctx), "env_only": (env_only, ctx),
            "pendulum": (pend.rollout, pend)}
    times = {k: [] for k in runs}
    for r in range(args.warmup + args.repeats):
        for k, (fn, c) in runs.items():
            t = timed(fn, c)
            if r >= args.warmup:
                times[k].append(t)
    out = {"shape": "Acrobot-v1, obs 6, 3 actions, 2 x 64, %d minibatches x %d epochs" % (NMB, EPOCHS), "envs": N, "steps": T, "repeats": args.repeats,
           "rollout_workgroups": (N + 63) // 64}
    for k, ts in times.items():
        rate = sorted(N * T / t for t in ts)
        out["%s_ms" % k] = round(1e3 * statistics.median(ts), 4)
        out["%s_Msteps_per_s" % k] = {"median": round(statistics.median(rate) / 1e6, 2), "min": round(rate[0] / 1e6, 2), "max": round(rate[-1] / 1e6, 2)}
    out["one_launch_beats_2T_launches"] = out["rollout_ms"] < out["stepwise_ms"]
    print(json.dumps(out))
    for c in (ctx, pend):
        c.close()


if __name__ == "__main__":
    main()
