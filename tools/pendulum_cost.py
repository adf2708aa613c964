"""What the fused Gaussian rollout (PPO_ENV_PENDULUM: gauss_rollout_kernel, one launch for all T steps) buys over stepping the same env on the device through
the stand-alone calls, in one process on one GPU, at 4096 envs x 128 steps and at 16384 envs x 64 steps (4 minibatches x 4 epochs, max_episode_steps 200).

    python tools/pendulum_cost.py [--repeats 7] [--warmup 2] [--env pendulum|mountaincar_continuous|both]

--env picks the device env (default pendulum: the tool's first form, same output); both: one run measures the two envs one after the other, and for
PPO_ENV_MOUNTAINCAR_CONTINUOUS also the truncation fold (below).

fused     a Pendulum context: ppo_train_iteration (rollout = 3 launches, the scan, the update), and ppo_rollout alone
stepwise  a PPO_ENV_HOST Gaussian context with PPO_KERNEL_GAUSS_FUSED, fed per step by ppo_dev_act_f32, a second (Pendulum) context's ppo_env_step_f32 on the
          same device arrays and ppo_dev_observe: 3 launches per step, nothing copied to the host, no host wait inside the rollout; ppo_host_rollout_end is
          the rest of the iteration.  The rollout part is timed up to (not including) ppo_host_rollout_end.
Every timing is a host clock around work that ends in a synchronisation of both contexts; median and range over the repeats after the warm-up, as
env-steps/s = N * T / seconds.  No bar is set: the expectation is 3 launches against 3 T.  Prints one JSON line per env.
fold      (mountaincar_continuous) ppo_rollout at 4096 x 128 with max_episode_steps = 7 -- FIN_LEN is at the limit on about 1 / 7 of the rows -- with
          ppo_env_truncation_bootstrap on and off, alternating on one context, 20 rollouts per timed window: the difference of the medians is the
          fold launch (with its counter's clear and copy)."""
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

NMB, EPOCHS, MAXS = 4, 4, 200
FOLD_ROLLOUTS = 20   # rollouts per timed window of the fold measurement (a window of one is 1.5 ms)
ENVS = {"pendulum": ("ENV_PENDULUM", 3, "Pendulum-v1"), "mountaincar_continuous": ("ENV_MOUNTAINCAR_CONTINUOUS", 2, "MountainCarContinuous-v0")}


def config(P, env_kind, N, T, obs=3, max_steps=MAXS):
    return P.make_config(env_kind=env_kind, dist_kind=P.DIST_GAUSSIAN, obs_size=obs, head_dims=(1,), num_envs=N, num_steps=T, num_minibatches=NMB,
                         update_epochs=EPOCHS, max_episode_steps=max_steps, seed=3, total_timesteps=1 << 40, learning_rate=1e-4, anneal_lr=False,
                         kernel_flags=P.KERNEL_GAUSS_FUSED)


def fold_cost(P, kind, obs, repeats, warmup, N=4096, T=128, limit=7):
    ctx = P.Context(config(P, kind, N, T, obs, limit))
    ctx.init_orthogonal(3)
    ctx.env_reset()
    times = {0: [], 1: []}
    for k in range(warmup + repeats):
        for on in (0, 1):
            ctx.env_truncation_bootstrap(bool(on))
            t = timed(lambda: [ctx.rollout() for _ in range(FOLD_ROLLOUTS)], ctx) / FOLD_ROLLOUTS
            if k >= warmup:
                times[on].append(t)
    events = int(ctx.env_truncations()[0].size)
    ctx.close()
    off_ms, on_ms = (1e3 * statistics.median(times[k]) for k in (0, 1))
    return {"envs": N, "steps": T, "max_episode_steps": limit, "events_last_rollout": events, "rows": N * T, "rollout_off_ms": round(off_ms, 4),
            "rollout_on_ms": round(on_ms, 4), "fold_ms": round(on_ms - off_ms, 4)}


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
    ap.add_argument("--env", choices=sorted(ENVS) + ["both"], default="pendulum")
    args = ap.parse_args()
    P = load_package()
    for name in (sorted(ENVS, reverse=True) if args.env == "both" else [args.env]):   # both: Pendulum first
        measure(P, args, name)


def measure(P, args, name):
    L = P.binding.lib()
    kind, obs, title = getattr(P, ENVS[name][0]), ENVS[name][1], ENVS[name][2]
    out = {"shape": "%s, obs %d, D 1, 2 x 64, %d minibatches x %d epochs" % (title, obs, NMB, EPOCHS), "repeats": args.repeats, "sizes": []}
    for N, T in ((4096, 128), (16384, 64)):
        fused = P.Context(config(P, kind, N, T, obs))
        host = P.Context(config(P, P.ENV_HOST, N, T, obs))
        env = P.Context(config(P, kind, N, T, obs))
        for c in (fused, host):
            c.init_orthogonal(3)
        fused.env_reset()
        host.host_env_reset(env.env_reset())
        d_act, d_obs = env.empty((N, 1), np.float32), env.empty((N, obs), np.float32)
        d_rew, d_done = env.empty(N, np.float32), env.empty(N, np.int32)
        env_stream = C.c_void_p(env.stream())

        def stepwise_rollout():
            host.host_rollout_begin()
            for _ in range(T):
                host.dev_act_f32(d_act, stream=env_stream)
                P.binding._check(L.ppo_env_step_f32(env.h, d_act.ptr, d_obs.ptr, d_rew.ptr, d_done.ptr), env.h)
                host.dev_observe(d_obs, d_rew, d_done, stream=env_stream)

        def one(which):
            if which == "fused":
                return timed(fused.train_iteration, fused), timed(fused.rollout, fused)
            roll = timed(stepwise_rollout, host, env)
            return roll + timed(host.host_rollout_end, host, env), roll

        for _ in range(args.warmup):
            for which in ("fused", "stepwise"):
                one(which)
        times = {"fused": [], "stepwise": []}
        for _ in range(args.repeats):
            for which in ("fused", "stepwise"):
                times[which].append(one(which))
        size = {"envs": N, "steps": T, "rollout_workgroups": (N + 63) // 64}
        for which in ("fused", "stepwise"):
            for k, key in enumerate(("iteration", "rollout")):
                rate = sorted(N * T / t[k] for t in times[which])
                size["%s_%s_Msteps_per_s" % (which, key)] = {"median": round(statistics.median(rate) / 1e6, 2), "min": round(rate[0] / 1e6, 2),
                                                              "max": round(rate[-1] / 1e6, 2)}
                size["%s_%s_ms" % (which, key)] = round(1e3 * statistics.median(t[k] for t in times[which]), 4)
        size["fused_rollout_faster"] = size["fused_rollout_ms"] < size["stepwise_rollout_ms"]
        size["fused_iteration_faster"] = size["fused_iteration_ms"] < size["stepwise_iteration_ms"]
        out["sizes"].append(size)
        for c in (fused, host, env):
            c.close()
    if name == "mountaincar_continuous":
        out["fold"] = fold_cost(P, kind, obs, args.repeats, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
