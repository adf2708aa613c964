"""What reward normalisation of a fused device env costs (PPO_KERNEL_ENV_REWARD_NORM + ppo_reward_norm_enable): one GPU, 4096 envs x 128 steps, every variant
alternating in one process, 2 warm-up + 7 timed windows.

    python tools/env_reward_norm_cost.py [--repeats 7] [--warmup 2] [--envs 4096] [--steps 128] [--only pendulum acrobot frozenlake8x8]

rollout    ppo_rollout alone (the rollout kernel, the two critic launches and whatever the normaliser adds), three ways: the unflagged context; the flagged one
           with mode 0 (which must run what the unflagged one runs: the two figures should sit inside each other's spread); the flagged one with mode 1
           (three more launches: rewnorm_scan_kernel, rewnorm_moments_kernel, rewnorm_merge_apply_kernel).  A window is 50 rollouts.
yardstick  the route that existed: one launch of rewnorm_update_apply_kernel per env step.  A device-fed PPO_ENV_HOST context (2 x 64, obs_size 4) at the same
           N runs the T ppo_dev_act / ppo_dev_observe pairs of a rollout with reward normalisation on against off (two contexts, the same arrays); the
           difference per step, times T, is what T per-step launches cost a rollout.  A window is 4 rollouts' pairs (ppo_host_rollout_end, with its update, runs
           outside the clock).
Every timing is a host clock around work that ends in a synchronisation; per window the mean over its rollouts, then median with min .. max over the
windows, in milliseconds.  Nothing is asserted and no bar is set.  Prints one JSON line per env and one for the yardstick."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

WINDOW, HOST_WINDOW = 50, 4
ENVS = {   # name -> (env_kind, dist_kind, obs_size, actions, family flag, max_episode_steps)
    "pendulum": ("ENV_PENDULUM", "DIST_GAUSSIAN", 3, 1, "KERNEL_GAUSS_FUSED", 200),
    "acrobot": ("ENV_ACROBOT", "DIST_CATEGORICAL", 6, 3, "KERNEL_CAT_FUSED", 500),
    "frozenlake8x8": ("ENV_FROZENLAKE8X8", "DIST_CATEGORICAL", 64, 4, "KERNEL_CAT_FUSED", 200),
}


def summary(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def rollout_window(ctx):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(WINDOW):
        ctx.rollout()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0) / WINDOW


def measure(P, name, args):
    kind, dist, obs, actions, family, limit = ENVS[name]

    def ctx(flagged):
        c = P.Context(P.make_config(env_kind=getattr(P, kind), dist_kind=getattr(P, dist), obs_size=obs, head_dims=(actions,), num_envs=args.envs,
                                    num_steps=args.steps, num_minibatches=4, update_epochs=4, max_episode_steps=limit, seed=3, total_timesteps=1 << 40,
                                    learning_rate=1e-4, anneal_lr=False, kernel_flags=getattr(P, family) | (P.KERNEL_ENV_REWARD_NORM if flagged else 0)))
        c.init_orthogonal(3)
        c.env_reset()
        return c

    plain, off, on = ctx(False), ctx(True), ctx(True)
    off.reward_norm_enable(0)
    on.reward_norm_enable(1)
    variants = [("rollout_unflagged", plain), ("rollout_flagged_mode0", off), ("rollout_flagged_mode1", on)]
    times = {v[0]: [] for v in variants}
    for k in range(args.warmup + args.repeats):
        for label, c in variants:
            t = rollout_window(c)
            if k >= args.warmup:
                times[label].append(t)
    out = {"env": name, "envs": args.envs, "steps": args.steps, "max_episode_steps": limit, "windows": args.repeats, "rollouts_per_window": WINDOW}
    for label in times:
        out[label + "_ms"] = summary(times[label])
    out["mode0_minus_unflagged_ms"] = round(out["rollout_flagged_mode0_ms"]["median"] - out["rollout_unflagged_ms"]["median"], 4)
    out["mode1_cost_ms"] = round(out["rollout_flagged_mode1_ms"]["median"] - out["rollout_flagged_mode0_ms"]["median"], 4)
    out["return_variance"] = round(on.reward_norm_get()[1], 4)
    for c in (plain, off, on):
        c.close()
    print(json.dumps(out), flush=True)
    return out


def yardstick(P, args):
    """the per-step route: T act / observe pairs of a device-fed PPO_ENV_HOST context, reward normalisation on against off"""
    N, T, O = args.envs, args.steps, 4
    rng = np.random.default_rng(0)

    def ctx(on):
        c = P.Context(P.make_config(env_kind=P.ENV_HOST, obs_size=O, head_dims=(2,), num_envs=N, num_steps=T, num_minibatches=4, update_epochs=1, seed=3,
                                    total_timesteps=1 << 40, learning_rate=1e-4, anneal_lr=False))
        c.init_orthogonal(3)
        if on:
            c.reward_norm_enable(1)
        arrays = (c.dev(rng.standard_normal((N, O)).astype(np.float32)), c.dev((10.0 * rng.standard_normal(N)).astype(np.float32)),
                  c.dev((rng.random(N) < 0.01).astype(np.int32)), c.empty((N, c.H), np.int64))
        c.dev_env_reset(arrays[0])
        return c, arrays

    def window(c, arrays):
        obs, rew, done, act = arrays
        total = 0.0
        for _ in range(HOST_WINDOW):
            c.host_rollout_begin()
            c.sync()
            t0 = time.perf_counter()
            for _ in range(T):
                c.dev_act(act)
                c.dev_observe(obs, rew, done)
            c.sync()
            total += time.perf_counter() - t0
            c.host_rollout_end()
        return 1e3 * total / HOST_WINDOW

    variants = [("host_pairs_norm_off", ctx(False)), ("host_pairs_norm_on", ctx(True))]
    times = {v[0]: [] for v in variants}
    for k in range(args.warmup + args.repeats):
        for label, (c, arrays) in variants:
            t = window(c, arrays)
            if k >= args.warmup:
                times[label].append(t)
    out = {"yardstick": "T launches of rewnorm_update_apply_kernel", "envs": N, "steps": T, "windows": args.repeats, "rollouts_per_window": HOST_WINDOW}
    for label in times:
        out[label + "_ms"] = summary(times[label])
    out["per_step_route_cost_ms"] = round(out["host_pairs_norm_on_ms"]["median"] - out["host_pairs_norm_off_ms"]["median"], 4)
    out["per_step_us"] = round(1e3 * out["per_step_route_cost_ms"] / T, 3)
    for _, (c, _) in variants:
        c.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--only", nargs="+", choices=sorted(ENVS), default=list(ENVS))
    args = ap.parse_args()
    P = load_package()
    for name in args.only:
        measure(P, name, args)
    yardstick(P, args)


if __name__ == "__main__":
    main()
