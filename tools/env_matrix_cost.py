"""What PPO_KERNEL_ENV_MATRIX buys: each of the seven fused device envs at 4096 envs x 128 steps with the flag (kernels_env_matrix.hip: the one-launch rollout
behind the resident f32 matrix-core forward; act, critic and update on kernels_fused_matrix.hip) against the same context without it (the family's vector
kernels), alternated in one process on one GPU.

    python tools/env_matrix_cost.py [--repeats 7] [--warmup 2]

Per env and path, over the timed repeats, median and range of
  rollout_ms     one ppo_rollout (the one launch and its two critic launches): enqueue to completion, a synchronisation in front and behind
  iteration_ms   one whole iteration (rollout, advantages, 4 epochs x 4 minibatches), likewise
There is no threshold: the flag is opt-in either way, and every cell is reported, the ones the flag loses included.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

N, T = 4096, 128


def envs(P):
    """name -> (env_kind, dist_kind, obs_size, actions, family flag)"""
    g, c = P.KERNEL_GAUSS_FUSED, P.KERNEL_CAT_FUSED
    return {"Pendulum": (P.ENV_PENDULUM, P.DIST_GAUSSIAN, 3, 1, g), "MountainCarContinuous": (P.ENV_MOUNTAINCAR_CONTINUOUS, P.DIST_GAUSSIAN, 2, 1, g),
            "Acrobot": (P.ENV_ACROBOT, P.DIST_CATEGORICAL, 6, 3, c), "Taxi (masked)": (P.ENV_TAXI, P.DIST_MASKED, 19, 6, c),
            "FrozenLake 4x4": (P.ENV_FROZENLAKE, P.DIST_CATEGORICAL, 16, 4, c), "FrozenLake 8x8": (P.ENV_FROZENLAKE8X8, P.DIST_CATEGORICAL, 64, 4, c),
            "Blackjack": (P.ENV_BLACKJACK, P.DIST_CATEGORICAL, 45, 2, c)}


def make(P, env, flags):
    kind, dist, obs, actions, family = envs(P)[env]
    ctx = P.Context(P.make_config(env_kind=kind, dist_kind=dist, obs_size=obs, head_dims=(actions,), num_envs=N, num_steps=T, num_minibatches=4, update_epochs=4,
                                  max_episode_steps=200, seed=3, total_timesteps=1 << 30, learning_rate=3e-4, anneal_lr=False, gamma=0.99, gae_lambda=0.95,
                                  ent_coef=0.01, kernel_flags=family | flags))
    ctx.init_orthogonal(3)
    ctx.env_reset()
    return ctx


def timed_ms(ctx, call):
    ctx.sync()
    t0 = time.perf_counter()
    call()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    P = load_package()
    out = {"envs": N, "steps": T, "repeats": args.repeats, "rows": []}
    for env in envs(P):
        ctxs = {"vector": make(P, env, 0), "matrix": make(P, env, P.KERNEL_ENV_MATRIX)}
        times = {name: [] for name in ctxs}
        for rep in range(args.warmup + args.repeats):
            for name, ctx in ctxs.items():
                t = (timed_ms(ctx, ctx.rollout), timed_ms(ctx, ctx.train_iteration))
                if rep >= args.warmup:
                    times[name].append(t)
        row = {"env": env}
        for k, key in enumerate(("rollout_ms", "iteration_ms")):
            row[key] = {}
            for name in ctxs:
                v = [t[k] for t in times[name]]
                row[key].update({name + "_median": statistics.median(v), name + "_min": min(v), name + "_max": max(v)})
        out["rows"].append(row)
        for ctx in ctxs.values():
            ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
