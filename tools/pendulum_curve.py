"""Does the Gaussian path learn?  PPO on the device's Pendulum-v1 (PPO_ENV_PENDULUM), 1024 envs x 64 steps, max_episode_steps 200, five seeds.

    python tools/pendulum_curve.py [--iters 300] [--eval-every 1] [--seeds 1 2 3 4 5] [--gamma 0.95] [--lr 3e-4] [--epochs 10] [--minibatches 8] ...

Hyper-parameters (the defaults below): gamma 0.95 and gae_lambda 0.95 (the rewards are unnormalised, up to -16 a step -- these settings were chosen
without PPO_KERNEL_ENV_REWARD_NORM, tools/env_reward_norm_curve.py runs them with it: a short horizon keeps the returns small), learning rate 3e-4 without annealing, 10 epochs x 8 minibatches of 8192 rows, clip 0.2,
ent_coef 0, vf_coef 0.5, max_grad_norm 0.5, norm_adv on, clip_vloss off (a value clip of 0.2 on returns of order -100 would freeze the critic),
orthogonal init, log_std 0.  300 iterations = 19.7 M env steps take 2.3 s of training on an MI355X (profiles/NOTES.md has the curves; gamma 0.9 with
lr 1e-3 gets to -245 in 30 iterations and then wanders).
Per evaluated iteration it prints the mean GREEDY return over 256 fixed start states (theta ~ U(-pi, pi), theta_dot ~ U(-1, 1), numpy seed 0), 200 steps
each, stepped through policy_act_f32(greedy=True) and env_transition_f32; iteration 0 is the control, the untrained policy on the same start states.
Prints one JSON line at the end: per seed the untrained and the final return, the improvement, the training seconds (evaluations excluded)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

N, T, MAXS, EVAL_STATES = 1024, 64, 200, 256


def start_states():
    rng = np.random.default_rng(0)
    return np.stack([rng.uniform(-np.pi, np.pi, EVAL_STATES), rng.uniform(-1, 1, EVAL_STATES)], 1).astype(np.float32)


def greedy_return(P, ctx, states, steps=MAXS):
    """mean over the start states of the undiscounted return of `steps` greedy steps (float64 sum of the f32 rewards)"""
    s = states
    obs = np.stack([np.cos(s[:, 0].astype(np.float64)), np.sin(s[:, 0].astype(np.float64)), s[:, 1]], 1).astype(np.float32)
    total = np.zeros(len(s), np.float64)
    for _ in range(steps):
        a = ctx.policy_act_f32(obs, greedy=True)[0]
        s, obs, r, _ = P.env_transition_f32(ctx, P.ENV_PENDULUM, s, a)
        total += r
    return float(total.mean())


def make_ctx(P, seed, a):
    return P.Context(P.make_config(env_kind=P.ENV_PENDULUM, dist_kind=P.DIST_GAUSSIAN, obs_size=3, head_dims=(1,), num_envs=N, num_steps=T,
                                   num_minibatches=a.minibatches, update_epochs=a.epochs, max_episode_steps=MAXS, seed=seed, total_timesteps=1 << 40,
                                   learning_rate=a.lr, anneal_lr=False, gamma=a.gamma, gae_lambda=a.gae_lambda, clip_coef=0.2, ent_coef=a.ent_coef, vf_coef=0.5,
                                   max_grad_norm=0.5, norm_adv=True, clip_vloss=False, kernel_flags=P.KERNEL_GAUSS_FUSED))


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--eval-every", type=int, default=1)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3, 4, 5])
    ap.add_argument("--gamma", type=float, default=0.95)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--minibatches", type=int, default=8)
    ap.add_argument("--ent-coef", type=float, default=0.0)
    return ap.parse_args(argv)


def main():
    a = parse()
    P = load_package()
    states = start_states()
    out = {"envs": N, "steps": T, "iters": a.iters, "hyper": {k: getattr(a, k) for k in ("gamma", "gae_lambda", "lr", "epochs", "minibatches", "ent_coef")}, "seeds": []}
    for seed in a.seeds:
        ctx = make_ctx(P, seed, a)
        ctx.init_orthogonal(seed)
        ctx.env_reset()
        first = last = greedy_return(P, ctx, states)
        print("seed %d iteration %4d greedy return %9.2f (untrained)" % (seed, 0, first), flush=True)
        train_s = 0.0
        for it in range(1, a.iters + 1):
            t0 = time.perf_counter()
            ctx.train_iteration()
            if it % a.eval_every == 0 or it == a.iters:
                ctx.sync()
                train_s += time.perf_counter() - t0
                last = greedy_return(P, ctx, states)
                print("seed %d iteration %4d greedy return %9.2f" % (seed, it, last), flush=True)
            else:
                train_s += time.perf_counter() - t0
        st = ctx.stats()
        out["seeds"].append({"seed": seed, "untrained": round(first, 2), "final": round(last, 2), "improvement": round(last - first, 2),
                             "train_seconds": round(train_s, 2), "ep_rew_mean": round(st["ep_rew_mean"], 2), "log_std": round(float(ctx.get_params()[-1]), 3)})
        ctx.close()
    imp = [s["improvement"] for s in out["seeds"]]
    out["rises_in_every_seed"] = all(x > 0 for x in imp)
    out["smallest_improvement"] = min(imp)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
