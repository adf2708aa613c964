"""What is the action mask worth, and what is the time-limit bootstrap worth?  PPO on Taxi-v3 (PPO_ENV_TAXI), 512 envs x 64 steps, max_episode_steps 200.

    python tools/taxi_curve.py [--iters 60] [--eval-every 5] [--seeds 1 2 3] [--arms masked+boot masked unmasked+boot unmasked] [--lr 2.5e-3] ...

Four arms on the same seeds: PPO_DIST_MASKED against PPO_DIST_CATEGORICAL (the same env, PPO_BUF_MASKS all ones, the policy unmasked), each with
ppo_env_truncation_bootstrap on and off.  Hyper-parameters (the defaults below): gamma 0.99, gae_lambda 0.95, learning rate 2.5e-3 without annealing, 4 epochs
x 4 minibatches of 8 192 rows, clip 0.2, ent_coef 0.01, vf_coef 0.5, max_grad_norm 0.5, norm_adv on, clip_vloss off (returns are of order -100), orthogonal
init.  Per evaluated iteration it prints the mean SAMPLED return of ppo_evaluate over 512 fixed start states (reset 0 of envs 0 .. 511 under seed 0), at most
200 steps each; iteration 0 is the control, the untrained policy.  The model's yardsticks (tests/test_taxi_cpu.py): a uniformly random policy over the
allowed actions returns about -186.7, over all six about -769.8; the optimum is 2379 / 300 = 7.93.  Prints one JSON line at the end: per arm and seed the
untrained and the final return and the training seconds (evaluations excluded)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

N, T, MAXS, EVAL_EPISODES, EVAL_SEED = 512, 64, 200, 512, 0
ARMS = {"masked+boot": (True, True), "masked": (True, False), "unmasked+boot": (False, True), "unmasked": (False, False)}


def sampled_return(ctx):
    """mean undiscounted return of EVAL_EPISODES sampled episodes from the fixed start states (one launch: cat_eval_kernel)"""
    return float(ctx.evaluate(EVAL_EPISODES, EVAL_SEED, greedy=False)[0]["return_mean"])


def make_ctx(P, seed, a, masked=True, bootstrap=True):
    ctx = P.Context(P.make_config(env_kind=P.ENV_TAXI, dist_kind=P.DIST_MASKED if masked else P.DIST_CATEGORICAL, obs_size=19, head_dims=(6,), num_envs=N,
                                  num_steps=T, num_minibatches=a.minibatches, update_epochs=a.epochs, max_episode_steps=MAXS, seed=seed, total_timesteps=1 << 40,
                                  learning_rate=a.lr, anneal_lr=False, gamma=a.gamma, gae_lambda=a.gae_lambda, clip_coef=0.2, ent_coef=a.ent_coef, vf_coef=0.5,
                                  max_grad_norm=0.5, norm_adv=True, clip_vloss=False, kernel_flags=P.KERNEL_CAT_FUSED))
    if bootstrap:
        ctx.env_truncation_bootstrap(True)
    return ctx


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--eval-every", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--arms", nargs="+", default=list(ARMS), choices=list(ARMS))
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--lr", type=float, default=2.5e-3)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--ent-coef", type=float, default=0.01)
    return ap.parse_args(argv)


def main():
    a = parse()
    P = load_package()
    out = {"envs": N, "steps": T, "iters": a.iters, "hyper": {k: getattr(a, k) for k in ("gamma", "gae_lambda", "lr", "epochs", "minibatches", "ent_coef")}, "arms": {}}
    for arm in a.arms:
        masked, boot = ARMS[arm]
        rows = []
        for seed in a.seeds:
            ctx = make_ctx(P, seed, a, masked, boot)
            ctx.init_orthogonal(seed)
            ctx.env_reset()
            first = last = sampled_return(ctx)
            curve = [round(first, 2)]
            print("%-14s seed %d iteration %4d sampled return %9.2f (untrained)" % (arm, seed, 0, first), flush=True)
            train_s = 0.0
            for it in range(1, a.iters + 1):
                t0 = time.perf_counter()
                ctx.train_iteration()
                if it % a.eval_every == 0 or it == a.iters:
                    ctx.sync()
                    train_s += time.perf_counter() - t0
                    last = sampled_return(ctx)
                    curve.append(round(last, 2))
                    print("%-14s seed %d iteration %4d sampled return %9.2f" % (arm, seed, it, last), flush=True)
                else:
                    train_s += time.perf_counter() - t0
            rows.append({"seed": seed, "untrained": round(first, 2), "final": round(last, 2), "curve": curve, "train_seconds": round(train_s, 2)})
            ctx.close()
        out["arms"][arm] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
