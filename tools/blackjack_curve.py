"""Does PPO learn Blackjack on the device?  PPO_ENV_BLACKJACK (gymnasium's Blackjack-v1, natural = False, sab = False, the infinite deck), 512 envs x 64 steps,
max_episode_steps 100 (an episode takes at most 20 steps: nothing is ever cut off).

    python tools/blackjack_curve.py [--iters 60] [--eval-every 10] [--seeds 1 2 3] [--lr 2.5e-3] ...

Hyper-parameters (the defaults below): gamma 1.0 (episodes are short and the return is the one reward at the end), gae_lambda 0.95, learning rate 2.5e-3
without annealing, 4 epochs x 4 minibatches of 8 192 rows, clip 0.2, ent_coef 0.01, vf_coef 0.5, max_grad_norm 0.5, norm_adv on, clip_vloss off, orthogonal
init.  Per evaluated iteration it prints the mean SAMPLED return of ppo_evaluate over 16 384 fixed episodes (reset 0 of envs 0 .. 16 383 under seed 0: each
episode with its own key, so its own deal and its own deck); a return is -1, 0 or +1, so the standard error of that mean is at most 1 / sqrt(16 384) = 0.0079.
Iteration 0 is the control, the untrained policy.  The model's yardsticks (tests/test_blackjack_cpu.py, exact dynamic programming): a uniformly random policy
returns -0.3958960, always sticking -0.1863677, the optimum -0.0465560.  Prints one JSON line at the end: per seed the untrained and the final mean return,
the curve and the training seconds (evaluations excluded)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

N, T, EVAL_EPISODES, EVAL_SEED = 512, 64, 16384, 0
MAXS = 100            # never met: an episode takes at most 20 steps
RANDOM_RETURN = -0.3958960
STICK_RETURN = -0.1863677
OPTIMUM = -0.0465560


def sampled_return(ctx):
    """mean undiscounted return of EVAL_EPISODES sampled episodes (one launch: cat_eval_kernel)"""
    return float(ctx.evaluate(EVAL_EPISODES, EVAL_SEED, greedy=False)[0]["return_mean"])


def make_ctx(P, seed, a):
    return P.Context(P.make_config(env_kind=P.ENV_BLACKJACK, dist_kind=P.DIST_CATEGORICAL, obs_size=45, head_dims=(2,), num_envs=N, num_steps=T,
                                   num_minibatches=a.minibatches, update_epochs=a.epochs, max_episode_steps=MAXS, seed=seed, total_timesteps=1 << 40,
                                   learning_rate=a.lr, anneal_lr=False, gamma=a.gamma, gae_lambda=a.gae_lambda, clip_coef=0.2, ent_coef=a.ent_coef, vf_coef=0.5,
                                   max_grad_norm=0.5, norm_adv=True, clip_vloss=False, kernel_flags=P.KERNEL_CAT_FUSED))


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--eval-every", type=int, default=10)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--lr", type=float, default=2.5e-3)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--ent-coef", type=float, default=0.01)
    return ap.parse_args(argv)


def main():
    a = parse()
    P = load_package()
    out = {"envs": N, "steps": T, "max_episode_steps": MAXS, "iters": a.iters, "eval_episodes": EVAL_EPISODES, "random_policy": RANDOM_RETURN,
           "always_stick": STICK_RETURN, "optimum": OPTIMUM, "hyper": {k: getattr(a, k) for k in ("gamma", "gae_lambda", "lr", "epochs", "minibatches", "ent_coef")}, "seeds": []}
    for seed in a.seeds:
        ctx = make_ctx(P, seed, a)
        ctx.init_orthogonal(seed)
        ctx.env_reset()
        first = last = sampled_return(ctx)
        curve = [round(first, 4)]
        print("seed %d iteration %4d mean return %8.4f (untrained)" % (seed, 0, first), flush=True)
        train_s = 0.0
        for it in range(1, a.iters + 1):
            t0 = time.perf_counter()
            ctx.train_iteration()
            if it % a.eval_every == 0 or it == a.iters:
                ctx.sync()
                train_s += time.perf_counter() - t0
                last = sampled_return(ctx)
                curve.append(round(last, 4))
                print("seed %d iteration %4d mean return %8.4f" % (seed, it, last), flush=True)
            else:
                train_s += time.perf_counter() - t0
        out["seeds"].append({"seed": seed, "untrained": round(first, 4), "final": round(last, 4), "curve": curve, "train_seconds": round(train_s, 2)})
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
