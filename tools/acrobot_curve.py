"""Does the fused categorical path learn on its device env?  PPO on Acrobot-v1 (PPO_ENV_ACROBOT), 1024 envs x 64 steps, max_episode_steps 200, five seeds.

    python tools/acrobot_curve.py [--iters 50] [--eval-every 10] [--seeds 1 2 3 4 5] [--gamma 0.99] [--lr 1e-3] [--epochs 4] [--minibatches 4] ...

Hyper-parameters (the defaults below): gamma 0.99, gae_lambda 0.95, learning rate 1e-3 without annealing, 4 epochs x 4 minibatches of 16 384 rows, clip 0.2,
ent_coef 0.01, vf_coef 0.5, max_grad_norm 0.5, norm_adv on, clip_vloss off (returns are of order -100), orthogonal init.  50 iterations = 3.3 M env steps
take 0.15 s of training on an MI355X; four of five seeds are at -84 after 10 iterations, the fifth after 50 (profiles/NOTES.md has the curves to 150).
Per evaluated iteration it prints the mean GREEDY return of ppo_evaluate over 256 fixed start states (reset 0 of envs 0 .. 255 under seed 0), at most 200
steps each; iteration 0 is the control, the untrained policy on the same start states, which sits at or near -200 (a policy that never swings up).
Prints one JSON line at the end: per seed the untrained and the final return, the improvement, the training seconds (evaluations excluded)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

N, T, MAXS, EVAL_EPISODES, EVAL_SEED = 1024, 64, 200, 256, 0


def greedy_return(ctx):
    """mean undiscounted return of EVAL_EPISODES greedy episodes from the fixed start states (one launch: cat_eval_kernel)"""
    return float(ctx.evaluate(EVAL_EPISODES, EVAL_SEED, greedy=True)[0]["return_mean"])


def make_ctx(P, seed, a):
    return P.Context(P.make_config(env_kind=P.ENV_ACROBOT, dist_kind=P.DIST_CATEGORICAL, obs_size=6, head_dims=(3,), num_envs=N, num_steps=T,
                                   num_minibatches=a.minibatches, update_epochs=a.epochs, max_episode_steps=MAXS, seed=seed, total_timesteps=1 << 40,
                                   learning_rate=a.lr, anneal_lr=False, gamma=a.gamma, gae_lambda=a.gae_lambda, clip_coef=0.2, ent_coef=a.ent_coef, vf_coef=0.5,
                                   max_grad_norm=0.5, norm_adv=True, clip_vloss=False, kernel_flags=P.KERNEL_CAT_FUSED))


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--eval-every", type=int, default=10)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3, 4, 5])
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--ent-coef", type=float, default=0.01)
    return ap.parse_args(argv)


def main():
    a = parse()
    P = load_package()
    out = {"envs": N, "steps": T, "iters": a.iters, "hyper": {k: getattr(a, k) for k in ("gamma", "gae_lambda", "lr", "epochs", "minibatches", "ent_coef")}, "seeds": []}
    for seed in a.seeds:
        ctx = make_ctx(P, seed, a)
        ctx.init_orthogonal(seed)
        ctx.env_reset()
        first = last = greedy_return(ctx)
        print("seed %d iteration %4d greedy return %9.2f (untrained)" % (seed, 0, first), flush=True)
        train_s = 0.0
        for it in range(1, a.iters + 1):
            t0 = time.perf_counter()
            ctx.train_iteration()
            if it % a.eval_every == 0 or it == a.iters:
                ctx.sync()
                train_s += time.perf_counter() - t0
                last = greedy_return(ctx)
                print("seed %d iteration %4d greedy return %9.2f" % (seed, it, last), flush=True)
            else:
                train_s += time.perf_counter() - t0
        st = ctx.stats()
        out["seeds"].append({"seed": seed, "untrained": round(first, 2), "final": round(last, 2), "improvement": round(last - first, 2),
                             "train_seconds": round(train_s, 2), "ep_rew_mean": round(st["ep_rew_mean"], 2)})
        ctx.close()
    imp = [s["improvement"] for s in out["seeds"]]
    out["rises_in_every_seed"] = all(x > 0 for x in imp)
    out["smallest_improvement"] = min(imp)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
