"""Does PPO learn the slippery FrozenLake on the device?  PPO_ENV_FROZENLAKE (4x4, max_episode_steps 100) or PPO_ENV_FROZENLAKE8X8 (8x8, 200), 512 envs x 64
steps.

    python tools/frozenlake_curve.py [--side 4] [--iters 40] [--eval-every 5] [--seeds 1 2 3] [--lr 2.5e-3] ...

Hyper-parameters (the defaults below): gamma 0.99, gae_lambda 0.95, learning rate 2.5e-3 without annealing, 4 epochs x 4 minibatches of 8 192 rows, clip 0.2,
ent_coef 0.01, vf_coef 0.5, max_grad_norm 0.5, norm_adv on, clip_vloss off, orthogonal init.  Per evaluated iteration it prints the mean SAMPLED return of
ppo_evaluate over 512 fixed episodes (reset 0 of envs 0 .. 511 under seed 0: every episode starts in cell 0, each with its own key), which is the success
rate: a return is 0 or 1.  Iteration 0 is the control, the untrained policy.  The model's yardsticks (tests/test_frozenlake_cpu.py): a uniformly random
policy succeeds in 0.0139 (4x4, 100 steps) resp. 0.0019 (8x8, 200 steps) of its episodes; the optimum within the limit is 0.7442 resp. 0.9132.  Prints one
JSON line at the end: per seed the untrained and the final success rate, the curve and the training seconds (evaluations excluded)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

N, T, EVAL_EPISODES, EVAL_SEED = 512, 64, 512, 0
MAXS = {4: 100, 8: 200}   # gymnasium's time limits
RANDOM_SUCCESS = {4: 0.0139398, 8: 0.0019014}
OPTIMUM = {4: 0.7441903, 8: 0.9132202}


def sampled_return(ctx):
    """mean undiscounted return -- the success rate -- of EVAL_EPISODES sampled episodes (one launch: cat_eval_kernel)"""
    return float(ctx.evaluate(EVAL_EPISODES, EVAL_SEED, greedy=False)[0]["return_mean"])


def make_ctx(P, seed, a):
    kind = P.ENV_FROZENLAKE8X8 if a.side == 8 else P.ENV_FROZENLAKE
    return P.Context(P.make_config(env_kind=kind, dist_kind=P.DIST_CATEGORICAL, obs_size=a.side * a.side, head_dims=(4,), num_envs=N, num_steps=T,
                                   num_minibatches=a.minibatches, update_epochs=a.epochs, max_episode_steps=MAXS[a.side], seed=seed, total_timesteps=1 << 40,
                                   learning_rate=a.lr, anneal_lr=False, gamma=a.gamma, gae_lambda=a.gae_lambda, clip_coef=0.2, ent_coef=a.ent_coef, vf_coef=0.5,
                                   max_grad_norm=0.5, norm_adv=True, clip_vloss=False, kernel_flags=P.KERNEL_CAT_FUSED))


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4, choices=[4, 8])
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--eval-every", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
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
    out = {"side": a.side, "envs": N, "steps": T, "max_episode_steps": MAXS[a.side], "iters": a.iters, "random_policy": RANDOM_SUCCESS[a.side],
           "optimum": OPTIMUM[a.side], "hyper": {k: getattr(a, k) for k in ("gamma", "gae_lambda", "lr", "epochs", "minibatches", "ent_coef")}, "seeds": []}
    for seed in a.seeds:
        ctx = make_ctx(P, seed, a)
        ctx.init_orthogonal(seed)
        ctx.env_reset()
        first = last = sampled_return(ctx)
        curve = [round(first, 4)]
        print("seed %d iteration %4d success rate %7.4f (untrained)" % (seed, 0, first), flush=True)
        train_s = 0.0
        for it in range(1, a.iters + 1):
            t0 = time.perf_counter()
            ctx.train_iteration()
            if it % a.eval_every == 0 or it == a.iters:
                ctx.sync()
                train_s += time.perf_counter() - t0
                last = sampled_return(ctx)
                curve.append(round(last, 4))
                print("seed %d iteration %4d success rate %7.4f" % (seed, it, last), flush=True)
            else:
                train_s += time.perf_counter() - t0
        out["seeds"].append({"seed": seed, "untrained": round(first, 4), "final": round(last, 4), "curve": curve, "train_seconds": round(train_s, 2)})
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
