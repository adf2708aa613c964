"""Does reward normalisation change what the fused device envs learn?  PPO on PPO_ENV_PENDULUM, PPO_ENV_MOUNTAINCAR_CONTINUOUS and PPO_ENV_TAXI with
PPO_KERNEL_ENV_REWARD_NORM, ppo_reward_norm_enable off against on (mode 1, clip 10, eps 1e-8), three seeds each.

    python tools/env_reward_norm_curve.py [--seeds 1 2 3] [--env pendulum mcc taxi] [--pendulum-iters 300] [--mcc-iters 300] [--taxi-iters 60] [--checkpoints 6]

Hyper-parameters, sizes and metric are the env's own curve tool's, imported from there: tools/pendulum_curve.py (1024 envs x 64 steps, limit 200, mean GREEDY
return over 256 fixed start states) and tools/taxi_curve.py (512 x 64, limit 200, masked, time-limit bootstrap on, mean SAMPLED return of ppo_evaluate over
512 fixed start states).  MountainCarContinuous has no curve tool: it runs Pendulum's hyper-parameters and sizes with its own limit of 999, judged by the mean
greedy return of ppo_evaluate over 256 fixed start states.  The metric is the raw, undiscounted return: it does not depend on the normaliser, so both variants
are judged alike.  Those hyper-parameters were chosen WITHOUT a normaliser (a short horizon, clip_vloss off, because the returns are large); nothing is
retuned here.  Prints one line per (env, seed, variant, checkpoint) and one JSON line per env.  Nothing is asserted: the table is written down whatever it shows."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

import pendulum_curve  # noqa: E402
import taxi_curve  # noqa: E402

MCC_LIMIT, MCC_EVAL_EPISODES, MCC_EVAL_SEED = 999, 256, 0


def flagged(P, build):
    """build()'s context with PPO_KERNEL_ENV_REWARD_NORM beside its family flag"""
    make = P.make_config

    def with_flag(**kw):
        kw["kernel_flags"] |= P.KERNEL_ENV_REWARD_NORM
        return make(**kw)

    P.make_config = with_flag
    try:
        return build()
    finally:
        P.make_config = make


def mcc_ctx(P, seed, a):
    return P.Context(P.make_config(env_kind=P.ENV_MOUNTAINCAR_CONTINUOUS, dist_kind=P.DIST_GAUSSIAN, obs_size=2, head_dims=(1,), num_envs=pendulum_curve.N,
                                   num_steps=pendulum_curve.T, num_minibatches=a.minibatches, update_epochs=a.epochs, max_episode_steps=MCC_LIMIT, seed=seed,
                                   total_timesteps=1 << 40, learning_rate=a.lr, anneal_lr=False, gamma=a.gamma, gae_lambda=a.gae_lambda, clip_coef=0.2,
                                   ent_coef=a.ent_coef, vf_coef=0.5, max_grad_norm=0.5, norm_adv=True, clip_vloss=False, kernel_flags=P.KERNEL_GAUSS_FUSED))


def plan(P, env):
    """-> (context builder (seed), metric (ctx), description)"""
    if env == "pendulum":
        hyper, states = pendulum_curve.parse([]), pendulum_curve.start_states()
        return (lambda seed: pendulum_curve.make_ctx(P, seed, hyper)), (lambda c: pendulum_curve.greedy_return(P, c, states)), "greedy return, 256 start states"
    if env == "mcc":
        hyper = pendulum_curve.parse([])
        return ((lambda seed: mcc_ctx(P, seed, hyper)), (lambda c: float(c.evaluate(MCC_EVAL_EPISODES, MCC_EVAL_SEED, greedy=True)[0]["return_mean"])),
                "greedy return of ppo_evaluate, 256 start states")
    hyper = taxi_curve.parse([])
    return (lambda seed: taxi_curve.make_ctx(P, seed, hyper, True, True)), taxi_curve.sampled_return, "sampled return of ppo_evaluate, 512 start states"


def run(P, env, seeds, iters, checkpoints):
    build, metric, what = plan(P, env)
    at = sorted({round(iters * k / checkpoints) for k in range(checkpoints + 1)})
    curves, final_var = {False: [], True: []}, []
    for seed in seeds:
        for on in (False, True):
            ctx = flagged(P, lambda: build(seed))
            ctx.init_orthogonal(seed)
            ctx.env_reset()
            if on:
                ctx.reward_norm_enable()
            curve = []
            for it in range(iters + 1):
                if it:
                    ctx.train_iteration()
                if it in at:
                    curve.append(metric(ctx))
                    print("%s seed %d norm_reward %-3s iteration %4d return %9.2f" % (env, seed, "on" if on else "off", it, curve[-1]), flush=True)
            if on:
                final_var.append(round(ctx.reward_norm_get()[1], 4))
            curves[on].append(curve)
            ctx.close()
    mean = lambda rows: [round(sum(r[k] for r in rows) / len(rows), 2) for k in range(len(at))]   # noqa: E731
    print(json.dumps({"env": env, "metric": what, "seeds": list(seeds), "iterations": at, "mean_return_norm_off": mean(curves[False]),
                      "mean_return_norm_on": mean(curves[True]), "per_seed_final_off": [round(c[-1], 2) for c in curves[False]],
                      "per_seed_final_on": [round(c[-1], 2) for c in curves[True]], "return_variance_on": final_var}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--env", nargs="+", choices=["pendulum", "mcc", "taxi"], default=["pendulum", "mcc", "taxi"])
    ap.add_argument("--pendulum-iters", type=int, default=300)
    ap.add_argument("--mcc-iters", type=int, default=300)
    ap.add_argument("--taxi-iters", type=int, default=60)
    ap.add_argument("--checkpoints", type=int, default=6)
    a = ap.parse_args()
    P = load_package()
    for env in a.env:
        run(P, env, a.seeds, {"pendulum": a.pendulum_iters, "mcc": a.mcc_iters, "taxi": a.taxi_iters}[env], a.checkpoints)


if __name__ == "__main__":
    main()
