"""Does bootstrapping at the time limit change what Pendulum and Acrobot learn?  PPO on PPO_ENV_PENDULUM and PPO_ENV_ACROBOT with PPO_KERNEL_ENV_CUT_STATE,
ppo_env_truncation_bootstrap off against on, three seeds each, with the hyper-parameters, sizes and evaluations of tools/pendulum_curve.py and
tools/acrobot_curve.py (imported from there: 1024 envs x 64 steps, max_episode_steps 200; Pendulum 300 iterations, Acrobot 50).

    python tools/cut_state_curve.py [--seeds 1 2 3] [--env pendulum acrobot] [--pendulum-iters 300] [--acrobot-iters 50] [--checkpoints K]

Per checkpoint (iteration 0, the untrained policy, and evenly spaced iterations up to the last: every 50th of Pendulum, every 10th of Acrobot) it evaluates
the mean GREEDY return over the curve tools' 256 fixed start states -- Pendulum stepped through policy_act_f32(greedy) and env_transition_f32, Acrobot by
ppo_evaluate -- which does not depend on the switch: both variants are judged by the same raw, undiscounted return.  Prints one line per (env, seed, switch, checkpoint) and one JSON line
per env with the mean over the seeds per checkpoint for both variants.  Nothing is asserted: the table is written down whatever it shows."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

import acrobot_curve  # noqa: E402
import pendulum_curve  # noqa: E402


def flagged_ctx(P, tool, seed, hyper):
    """the curve tool's context with PPO_KERNEL_ENV_CUT_STATE beside its family flag"""
    make = P.make_config

    def with_flag(**kw):
        kw["kernel_flags"] |= P.KERNEL_ENV_CUT_STATE
        return make(**kw)

    P.make_config = with_flag
    try:
        return tool.make_ctx(P, seed, hyper)
    finally:
        P.make_config = make


def run(P, env, seeds, iters, checkpoints):
    tool = pendulum_curve if env == "pendulum" else acrobot_curve
    hyper = tool.parse([])
    states = pendulum_curve.start_states() if env == "pendulum" else None
    evaluate = (lambda c: pendulum_curve.greedy_return(P, c, states)) if env == "pendulum" else acrobot_curve.greedy_return
    at = sorted({round(iters * k / checkpoints) for k in range(checkpoints + 1)})
    curves = {False: [], True: []}
    events = []
    for seed in seeds:
        for on in (False, True):
            ctx = flagged_ctx(P, tool, seed, hyper)
            ctx.init_orthogonal(seed)
            ctx.env_reset()
            ctx.env_truncation_bootstrap(on)
            curve = []
            for it in range(iters + 1):
                if it:
                    ctx.train_iteration()
                if it in at:
                    curve.append(evaluate(ctx))
                    print("%s seed %d bootstrap %-3s iteration %4d greedy return %9.2f" % (env, seed, "on" if on else "off", it, curve[-1]), flush=True)
            if on:
                events.append(int(ctx.env_truncations()[0].size))
            curves[on].append(curve)
            ctx.close()
    mean = lambda rows: [round(sum(r[k] for r in rows) / len(rows), 2) for k in range(len(at))]   # noqa: E731
    print(json.dumps({"env": env, "seeds": list(seeds), "envs": tool.N, "steps": tool.T, "max_episode_steps": tool.MAXS, "iterations": at,
                      "mean_return_bootstrap_off": mean(curves[False]), "mean_return_bootstrap_on": mean(curves[True]),
                      "per_seed_final_off": [round(c[-1], 2) for c in curves[False]], "per_seed_final_on": [round(c[-1], 2) for c in curves[True]],
                      "events_last_rollout_on": events}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--env", nargs="+", choices=["pendulum", "acrobot"], default=["pendulum", "acrobot"])
    ap.add_argument("--pendulum-iters", type=int, default=300)
    ap.add_argument("--acrobot-iters", type=int, default=50)
    ap.add_argument("--checkpoints", type=int, default=0, help="0: every 50 iterations of Pendulum, every 10 of Acrobot")
    a = ap.parse_args()
    P = load_package()
    for env in a.env:
        iters = a.pendulum_iters if env == "pendulum" else a.acrobot_iters
        run(P, env, a.seeds, iters, a.checkpoints or max(1, iters // (50 if env == "pendulum" else 10)))


if __name__ == "__main__":
    main()
