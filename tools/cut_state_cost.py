"""What PPO_KERNEL_ENV_CUT_STATE costs: per fused device env one unflagged and one flagged context at 4096 envs x 128 steps, alternating in one process on
one GPU, 2 warm-up + 7 timed windows of 20 ppo_rollout calls each (a single rollout is about a millisecond: a window of one would time the host).

    python tools/cut_state_cost.py [--repeats 7] [--warmup 2] [--envs 4096] [--steps 128] [--limit 7] [--only pendulum acrobot ...]

rollout   ppo_rollout alone (the rollout kernel and the two critic launches), switch off: the unflagged context (KEEP = false) against the flagged one
          (KEEP = true: STATE + 1 scattered stores where an episode reaches the limit).  max_episode_steps = --limit, so about 1 / limit of the samples are
          cut-offs -- far more than a trained run sees; the flag's cost at gym's limits is below this one.
fold      the flagged context with ppo_env_truncation_bootstrap on minus the same context with it off: the fold launch (cut_state_fold_kernel) with the
          event counter's clear and copy; and the number of events of the last rollout.
old fold  PPO_ENV_MOUNTAINCAR_CONTINUOUS and PPO_ENV_TAXI only: the same difference on the unflagged context (gauss_trunc_fold_kernel / cat_trunc_fold_kernel,
          which rebuild the state from PPO_BUF_OBS and step it again).
Every timing is a host clock around work that ends in a synchronisation; per window the mean over its 20 rollouts, then median with min .. max over the
windows, in milliseconds.  Nothing is asserted and no bar is set.  Prints one JSON line per env."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

WINDOW = 20
ENVS = {   # name -> (env_kind, dist_kind, obs_size, actions, family flag, the unflagged context folds)
    "pendulum": ("ENV_PENDULUM", "DIST_GAUSSIAN", 3, 1, "KERNEL_GAUSS_FUSED", False),
    "mountaincar_continuous": ("ENV_MOUNTAINCAR_CONTINUOUS", "DIST_GAUSSIAN", 2, 1, "KERNEL_GAUSS_FUSED", True),
    "acrobot": ("ENV_ACROBOT", "DIST_CATEGORICAL", 6, 3, "KERNEL_CAT_FUSED", False),
    "taxi": ("ENV_TAXI", "DIST_MASKED", 19, 6, "KERNEL_CAT_FUSED", True),
    "frozenlake": ("ENV_FROZENLAKE", "DIST_CATEGORICAL", 16, 4, "KERNEL_CAT_FUSED", False),
    "frozenlake8x8": ("ENV_FROZENLAKE8X8", "DIST_CATEGORICAL", 64, 4, "KERNEL_CAT_FUSED", False),
    "blackjack": ("ENV_BLACKJACK", "DIST_CATEGORICAL", 45, 2, "KERNEL_CAT_FUSED", False),
}


def timed_window(ctx):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(WINDOW):
        ctx.rollout()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0) / WINDOW


def summary(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def measure(P, name, args):
    kind, dist, obs, actions, family, old_fold = ENVS[name]

    def ctx(flagged):
        c = P.Context(P.make_config(env_kind=getattr(P, kind), dist_kind=getattr(P, dist), obs_size=obs, head_dims=(actions,), num_envs=args.envs,
                                    num_steps=args.steps, num_minibatches=4, update_epochs=4, max_episode_steps=args.limit, seed=3, total_timesteps=1 << 40,
                                    learning_rate=1e-4, anneal_lr=False, kernel_flags=getattr(P, family) | (P.KERNEL_ENV_CUT_STATE if flagged else 0)))
        c.init_orthogonal(3)
        c.env_reset()
        return c

    plain, keep = ctx(False), ctx(True)
    # the variants of one pass, in this order, every pass: (context, switch)
    variants = [("rollout_unflagged", plain, False), ("rollout_flagged", keep, False), ("flagged_switch_on", keep, True)]
    if old_fold:
        variants.append(("unflagged_switch_on", plain, True))
    times = {v[0]: [] for v in variants}
    for k in range(args.warmup + args.repeats):
        for label, c, on in variants:
            if on or old_fold or c is keep:
                c.env_truncation_bootstrap(on)
            t = timed_window(c)
            if k >= args.warmup:
                times[label].append(t)
    keep.env_truncation_bootstrap(True)
    keep.rollout()
    events = int(keep.env_truncations()[0].size)
    out = {"env": name, "envs": args.envs, "steps": args.steps, "max_episode_steps": args.limit, "rows": args.envs * args.steps, "events_last_rollout": events,
           "windows": args.repeats, "rollouts_per_window": WINDOW}
    for label in times:
        out[label + "_ms"] = summary(times[label])
    out["flag_cost_ms"] = round(out["rollout_flagged_ms"]["median"] - out["rollout_unflagged_ms"]["median"], 4)
    out["fold_ms"] = round(out["flagged_switch_on_ms"]["median"] - out["rollout_flagged_ms"]["median"], 4)
    if old_fold:
        out["old_fold_ms"] = round(out["unflagged_switch_on_ms"]["median"] - out["rollout_unflagged_ms"]["median"], 4)
    for c in (plain, keep):
        c.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--limit", type=int, default=7)
    ap.add_argument("--only", nargs="+", choices=sorted(ENVS), default=list(ENVS))
    args = ap.parse_args()
    P = load_package()
    for name in args.only:
        measure(P, name, args)


if __name__ == "__main__":
    main()
