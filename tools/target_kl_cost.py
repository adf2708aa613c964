"""What a target KL costs when it never stops anything: the headline shape of bench.py (CartPole, 4096 envs x 128 steps, 4 minibatches x 10 epochs,
one GPU) with no target and with a target that is never reached (1e30), alternated in one process -- the difference is the update's E + 1 gate launches
and the wait for the previous update's outcome in front of each update's coefficient table (include/ppo_hip.h: ppo_target_kl_set).

    python tools/target_kl_cost.py [--steps 200] [--warmup 5] [--rounds 3]

Prints one JSON line: env-steps/s of every timed region, off and on in turn, their medians and the relative cost."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--num-steps", type=int, default=128)
    args = ap.parse_args()
    P = load_package()
    N, T = args.envs, args.num_steps
    updates = 2 * args.rounds * args.steps + args.warmup
    ctx = P.Context(P.make_config(num_envs=N, num_steps=T, num_minibatches=4, update_epochs=10, seed=2, total_timesteps=updates * N * T, learning_rate=1e-3,
                                  gamma=0.98, gae_lambda=0.95, anneal_lr=True))
    ctx.init_orthogonal(2)
    ctx.env_reset()
    for _ in range(args.warmup):
        ctx.train_iteration()
    ctx.sync()
    rates = {"off": [], "on": []}
    for _ in range(args.rounds):
        for name, target in (("off", 0.0), ("on", 1e30)):
            ctx.target_kl_set(target)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ctx.train_iteration()
            ctx.sync()
            rates[name].append(args.steps * N * T / (time.perf_counter() - t0))
            es = ctx.early_stop()
            assert es["stopped"] == 0 and es["epochs_run"] == 10, es
    st = ctx.stats()
    off, on = statistics.median(rates["off"]), statistics.median(rates["on"])
    print(json.dumps({"shape": "cartpole %d x %d, 4 x 10" % (N, T), "steps": args.steps, "off_env_steps_per_s": rates["off"], "on_env_steps_per_s": rates["on"],
                      "off_median": off, "on_median": on, "on_cost_percent": 100.0 * (off / on - 1.0),
                      "on_cost_us_per_iteration": 1e6 * N * T * (1.0 / on - 1.0 / off), "optimizer_steps": st["optimizer_steps"]}))
    ctx.close()


if __name__ == "__main__":
    main()
