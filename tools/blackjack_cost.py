"""What the fused rollout of Blackjack (PPO_ENV_BLACKJACK: cat_rollout_kernel, one launch for all T steps, the env's cards drawn on the chip from a key the state
carries -- a hit one card, a stick the dealer's play-out, a reset the deal) buys over stepping the same env on the same context through the stand-alone
calls, in one process on one GPU, at 4096 envs x 128 steps (4 minibatches x 4 epochs; max_episode_steps 100).

    python tools/blackjack_cost.py [--repeats 7] [--warmup 2] [--envs 4096] [--steps 128]

rollout    ppo_rollout alone: cat_rollout_kernel and the two critic launches
iteration  ppo_train_iteration: the rollout, the scan, the update
stepwise   the same T steps as a loop of ppo_policy_act(step_index = rollout_steps + t) and ppo_env_step on device arrays of the same context: 2 T launches,
           nothing copied to the host, no host wait inside the loop.  The loop does less: the rollout's stores and its critic are not in it
and, in the same run,
lake4      ppo_rollout of a PPO_ENV_FROZENLAKE context of the same size (the same kernel on gf_carve(16, 4)): one Philox call per step and lane, the same for
           every lane, against Blackjack's work that differs between the lanes of wave 0 (about three steps in four under a near-uniform policy end an
           episode: the hidden card's call, the dealer's, and the two of the reset)
lake8      ppo_rollout of a PPO_ENV_FROZENLAKE8X8 context (obs 64): with lake4 it gives the kernel's cost per observation column at one Philox call per step,
           so what Blackjack's obs 45 would cost without its variable work is an interpolation inside one run (obs45_interpolated_ms)
Every timing is a host clock around work that ends in a synchronisation; median and range over the repeats after the warm-up.  No bar is set.  Also reports
the share of the rollout's steps that ended an episode.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

NMB, EPOCHS = 4, 4


def timed(fn, *ctxs):
    for c in ctxs:
        c.sync()
    t0 = time.perf_counter()
    fn()
    for c in ctxs:
        c.sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    args = ap.parse_args()
    P = load_package()
    L = P.binding.lib()
    N, T = args.envs, args.steps
    common = dict(num_envs=N, num_steps=T, num_minibatches=NMB, update_epochs=EPOCHS, seed=3, total_timesteps=1 << 40, learning_rate=1e-4, anneal_lr=False,
                  kernel_flags=P.KERNEL_CAT_FUSED, dist_kind=P.DIST_CATEGORICAL, max_episode_steps=100)
    jack = P.Context(P.make_config(env_kind=P.ENV_BLACKJACK, obs_size=45, head_dims=(2,), **common))
    lake = P.Context(P.make_config(env_kind=P.ENV_FROZENLAKE, obs_size=16, head_dims=(4,), **common))
    lake8 = P.Context(P.make_config(env_kind=P.ENV_FROZENLAKE8X8, obs_size=64, head_dims=(4,), **common))
    for c in (jack, lake, lake8):
        c.init_orthogonal(3)
        c.env_reset()
    chk = P.binding._check
    d_obs, d_act = jack.empty((N, jack.O), np.float32), jack.empty((N, 1), np.int64)
    d_lp, d_rew, d_done = jack.empty(N, np.float32), jack.empty(N, np.float32), jack.empty(N, np.int32)
    next_obs = jack.buffer_ptr("NEXT_OBS")[0]

    def stepwise():
        obs = next_obs
        for t in range(T):
            chk(L.ppo_policy_act(jack.h, obs, None, None, C.c_int64(N), C.c_int64(t), d_act.ptr, d_lp.ptr, None, None), jack.h)
            chk(L.ppo_env_step(jack.h, d_act.ptr, d_obs.ptr, d_rew.ptr, d_done.ptr), jack.h)
            obs = d_obs.ptr

    runs = {"blackjack_rollout": (jack.rollout, jack), "blackjack_iteration": (jack.train_iteration, jack), "blackjack_stepwise": (stepwise, jack),
            "lake4_rollout": (lake.rollout, lake), "lake8_rollout": (lake8.rollout, lake8)}
    times = {k: [] for k in runs}
    for r in range(args.warmup + args.repeats):
        for k, (fn, c) in runs.items():
            t = timed(fn, c)
            if r >= args.warmup:
                times[k].append(t)
    jack.rollout()
    jack.sync()
    ending = float((jack.read("FIN_LEN") > 0).mean())
    out = {"shape": "Blackjack-v1 (obs 45, 2 actions) and FrozenLake-v1 (obs 16, 4 actions), 2 x 64, %d minibatches x %d epochs" % (NMB, EPOCHS), "envs": N,
           "steps": T, "repeats": args.repeats, "rollout_workgroups": (N + 63) // 64, "blackjack_steps_ending_an_episode": round(ending, 4)}
    for k, ts in times.items():
        rate = sorted(N * T / t for t in ts)
        ms = sorted(1e3 * t for t in ts)
        out["%s_ms" % k] = {"median": round(statistics.median(ms), 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}
        out["%s_Msteps_per_s" % k] = {"median": round(statistics.median(rate) / 1e6, 2), "min": round(rate[0] / 1e6, 2), "max": round(rate[-1] / 1e6, 2)}
    out["one_launch_beats_2T_launches"] = out["blackjack_rollout_ms"]["median"] < out["blackjack_stepwise_ms"]["median"]
    out["blackjack_rollout_over_lake4"] = round(out["blackjack_rollout_ms"]["median"] / out["lake4_rollout_ms"]["median"], 3)
    l4, l8 = out["lake4_rollout_ms"]["median"], out["lake8_rollout_ms"]["median"]
    out["obs45_interpolated_ms"] = round(l4 + (l8 - l4) * (45 - 16) / (64 - 16), 4)
    print(json.dumps(out))
    for c in (jack, lake, lake8):
        c.close()


if __name__ == "__main__":
    main()
