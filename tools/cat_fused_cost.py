"""What PPO_KERNEL_CAT_FUSED buys: a masked multi-head policy (obs 17, heads (5, 3, 4)) on the 2 x 64 network, with the flag off (the generic engine: the
flag-off path is the code as it was before the flag existed) and on (kernels_gauss_fused.hip: cat_act_kernel, gauss_values_kernel, cat_fwd_bwd_kernel),
alternated in one process on one GPU, at 64 envs x 128 steps and at 4096 envs x 32 steps (4 minibatches x 4 epochs).

    python tools/cat_fused_cost.py [--repeats 7] [--warmup 2]

Per size and path, over the timed repeats (one device-fed rollout and its end each), median and range of
  act_ms      one ppo_dev_act step: enqueue to completion (a synchronisation in front and behind), mean over the rollout's steps
  step_ms     one minibatch step: a whole ppo_update on the rollout's buffers / (epochs x minibatches)
  end_ms      one whole ppo_host_rollout_end (critic batch, advantages, update): call to completion
and whether the fused path's median is below the MINIMUM of the generic path's repeats.  There is no threshold: the flag is opt-in either way.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

OBS, HEADS, NMB, EPOCHS = 17, (5, 3, 4), 4, 4


def one_repeat(ctx, dev):
    """a device-fed rollout on fixed arrays, its end, and one more update on the same buffers; returns (act_ms, step_ms, end_ms)"""
    T = ctx.T
    ctx.host_rollout_begin()
    act = 0.0
    for t in range(T):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.dev_act(dev["act"], mask=dev["mask"][t & 1])
        ctx.sync()
        act += time.perf_counter() - t0
        ctx.dev_observe(dev["obs"][t & 1], dev["rew"], dev["done"])
    ctx.sync()
    t0 = time.perf_counter()
    ctx.host_rollout_end()
    ctx.sync()
    end = time.perf_counter() - t0
    t0 = time.perf_counter()
    ctx.update()
    ctx.sync()
    upd = time.perf_counter() - t0
    steps = EPOCHS * -(-ctx.B // (ctx.B // NMB))
    return 1e3 * act / T, 1e3 * upd / steps, 1e3 * end


def random_masks(rng, N):
    """every logit allowed with probability 0.6, and one allowed action per head for certain"""
    m = (rng.uniform(0, 1, (N, sum(HEADS))) < 0.6).astype(np.uint8)
    off = 0
    for w in HEADS:
        m[np.arange(N), off + rng.integers(0, w, N)] = 1
        off += w
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    P = load_package()
    out = {"shape": "obs %d, heads %s masked, 2 x 64, %d minibatches x %d epochs" % (OBS, list(HEADS), NMB, EPOCHS), "repeats": args.repeats, "sizes": []}
    for N, T in ((64, 128), (4096, 32)):
        rng = np.random.default_rng(N)
        ctxs = {}
        for name, flags in (("generic", 0), ("fused", P.KERNEL_CAT_FUSED)):
            ctx = P.Context(P.make_config(env_kind=P.ENV_HOST, dist_kind=P.DIST_MASKED, obs_size=OBS, head_dims=HEADS, hidden=64, n_hidden=2, num_envs=N, num_steps=T,
                                          num_minibatches=NMB, update_epochs=EPOCHS, seed=3, total_timesteps=1 << 40, learning_rate=1e-4, anneal_lr=False,
                                          max_episode_steps=1000, kernel_flags=flags))
            ctx.init_orthogonal(3)
            dev = dict(act=ctx.empty((N, len(HEADS)), np.int64), obs=[ctx.dev(rng.uniform(-1, 1, (N, OBS)).astype(np.float32)) for _ in range(2)],
                       mask=[ctx.dev(random_masks(rng, N), np.uint8) for _ in range(2)], rew=ctx.dev(rng.normal(0, 1, N).astype(np.float32)),
                       done=ctx.dev((rng.uniform(0, 1, N) < 0.01).astype(np.int32), np.int32))
            ctx.dev_env_reset(dev["obs"][0])
            ctxs[name] = (ctx, dev)
        for _ in range(args.warmup):
            for name in ("generic", "fused"):
                one_repeat(*ctxs[name])
        times = {"generic": [], "fused": []}
        for _ in range(args.repeats):
            for name in ("generic", "fused"):
                times[name].append(one_repeat(*ctxs[name]))
        size = {"envs": N, "steps": T, "minibatch_rows": N * T // NMB}
        for k, key in enumerate(("act_ms", "step_ms", "end_ms")):
            g, f = [t[k] for t in times["generic"]], [t[k] for t in times["fused"]]
            size[key] = {"generic_median": statistics.median(g), "generic_min": min(g), "generic_max": max(g), "fused_median": statistics.median(f), "fused_min": min(f),
                         "fused_max": max(f), "fused_median_below_generic_min": statistics.median(f) < min(g)}
        a, v, u = ctxs["fused"][0].cat_fused_launches()
        runs = args.warmup + args.repeats
        assert (a, v, u) == (runs * T, runs * 2, runs * 2 * EPOCHS * NMB), (a, v, u)
        assert ctxs["generic"][0].cat_fused_launches() == (0, 0, 0)
        size["fused_launches"] = [a, v, u]
        out["sizes"].append(size)
        for name in ctxs:
            ctxs[name][0].close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
