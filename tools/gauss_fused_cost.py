"""What PPO_KERNEL_GAUSS_FUSED buys: a Gaussian policy (obs 17, D 6: Walker / HalfCheetah) on the 2 x 64 network, with the flag off (the generic engine)
and on (kernels_gauss_fused.hip), alternated in one process on one GPU, at 64 envs x 128 steps and at 4096 envs x 32 steps (4 minibatches x 4 epochs).

    python tools/gauss_fused_cost.py [--repeats 7] [--warmup 2]

Per size and path, over the timed repeats (one device-fed rollout and its end each), median and range of
  act_ms      one ppo_dev_act_f32 step: enqueue to completion (a synchronisation in front and behind), mean over the rollout's steps
  step_ms     one minibatch step: a whole ppo_update on the rollout's buffers / (epochs x minibatches)
  end_ms      one whole ppo_host_rollout_end (critic batch, advantages, update): call to completion
and whether the fused path's median is below the MINIMUM of the generic path's repeats (the flag's acceptance condition).
Prints one JSON line.

    python tools/gauss_fused_cost.py --truncated [--repeats 25] [--warmup 3]

measures instead what truncation flags in ppo_dev_observe cost a device-fed step of the fused context (truncated_cost below; DESIGN.md, "Envs on the device")."""
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

OBS, D, NMB, EPOCHS = 17, 6, 4, 4


def one_repeat(ctx, dev):
    """a device-fed rollout on fixed arrays, its end, and one more update on the same buffers; returns (act_ms, step_ms, end_ms)"""
    T = ctx.T
    ctx.host_rollout_begin()
    act = 0.0
    for t in range(T):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.dev_act_f32(dev["act"])
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


class HipEvents:
    """Two timing events of the HIP runtime the library is linked against (by its soname: it is already in the process)"""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so.7")
        self.lib.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.hipEventSynchronize.argtypes = [C.c_void_p]
        self.lib.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.lib.hipEventCreate(C.byref(e)) == 0

    def record(self, which, stream):
        assert self.lib.hipEventRecord(self.ev[which], stream) == 0

    def elapsed_ms(self):
        ms = C.c_float()
        assert self.lib.hipEventSynchronize(self.ev[1]) == 0
        assert self.lib.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) == 0
        return ms.value


TRUNC_N, TRUNC_T = 4096, 16


def truncated_cost(P, args):
    """--truncated: what a time-limit bootstrap costs a device-fed step of a PPO_KERNEL_GAUSS_FUSED context (N = 4096, obs 17, D 6).  One step =
    ppo_dev_act_f32 + ppo_dev_observe on the context's own stream; HIP events around the T = 16 steps of a rollout; median over the timed rollouts, us per step:
      no_flags        ppo_dev_observe without `truncated`
      flags_none_set  `truncated` passed, no row flagged: the common step (act + commit + a fold launch whose every workgroup leaves after its flags)
      flags_one_in_7  about 1 / 7 of the rows flagged (and done) on one step in seven
      host_read       the route without the fold: observe without flags, then a blocking read of the step's flags to learn K and, where K > 0,
                      ppo_bootstrap_rewards on the K rows.  The K final observations and indices wait in device arrays made beforehand: the gather a real
                      caller also pays is NOT in this number."""
    N, T = TRUNC_N, TRUNC_T
    rng = np.random.default_rng(5)
    ctx = P.Context(P.make_config(env_kind=P.ENV_HOST, dist_kind=P.DIST_GAUSSIAN, obs_size=OBS, head_dims=(D,), hidden=64, n_hidden=2, num_envs=N, num_steps=T,
                                  num_minibatches=1, update_epochs=1, seed=3, total_timesteps=1 << 40, learning_rate=1e-4, anneal_lr=False,
                                  max_episode_steps=1000, kernel_flags=P.KERNEL_GAUSS_FUSED))
    ctx.init_orthogonal(3)
    lib, stream = P.binding.lib(), C.c_void_p(ctx.stream())
    hit = (rng.uniform(0, 1, N) < 1.0 / 7.0).astype(np.int32)
    rows = np.flatnonzero(hit)
    final_h = rng.uniform(-1, 1, (N, OBS)).astype(np.float32)
    act = ctx.empty((N, D), np.float32)
    obs = [ctx.dev(rng.uniform(-1, 1, (N, OBS)).astype(np.float32)) for _ in range(2)]
    rew, final = ctx.dev(rng.normal(0, 1, N).astype(np.float32)), ctx.dev(final_h)
    zeros, ones = ctx.dev(np.zeros(N, np.int32)), ctx.dev(hit)
    final_rows = ctx.dev(final_h[rows])
    index = [ctx.dev((t * N + rows).astype(np.int32)) for t in range(T)]
    rewards_buf = ctx.buffer_ptr("REWARDS")[0]
    ctx.dev_env_reset(obs[0])
    ev = HipEvents()

    def flagged(t, variant):
        return variant in ("flags_one_in_7", "host_read") and t % 7 == 6

    def rollout(variant):
        ctx.host_rollout_begin()
        ctx.sync()
        ev.record(0, stream)
        for t in range(T):
            ctx.dev_act_f32(act)
            flags = ones if flagged(t, variant) else zeros   # the step's `done` is the same array: a flagged row is done
            if variant == "no_flags":
                ctx.dev_observe(obs[t & 1], rew, flags)
            elif variant == "host_read":
                ctx.dev_observe(obs[t & 1], rew, flags)
                k = int(np.count_nonzero(flags.download()))   # the host wait
                if k:
                    P.binding._check(lib.ppo_bootstrap_rewards(ctx.h, final_rows.ptr, index[t].ptr, C.c_int64(k), C.c_float(ctx.cfg.gamma), rewards_buf, None), ctx.h)
            else:
                ctx.dev_observe(obs[t & 1], rew, flags, truncated=flags, final_obs=final)
        ev.record(1, stream)
        us = 1e3 * ev.elapsed_ms() / T
        ctx.host_rollout_end()
        return us

    variants = ("no_flags", "flags_none_set", "flags_one_in_7", "host_read")
    for _ in range(args.warmup):
        for v in variants:
            rollout(v)
    times = {v: [] for v in variants}
    for _ in range(args.repeats):
        for v in variants:
            times[v].append(rollout(v))
    out = {"shape": "N %d, obs %d, D %d, 2 x 64, T %d, PPO_KERNEL_GAUSS_FUSED" % (N, OBS, D, T), "repeats": args.repeats, "rows_flagged": int(rows.size),
           "us_per_step": {v: {"median": statistics.median(times[v]), "min": min(times[v]), "max": max(times[v])} for v in variants}}
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--truncated", action="store_true", help="the cost of truncation flags in ppo_dev_observe instead (four variants of a device-fed step)")
    args = ap.parse_args()
    P = load_package()
    if args.truncated:
        args.repeats, args.warmup = args.repeats or 25, 3 if args.warmup is None else args.warmup
        return truncated_cost(P, args)
    args.repeats, args.warmup = args.repeats or 7, 2 if args.warmup is None else args.warmup
    out = {"shape": "obs %d, D %d, 2 x 64, %d minibatches x %d epochs" % (OBS, D, NMB, EPOCHS), "repeats": args.repeats, "sizes": []}
    for N, T in ((64, 128), (4096, 32)):
        rng = np.random.default_rng(N)
        ctxs = {}
        for name, flags in (("generic", 0), ("fused", P.KERNEL_GAUSS_FUSED)):
            ctx = P.Context(P.make_config(env_kind=P.ENV_HOST, dist_kind=P.DIST_GAUSSIAN, obs_size=OBS, head_dims=(D,), hidden=64, n_hidden=2, num_envs=N, num_steps=T,
                                          num_minibatches=NMB, update_epochs=EPOCHS, seed=3, total_timesteps=1 << 40, learning_rate=1e-4, anneal_lr=False,
                                          max_episode_steps=1000, kernel_flags=flags))
            ctx.init_orthogonal(3)
            dev = dict(act=ctx.empty((N, D), np.float32), obs=[ctx.dev(rng.uniform(-1, 1, (N, OBS)).astype(np.float32)) for _ in range(2)],
                       rew=ctx.dev(rng.normal(0, 1, N).astype(np.float32)), done=ctx.dev((rng.uniform(0, 1, N) < 0.01).astype(np.int32), np.int32))
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
        a, v, u = ctxs["fused"][0].gauss_fused_launches()
        runs = args.warmup + args.repeats
        assert (a, v, u) == (runs * T, runs * 2, runs * 2 * EPOCHS * NMB), (a, v, u)
        assert ctxs["generic"][0].gauss_fused_launches() == (0, 0, 0)
        size["fused_launches"] = [a, v, u]
        out["sizes"].append(size)
        for name in ctxs:
            ctxs[name][0].close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
