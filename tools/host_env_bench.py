"""Where the time of a host-stepped env step goes (PPO_ENV_HOST, include/ppo_hip.h ppo_host_*).  Prints one JSON line:

  (a) launch_wait_us      round trip of a trivial launch (a one-env ppo_env_transition) plus the wait for it
  (b) act_us[N]           ppo_host_act + ppo_host_observe per step with a zero-cost env (fixed arrays), N in {256, 4096, 16384}
  (c) end_ms              ppo_host_rollout_end (commit, values, scan, update) until the stream is idle, 4096 x 128
  (d) host_sps            env-steps/s of full host-stepped iterations at 4096 x 128 (zero-cost env), next to device_sps: ppo_train_iteration's

  --one-rollout           only one host-stepped rollout at 4096 x 128 (for a rocprofv3 --kernel-trace --memory-copy-trace --stats run around it)

  --groups G [G ...] --env-cost-us X   env groups (ppo_host_group_*) against the ungrouped calls in ONE process: a worker thread stands for the caller's
                          envs -- stepping n of the N envs takes X n / N us there (a sleep that releases the interpreter; its real cost is measured and
                          printed as env_us) -- while the main thread makes the policy call of the next group.  Prints, for --envs N and num_steps 128, the
                          ungrouped round trip R (X = 0), and the time of one iteration (rollout + update, stream idle) ungrouped and with each G,
                          at X = 0 and at X = --env-cost-us (default: R), next to the ideal gain (E + R) / max(E, R) with E the measured env_us.

  --dist gaussian         a diagonal-Gaussian context (PPO_DIST_GAUSSIAN, D = 6) beside the categorical context of the same shape on the same generic
                          engine (obs 11, 2 x 64, one head of 6; --envs N, 64 steps, 4 epochs x 4 minibatches) in ONE process: per-step act + observe
                          time and the ppo_host_rollout_end time of each (zero-cost env).
"""
import argparse
import concurrent.futures
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

P = load_package()


def host_ctx(N, T, flags=0, iters=4):
    c = P.Context(P.make_config(env_kind=P.ENV_HOST, num_envs=N, num_steps=T, num_minibatches=4, update_epochs=4, seed=1,
                                total_timesteps=N * T * iters, kernel_flags=flags))
    c.init_orthogonal(1)
    return c


class ZeroEnv:
    """Fixed arrays: the cost of the env is nil, what is left is the library's."""

    def __init__(self, N):
        rng = np.random.default_rng(0)
        self.obs = rng.uniform(-0.05, 0.05, (N, 4)).astype(np.float32)
        self.rew = np.ones(N, np.float32)
        self.done = (rng.random(N) < 0.02).astype(np.int32)
        self.args = [np.ascontiguousarray(x).ctypes.data_as(C.c_void_p) for x in (self.obs, self.rew, self.done)]
        self.act = np.empty((N, 1), np.int64)
        self.act_p = self.act.ctypes.data_as(C.c_void_p)


def rollout_steps(c, env, T):
    L = P.binding.lib()
    for _ in range(T):
        P.binding._check(L.ppo_host_act(c.h, None, env.act_p), c.h)
        P.binding._check(L.ppo_host_observe(c.h, env.args[0], env.args[1], env.args[2], None, None), c.h)


def launch_wait_us(reps=2000):
    c = P.Context(P.make_config(num_envs=8, num_steps=4, num_minibatches=1, update_epochs=1))
    L = P.binding.lib()
    st, a = c.dev(np.zeros((1, 4), np.float32)), c.dev(np.zeros(1, np.int64))
    ns, r, d = c.empty((1, 4), np.float32), c.empty(1, np.float32), c.empty(1, np.int32)
    stream = C.c_void_p(c.stream())

    def once():
        P.binding._check(L.ppo_env_transition(0, st.ptr, a.ptr, C.c_int64(1), ns.ptr, r.ptr, d.ptr, stream))
        P.binding._check(L.ppo_sync(c.h), c.h)
    for _ in range(200):
        once()
    t0 = time.perf_counter()
    for _ in range(reps):
        once()
    us = (time.perf_counter() - t0) / reps * 1e6
    c.close()
    return us


def act_us(N, flags=0, T=64, rounds=3):
    c = host_ctx(N, T, flags)
    env = ZeroEnv(N)
    c.host_env_reset(env.obs)
    best = None
    for r in range(rounds + 1):
        c.host_rollout_begin()
        t0 = time.perf_counter()
        rollout_steps(c, env, T)
        dt = (time.perf_counter() - t0) / T * 1e6
        c.host_rollout_end()
        c.sync()
        if r > 0:
            best = dt if best is None else min(best, dt)
    c.close()
    return best


def iteration_times(flags=0, N=4096, T=128, iters=4):
    c = host_ctx(N, T, flags, iters + 1)
    env = ZeroEnv(N)
    c.host_env_reset(env.obs)
    ends, its = [], []
    for i in range(iters + 1):
        t0 = time.perf_counter()
        c.host_rollout_begin()
        rollout_steps(c, env, T)
        t1 = time.perf_counter()
        c.host_rollout_end()
        c.sync()
        t2 = time.perf_counter()
        if i > 0:
            ends.append((t2 - t1) * 1e3)
            its.append(t2 - t0)
    c.close()
    return min(ends), N * T / min(its)


def device_sps(N=4096, T=128, iters=5):
    c = P.Context(P.make_config(num_envs=N, num_steps=T, num_minibatches=4, update_epochs=4, seed=1, total_timesteps=N * T * (iters + 1)))
    c.init_orthogonal(1)
    c.env_reset()
    c.train_iteration()
    c.sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        c.train_iteration()
    c.sync()
    sps = N * T * iters / (time.perf_counter() - t0)
    c.close()
    return sps


def dist_bench(N, T=64, rounds=3, obs=11, width=6):
    """(act + observe us per step, rollout_end ms) of a Gaussian and of a categorical generic context of the same shape, interleaved round by round"""
    L = P.binding.lib()
    rng = np.random.default_rng(0)
    o = np.ascontiguousarray(rng.uniform(-1, 1, (N, obs)).astype(np.float32))
    rew, done = np.ones(N, np.float32), (rng.random(N) < 0.02).astype(np.int32)
    args = [x.ctypes.data_as(C.c_void_p) for x in (o, rew, done)]
    ctxs, acts = {}, {}
    for name, dist in (("categorical", P.DIST_CATEGORICAL), ("gaussian", P.DIST_GAUSSIAN)):
        c = P.Context(P.make_config(env_kind=P.ENV_HOST, dist_kind=dist, obs_size=obs, head_dims=(width,), num_envs=N, num_steps=T, num_minibatches=4,
                                    update_epochs=4, seed=1, total_timesteps=N * T * (rounds + 2)))
        c.init_orthogonal(1)
        c.host_env_reset(o)
        ctxs[name] = c
        acts[name] = np.empty((N, width), np.float32) if dist == P.DIST_GAUSSIAN else np.empty((N, 1), np.int64)
    out = {name: {"act_us": None, "end_ms": None} for name in ctxs}
    for r in range(rounds + 1):
        for name, c in ctxs.items():
            a = acts[name].ctypes.data_as(C.c_void_p)
            c.host_rollout_begin()
            t0 = time.perf_counter()
            for _ in range(T):
                P.binding._check(L.ppo_host_act_f32(c.h, a) if name == "gaussian" else L.ppo_host_act(c.h, None, a), c.h)
                P.binding._check(L.ppo_host_observe(c.h, args[0], args[1], args[2], None, None), c.h)
            t1 = time.perf_counter()
            c.host_rollout_end()
            c.sync()
            t2 = time.perf_counter()
            if r > 0:
                us, ms = (t1 - t0) / T * 1e6, (t2 - t1) * 1e3
                out[name]["act_us"] = us if out[name]["act_us"] is None else min(out[name]["act_us"], us)
                out[name]["end_ms"] = ms if out[name]["end_ms"] is None else min(out[name]["end_ms"], ms)
    for c in ctxs.values():
        c.close()
    return {"N": N, "T": T, "obs": obs, "width": width, **out}


class WorkerEnv:
    """The caller's envs on a thread of their own: step(n) occupies that thread for cost_us * n / N and returns a future."""

    def __init__(self, N, cost_us):
        self.N, self.cost_us = N, cost_us
        self.libc = C.CDLL(None)
        self.pool = concurrent.futures.ThreadPoolExecutor(1, initializer=self._init)

    def _init(self):
        self.libc.prctl(29, C.c_ulong(1), C.c_ulong(0), C.c_ulong(0), C.c_ulong(0))   # PR_SET_TIMERSLACK of THIS thread: 1 ns instead of 50 us

    def _busy(self, us):
        if us > 0:
            self.libc.usleep(C.c_uint(int(round(us))))   # (ctypes releases the interpreter lock for the call: the main thread runs)

    def step(self, n):
        return self.pool.submit(self._busy, self.cost_us * n / self.N)

    def measured_us(self, reps=200):
        t0 = time.perf_counter()
        for _ in range(reps):
            self.step(self.N).result()
        return (time.perf_counter() - t0) / reps * 1e6

    def close(self):
        self.pool.shutdown()


def grouped_iteration_ms(c, env, work, T, G, iters=3):
    """min over iters of one full iteration; G = 0: the ungrouped calls (ppo_host_act waits, the worker steps all envs, ppo_host_observe)"""
    L, chk, N = P.binding.lib(), P.binding._check, c.N
    bounds = [g * (N // G) for g in range(G)] + [N] if G else None
    ptr = lambda a, off: C.c_void_p(a.ctypes.data + off * a.strides[0])
    best = None
    for it in range(iters + 1):
        t0 = time.perf_counter()
        if not G:
            c.host_rollout_begin()
            for _ in range(T):
                chk(L.ppo_host_act(c.h, None, env.act_p), c.h)
                work.step(N).result()
                chk(L.ppo_host_observe(c.h, env.args[0], env.args[1], env.args[2], None, None), c.h)
        else:
            c.host_rollout_begin(bounds)
            for g in range(G):
                chk(L.ppo_host_group_act(c.h, g, None), c.h)
            t_of, stepping, fut = [0] * G, -1, [None] * G

            def finish(g):
                fut[g].result()
                b0 = bounds[g]
                chk(L.ppo_host_group_observe(c.h, g, ptr(env.obs, b0), ptr(env.rew, b0), ptr(env.done, b0), None, None), c.h)
                t_of[g] += 1
                if t_of[g] < T:
                    chk(L.ppo_host_group_act(c.h, g, None), c.h)
            for k in range(T * G):
                g = k % G
                chk(L.ppo_host_group_actions(c.h, g, ptr(env.act, bounds[g])), c.h)
                fut[g] = work.step(bounds[g + 1] - bounds[g])
                if stepping >= 0:
                    finish(stepping)
                stepping = g
            finish(stepping)
        c.host_rollout_end()
        c.sync()
        dt = (time.perf_counter() - t0) * 1e3
        if it > 0:
            best = dt if best is None else min(best, dt)
    return best


def groups_bench(N, groups, env_cost_us, T=128):
    c = host_ctx(N, T, iters=64)
    env = ZeroEnv(N)
    c.host_env_reset(env.obs)
    R = None   # the ungrouped round trip per step with a zero-cost env, as act_us measures it
    for r in range(3):
        c.host_rollout_begin()
        t0 = time.perf_counter()
        rollout_steps(c, env, T)
        dt = (time.perf_counter() - t0) / T * 1e6
        c.host_rollout_end()
        c.sync()
        if r > 0:
            R = dt if R is None else min(R, dt)
    out = {"N": N, "T": T, "round_trip_us": R, "runs": []}
    for X in (0.0, R if env_cost_us is None else env_cost_us):
        work = WorkerEnv(N, X)
        E = work.measured_us()   # what one env batch step really costs the caller, hand-over to the worker thread included
        run = {"env_cost_us": X, "env_us": E, "iteration_ms": {"ungrouped": grouped_iteration_ms(c, env, work, T, 0)},
               "ideal_gain": (E + R) / max(E, R)}
        for G in groups:
            run["iteration_ms"]["G%d" % G] = grouped_iteration_ms(c, env, work, T, G)
        run["gain"] = {k: run["iteration_ms"]["ungrouped"] / v for k, v in run["iteration_ms"].items() if k != "ungrouped"}
        out["runs"].append(run)
        work.close()
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one-rollout", action="store_true")
    ap.add_argument("--groups", type=int, nargs="+", default=None, help="env groups to compare with the ungrouped calls, e.g. --groups 2 4")
    ap.add_argument("--env-cost-us", type=float, default=None, help="cost of one step of all N envs on the worker thread (default: the measured round trip)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--dist", choices=["gaussian"], default=None, help="a Gaussian context beside the categorical generic context of the same shape")
    args = ap.parse_args()
    if args.dist:
        print(json.dumps({"dist_bench": dist_bench(args.envs)}))
        return
    if args.groups:
        print(json.dumps({"groups_bench": groups_bench(args.envs, args.groups, args.env_cost_us)}))
        return
    if args.one_rollout:
        N, T = 4096, 128
        c = host_ctx(N, T)
        env = ZeroEnv(N)
        c.host_env_reset(env.obs)
        c.host_rollout_begin()
        rollout_steps(c, env, T)
        c.host_rollout_end()
        c.sync()
        c.close()
        print(json.dumps({"one_rollout": True, "N": N, "T": T}))
        return
    out = {"launch_wait_us": launch_wait_us(), "act_us": {N: act_us(N) for N in (256, 4096, 16384)}}
    out["end_ms"], out["host_sps"] = iteration_times()
    out["device_sps"] = device_sps()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
