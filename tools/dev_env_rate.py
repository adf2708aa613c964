"""Env-steps/s of a caller-stepped rollout with the env ON the GPU (include/ppo_hip.h ppo_dev_*), next to the same env behind the host calls.
Prints one JSON line.

The env is trivial and lives in device arrays: one device operation per step on the caller's stream (the observations are rewritten from a second device
array, an asynchronous device-to-device copy), fixed reward and done.  The caller's side is plain HIP through ctypes (the runtime libppo_hip.so is linked
against), so the tool runs wherever the library does.

  dev_sps            ppo_dev_act / env op / ppo_dev_observe on a side stream: nothing crosses PCIe and the host never waits inside the rollout
  host_sps           the same env stepped the only way the host calls allow: ppo_host_act (waits, actions to the host), actions copied up, the env op,
                     observations copied down, a wait, ppo_host_observe
  host_groups_sps    the host calls with --groups env groups (ppo_host_group_*): a group's next policy call is enqueued while the others are stepped

Each figure: whole iterations (rollout + update, streams idle at the end), best of --iters, at --envs x --steps (default 4096 x 128, obs 4, 2 x 64).
  --one-rollout      one device-fed rollout only (for a rocprofv3 --kernel-trace --stats run around it)
"""
import argparse
import ctypes as C
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

P = load_package()
P.binding.lib()
HIP = C.CDLL("libamdhip64.so.7")   # by soname: the runtime the library brought into the process
HIP.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
HIP.hipStreamSynchronize.argtypes = [C.c_void_p]
H2D, D2H, D2D = 1, 2, 3


def chk(status):
    if status != 0:
        raise RuntimeError("HIP status %d" % status)


def ctx(N, T, iters):
    c = P.Context(P.make_config(env_kind=P.ENV_HOST, num_envs=N, num_steps=T, num_minibatches=4, update_epochs=4, seed=1, total_timesteps=N * T * (iters + 2)))
    c.init_orthogonal(1)
    return c


class DevEnv:
    """obs <- obs_src (one device op per step), reward 1, done with probability 0.02 (fixed)"""

    def __init__(self, c):
        N = c.N
        rng = np.random.default_rng(0)
        self.obs_h = rng.uniform(-0.05, 0.05, (N, 4)).astype(np.float32)
        self.rew_h = np.ones(N, np.float32)
        self.done_h = (rng.random(N) < 0.02).astype(np.int32)
        self.obs_src, self.obs = c.dev(self.obs_h), c.dev(self.obs_h)
        self.rew, self.done = c.dev(self.rew_h), c.dev(self.done_h)
        self.act = c.empty((N, 1), np.int64)
        self.stream = C.c_void_p()
        chk(HIP.hipStreamCreateWithFlags(C.byref(self.stream), C.c_uint(1)))   # non-blocking
        self.row_bytes = 16

    def step(self, row0=0, rows=None):
        rows = self.obs_h.shape[0] if rows is None else rows
        off = row0 * self.row_bytes
        chk(HIP.hipMemcpyAsync(self.obs.ptr.value + off, self.obs_src.ptr.value + off, rows * self.row_bytes, D2D, self.stream))


def dev_iteration(c, env):
    c.host_rollout_begin()
    for _ in range(c.T):
        c.dev_act(env.act, stream=env.stream)
        env.step()
        c.dev_observe(env.obs, env.rew, env.done, stream=env.stream)
    c.host_rollout_end()


def host_step(c, env, a, out, row0, rows):
    """actions up, the env op, observations down, the wait: what a device env costs behind host arrays"""
    chk(HIP.hipMemcpyAsync(env.act.ptr.value + row0 * 8, a.ctypes.data, rows * 8, H2D, env.stream))
    env.step(row0, rows)
    chk(HIP.hipMemcpyAsync(out.ctypes.data + row0 * 16, env.obs.ptr.value + row0 * 16, rows * 16, D2H, env.stream))
    chk(HIP.hipStreamSynchronize(env.stream))


def host_iteration(c, env, out):
    c.host_rollout_begin()
    for _ in range(c.T):
        a = c.host_act()
        host_step(c, env, a, out, 0, c.N)
        c.host_observe(out, env.rew_h, env.done_h)
    c.host_rollout_end()


def group_iteration(c, env, out, G):
    N = c.N
    bounds = [g * (N // G) for g in range(G)] + [N]
    c.host_rollout_begin(bounds)
    for g in range(G):
        c.host_group_act(g)
    for t in range(c.T):
        for g in range(G):
            b0, b1 = bounds[g], bounds[g + 1]
            a = c.host_group_actions(g)
            host_step(c, env, a, out, b0, b1 - b0)
            c.host_group_observe(g, out[b0:b1], env.rew_h[b0:b1], env.done_h[b0:b1])
            if t + 1 < c.T:
                c.host_group_act(g)
    c.host_rollout_end()


def best_sps(c, env, run, iters):
    best = None
    for i in range(iters + 1):
        t0 = time.perf_counter()
        run()
        c.sync()
        chk(HIP.hipStreamSynchronize(env.stream))
        dt = time.perf_counter() - t0
        if i > 0:
            best = dt if best is None else min(best, dt)
    return c.N * c.T / best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--one-rollout", action="store_true")
    args = ap.parse_args()
    N, T = args.envs, args.steps
    out = {"box": socket.gethostname(), "N": N, "T": T}

    c = ctx(N, T, args.iters)
    env = DevEnv(c)
    c.dev_env_reset(env.obs, stream=env.stream)
    if args.one_rollout:
        dev_iteration(c, env)
        c.sync()
        chk(HIP.hipStreamSynchronize(env.stream))
        c.close()
        print(json.dumps(dict(out, one_rollout=True)))
        return
    out["dev_sps"] = best_sps(c, env, lambda: dev_iteration(c, env), args.iters)
    c.close()

    for key, G in (("host_sps", 0), ("host_groups_sps", args.groups)):
        c = ctx(N, T, args.iters)
        env = DevEnv(c)
        obs_out = env.obs_h.copy()
        c.host_env_reset(env.obs_h)
        run = (lambda: host_iteration(c, env, obs_out)) if G == 0 else (lambda: group_iteration(c, env, obs_out, G))
        out[key] = best_sps(c, env, run, args.iters)
        c.close()
    out["groups"] = args.groups
    print(json.dumps(out))


if __name__ == "__main__":
    main()
