#!/usr/bin/env python3
"""bench.py -- env-steps/sec (rollout + GAE + update) of the MI355X-native PPO hot path, BASELINE.json's metric.

  python bench.py --gpus N --steps K --warmup W [--workload cartpole|mountaincar|config4] [--dump-outputs DIR] [--full]
  N > 1, either way:  * the plain command above: before anything touches HIP the process starts N FRESH rank processes
                        (python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py <same flags>), relays rank 0's JSON
                        line and exits with their return code;
                      * python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ... (RANK / WORLD_SIZE in the environment).
  Gradient all-reduce of N > 1 (--transport): auto = RCCL (ncclAllReduce over xGMI, the transport BASELINE.json names); only when its bring-up fails,
  the one-shot direct exchange, brought up in checked stages.  exchange / both = the direct exchange as an opt-in A/B (both: RCCL is `value`, the
  exchange is reported beside it in `transport_ab`).  The transport that ran and why are top-level fields of the line.

A "step" is one pass of the hot path over one batch: one iteration of PPO_Discrete::train()'s loop (reference
PPO/PPO_Discrete.cpp:511-659) = rollout of num_steps x num_envs env-steps, GAE scan, update_epochs x num_minibatches optimizer
steps.  Default workload (the one BASELINE.json's metric is quoted on): configs[1] at N = 1 (CartPole-v1, 4096 envs x 128 steps,
2x64 MLP, 4 minibatches x 10 epochs, hyper-parameters of the reference's CartPoleRecommendedSettings.toml with action_size = 2);
N > 1: every rank owns 4096 envs (weak scaling, configs[2] at N = 8) and ONE gradient all-reduce per optimizer step crosses xGMI.
--workload mountaincar = configs[3] (8192 envs, CategoricalMasked); --workload config4 = one GPU's share of configs[4] (synthetic env,
obs 376, heads [3,3,3,2], 4x256 MLP, bf16 MFMA GEMMs, 2048 envs per GPU).
value = env-steps of all ranks / max-over-ranks wall time of the K timed steps; the reference prints the same quantity as `fps`
(PPO_Discrete.cpp:650-652,718).  Everything is resident in HBM when the timed region starts.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps, writes the last step's outputs (--dump-outputs DIR) and prints
the line; what else the line can carry is measured only with --full.  Extra objects of every run:
  roofline      dominant kernel (fused gather+forward+loss+backward): algorithmic FLOPs per launch / its average launch
                duration measured with HIP events on the kernel's own stream inside the timed region (--full adds the committed counter traffic and trace duration)
With --full besides:
  profiles      the committed profile set the quoted fields come from (see profile_tie)
  gae_roofline  the GAE scan (the kernel BASELINE.json's HBM-roofline target names), algorithmic bytes / launch time: 200 launches in a row
                on this workload's buffers (live; the duration the committed rocprofv3 trace agrees with), the in-iteration HIP-event
                reading beside it, the same at 4096 / 8192 / 32768 envs, and the floor probe
  value_runs    the headline's K-step region timed R more times (same bracket each): median / min / max -- `value` itself stays the FIRST region, the one
                the round contract defines
  other_workloads  BASELINE configs[3] (MountainCar, 8192 envs) and one GPU's share of configs[4] (2048 envs, bf16) timed live in this same run, >= 0.5 s each:
                value, ms_per_step and the dominant kernel's roofline fraction (N = 1, default workload only; --no-other-workloads skips them)
  cpu_baseline  the reference's own CPU ThreadPool path (oracle/_ref/ref_harness = the unmodified reference compiled against
                LibTorch CPU) timed on this host, or the C port when that binary is absent -- a reported baseline
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F32_PEAK_TFLOPS = 157.3   # MI355X dense f32 (vector = f32-input MFMA) peak, MI355X_MICROARCH.md "Chip-level parameters"
BF16_PEAK_TFLOPS = 2500.0  # dense bf16 / f16 MFMA peak (same table)
HBM_PEAK_GBS = 8000.0     # HBM3E spec peak


def flops_per_sample(obs, act, hidden=64, n_hidden=2):
    """Algorithmic FLOPs of forward + backward of both MLPs for one sample (2 FLOP per MAC; backward = 2 x forward)."""
    macs = 0
    for out in (1, act):
        macs += obs * hidden + (n_hidden - 1) * hidden * hidden + hidden * out
    return 3 * 2 * macs


_PROFILE_TIE = None


def profile_tie():
    """The committed profile set whose numbers this run may quote: the NEWEST profiles/<tag>_meta.json (tools/collect_profiles.sh) whose source fingerprint
    equals this tree's (tools/src_fingerprint.py: every kernel source, header and the Makefile of the library the run loads).  Counters and the tracer cannot
    run inside the timed region, so `traffic`, the in-trace durations, the floor probe and the curve comparison come from that set -- or are null, with the reason
    here, when the sources have changed since it was measured."""
    global _PROFILE_TIE
    if _PROFILE_TIE is not None:
        return _PROFILE_TIE
    import importlib.util
    spec = importlib.util.spec_from_file_location("src_fingerprint", os.path.join(ROOT, "tools", "src_fingerprint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    here = mod.source_fingerprint()
    metas = []
    for f in glob.glob(os.path.join(ROOT, "profiles", "*_meta.json")):
        try:
            with open(f) as fh:
                metas.append(json.load(fh))
        except Exception:
            pass
    metas.sort(key=lambda d: d.get("collected_unix", 0))
    match = [d for d in metas if d.get("src_sha16") == here]
    if match:
        d = match[-1]
        _PROFILE_TIE = {"tied": True, "tag": d["tag"], "src_sha16": here, "lib_sha16_at_collection": d.get("lib_sha16"), "git_head_at_collection": d.get("git_head")}
    else:
        newest = metas[-1] if metas else None
        _PROFILE_TIE = {"tied": False, "tag": None, "src_sha16": here,
                        "reason": ("no committed profile set was measured on these sources" +
                                   (" (the newest, %s, on sources %s)" % (newest["tag"], newest.get("src_sha16")) if newest else " (no profiles/*_meta.json)") +
                                   ": the fields that would quote it are null")}
    return _PROFILE_TIE


def newest_profile(suffix):
    t = profile_tie()
    if not t["tied"]:
        return None
    f = os.path.join(ROOT, "profiles", t["tag"] + suffix)
    return f if os.path.exists(f) else None


UPDATE_KERNEL_C1 = "fwd_bwd_mfma_ws_kernel<0, 4, 2>"   # configs[1]'s instantiation (plain Categorical, obs 4, two logits); MountainCar's is <1, 2, 3>
GAE_EXACT_4096 = "gae_kernel<16, 0, true, false, 128"   # the exact scan configs[1] launches (kernels_gae.hip: launch_scan; <strip columns, GAE, 16-byte accesses, not ppo_gae_fast, 128-row tile, ...>)


def pmc_traffic(prefix):
    """HBM-side bytes per launch of the kernel whose name starts with `prefix`, from the newest committed rocprofv3 --pmc summary
    (profiles/*_pmc_per_dispatch.json, written by tools/collect_profiles.sh: FETCH_SIZE and WRITE_SIZE in separate passes, corrected
    as MI355X_MICROARCH.md prescribes -- see tools/pmc_summary.py).  Counters cannot be read from inside the timed run, so this is the
    committed measurement of the same command, or None."""
    f = newest_profile("_pmc_per_dispatch.json")
    if not f:
        return None
    try:
        with open(f) as fh:
            d = json.load(fh)
        for k, v in d.items():
            if k.startswith(prefix) and "hbm_read_bytes" in v and "hbm_write_bytes" in v:
                return {"bytes": v["hbm_read_bytes"] + v["hbm_write_bytes"], "read": v["hbm_read_bytes"], "write": v["hbm_write_bytes"],
                        "source": "profiles/" + os.path.basename(f)}
    except Exception:
        return None
    return None


def rocprof_kernel_us(prefix):
    """Average in-trace duration (us) of a kernel from the newest committed rocprofv3 --kernel-trace --stats summary."""
    f = newest_profile("_kernel_stats.csv")
    if not f:
        return None
    try:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if prefix in row["Name"]:
                    return {"avg_us": float(row["AverageNs"]) / 1e3, "calls": int(row["Calls"]), "source": "profiles/" + os.path.basename(f)}
    except Exception:
        return None
    return None


def curve_parity_summary():
    """The committed measurement of tests/test_gpu_curves.py (profiles/r*_curves.json): the free-running build against the unmodified reference's
    learning curves (ten seeds each, tests/golden/curves_*.json), two lines per scenario."""
    f = newest_profile("_curves.json")
    if not f:
        return None
    try:
        with open(f) as fh:
            rows = json.load(fh)
        return {"source": "profiles/" + os.path.basename(f) + " (python tests/test_gpu_curves.py)",
                "scenarios": [{"scenario": r["scenario"],
                               "steps_to_ep_len_195": "build median %.0f, reference median %.0f [min %.0f, max %.0f], Mann-Whitney p = %.2f"
                                                      % (r["steps_to_195"]["build_median"], r["steps_to_195"]["ref_median"], r["steps_to_195"]["ref_min"], r["steps_to_195"]["ref_max"], r["steps_to_195"]["mannwhitney_p"]),
                               "plateau_ep_len": "build median %.1f, reference median %.1f [min %.1f, max %.1f], Mann-Whitney p = %.2f"
                                                 % (r["plateau"]["build_median"], r["plateau"]["ref_median"], r["plateau"]["ref_min"], r["plateau"]["ref_max"], r["plateau"]["mannwhitney_p"])}
                              for r in rows]}
    except Exception:
        return None


def c4_traffic():
    f = newest_profile("_config4_traffic.json")
    if not f:
        return None
    try:
        with open(f) as fh:
            d = json.load(fh)
        return {"bytes_per_minibatch_step": d["bytes_per_minibatch_step"], "read": d["read_per_step"], "write": d["write_per_step"], "source": "profiles/" + os.path.basename(f)}
    except Exception:
        return None


def committed_jsonl(suffix):
    f = newest_profile(suffix)
    if not f:
        return None
    try:
        with open(f) as fh:
            return {"rows": [json.loads(l) for l in fh if l.strip().startswith("{")], "source": "profiles/" + os.path.basename(f)}
    except Exception:
        return None


def gae_in_trace_by_size():
    """rocprofv3 --kernel-trace durations of the scan by size (profiles/<tag>_gae_by_size.json): the method BASELINE.md section 4 prescribes for the 40 % bar."""
    f = newest_profile("_gae_by_size.json")
    if not f:
        return None
    try:
        with open(f) as fh:
            d = json.load(fh)
        return {"rows": [{"envs": r["envs"], "avg_us": r["avg_ns"] / 1e3, "frac": r["frac_of_8TBps"], "launches": r["launches"]} for r in d["rows"]],
                "source": "profiles/" + os.path.basename(f)}
    except Exception:
        return None


def gae_floor_us():
    """Committed floor probe (tools/probes/gae_floor: the scan's own strip decomposition with the chain replaced by nothing), back-to-back us at 4096 envs."""
    d = committed_jsonl("_gae_floor.jsonl")
    if not d:
        return None
    for row in d["rows"]:
        if row.get("N") == 4096:
            out = {"empty_launch_us": row.get("empty_us"), "plain_stream_us": row.get("stream_us"), "chain_free_strip_us": row.get("column_us"), "source": d["source"]}
            if row.get("chain_us") is not None:
                # the 128-step walk with nothing else in its way (no global traffic), and the sum no overlap can beat: the strip's memory round trip + drain
                # (chain-free strip) plus the walk, which can start only when its first rows are there and must end before its last rows leave
                out.update({"chain_only_us": row.get("chain_us"), "chain_minus_empty_us": row.get("chain_minus_empty_us"),
                            "strip_plus_chain_us": row.get("column_plus_chain_us"),
                            "verdict": "probes, not a bound: the bar at 4096 envs allows 3.28 us per launch, an empty launch and a plain stream of the same bytes leave it 0.9 and 0.2 us; the scan pipelined in time (gae_pipe_kernel: load, walk and store overlapped) was built and runs 4.3 - 4.8 us there, no faster than the three-phase kernel; the bar is met from 8192 envs (in trace)"
                                       if (row.get("column_plus_chain_us") or 0) > 3.29 else None})
            return out
    return None


def run_reference(num_envs, num_steps, updates, threads=0, timeout=900):
    ref = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
    if not os.path.exists(ref):
        return None
    try:
        out = subprocess.run([ref, "bench", str(num_envs), str(num_steps), str(updates), str(threads)], capture_output=True, text=True, timeout=timeout).stdout
        m = re.search(r"REF_BENCH (\{.*\})", out)
        return json.loads(m.group(1)) if m else None
    except Exception as ex:
        sys.stderr.write("reference harness failed: %r\n" % (ex,))
        return None


def cpu_baseline(num_envs, num_steps, obs, act):
    # ONE full update iteration (rollout + GAE + 40 optimizer steps) of the unmodified reference's PPO_Discrete::train() on the FULL headline workload
    # (4096 envs x 128 steps), twice: with the pool the reference builds itself -- ThreadPool(hardware_concurrency) (PPO_Discrete.cpp:40), oversubscribed on
    # a many-core host: one job per env per step, the queue lock dominates -- and with the same pool class at 16 threads (+ LibTorch's intra-op threads capped
    # to match), a width at which the number is not an artefact of lock contention.  ~1 min + ~10 s of CPU work.
    r = run_reference(num_envs, num_steps, 1)
    if r:
        what = "1 full update iteration (rollout+GAE+update) of the unmodified reference's PPO_Discrete::train() on LibTorch CPU, %d envs x %d steps (the full headline workload)" % (num_envs, num_steps)
        out = {"value": r["env_steps_per_sec"], "unit": "env-steps/s", "cores": int(r["threads"]), "kind": "reference",
               "sample": what + ", ThreadPool(hardware_concurrency) as the reference builds it",
               "note": "a reported baseline -- the GPU/CPU ratio says nothing about kernel quality; with %d threads the reference's pool is oversubscribed "
                       "(one job per env per step: its queue lock dominates), see `capped_pool` for a sane width" % int(r["threads"])}
        c = run_reference(num_envs, num_steps, 1, threads=16)
        if c:
            out["capped_pool"] = {"value": c["env_steps_per_sec"], "unit": "env-steps/s", "cores": int(c["threads"]),
                                  "sample": what + ", the reference's ThreadPool class at 16 threads (public member replaced before train()), at::set_num_threads(16)"}
        # BASELINE.json configs[0]: the reference's own CPU-runnable case, 8 envs x 128 steps
        c1 = run_reference(8, 128, 20)
        if c1:
            out["configs0"] = {"value": c1["env_steps_per_sec"], "unit": "env-steps/s", "cores": int(c1["threads"]),
                               "workload": "BASELINE.json configs[0]: CartPole-v1, PPO_Discrete, 8 envs x 128 steps, 20 update iterations, reference CPU ThreadPool path"}
        return out
    # C port (scalar, single thread): one rollout of a bounded env count + one minibatch of the update, scaled per env-step
    import numpy as np
    import oracle as O
    n = 256
    net = O.Net.make(obs, [act])
    rng = np.random.default_rng(0)
    params = (rng.standard_normal(O.param_count(net)) * 0.1).astype(np.float32)
    env = O.VecEnv(O.ENV_CARTPOLE, n, 2, 500)
    t0 = time.perf_counter()
    x = env.init()
    for t in range(num_steps):
        a, lp, en, v = O.act(net, params, x, 2, t)
        x, r, d = env.step(a[:, 0])
    t_roll = time.perf_counter() - t0
    B = n * num_steps
    hp = O.HParams(gamma=0.98, gae_lambda=0.95, clip_coef=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, norm_adv=1, clip_vloss=1)
    obs_b = rng.standard_normal((B, obs)).astype(np.float32)
    z = rng.standard_normal(B).astype(np.float32)
    t0 = time.perf_counter()
    O.minibatch_grads(net, hp, params, obs_b, (rng.random(B) < 0.5).astype(np.float32), z * 0.1 - 0.7, z, z, z, np.arange(B))
    t_upd = (time.perf_counter() - t0) * 10  # 10 epochs over the batch
    return {"value": B / (t_roll + t_upd), "unit": "env-steps/s", "cores": 1, "kind": "port",
            "sample": "scalar C restatement, 1 thread: %d envs x %d steps rollout + 10 epochs of forward/backward over that batch" % (n, num_steps)}


DUMP_CAP = 1 << 20   # elements per dumped array: eleven arrays of at most 4 MiB each stay under 64 MB


def dump_outputs(ctx, out_dir):
    """What the timed path hands its caller after its last step, as <out_dir>/<name>.npy: the trained parameters and AdamW moments, the rollout
    the update trained on, its advantages and returns (float32, flattened), and the update's statistics (stats.npy: float64, in the field order
    of ppo_stats).  An array of more than DUMP_CAP elements is written as a fixed sample -- sorted flat indices drawn from a generator seeded by
    the array's size -- so runs with the same arguments dump the same positions."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    m, v, _ = ctx.get_optimizer()
    arrays = {"params": ctx.get_params(), "exp_avg": m, "exp_avg_sq": v}
    for name in ("OBS", "ACTIONS", "LOGPROBS", "REWARDS", "DONES", "VALUES", "ADVANTAGES", "RETURNS"):
        arrays[name.lower()] = ctx.read(name)
    for name, a in arrays.items():
        a = a.astype(np.float32).ravel()
        if a.size > DUMP_CAP:
            a = a[np.sort(np.random.default_rng(a.size).choice(a.size, DUMP_CAP, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)
    np.save(os.path.join(out_dir, "stats.npy"), np.array(list(ctx.stats().values()), np.float64))


WORKLOADS = {
    # name: (BASELINE.json configs index at N = 1, at N = 8)
    "cartpole": dict(envs=4096, obs=4, heads=(2,), hidden=64, n_hidden=2, max_steps=500, cfg1=1, cfg8=2,
                     label="CartPole-v1 PPO_Discrete, %d envs x %d steps per GPU, 2x64 MLP, 4 minibatches x 10 epochs"),
    "mountaincar": dict(envs=8192, obs=2, heads=(3,), hidden=64, n_hidden=2, max_steps=200, cfg1=3, cfg8=3,
                        label="MountainCar PPO_MultiDiscrete (CategoricalMasked), %d envs x %d steps per GPU, 2x64 MLP, 4 minibatches x 10 epochs"),
    "config4": dict(envs=2048, obs=376, heads=(3, 3, 3, 2), hidden=256, n_hidden=4, max_steps=1000, cfg1=4, cfg8=4,
                    label="PPO_MultiDiscrete synthetic env obs 376 heads [3,3,3,2], %d envs x %d steps per GPU (16384 / 8), 4x256 MLP bf16 MFMA GEMMs, 4 minibatches x 10 epochs"),
}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: a timed region of ~0.5 s at the headline workload (200 x 2.5 ms) -- long enough for an outside observer's GPU-activity sampling to see it
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="cartpole")
    ap.add_argument("--envs", type=int, default=0, help="envs per GPU (default: the workload's)")
    ap.add_argument("--num-steps", type=int, default=128)
    ap.add_argument("--full", action="store_true", help="measure more than the headline: value_runs, the GAE scan's back-to-back runs (gae_roofline), "
                    "other_workloads, cpu_baseline, and the fields quoted from the committed profile set")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one computed as DIR/<name>.npy (rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: no cpu_baseline")
    ap.add_argument("--no-other-workloads", action="store_true", help="--full, N = 1, default workload: do not time configs[3] / configs[4] after the headline")
    ap.add_argument("--repeats", type=int, default=5, help="--full, N = 1: further timed repetitions of the K-step region after the headline one (value_runs); 0 = none")
    ap.add_argument("--comm-selftest", action="store_true", help="N = 1 only: drive the multi-rank code path (RCCL all-reduces over a one-rank communicator, "
                    "three-kernel optimizer step) to see its per-step cost on one GPU; not a valid headline number")
    ap.add_argument("--transport", choices=("auto", "rccl", "exchange", "both"), default="auto", help="N > 1: the gradient all-reduce. rccl = ncclAllReduce over xGMI; "
                    "exchange = one-shot direct exchange over HIP-IPC peer buffers (one kernel per rank and call), brought up in checked stages; auto = RCCL, the "
                    "exchange only if RCCL cannot be brought up (with --same-device: the exchange, RCCL refuses two ranks on one device); both = RCCL timed as "
                    "`value`, then the exchange timed beside it (`transport_ab`)")
    ap.add_argument("--same-device", action="store_true", help="rehearsal on a one-GPU box: every rank uses device 0 (exchange transport only)")
    ap.add_argument("--preflight", action="store_true", help="N > 1: fresh rank processes only create a small context each, bring the RCCL communicator up and run five "
                    "all-reduces of small integers (checked exactly), then exit: the first minute of a multi-GPU lease says whether the transport works at all, "
                    "with a reason, before any warm-up is spent")
    ap.add_argument("--kernel-flags", type=int, default=0, help="ppo_config.kernel_flags (include/ppo_hip.h PPO_KERNEL_*: 1 vector rollout, 2 vector update, "
                    "4 one-wave matrix-core update): A/B runs of the hand-written kernels; 0 = the defaults")
    ap.add_argument("--profile", type=int, default=-1, help="HIP-event timing inside the timed region: 0 off, 1 every kernel, 2 dominant kernel (1 launch in 8) + GAE, "
                    "4 the same with 1 launch in 41; default: 4 from 20 steps up (>= 20 samples), 2 below")
    ap.add_argument("--bringup-timeout", type=float, default=300.0, help="N > 1: seconds a rank may spend between start and the end of the warm-up before it gives up "
                    "and exits non-zero (a hung communicator bring-up must not hang the job)")
    ap.add_argument("--launch-timeout", type=float, default=1500.0, help="self-launcher: seconds the rank processes may run before their process group is killed")
    ap.add_argument("--fallback-reason", default=None, help=argparse.SUPPRESS)   # set by the self-launcher on its one retry
    ap.add_argument("--launch-worker", default=None, help=argparse.SUPPRESS)     # tests: the script the self-launcher starts instead of this file
    args, unknown = ap.parse_known_args(argv)
    if unknown and not args.launch_worker:   # a stand-in worker of the tests may take flags of its own
        ap.error("unrecognized arguments: %s" % " ".join(unknown))
    return args


def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args, argv):
    """`python bench.py --gpus N` with no torchrun environment: this process has not touched HIP and never will -- it starts N FRESH rank processes
    through torch.distributed.run, relays their stderr as it comes and rank 0's JSON line at the end, and exits with their return code.  A failed
    run with --transport auto is retried ONCE, in fresh processes again, on the other transport (never in place, never by re-executing a process
    that has initialised the GPU)."""
    import signal

    def visible_gpus():
        try:
            import torch   # device_count() does not initialise HIP
            return int(torch.cuda.device_count())
        except Exception:
            return -1
    n_vis = visible_gpus()
    if not args.same_device and 0 <= n_vis < args.gpus and not args.launch_worker:
        sys.stderr.write("bench.py: --gpus %d but %d GPU(s) visible; on a one-GPU box rehearse with --same-device\n" % (args.gpus, n_vis))
        return 2
    worker = args.launch_worker or os.path.abspath(__file__)
    passthrough = [a for a in argv]

    def attempt(extra):
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL and the direct exchange both share device memory across processes
        env.setdefault("OMP_NUM_THREADS", "1")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(free_port()), worker] + passthrough + extra
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env, start_new_session=True)
        try:
            out, _ = proc.communicate(timeout=args.launch_timeout)
            rc = proc.returncode
        except subprocess.TimeoutExpired:
            try:
                os.killpg(proc.pid, signal.SIGKILL)   # exactly the process group started above
            except ProcessLookupError:
                pass
            out, _ = proc.communicate()
            rc = 124
            sys.stderr.write("bench.py: rank processes killed after %.0f s (--launch-timeout)\n" % args.launch_timeout)
        lines = [l for l in (out or "").splitlines() if l.startswith("{") and l.rstrip().endswith("}")]
        for l in (out or "").splitlines():
            if l not in lines:
                sys.stderr.write(l + "\n")   # anything a rank printed besides the line
        return rc, (lines[-1] if lines else None)

    rc, line = attempt([])
    if (rc != 0 or line is None) and args.transport == "auto" and not args.same_device:
        sys.stderr.write("bench.py: run on RCCL failed (rc %d); one retry in fresh processes on the direct exchange\n" % rc)
        rc, line = attempt(["--transport", "exchange", "--fallback-reason", "the run with --transport auto (RCCL first) exited with rc %d" % rc])
    if line is not None and rc == 0:
        print(line, flush=True)
    return rc if rc != 0 else (0 if line is not None else 1)


def preflight(P, dist, rank, world, local_rank, args, watchdog):
    """RCCL first contact, nothing else: a 64-env context per rank, ncclGetUniqueId / ncclCommInitRank, five all-reduces of small integers through the
    library's own gradient all-reduce (ppo_allreduce_grads: the call a training step makes), each checked exactly, one JSON line from rank 0.  Every
    stage is agreed over the ranks (gloo), so a failure names its stage and rank instead of hanging its peers; the watchdog covers a hang."""
    import numpy as np
    stage, err, ctx = "context", None, None
    t0 = time.perf_counter()

    def agree(ok_here, what):
        ok = True if dist is None else P.dist.all_ranks_agree(dist, ok_here)
        if not ok_here:
            sys.stderr.write("preflight rank %d: %s failed: %r\n" % (rank, what, err))
        return ok
    try:
        cfg = P.dist.shard_config(P.make_config, rank, world, 64 * world, num_steps=8, num_minibatches=1, update_epochs=1, device=0 if args.same_device else local_rank)
        ctx = P.Context(cfg)
    except Exception as ex:
        err = ex
    if not agree(err is None, stage):
        return 5
    stage = "ncclGetUniqueId / ncclCommInitRank"
    ident = None
    if rank == 0:
        try:
            ident = P.comm_unique_id()
        except Exception as ex:
            err = ex
    if dist is not None:
        ident = P.dist.broadcast_bytes(dist, ident, src=0)
    if err is None:
        try:
            if ident is None:
                raise RuntimeError("rank 0 could not make an RCCL unique id")
            ctx.comm_init(ident, rank, world)
        except Exception as ex:
            err = ex
    if not agree(err is None, stage):
        return 6
    t_up = time.perf_counter() - t0
    stage = "all-reduce"
    pattern = (np.arange(ctx.P) % 97).astype(np.float32)
    try:
        for rep in range(5):
            ctx.write("GRADS", pattern * (rank + 1) * (rep + 1))
            P.binding._check(P.binding.lib().ppo_allreduce_grads(ctx.h), ctx.h)
            got = ctx.read("GRADS")
            if not np.array_equal(got, pattern * (rep + 1) * (world * (world + 1) // 2)):
                raise RuntimeError("all-reduce %d returned wrong sums on rank %d" % (rep, rank))
    except Exception as ex:
        err = ex
    if not agree(err is None, stage):
        return 7
    watchdog.disarm()
    if rank == 0:
        print(json.dumps({"preflight": "ok", "n_gpus": world, "transport": "rccl" if world > 1 else "none", "bringup_s": t_up,
                          "allreduces_checked": 5, "payload_floats": int(ctx.P)}), flush=True)
    if dist is not None:
        dist.barrier()
    ctx.close()
    return 0


def main():
    argv = sys.argv[1:]
    args = parse_args(argv)
    W = WORKLOADS[args.workload]

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args, argv))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        args.gpus = world
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # before this process's first HIP call (ppo_hip.h, direct exchange; RCCL needs it too)

    # N > 1: nothing between here and the end of the warm-up may hang the job -- a rank that is still bringing its communicator up after
    # --bringup-timeout seconds exits non-zero (torch.distributed.run then ends the other ranks)
    class Watchdog:
        """Ends this rank (exit code 3) when a bring-up stage is still running after --bringup-timeout seconds; armed around EVERY bring-up -- the
        first transport's and, with --transport both, the second one's -- and disarmed only while the timed regions run."""
        def __init__(self):
            self.t = None

        def arm(self, what):
            self.disarm()
            if world > 1 and args.bringup_timeout > 0:
                import threading

                def give_up():
                    sys.stderr.write("bench.py rank %d: %s still running after %.0f s -- giving up\n" % (rank, what, args.bringup_timeout))
                    sys.stderr.flush()
                    os._exit(3)
                self.t = threading.Timer(args.bringup_timeout, give_up)
                self.t.daemon = True
                self.t.start()

        def disarm(self):
            if self.t is not None:
                self.t.cancel()
                self.t = None
    watchdog = Watchdog()
    watchdog.arm("communicator bring-up / warm-up")

    from __graft_entry__ import load_package
    P = load_package()
    dist = None
    if world > 1:
        dist, rank, world = P.dist.init_process_group("gloo")  # plumbing only: rendezvous, id broadcast, barrier, max over ranks
    if args.preflight:
        sys.exit(preflight(P, dist, rank, world, local_rank, args, watchdog))
    obs, heads = W["obs"], W["heads"]
    act = sum(heads)
    N, T = args.envs or W["envs"], args.num_steps
    # the learning-rate schedule covers every iteration a --full run makes; a plain run keeps the same schedule, so both compute the same K steps
    total_updates = args.steps + args.warmup + max(args.repeats, 0) * args.steps

    def make_cfg(workload, n_envs, updates):
        w = WORKLOADS[workload]
        kind = dict(cartpole=(P.ENV_CARTPOLE, P.DIST_CATEGORICAL), mountaincar=(P.ENV_MOUNTAINCAR, P.DIST_MASKED), config4=(P.ENV_SYNTHETIC, P.DIST_MASKED))[workload]
        return P.dist.shard_config(P.make_config, rank, world, n_envs * world, env_kind=kind[0], dist_kind=kind[1], obs_size=w["obs"],
                                   head_dims=w["heads"], hidden=w["hidden"], n_hidden=w["n_hidden"], num_steps=T, num_minibatches=4, update_epochs=10,
                                   max_episode_steps=w["max_steps"], seed=2, total_timesteps=updates * n_envs * T * world, learning_rate=1e-3, gamma=0.98,
                                   gae_lambda=0.95, clip_coef=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, anneal_lr=True,
                                   device=0 if args.same_device else local_rank,
                                   compute_dtype=P.DTYPE_BF16 if workload == "config4" else P.DTYPE_F32,
                                   # ppo_config.kernel_flags: which kernel runs a stage (A/B runs); --same-device with more than two ranks: the vector update
                                   # kernel (ranks waiting in the exchange sit on every CU, and a matrix-core update workgroup needs a CU's whole register
                                   # file: tests/test_gpu_exchange.py); --comm-selftest: a real one-rank RCCL communicator
                                   kernel_flags=args.kernel_flags | (P.KERNEL_UPDATE_VECTOR if args.same_device and world > 2 else 0)
                                                | (P.KERNEL_COMM_SELFTEST if args.comm_selftest and world == 1 else 0))
    cfg = make_cfg(args.workload, N, total_updates)

    def warm(c):
        try:
            c.init_orthogonal(2)   # same seed on every rank: replicated weights
            c.env_reset()
            c.sync()
        finally:
            # every rank has its code object loaded and its envs reset before anyone starts the first iteration: a kernel of the direct exchange
            # waits a bounded time for a peer's share, and a rank that is still loading must not use that up (reached by every rank: see the callers)
            if dist is not None:
                dist.barrier()
        for _ in range(args.warmup):
            c.train_iteration()
        c.sync()

    def start_rccl():
        """RCCL bring-up in agreed stages (every rank walks the same host collectives whether or not its own stage failed).  None = some rank failed."""
        c, err = None, None
        try:
            c = P.Context(cfg)
            if args.comm_selftest and world == 1:
                c.comm_init(P.comm_unique_id(), 0, 1)
        except Exception as ex:
            err = ex
        if world > 1:
            # stage 1: every rank has its context (device, buffers) before anyone enters ncclCommInitRank -- a rank that failed here would leave its
            # peers blocked inside it until the watchdog fires
            if not P.dist.all_ranks_agree(dist, err is None):
                if err is not None:
                    sys.stderr.write("rank %d: context creation failed (%r)\n" % (rank, err))
                if c is not None:
                    c.close()
                return None, repr(err) if err is not None else "a peer failed to create its context"
            ident = None
            if rank == 0 and err is None:
                try:
                    ident = P.comm_unique_id()
                except Exception as ex:
                    err = ex
            ident = P.dist.broadcast_bytes(dist, ident, src=0)
            if err is None:
                try:
                    if ident is None:
                        raise RuntimeError("rank 0 could not make an RCCL unique id")
                    c.comm_init(ident, rank, world)
                except Exception as ex:
                    err = ex
            if not P.dist.all_ranks_agree(dist, err is None):
                if err is not None:
                    sys.stderr.write("rank %d: RCCL bring-up failed (%r)\n" % (rank, err))
                if c is not None:
                    c.close()
                return None, repr(err) if err is not None else "a peer failed RCCL bring-up"
        elif err is not None:
            raise err
        warm(c)
        return c, None

    def start_exchange():
        # brought up in checked stages (dist.start_exchange_checked): None = some rank failed a stage, nothing is left open
        return P.dist.start_exchange_checked(lambda: P.Context(cfg), warm, dist, rank, world)

    def timed(c, steps=None):
        """K steps bracketed by barrier + synchronize on both sides; max over ranks.  A direct-exchange wait that ran out makes ctx.sync() raise
        (PPO_ERR_COMM) and the count is agreed over the ranks besides: a run whose replicas diverged prints no number."""
        def barrier():
            c.sync()
            if dist is not None:
                dist.barrier()
            c.sync()
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps or args.steps):
            c.train_iteration()
        c.sync()
        dt_own = time.perf_counter() - t0      # this rank's own K steps, before it waits for the others
        if dist is not None:
            dist.barrier()
        c.sync()
        dt = time.perf_counter() - t0
        rank_times.append(dt_own)
        if dist is not None:
            dt = P.dist.max_over_ranks(dist, dt)
            if not P.dist.all_ranks_agree(dist, c.comm_exchange_timeouts() == 0):
                sys.stderr.write("rank %d: a direct-exchange wait ran out inside the timed region: no number\n" % rank)
                sys.stderr.flush()
                os._exit(4)
        return dt

    rank_times = []   # this rank's own seconds for the K steps of each timed() call
    requested = args.transport
    fallback_reason = args.fallback_reason
    if world == 1:
        transport = "none"
        ctx, _ = start_rccl()
    else:
        first = "exchange" if (requested == "exchange" or (requested == "auto" and args.same_device)) else "rccl"
        if requested in ("rccl", "both") and args.same_device:
            sys.exit("RCCL refuses two ranks on one device: --same-device rehearses the direct exchange only")
        if requested == "auto" and args.same_device:
            fallback_reason = fallback_reason or "--same-device: RCCL cannot place two ranks on one device"
        ctx, transport = None, first
        if first == "rccl":
            ctx, why = start_rccl()
            if ctx is None:
                if requested != "auto":
                    sys.exit("RCCL transport failed its bring-up: %s" % why)
                fallback_reason = "RCCL bring-up failed: %s" % why
                transport = "exchange"
        if ctx is None:
            ctx = start_exchange()
            if ctx is None:
                sys.exit("direct-exchange transport failed its start-up checks")
    watchdog.disarm()

    if args.profile < 0:
        args.profile = 4 if args.steps >= 20 else 2
    ctx.profile_enable(args.profile)
    dt = timed(ctx)
    prof = ctx.profile_read()
    if args.dump_outputs and rank == 0:
        dump_outputs(ctx, args.dump_outputs)
    # the same K-step region R more times, bracketed the same way, with the same event sampling running: how far one 41-ms region is from the next on this box
    value_runs = None
    if args.full and world == 1 and args.repeats > 0:
        reps = [timed(ctx) for _ in range(args.repeats)]
        vals = sorted(args.steps * N * T / d for d in [dt] + reps)
        value_runs = {"runs": len(vals), "values": [args.steps * N * T / d for d in [dt] + reps], "median": vals[len(vals) // 2] if len(vals) % 2 else 0.5 * (vals[len(vals) // 2 - 1] + vals[len(vals) // 2]),
                      "min": vals[0], "max": vals[-1], "unit": "env-steps/s",
                      "note": "the first entry is `value` (the contract's K steps after W warm-up steps); the others are the same K-step region again, each between its own "
                              "synchronisations"}
    ctx.profile_enable(0)
    st = ctx.stats()
    # N > 1: what every rank measured by itself, so that a scaling record can be read in one pass -- its own time for the K steps (min / max show a
    # straggler) and the device time of its gradient all-reduces (HIP events around the collective on the context's stream: the wait for the slowest
    # peer is inside)
    per_rank = None
    if dist is not None:
        ar_n = prof["allreduce_launches"]
        rows = P.dist.values_of_ranks(dist, [1e3 * rank_times[0] / args.steps, (1e3 * prof["allreduce_ms"] / ar_n) if ar_n else -1.0, float(ar_n)])
        per_rank = {"rank_ms_per_step": [r[0] for r in rows], "rank_ms_per_step_min": min(r[0] for r in rows), "rank_ms_per_step_max": max(r[0] for r in rows),
                    "allreduce_us_per_call": [r[1] if r[1] >= 0 else None for r in rows], "allreduce_calls_sampled": [int(r[2]) for r in rows],
                    "allreduce_us_per_step": [(40 * r[1]) if r[1] >= 0 else None for r in rows],
                    "note": "allreduce_us_per_call: HIP events around one gradient all-reduce in 41 (every optimizer step has one; x 40 = per bench step); the "
                            "statistics all-reduce (one per update) is not in it"}

    # opt-in A/B: the same K steps on the one-shot direct exchange, in a second context, after the RCCL number is in hand
    transport_ab = None
    if world > 1 and requested == "both":
        try:
            watchdog.arm("the second transport's bring-up (--transport both)")
            cx = start_exchange()
            watchdog.disarm()
            if cx is None:
                transport_ab = {"transport": "exchange", "failed": "start-up checks"}
            else:
                dtx = timed(cx)
                transport_ab = {"transport": "exchange", "value": args.steps * (args.envs or W["envs"]) * args.num_steps * world / dtx, "unit": "env-steps/s",
                                "ms_per_step": 1e3 * dtx / args.steps}
                cx.close()
        except Exception as ex:   # every rank takes the same branch: start_exchange_checked agrees on failures, timed() raises on all or none
            transport_ab = {"transport": "exchange", "failed": repr(ex)}

    # GAE scan back to back, outside the timed region: on the context's own buffers (this workload's size) and on fresh buffers of the three
    # sizes the roofline is quoted at -- wall time of 200 launches / 200: no event pair (~3 us on a 5 us launch), no foreign kernel in front
    def gae_b2b(n_envs, bufs=None, fast=False):
        import numpy as np
        if bufs is None:
            rng = np.random.default_rng(n_envs)
            bufs = [ctx.dev(np.where(rng.random((T, n_envs), dtype=np.float32) < 0.05, -1.0, 1.0).astype(np.float32)),
                    ctx.dev(rng.standard_normal((T, n_envs), dtype=np.float32)), ctx.dev((rng.random((T, n_envs), dtype=np.float32) < 0.05).astype(np.float32)),
                    ctx.dev(rng.standard_normal(n_envs, dtype=np.float32)), ctx.dev((rng.random(n_envs) < 0.05).astype(np.int32)),
                    ctx.empty((T, n_envs), np.float32), ctx.empty((T, n_envs), np.float32)]
        reps = 200
        for _ in range(3):
            P.gae_launch(ctx, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], T, n_envs, 0.98, 0.95, bufs[5], bufs[6], fast=fast)
        ctx.sync()
        tg = time.perf_counter()
        for _ in range(reps):
            P.gae_launch(ctx, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], T, n_envs, 0.98, 0.95, bufs[5], bufs[6], fast=fast)
        ctx.sync()
        ms = 1e3 * (time.perf_counter() - tg) / reps
        nbytes = 20 * n_envs * T + 8 * n_envs
        return {"envs": n_envs, "bytes_per_launch": nbytes, "avg_launch_ms": ms, "achieved": nbytes / (ms * 1e-3) / 1e9, "frac": nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}

    class _Ptr:
        def __init__(self, p):
            self.ptr = p
    gae_rows, gae_fast_rows = [], []
    if rank == 0 and args.full:
        own = [_Ptr(ctx.buffer_ptr(n)[0]) for n in ("REWARDS", "VALUES", "DONES", "NEXT_VALUE", "NEXT_DONE", "ADVANTAGES", "RETURNS")]
        gae_own = gae_b2b(N, own)
        gae_rows = [gae_b2b(n) for n in (4096, 8192, 32768, 131072)]
        gae_fast_rows = [gae_b2b(n, fast=True) for n in (4096, 8192, 32768)]   # the associative scan (ppo_gae_fast): NOT what training runs

    # BASELINE configs[3] and one GPU's share of configs[4], live in this run (N = 1, the default command): a context each, 5 warm-up iterations, then whole
    # iterations for >= 0.5 s between two synchronisations; the dominant kernel by HIP events on the context's stream as for the headline
    def measure_other(name):
        w = WORKLOADS[name]
        n_envs = w["envs"]
        probe_iters, min_seconds, warm_iters = 3, 0.5, 5
        budget = 400   # iterations the learning-rate schedule covers (far more than run)
        c = P.Context(make_cfg(name, n_envs, budget))
        try:
            c.init_orthogonal(2)
            c.env_reset()
            for _ in range(warm_iters):
                c.train_iteration()
            c.sync()
            t0 = time.perf_counter()
            for _ in range(probe_iters):
                c.train_iteration()
            c.sync()
            per_iter = (time.perf_counter() - t0) / probe_iters
            steps = max(10, min(budget - warm_iters - probe_iters - 1, int(min_seconds / per_iter) + 1))
            c.profile_enable(4)
            c.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                c.train_iteration()
            c.sync()
            dt_o = time.perf_counter() - t0
            pr = c.profile_read()
            c.profile_enable(0)
            st_o = c.stats()
        finally:
            c.close()
        m_rows = (n_envs * T) // 4
        fl_o = flops_per_sample(w["obs"], sum(w["heads"]), w["hidden"], w["n_hidden"]) * m_rows
        fb = pr["fwd_bwd_ms"] / pr["fwd_bwd_launches"] if pr["fwd_bwd_launches"] > 0 else None
        return {"config": {"workload": (w["label"] % (n_envs, T)) + " (BASELINE.json configs[%d]%s)" % (w["cfg1"], ", one GPU's share" if name == "config4" else ""),
                           "num_envs_per_gpu": n_envs, "num_steps": T, "minibatch_per_gpu": m_rows, "optimizer_steps_per_step": 40},
                "value": steps * n_envs * T / dt_o, "unit": "env-steps/s", "steps": steps, "warmup": warm_iters + probe_iters, "ms_per_step": 1e3 * dt_o / steps, "timed_seconds": dt_o,
                "dtype": "bf16" if name == "config4" else "f32 (update GEMMs: two-term f16 split on f16 MFMA, fp32 accumulate)",
                "roofline": {"kernel": ("one minibatch step of the generic path (forward with heads + loss + head backward in its epilogue, backward per layer, slab sums; both nets in every launch; the optimizer launch is outside the bracket)"
                                        if name == "config4" else "fwd_bwd_mfma_ws_kernel (gather+forward+PPO loss+backward)"),
                             "bound": "mfma", "flops_per_launch": fl_o, "avg_launch_ms": fb, "launches": pr["fwd_bwd_launches"],
                             "achieved": fl_o / (fb * 1e-3) / 1e12 if fb else None, "peak": BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                             "frac": fl_o / (fb * 1e-3) / 1e12 / BF16_PEAK_TFLOPS if fb else None,
                             "sampling": "HIP events on the context's stream around 1 launch in 41"},
                "train_stats": {k: st_o[k] for k in ("loss", "ep_len_mean", "explained_variance", "global_step")}}

    other_workloads = None
    if args.full and rank == 0 and world == 1 and args.workload == "cartpole" and not args.no_other_workloads and not args.comm_selftest and args.kernel_flags == 0:
        other_workloads = {}
        for name in ("mountaincar", "config4"):
            try:
                other_workloads[name] = measure_other(name)
            except Exception as ex:   # the headline line is printed whatever happens here
                other_workloads[name] = {"failed": repr(ex)}

    if rank == 0:
        env_steps = args.steps * N * T * world
        M = (N * T) // 4
        fl = flops_per_sample(obs, act, W["hidden"], W["n_hidden"]) * M

        def per_launch(kind_):
            n = prof[kind_ + "_launches"]
            return prof[kind_ + "_ms"] / n if n > 0 else None
        fb_ms, gae_ms = per_launch("fwd_bwd"), per_launch("gae")
        gae_bytes = 20 * N * T + 8 * N
        generic = args.workload == "config4"
        if generic:
            roof = {"kernel": "one minibatch step of the generic path, both nets in every launch: ONE fused forward launch (generic_forward_kernel, rows read in place through the "
                              "index list; heads, masked categorical, PPO loss and the head layers' backward in its epilogue on the tile still in LDS), one fused backward launch per "
                              "hidden layer and for layer 0 (bwd_layer_kernel: weight gradient + the gradient handed down from one LDS-DMA'd tile), slab sums; the optimizer launch is "
                              "outside the bracket: bf16 operands and activations, f32 accumulation", "bound": "mfma",
                    "achieved": fl / (fb_ms * 1e-3) / 1e12 if fb_ms else None, "peak": BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": fl / (fb_ms * 1e-3) / 1e12 / BF16_PEAK_TFLOPS if fb_ms else None}
        else:
            # what the matrix cores execute per 32-sample tile and net in fwd_bwd_mfma_ws_kernel: 82 v_mfma_f32_32x32x16_f16 (layer 1 with
            # its bias 6, the layer-2 bias 2, layer 2 / d(hidden) / dW2 24 each -- three f16 products per fp32 product --, dz2 2 [6 beyond two logits]) and
            # 12 v_mfma_f32_16x16x32_f16 (dW1, db1)
            tiles = (M + 31) // 32
            f16_fl = 2 * tiles * ((82 if act <= 2 else 86) * (2 * 32 * 32 * 16) + 12 * (2 * 16 * 16 * 32))
            roof = {"kernel": "fwd_bwd_mfma_ws_kernel (gather+forward+PPO loss+backward, wave-specialised: 8 forward + 4 gradient waves per workgroup; fp32 carried "
                              "as two fp16 terms, three f16 MFMA products per fp32 product)",
                    # `frac` = ALGORITHMIC work (53 376 FLOP per sample, forward + backward of both nets) / launch duration / the dense f16
                    # matrix peak, i.e. the peak of the pipe the kernel issues on.  `frac_executed` counts what that pipe executes (the three-product
                    # emulation of fp32 plus the zero padding of the small products: 3.4 x the algorithmic FLOP) -- the pipe's utilisation, not a roofline fraction.
                    "bound": "mfma", "limiter": "lds+valu (LDS pipe ~55 % busy, ~15 vector instructions per MFMA: DESIGN.md section 4)",
                    "achieved": fl / (fb_ms * 1e-3) / 1e12 if fb_ms else None, "peak": BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": fl / (fb_ms * 1e-3) / 1e12 / BF16_PEAK_TFLOPS if fb_ms else None,
                    "achieved_executed": f16_fl / (fb_ms * 1e-3) / 1e12 if fb_ms else None,
                    "frac_executed": f16_fl / (fb_ms * 1e-3) / 1e12 / BF16_PEAK_TFLOPS if fb_ms else None,
                    "executed_flops_per_launch": f16_fl,
                    # yardstick only: 157.3 TFLOP/s is the peak of the fp32 matrix instruction, which this kernel does not issue
                    "fp32_mfma_peak": F32_PEAK_TFLOPS, "frac_of_fp32_mfma_peak": fl / (fb_ms * 1e-3) / 1e12 / F32_PEAK_TFLOPS if fb_ms else None}
        roof.update({"flops_per_launch": fl, "avg_launch_ms": fb_ms, "launches": prof["fwd_bwd_launches"],
                     "sampling": "HIP events on the context's stream around 1 launch in %s (--profile %d)" % ({1: "1", 2: "8", 4: "41"}.get(args.profile, "?"), args.profile)})
        phases = {"rollout": "rollout", "gae": "gae", "grad_reduce": "reduce", "clip_adamw": "optimizer"}
        out = {
            "metric": "env-steps/sec (rollout+update)", "value": env_steps / dt, "unit": "env-steps/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16" if generic else "f32 (update GEMMs: two-term f16 split on f16 MFMA, fp32 accumulate; everything else IEEE f32)",
            # the gradient all-reduce that ran (N > 1), what was asked for, and why they differ if they do
            "transport": transport, "transport_requested": requested if world > 1 else None, "transport_fallback_reason": fallback_reason,
            "comm_ranks": world, "transport_ab": transport_ab, "per_rank": per_rank,
            "data": "synthetic (counter-based env, random-init 4x256 actor/critic)" if generic else "synthetic (fixed-seed %s, random-init 2x64 actor/critic)" % ("CartPole-v1" if args.workload == "cartpole" else "MountainCar"),
            "config": {"workload": (W["label"] % (N, T)) + " (BASELINE.json configs[%d]%s)" % (W["cfg1"] if world == 1 else W["cfg8"], ", one GPU's share" if generic and world == 1 else ""),
                       "num_envs_per_gpu": N, "num_steps": T, "global_batch": N * T * world,
                       "minibatch_per_gpu": M, "optimizer_steps_per_step": 40, "parallelism": "dp%d (env-sharded, 1 gradient all-reduce per optimizer step%s)" % (world, {"exchange": ": one-shot direct exchange over IPC peer buffers", "rccl": ": RCCL", "none": ""}[transport]) + (" [comm self-test]" if args.comm_selftest else "") + (" [all ranks on ONE device: rehearsal]" if args.same_device and world > 1 else "")},
            "roofline": roof,
            # HIP-event time per iteration of the phases that were bracketed (--profile 1 brackets all of them); null = not sampled in this run
            "phase_ms_per_step": dict({k: (prof[v + "_ms"] / args.steps if prof[v + "_launches"] > 0 else None) for k, v in phases.items()},
                                      fwd_bwd=40 * fb_ms if fb_ms else None),
            "train_stats": {k: st[k] for k in ("loss", "ep_len_mean", "ep_rew_mean", "explained_variance", "global_step")},
        }
        if args.full:
            gae_tr = pmc_traffic(GAE_EXACT_4096) if args.workload == "cartpole" else None
            if generic:
                # HBM bytes of one minibatch step: the committed --pmc measurement of this workload (tools/collect_profiles.sh, tools/c4_traffic.py)
                roof.update({"traffic": (c4_traffic() or {}).get("bytes_per_minibatch_step"), "traffic_detail": c4_traffic()})
            else:
                fb_tr = pmc_traffic(UPDATE_KERNEL_C1) if args.workload == "cartpole" else None
                roof.update({"traffic": (fb_tr or {}).get("bytes"), "traffic_detail": fb_tr,
                             "rocprof": rocprof_kernel_us(UPDATE_KERNEL_C1) if args.workload == "cartpole" else None})
            out["train_stats"]["learning_curve_parity"] = curve_parity_summary()
            out.update({
                "value_runs": value_runs, "other_workloads": other_workloads,
                # which committed profile set the fields measured outside this run (traffic, in-trace durations, floor probe, curve comparison) come from, tied to
                # the sources of the library this run loaded -- or why they are null
                "profiles": profile_tie(),
                # primary numbers: the launch by itself (200 in a row on this workload's own buffers, live, after the timed region) -- the duration
                # the rocprofv3 kernel trace agrees with; the in-iteration HIP-event reading (an event pair adds ~3 us to a ~5 us launch) is kept beside it
                "gae_roofline": {"kernel": "gae_kernel (exact mode; 4096 < envs <= 8192 take gae_pipe_kernel, the same scan pipelined in time; from 16384 envs 64-column strips x 32-row time tiles)", "bound": "hbm", "achieved": gae_own["achieved"], "peak": HBM_PEAK_GBS,
                                 "unit": "GB/s", "frac": gae_own["frac"],
                                 "traffic": (gae_tr or {}).get("bytes"), "traffic_detail": gae_tr, "bytes_per_launch": gae_bytes,
                                 "avg_launch_ms": gae_own["avg_launch_ms"], "launches": 200,
                                 "timing": "wall time of 200 back-to-back launches on this workload's buffers / 200, measured live after the timed region (no event pair, no foreign kernel in front)",
                                 "in_iteration": {"avg_launch_ms": gae_ms, "launches": prof["gae_launches"],
                                                  "achieved": gae_bytes / (gae_ms * 1e-3) / 1e9 if gae_ms else None,
                                                  "frac": gae_bytes / (gae_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if gae_ms else None,
                                                  "timing": "HIP events around the launch inside the iteration (the event pair adds ~3 us to a ~5 us launch)"},
                                 "back_to_back_sizes": gae_rows,
                                 "fast_mode": {"what": "ppo_gae_fast: the recurrence as a segmented scan of affine maps (all 256 lanes busy, chain 2 x 31 instead of 2 x 128 "
                                                       "operations); NOT bit-identical to the reference (<= 6 ulp of the largest advantage the chain carried, tests bound 16: profiles/r03_v4_gae_fast_report.jsonl), so training "
                                                       "does not use it; timed here to state what giving up the reference's association order would buy",
                                               "back_to_back_sizes": gae_fast_rows},
                                 # the 40 % bar of BASELINE.json, stated in one place: the smallest measured size that clears it, what the headline's
                                 # per-GPU size (configs[1] / [2]: 4096 envs) reaches, and the committed floor of a launch that moves the same bytes
                                 # (size_met_from_envs / frac_at_config1 are read off the IN-TRACE table -- rocprofv3 kernel time, the method BASELINE.md section 4
                                 # prescribes -- when a profile set is tied to this binary; back-to-back wall times overlap consecutive launches and read higher)
                                 "bar": {"target_frac": 0.40,
                                         "size_met_from_envs": next((r["envs"] for r in sorted((gae_in_trace_by_size() or {"rows": []})["rows"], key=lambda r: r["envs"]) if r["frac"] >= 0.40), None),
                                         "frac_at_config1": next((r["frac"] for r in (gae_in_trace_by_size() or {"rows": []})["rows"] if r["envs"] == 4096), None),
                                         "in_trace": gae_in_trace_by_size(),
                                         "size_met_from_envs_back_to_back": next((r["envs"] for r in gae_rows if r["frac"] >= 0.40), None),
                                         "frac_at_config1_back_to_back": next((r["frac"] for r in gae_rows if r["envs"] == 4096), None),
                                         "budget_us_at_config1": (20 * 4096 * T + 8 * 4096) / (0.40 * HBM_PEAK_GBS * 1e9) * 1e6,
                                         "floor_us": gae_floor_us()},
                                 "rocprof": rocprof_kernel_us(GAE_EXACT_4096) if args.workload == "cartpole" else None,
                                 "floor_probe": committed_jsonl("_gae_floor.jsonl")}})
            if world == 1 and not args.no_cpu_baseline and args.workload == "cartpole":
                out["cpu_baseline"] = cpu_baseline(N, T, obs, act)
        print(json.dumps(out), flush=True)
    ctx.close()
    if dist is not None:
        # the measurement is complete and rank 0's line is out: a hiccup of the host-side rendezvous while the ranks leave (a peer that has already closed its
        # sockets) is reported, not turned into a failed run
        try:
            dist.barrier()
            dist.destroy_process_group()
        except Exception as e:   # noqa: BLE001
            sys.stderr.write("bench.py: rank %d: host-side teardown: %s\n" % (rank, e))


if __name__ == "__main__":
    main()
