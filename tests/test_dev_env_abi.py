"""Caller-stepped environments on the device (include/ppo_hip.h, "Caller-stepped environments on the device": ppo_dev_env_reset / ppo_dev_act /
ppo_dev_observe) without a GPU: the header declares the three calls and cites the reference lines they replace, the binding lists them and has the
Context methods with the documented parameters, and the built library exports them.  tests/test_gpu_dev_env.py runs them."""
import inspect
import os
import re
import subprocess

from __graft_entry__ import ROOT, load_package

HDR = os.path.join(ROOT, "include", "ppo_hip.h")
CALLS = ["ppo_dev_env_reset", "ppo_dev_act", "ppo_dev_observe"]


def test_header_declares_the_device_calls():
    src = open(HDR).read()
    assert re.search(r"#define PPO_ABI_VERSION 5\b", src)   # additions only
    for name in CALLS:
        assert re.search(r"PPO_API\s+ppo_status\s+%s\s*\(" % name, src), name
    # the block sits behind the truncation block, cites the reference's loop, and states the stream rules
    block = src[src.index("Caller-stepped environments on the device"):src.index("ppo_dev_observe(ppo_ctx")]
    assert src.index("ppo_bootstrap_rewards(ppo_ctx") < src.index("Caller-stepped environments on the device")
    assert "PPO_Discrete.cpp:365-483, 524-548" in block
    for phrase in ("hipStreamNonBlocking", "only enqueues", "NULL is the null stream", "PPO_ERR_UNSUPPORTED", "IGNORED"):
        assert phrase in block, phrase
    # every bulk argument of the three calls is a pointer and the last one is the caller's stream
    for name in CALLS:
        args = re.search(r"PPO_API\s+ppo_status\s+%s\s*\(([^;]*)\);" % name, src).group(1)
        assert re.sub(r"/\*.*?\*/", "", args, flags=re.S).strip().endswith("void* caller_stream"), name


def test_binding_lists_the_device_calls():
    P = load_package()
    for name in CALLS:
        assert name in P.binding.ABI_SYMBOLS, name
    want = {"dev_env_reset": ["self", "obs", "stream"],
            "dev_act": ["self", "action", "mask", "stream"],
            "dev_observe": ["self", "obs", "reward", "done", "fin_len", "fin_rew", "truncated", "final_obs", "stream"]}
    for meth, names in want.items():
        sig = inspect.signature(getattr(P.Context, meth))
        assert list(sig.parameters) == names, (meth, list(sig.parameters))
        for opt in names[1:]:
            if opt not in ("obs", "action", "reward", "done"):
                assert sig.parameters[opt].default is None, (meth, opt)
    # data_ptr() is duck-typed: the binding does not import torch
    text = open(os.path.join(ROOT, "ppo-libtorch_amd", "binding.py")).read()
    assert not re.search(r"^\s*(import|from)\s+torch\b", text, flags=re.M)

    class Tensor:
        def data_ptr(self):
            return 0x7f0000001000

    class Stream:
        cuda_stream = 0x5000

    assert P.Context._dev_ptr(Tensor()).value == 0x7f0000001000 and P.Context._dev_ptr(None) is None
    assert P.Context._dev_ptr(0x1234).value == 0x1234 and P.Context._dev_ptr(P.binding.C.c_void_p(16)).value == 16
    assert P.Context._dev_stream(None, Stream()).value == 0x5000 and P.Context._dev_stream(None, 0).value is None


def test_library_exports_the_device_calls():
    P = load_package()
    subprocess.check_call(["make", "-s", "-j", "4", "-C", os.path.join(ROOT, "ppo-libtorch_amd", "csrc")])
    out = subprocess.check_output(["nm", "-D", "--defined-only", P.binding.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in CALLS:
        assert name in exported, name
        assert hasattr(P.binding.lib(), name)


def test_the_device_calls_never_wait():
    """The three entry points only enqueue: no stream / event / device synchronisation and no blocking copy in their bodies."""
    src = open(os.path.join(ROOT, "ppo-libtorch_amd", "csrc", "api.hip")).read()
    for name in CALLS:
        start = src.index('extern "C" ppo_status %s(' % name)
        body = src[start:src.index("\n}\n", start)]
        assert len(body) > 400 and not re.search(r"Synchronize|hipMemcpy\(", body), name
