"""The host half of the device event lists (ppo-libtorch_amd/csrc/trunc_events.hpp: the count clamp, sort_events, copy_events_out) without a GPU:
host/tests/trunc_events_test.cpp, a program of its own with no HIP in it, built and run under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ppo-libtorch_amd")


def test_host_half_under_sanitizers(tmp_path):
    exe = str(tmp_path / "trunc_events_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "tests", "trunc_events_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "trunc_events_test ok" in r.stdout and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
