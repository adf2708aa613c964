#!/usr/bin/env python3
"""Writes tests/golden/device_env_refusals.json: the answers of the context-level refusals of the fused device envs (tests/refusal_grid.py: device_env_cases),
one small context per env kind on the GPU.  The committed file is the record of the library BEFORE a change to those entry points: to compare a new build
against it, write to another path (--out) and diff; tests/test_gpu_device_env_refusals.py does the same comparison case by case.

    python tools/record_device_env_refusals.py [--out FILE]      (PPO_HIP_LIBRARY names another build of the library)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from __graft_entry__ import load_package  # noqa: E402
import refusal_grid as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "device_env_refusals.json"))
    args = ap.parse_args()
    cases = G.device_env_cases(load_package())
    with open(args.out, "w") as f:
        json.dump(cases, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d answers -> %s" % (len(cases), args.out))


if __name__ == "__main__":
    main()
