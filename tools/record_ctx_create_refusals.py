#!/usr/bin/env python3
"""Writes tests/golden/ctx_create_refusals.json: status and message of every config of tests/refusal_grid.py's grid that ppo_ctx_create refuses with
PPO_ERR_INVALID (1) or PPO_ERR_UNSUPPORTED (5).  Needs no GPU.  The committed file is the record of the library BEFORE a change to the checks: to compare a
new build against it, write to another path (--out) and diff; tests/test_ctx_create_refusals_cpu.py does the same comparison case by case.

    python tools/record_ctx_create_refusals.py [--out FILE]      (PPO_HIP_LIBRARY names another build of the library)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ctx_create_refusals.json"))
    args = ap.parse_args()
    cases = G.ctx_create_cases(load_package())
    recorded = G.by_message(cases, keep=lambda status: status in (1, 5))
    with open(args.out, "w") as f:
        json.dump(recorded, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d configs, %d refused with status 1 or 5, %d distinct messages -> %s" % (len(cases), sum(len(g["cases"]) for g in recorded), len(recorded), args.out))


if __name__ == "__main__":
    main()
