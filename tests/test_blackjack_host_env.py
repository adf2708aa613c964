"""The host-side Blackjack class (ppo-libtorch_amd/host/Environments/Blackjack.cpp, the CPU twin of PPO_ENV_BLACKJACK with its own Philox) without a GPU: the env
part of host/tests/host_blackjack_test.cpp built as a program of its own (-DBLACKJACK_ENV_ONLY) under the address and undefined-behaviour sanitizers, and its
tallies over the 19 200 exhaustive rows against the numpy model's (tests/blackjack_model.py) on the same rows."""
import os
import re
import subprocess

import numpy as np

import blackjack_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppo-libtorch_amd", "host")
KEYS = ((11259375, 16777215), (20927, 3321251))


def test_env_part_under_sanitizers_and_against_the_model(tmp_path):
    import oracle
    oracle.build()
    exe = str(tmp_path / "host_blackjack_env_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DBLACKJACK_ENV_ONLY", "-I", HOST, os.path.join(HOST, "tests", "host_blackjack_test.cpp"),
                           os.path.join(HOST, "Environments", "Blackjack.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host_blackjack_env_test ok" in r.stdout and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    got = re.search(r"host Blackjack alone: (\d+) rows, sticks won (\d+) drew (\d+) lost (\d+), dealer play-outs of 0 cards (\d+), longest (\d+)", r.stdout)
    assert got, r.stdout
    rows = np.array([(int(M.pack(t, ace, show)), n, k0, k1) for (k0, k1) in KEYS for n in range(4, 12) for t in range(2, 32) for ace in (0, 1)
                     for show in range(1, 11)], np.int64)
    _, rew, _, drew = M.step(oracle, rows, np.zeros(len(rows), np.int64), with_draws=True)
    live = M.unpack(rows[:, 0])[0] <= 21
    want = (2 * len(rows), int((rew[live] == 1).sum()), int((rew[live] == 0).sum()), int((rew[live] == -1).sum()), int((drew[live] == 0).sum()), int(drew.max()))
    assert tuple(int(x) for x in got.groups()) == want, (got.groups(), want)
