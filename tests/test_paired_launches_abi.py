"""PPO_KERNEL_SEPARATE_LAUNCHES's surface without a GPU: include/ppo_hip.h defines it on a bit of its own beside the PPO_KERNEL_* enumerators, the binding
mirrors it, and a config carries it."""
import os
import re

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()


def test_header_defines_the_flag_on_a_free_bit():
    m = re.search(r"^#define\s+PPO_KERNEL_SEPARATE_LAUNCHES\s+(\d+)\b", HEADER, re.M)
    assert m and int(m.group(1)) == 128
    others = [int(v) for _, v in re.findall(r"(PPO_KERNEL_[A-Z_0-9]+)\s*=\s*(\d+)", HEADER)]
    assert others and all(v & (v - 1) == 0 for v in others + [128])   # one bit each ...
    assert 128 not in others and 128 == 2 * max(others)               # ... none reused, the next free one


def test_binding_mirrors_it():
    P = load_package()
    assert P.KERNEL_SEPARATE_LAUNCHES == 128 and P.binding.KERNEL_SEPARATE_LAUNCHES == 128
    assert P.make_config(kernel_flags=P.KERNEL_SEPARATE_LAUNCHES).kernel_flags == 128
