"""PPO_KERNEL_GAUSS_FUSED's surface without a GPU: the header declares the flag (64) and ppo_gauss_fused_launches, the binding mirrors both, and the built
library answers a null context with an error instead of crashing."""
import ctypes as C
import os
import re

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()


def test_header_declares_the_flag_and_the_symbol():
    flags = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"(PPO_KERNEL_[A-Z_0-9]+)\s*=\s*(\d+)", HEADER))
    assert flags["PPO_KERNEL_GAUSS_FUSED"] == 64
    assert sorted(flags.values()) == [1, 2, 4, 8, 16, 32, 64]   # one bit each, none reused
    assert re.search(r"PPO_API\s+ppo_status\s+ppo_gauss_fused_launches\(ppo_ctx\*\s*\w+,\s*int64_t\*\s*act,\s*int64_t\*\s*value,\s*int64_t\*\s*update\);", HEADER)
    assert re.search(r"#define\s+PPO_ABI_VERSION\s+5\b", HEADER)


def test_binding_mirrors_both():
    P = load_package()
    assert P.KERNEL_GAUSS_FUSED == 64 and P.binding.KERNEL_GAUSS_FUSED == 64
    assert P.binding.ABI_SYMBOLS.count("ppo_gauss_fused_launches") == 1
    assert hasattr(P.Context, "gauss_fused_launches")
    assert P.make_config(kernel_flags=P.KERNEL_GAUSS_FUSED).kernel_flags == 64


def test_null_context_is_an_error():
    P = load_package()
    L = P.binding.lib()
    a, v, u = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert L.ppo_gauss_fused_launches(None, C.byref(a), C.byref(v), C.byref(u)) != 0
    assert (a.value, v.value, u.value) == (-1, -1, -1)
    assert L.ppo_last_error(None)
