"""PPO_KERNEL_ENV_CUT_STATE's surface without a GPU: the header defines the flag on bit 10 and its entry names the five envs it opens the truncation calls on,
the binding mirrors it, the ABI version and the exported set are what they were (the feature rides on one bit of kernel_flags: no symbol, no PPO_BUF_* id),
and ppo_ctx_create -- whose refusals are answered before the device is touched -- refuses the flag everywhere but on a fused device env."""
import ctypes as C
import os
import re
import subprocess

import pytest

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
NEW_ENVS = ("PPO_ENV_PENDULUM", "PPO_ENV_ACROBOT", "PPO_ENV_FROZENLAKE", "PPO_ENV_FROZENLAKE8X8", "PPO_ENV_BLACKJACK")


def flat(text):
    return " ".join(text.replace(" *", " ").split())


@pytest.fixture(scope="module")
def P():
    return load_package()


def test_header_defines_the_flag_with_value_1024(P, tmp_path):
    assert re.search(r"^#define\s+PPO_KERNEL_ENV_CUT_STATE\s+\(1 << 10\)", HEADER, re.M)
    exe = str(tmp_path / "flag_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], check=True,
                   input=b'#include <stdio.h>\n#include "ppo_hip.h"\nint main(void) { printf("%d %d %d %d\\n", (int)PPO_KERNEL_ENV_CUT_STATE, (int)PPO_ABI_VERSION, '
                         b'(int)sizeof(ppo_config), (int)(PPO_KERNEL_ENV_CUT_STATE | PPO_KERNEL_CAT_FUSED)); return 0; }\n')
    flag, abi, size, both = (int(x) for x in subprocess.check_output([exe]).split())
    assert (flag, abi, both) == (1024, 5, 1280) and size == C.sizeof(P.binding.Config)


def test_header_entry_names_the_envs_and_the_cost():
    start = HEADER.index(" *   PPO_KERNEL_ENV_CUT_STATE ")
    para = flat(HEADER[start:HEADER.index("enum { PPO_KERNEL_ROLLOUT_VECTOR")])
    for words in NEW_ENVS + ("PPO_ENV_MOUNTAINCAR_CONTINUOUS", "PPO_ENV_TAXI", "BEFORE the auto-reset", "[STATE + 1, T N]", "ppo_get_buffer does not reach it",
                             "no store at any other sample", "nothing cleared between rollouts", "KEEP = true", "cut_state_fold_kernel",
                             "ppo_env_truncation_bootstrap and ppo_env_truncations", "Opt-in, never implied", "PPO_ERR_UNSUPPORTED",
                             "beside PPO_KERNEL_ENV_GENERIC", "59 680 bytes at 2 and 3", "63 840 at 6", "68 064 at 16", "84 960 at 45", "93 408 at 64",
                             "neither claimed nor tested"):
        assert words in para, words


def test_each_env_block_says_what_the_flag_serves():
    text = flat(HEADER)
    for name in NEW_ENVS:
        if name == "PPO_ENV_FROZENLAKE8X8":
            continue   # the two FrozenLake kinds share a block
        block = text[text.index("/* %s (new" % name):]
        block = block[:block.index("enum {")]
        assert "With PPO_KERNEL_ENV_CUT_STATE in kernel_flags" in block and "served from that record" in block, name
    boot = text[text.index("Time-limit truncations of the context's own environments"):text.index("PPO_API ppo_status ppo_env_truncation_bootstrap")]
    assert "PPO_KERNEL_ENV_CUT_STATE" in boot and "recomputes nothing" in boot


def test_binding_mirrors_it(P):
    assert P.KERNEL_ENV_CUT_STATE == 1024 == P.binding.KERNEL_ENV_CUT_STATE
    assert "KERNEL_ENV_CUT_STATE" in P.binding.Context.env_truncation_bootstrap.__doc__


def test_abi_version_and_symbols_are_unchanged(P):
    lib = P.binding.lib()
    assert lib.ppo_abi_version() == 5 == P.binding.ABI_VERSION
    assert len(P.binding.ABI_SYMBOLS) == len(set(P.binding.ABI_SYMBOLS)) == 92
    for name in P.binding.ABI_SYMBOLS:
        assert hasattr(lib, name), name


def create(P, **kw):
    """-> (status, message) of ppo_ctx_create; a context that comes to life (a machine with a GPU) is closed at once"""
    d = dict(num_envs=8, num_steps=4)
    d.update(kw)
    cfg = P.make_config(**d)
    h = C.c_void_p()
    st = P.binding.lib().ppo_ctx_create(C.byref(cfg), C.byref(h))
    msg = P.binding.lib().ppo_last_error(None)
    if st == 0:
        P.binding.lib().ppo_ctx_destroy(h)
    return st, (msg.decode() if msg else "")


@pytest.mark.parametrize("kw", [dict(), dict(env_kind=1, obs_size=2, head_dims=(3,)), dict(env_kind=2, obs_size=16), dict(env_kind=3),
                                dict(kernel_flags=512), dict(kernel_flags=512, hidden=128)],
                         ids=["cartpole", "mountaincar", "synthetic", "host", "beside-env-generic", "beside-env-generic-wide"])
def test_ctx_create_refuses_the_flag_off_the_fused_envs(P, kw):
    kw = dict(kw)
    kw["kernel_flags"] = kw.get("kernel_flags", 0) | P.KERNEL_ENV_CUT_STATE
    st, msg = create(P, **kw)
    assert st == 5 and "PPO_KERNEL_ENV_CUT_STATE" in msg, (st, msg)
    assert ("excludes PPO_KERNEL_ENV_GENERIC" in msg) == bool(kw["kernel_flags"] & 512), msg


def test_the_next_bit_is_still_unknown(P):
    for flags in (2048, 2048 | 1024, 2048 | 512):
        st, msg = create(P, kernel_flags=flags)
        assert st == 1 and "unknown bits in kernel_flags 0x%x" % flags in msg, (st, msg)


def test_a_fused_env_accepts_the_flag_beside_its_family_flag(P):
    """accepted: a live context on a machine with a GPU, or the end at hipSetDevice (status 2) without one; without the family flag the env's own refusal"""
    forms = {4: (P.DIST_GAUSSIAN, 3, 1, 64), 5: (P.DIST_GAUSSIAN, 2, 1, 64), 6: (0, 6, 3, 256), 8: (P.DIST_MASKED, 19, 6, 256), 10: (0, 16, 4, 256),
             11: (0, 64, 4, 256), 13: (0, 45, 2, 256)}
    for kind, (dist, obs, actions, family) in forms.items():
        kw = dict(env_kind=kind, dist_kind=dist, obs_size=obs, head_dims=(actions,), max_episode_steps=3)
        st, msg = create(P, kernel_flags=family | P.KERNEL_ENV_CUT_STATE, **kw)
        assert st in (0, 2), (kind, st, msg)
        st, msg = create(P, kernel_flags=P.KERNEL_ENV_CUT_STATE, **kw)
        assert st == 5 and "needs PPO_KERNEL_" in msg, (kind, st, msg)
