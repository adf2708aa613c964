"""PPO_KERNEL_ENV_REWARD_NORM's surface without a GPU: the header defines the flag on bit 13, spelt as the shift (bits 11 and 12 stay unassigned), and the
reward-normalisation block states the device envs' contract; the binding mirrors the flag; the ABI version, ppo_config and the exported set are what they were
(the feature rides on one bit of kernel_flags and three existing calls: no symbol, no PPO_BUF_* id); and ppo_ctx_create -- whose refusals are answered before
the device is touched -- accepts the flag exactly where PPO_KERNEL_ENV_CUT_STATE is accepted.  tests/test_gpu_env_reward_norm.py runs the kernels."""
import ctypes as C
import os
import re
import subprocess

import pytest

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
CSRC = os.path.join(ROOT, "ppo-libtorch_amd", "csrc")
FLAG = 1 << 13
# env_kind -> (dist_kind, obs_size, actions, family flag): the seven fused device envs
FORMS = {4: (2, 3, 1, 64), 5: (2, 2, 1, 64), 6: (0, 6, 3, 256), 8: (1, 19, 6, 256), 10: (0, 16, 4, 256), 11: (0, 64, 4, 256), 13: (0, 45, 2, 256)}


def flat(text):
    return " ".join(text.replace(" *", " ").split())


@pytest.fixture(scope="module")
def P():
    return load_package()


def test_header_spells_the_flag_as_the_shift(P, tmp_path):
    assert re.search(r"^#define\s+PPO_KERNEL_ENV_REWARD_NORM\s+\(1 << 13\)", HEADER, re.M)
    assert not re.search(r"^#define\s+PPO_KERNEL_\w+\s+\(1 << 1[124]\)", HEADER, re.M)   # 11, 12 and 14 are nobody's
    exe = str(tmp_path / "flag_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], check=True,
                   input=b'#include <stdio.h>\n#include "ppo_hip.h"\nint main(void) { printf("%d %d %d %d\\n", (int)PPO_KERNEL_ENV_REWARD_NORM, (int)PPO_ABI_VERSION, '
                         b'(int)sizeof(ppo_config), (int)(PPO_KERNEL_ENV_REWARD_NORM | PPO_KERNEL_ENV_CUT_STATE | PPO_KERNEL_GAUSS_FUSED)); return 0; }\n')
    flag, abi, size, three = (int(x) for x in subprocess.check_output([exe]).split())
    assert (flag, abi, three) == (FLAG, 5, FLAG | 1024 | 64) and size == C.sizeof(P.binding.Config)


def test_header_states_the_contract():
    text = flat(HEADER)
    entry = text[text.index("/* PPO_KERNEL_ENV_REWARD_NORM (8192"):text.index("#define PPO_KERNEL_ENV_REWARD_NORM")]
    for words in ("PPO_ENV_PENDULUM", "PPO_ENV_MOUNTAINCAR_CONTINUOUS", "PPO_ENV_ACROBOT", "PPO_ENV_TAXI", "PPO_ENV_FROZENLAKE8X8", "PPO_ENV_BLACKJACK",
                  "beside PPO_KERNEL_ENV_CUT_STATE", "8 T N bytes", "no PPO_BUF_*", "launch for launch and bit for bit", "Opt-in, never implied",
                  "PPO_ERR_UNSUPPORTED", "beside PPO_KERNEL_ENV_GENERIC", "bits 11 and 12 stay unassigned"):
        assert words in entry, words
    block = text[text.index("Reward normalisation of caller-stepped environments"):text.index("PPO_API ppo_status ppo_reward_norm_enable(")]
    for words in ("PPO_KERNEL_ENV_REWARD_NORM", "ppo_env_reset zeroes ret and keeps the statistics", "ppo_env_set_state_h touches neither", "the same bits",
                  "(PPO_BUF_FIN_LEN[t][n] != 0)", "w, w + 256", "in slot order", "Mode 2 applies the frozen variance to all T N rewards",
                  "PPO_BUF_EP_REW, PPO_BUF_FIN_REW, ep_rew_mean and ppo_evaluate", "precedes the time-limit fold", "cut-state record", "THREE per rollout whatever T is",
                  "no host wait", "no floating-point atomics"):
        assert words in block, words


def test_binding_mirrors_it(P):
    assert P.KERNEL_ENV_REWARD_NORM == FLAG == P.binding.KERNEL_ENV_REWARD_NORM
    assert "KERNEL_ENV_REWARD_NORM" in P.binding.Context.reward_norm_enable.__doc__


def test_abi_version_and_symbols_are_unchanged(P):
    lib = P.binding.lib()
    assert lib.ppo_abi_version() == 5 == P.binding.ABI_VERSION
    assert len(P.binding.ABI_SYMBOLS) == len(set(P.binding.ABI_SYMBOLS)) == 92
    out = subprocess.check_output(["nm", "-D", "--defined-only", P.binding.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("ppo_")}
    assert exported == set(P.binding.ABI_SYMBOLS), exported ^ set(P.binding.ABI_SYMBOLS)


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


@pytest.mark.parametrize("kind", sorted(FORMS))
def test_a_fused_env_accepts_the_flag_beside_its_family_flag(P, kind):
    """accepted: a live context on a machine with a GPU, or the end at hipSetDevice (status 2) without one; without the family flag the env's own refusal"""
    dist, obs, actions, family = FORMS[kind]
    kw = dict(env_kind=kind, dist_kind=dist, obs_size=obs, head_dims=(actions,), max_episode_steps=3)
    for flags in (family | FLAG, family | FLAG | P.KERNEL_ENV_CUT_STATE):
        st, msg = create(P, kernel_flags=flags, **kw)
        assert st in (0, 2), (kind, flags, st, msg)
    st, msg = create(P, kernel_flags=FLAG, **kw)
    assert st == 5 and "needs PPO_KERNEL_" in msg, (kind, st, msg)


@pytest.mark.parametrize("kw", [dict(), dict(env_kind=1, obs_size=2, head_dims=(3,)), dict(env_kind=2, obs_size=16), dict(env_kind=3),
                                dict(kernel_flags=512), dict(kernel_flags=512, hidden=128)],
                         ids=["cartpole", "mountaincar", "synthetic", "host", "beside-env-generic", "beside-env-generic-wide"])
def test_ctx_create_refuses_the_flag_off_the_fused_envs(P, kw):
    kw = dict(kw)
    kw["kernel_flags"] = kw.get("kernel_flags", 0) | FLAG
    st, msg = create(P, **kw)
    assert st == 5 and "PPO_KERNEL_ENV_REWARD_NORM" in msg, (st, msg)
    assert ("excludes PPO_KERNEL_ENV_GENERIC" in msg) == bool(kw["kernel_flags"] & 512), msg


def test_the_neighbouring_bits_are_still_unknown(P):
    pend = dict(env_kind=4, dist_kind=2, obs_size=3, head_dims=(1,), max_episode_steps=3)
    for bit in (2048, 4096, 16384):
        for flags, kw in ((bit, {}), (bit | FLAG, {}), (bit | 512, {}), (bit | FLAG | 64, pend), (bit | 1024 | 64, pend)):
            st, msg = create(P, kernel_flags=flags, **kw)
            assert st == 1 and "unknown bits in kernel_flags 0x%x" % flags in msg, (flags, st, msg)


def test_the_kernels_are_in_the_reward_normaliser_file_and_count_no_step():
    """three launches whatever T is, ordered by their launch boundaries: no atomics, no wait, and the per-step kernel is still launched as it was"""
    src = open(os.path.join(CSRC, "kernels_rewnorm.hip")).read()
    body = src[src.index("hipError_t launch_rewnorm_rollout("):]
    body = body[:body.index("\n}\n")]
    assert body.count("hipLaunchKernelGGL(") == 4   # mode 2's one, mode 1's three
    for k in ("rewnorm_scan_kernel", "rewnorm_moments_kernel", "rewnorm_merge_apply_kernel", "rewnorm_apply_inplace_kernel"):
        assert body.count("hipLaunchKernelGGL(" + k) == 1, k
    assert not re.search(r"\bfor\b|\bwhile\b|Synchronize|hipMemcpy", body)
    assert "atomic" not in src.replace("floating-point atomics", "")
    assert re.search(r"hipLaunchKernelGGL\(rewnorm_update_apply_kernel, dim3\(1\)", src)
    api = open(os.path.join(CSRC, "api.hip")).read()
    roll = api[api.index("static ppo_status fused_env_rollout("):]
    roll = roll[:roll.index("\n}\n")]
    assert roll.index("gen_values(c, r.next_obs") < roll.index("env_normalise_rewards(c)") < roll.index("env_fold_truncations(c)")
    norm = api[api.index("static ppo_status env_normalise_rewards("):]
    norm = norm[:norm.index("\n}\n")]
    assert norm.count("launch_rewnorm_rollout(") == 1 and not re.search(r"Synchronize|hipMemcpy", norm)
