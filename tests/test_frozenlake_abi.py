"""PPO_ENV_FROZENLAKE / PPO_ENV_FROZENLAKE8X8's surface without a GPU: the header declares the two env kinds (10 and 11, as sums, each in an enum of its own)
and states the env -- maps, state, step, the draw keyed by state words, reset map, the accepted form, the refusals -- the binding and the package mirror
them, the facade files exist, and the ABI version and the exported set are what they were (the envs ride on existing calls)."""
import ctypes as C
import os
import re
import subprocess

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()


def test_header_declares_the_envs_and_states_them(tmp_path):
    # enums of their own, written as sums: older tests pin the first list's text and every "PPO_ENV_x = digit" of the header
    assert re.search(r"enum\s*\{\s*PPO_ENV_FROZENLAKE\s*=\s*PPO_ENV_TAXI\s*\+\s*2\s*\}", HEADER)
    assert re.search(r"enum\s*\{\s*PPO_ENV_FROZENLAKE8X8\s*=\s*PPO_ENV_TAXI\s*\+\s*3\s*\}", HEADER)
    assert not re.search(r"PPO_ENV_FROZENLAKE\w*\s*=\s*\d", HEADER)
    exe = str(tmp_path / "frozenlake_enum_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], check=True,
                   input=b'#include <stdio.h>\n#include "ppo_hip.h"\nint main(void) { printf("%d %d %d\\n", (int)PPO_ENV_FROZENLAKE, (int)PPO_ENV_FROZENLAKE8X8, '
                         b'(int)PPO_ENV_TAXI); return 0; }\n')
    assert subprocess.check_output([exe]).split() == [b"10", b"11", b"8"]
    assert re.search(r"#define\s+PPO_ABI_VERSION\s+5\b", HEADER)
    # the block stands behind the PPO_ENV_TAXI enum line and in front of the distributions' text: nothing of Taxi's block moved
    taxi_enum = HEADER.index("enum { PPO_ENV_TAXI = PPO_ENV_ACROBOT + 2 }")
    start = HEADER.index("/* PPO_ENV_FROZENLAKE (new; value 10)")
    end = HEADER.index("PPO_DIST_CATEGORICAL reproduces", start)
    assert taxi_enum < start < HEADER.index("enum { PPO_ENV_FROZENLAKE = ") < HEADER.index("enum { PPO_ENV_FROZENLAKE8X8 = ") < end
    block = " ".join(HEADER[start:end].replace("\n *", " ").split())   # the comment as running text: a phrase may stand across a line break
    for words in ("PPO_ENV_FROZENLAKE8X8 (new; value 11)", "is_slippery = True", "THE STATE CARRIES", "pure function of (state, action)",
                  "SFFF FHFH FFFH HFFG", "holes {5, 7, 11, 12}", "0x18a0", "goal 15",
                  "SFFFFFFF FFFFFFFF FFFHFFFF FFFFFHFF FFFHFFFF FHHFFFHF FHFFHFHF FFFHFFFG", "holes {19, 29, 35, 41, 42, 46, 49, 52, 54, 59}",
                  "0x0852460820080000", "goal 63", "cell = row * n + col", "State (cell, j, k0, k1)", "PPO_BUF_ENV_STATE is f32 [4, N]",
                  "clamped into 0..3: 0 left, 1 down, 2 right, 3 up", "reward 0, terminated 1, cell unchanged, j' = min(j + 1, 2^24 - 1)",
                  "philox4x32_10(key = (k0, k1); counter = (j >> 2, 0, 0, 0x20))", "philox4x32_10(k0, k1, c0, c1, c2, c3)", "word = w[j & 3]",
                  "d = (uint64(word) * 3) >> 32", "eff = (a + d + 3) & 3", "[(a-1)%4, a, (a+1)%4]", "reward = cell' == goal ? 1.0f : 0.0f", "k0 and k1 stay",
                  "philox4x32_10(seed; e, k, 0, 1)", "cell = 0, j = 0, k0 = w.x >> 8, k1 = w.y >> 8", "Global env 0 takes reset 1",
                  "obs_size 16 resp. 64", "the one-hot of cell", "not j, k0, k1", "1..16 777 215", "Returns are 0 or 1",
                  "PPO_ERR_INVALID and changes nothing", "a NaN becomes 0", "saturated, not truncated",
                  # the accepted form, the launches, the refusals, and why 10
                  "dist_kind = PPO_DIST_CATEGORICAL", "PPO_DIST_MASKED is refused", "head_dims[0] = 4", "obs_size = 16 resp. 64", "hidden = 64",
                  "PPO_KERNEL_CAT_FUSED (required, never implied)", "1 <= max_episode_steps <= 16 777 215", "ppo_env_transition(10 | 11, state [n, 4], action i64 [n], ...)",
                  "cat_rollout_kernel", "62 912 bytes", "88 256 bytes", "cat_eval_kernel", "ppo_env_truncation_bootstrap and ppo_env_truncations",
                  "which the stored observation does not hold", "Sharding is neither claimed nor tested", "value 9 stays unassigned"):
        assert words in block, words


def test_binding_and_package_mirror_them():
    P = load_package()
    assert P.ENV_FROZENLAKE == 10 == P.binding.ENV_FROZENLAKE and P.ENV_FROZENLAKE8X8 == 11 == P.binding.ENV_FROZENLAKE8X8
    assert (P.ENV_CARTPOLE, P.ENV_MOUNTAINCAR, P.ENV_SYNTHETIC, P.ENV_HOST, P.ENV_PENDULUM, P.ENV_MOUNTAINCAR_CONTINUOUS, P.ENV_ACROBOT, P.ENV_TAXI) == \
        (0, 1, 2, 3, 4, 5, 6, 8)
    for kind, obs in ((P.ENV_FROZENLAKE, 16), (P.ENV_FROZENLAKE8X8, 64)):
        cfg = P.make_config(env_kind=kind, dist_kind=P.DIST_CATEGORICAL, obs_size=obs, head_dims=(4,), kernel_flags=P.KERNEL_CAT_FUSED, max_episode_steps=100)
        assert (cfg.env_kind, cfg.dist_kind, cfg.obs_size, cfg.n_heads, cfg.head_dims[0], cfg.kernel_flags, cfg.max_episode_steps) == (kind, 0, obs, 1, 4, 256, 100)


def test_abi_version_and_symbols_are_unchanged():
    P = load_package()
    lib = P.binding.lib()
    assert lib.ppo_abi_version() == 5 == P.binding.ABI_VERSION
    assert len(P.binding.ABI_SYMBOLS) == len(set(P.binding.ABI_SYMBOLS)) == 92
    for name in P.binding.ABI_SYMBOLS:
        assert "frozen" not in name.lower() and "lake" not in name.lower()
    cfg = P.make_config()
    assert cfg.struct_size == C.sizeof(type(cfg))   # sizeof(ppo_config) as the binding lays it out; the library refuses any other (tests/test_abi_symbols.py)


def test_transition_answers_bad_arguments_with_a_status():
    P = load_package()
    L = P.binding.lib()
    buf = (C.c_float * 8)()
    act = (C.c_int64 * 2)()
    term = (C.c_int32 * 2)()
    for kind in (10, 11):
        # null pointers, a negative count: PPO_ERR_INVALID (1); n = 0: nothing to do.  None of them launches anything.
        assert L.ppo_env_transition(kind, None, act, 1, buf, buf, term, None) == 1
        assert L.ppo_env_transition(kind, buf, None, 1, buf, buf, term, None) == 1
        assert L.ppo_env_transition(kind, buf, act, 1, None, buf, term, None) == 1
        assert L.ppo_env_transition(kind, buf, act, -1, buf, buf, term, None) == 1
        assert L.ppo_env_transition(kind, buf, act, 0, buf, buf, term, None) == 0
        assert L.ppo_env_transition_f32(kind, buf, buf, 0, buf, None, buf, term, None) == 5


def test_facade_files_exist():
    host = os.path.join(ROOT, "ppo-libtorch_amd", "host")
    for rel in ("Environments/FrozenLake.h", "Environments/FrozenLake.cpp", "PPO/PPO_DiscreteFrozenLake.h", "tests/host_frozenlake_test.cpp"):
        assert os.path.isfile(os.path.join(host, rel)), rel
    mk = open(os.path.join(host, "Makefile")).read()
    assert "host_frozenlake_test" in mk and "Environments/FrozenLake.cpp" in mk
    hdr = open(os.path.join(host, "PPO", "PPO_DiscreteFrozenLake.h")).read()
    assert "PPO_ENV_FROZENLAKE8X8" in hdr and "PPO_DIST_CATEGORICAL" in hdr and "fused_categorical" in hdr and "m_obs_size == 64" in hdr
    for rel in ("tools/frozenlake_cost.py", "tools/frozenlake_curve.py"):
        assert os.path.isfile(os.path.join(ROOT, rel)), rel
