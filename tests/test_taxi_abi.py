"""PPO_ENV_TAXI's surface without a GPU: the header declares the env kind (8, and says why not 7) and states the env -- stands, walls, step, mask,
observation, reset map, the accepted forms -- the binding and the package mirror it, the facade files exist, and the ABI version and the exported set are
what they were (the env rides on existing calls)."""
import ctypes as C
import os
import re
import subprocess

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()


def test_header_declares_the_env_and_states_it(tmp_path):
    # an enum of its own, written as a sum: older tests pin the first list's text and every "PPO_ENV_x = digit" of the header
    assert re.search(r"enum\s*\{\s*PPO_ENV_TAXI\s*=\s*PPO_ENV_ACROBOT\s*\+\s*2\s*\}", HEADER)
    exe = str(tmp_path / "taxi_enum_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], check=True,
                   input=b'#include <stdio.h>\n#include "ppo_hip.h"\nint main(void) { printf("%d %d\\n", (int)PPO_ENV_TAXI, (int)PPO_ENV_ACROBOT); return 0; }\n')
    assert subprocess.check_output([exe]).split() == [b"8", b"6"]
    assert re.search(r"#define\s+PPO_ABI_VERSION\s+5\b", HEADER)
    start = HEADER.index("/* PPO_ENV_TAXI (new; value 8)")
    block = HEADER[start:HEADER.index("PPO_DIST_CATEGORICAL reproduces", start)]
    for words in ("R = (0,0), G = (0,4), Y = (4,0), B = (4,3)", "c == 4, or r in {0,1} and c == 1, or r in {3,4} and c in {0,2}",
                  "c == 0 or east from (r, c-1) is blocked", "row = min(row+1, 4)", "row = max(row-1, 0)", "pass = dest, terminated 1, reward +20",
                  "clamped into 0..5", "[row < 4, row > 0, !east_blocked, !west_blocked, pass < 4 && on stand pass, pass == 4 && on a stand]",
                  "400, 400, 280, 280, 16, 16", "obs_size 19", "row in [0..4], col in [5..9], pass in [10..14], dest in [15..18]", "the first index on ties",
                  "philox4x32_10(seed; e, k, 0, 1)", "cell = (uint64(w.x) * 25) >> 32", "pass = (uint64(w.y) * 4) >> 32", "d = (uint64(w.z) * 3) >> 32",
                  "dest = d + (d >= pass)", "Global env 0 takes reset 1", "PPO_BUF_ENV_STATE is f32 [4, N]",
                  # the accepted forms, the masks, the fold, and why 8
                  "PPO_DIST_MASKED or PPO_DIST_CATEGORICAL", "head_dims[0] = 6", "obs_size = 19", "hidden = 64", "PPO_KERNEL_CAT_FUSED (required, never implied)",
                  "max_episode_steps >= 1", "PPO_BUF_MASKS (u8 [T, N, 6])", "cat_rollout_kernel", "cat_eval_kernel", "cat_trunc_fold_kernel",
                  "ppo_env_truncation_bootstrap and ppo_env_truncations", "value 7 stays unassigned", "PPO_ERR_INVALID and changes nothing"):
        assert words in block, words


def test_binding_and_package_mirror_it():
    P = load_package()
    assert P.ENV_TAXI == 8 == P.binding.ENV_TAXI
    assert (P.ENV_CARTPOLE, P.ENV_MOUNTAINCAR, P.ENV_SYNTHETIC, P.ENV_HOST, P.ENV_PENDULUM, P.ENV_MOUNTAINCAR_CONTINUOUS, P.ENV_ACROBOT) == (0, 1, 2, 3, 4, 5, 6)
    cfg = P.make_config(env_kind=P.ENV_TAXI, dist_kind=P.DIST_MASKED, obs_size=19, head_dims=(6,), kernel_flags=P.KERNEL_CAT_FUSED, max_episode_steps=200)
    assert (cfg.env_kind, cfg.dist_kind, cfg.obs_size, cfg.n_heads, cfg.head_dims[0], cfg.kernel_flags, cfg.max_episode_steps) == (8, 1, 19, 1, 6, 256, 200)


def test_abi_version_and_symbols_are_unchanged():
    P = load_package()
    lib = P.binding.lib()
    assert lib.ppo_abi_version() == 5 == P.binding.ABI_VERSION
    assert len(P.binding.ABI_SYMBOLS) == len(set(P.binding.ABI_SYMBOLS)) == 92
    for name in P.binding.ABI_SYMBOLS:
        assert "taxi" not in name.lower()


def test_transition_answers_bad_arguments_with_a_status():
    P = load_package()
    L = P.binding.lib()
    buf = (C.c_float * 8)()
    act = (C.c_int64 * 2)()
    term = (C.c_int32 * 2)()
    # null pointers, a negative count: PPO_ERR_INVALID (1); n = 0: nothing to do.  None of them launches anything.
    assert L.ppo_env_transition(8, None, act, 1, buf, buf, term, None) == 1
    assert L.ppo_env_transition(8, buf, None, 1, buf, buf, term, None) == 1
    assert L.ppo_env_transition(8, buf, act, -1, buf, buf, term, None) == 1
    assert L.ppo_env_transition(8, buf, act, 0, buf, buf, term, None) == 0
    assert L.ppo_env_transition_f32(8, buf, buf, 0, buf, None, buf, term, None) == 5


def test_facade_files_exist():
    host = os.path.join(ROOT, "ppo-libtorch_amd", "host")
    for rel in ("Environments/Taxi.h", "Environments/Taxi.cpp", "PPO/PPO_MultiDiscreteTaxi.h", "tests/host_taxi_test.cpp"):
        assert os.path.isfile(os.path.join(host, rel)), rel
    assert "host_taxi_test" in open(os.path.join(host, "Makefile")).read()
    hdr = open(os.path.join(host, "PPO", "PPO_MultiDiscreteTaxi.h")).read()
    assert "PPO_ENV_TAXI" in hdr and "PPO_DIST_MASKED" in hdr and "fused_categorical" in hdr
