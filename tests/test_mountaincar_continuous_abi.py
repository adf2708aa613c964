"""PPO_ENV_MOUNTAINCAR_CONTINUOUS's surface without a GPU: the header declares the env kind (5), the binding and the package mirror it, make_config builds the
one form the env accepts, the ABI version is still 5 and no symbol was added, and ppo_env_transition_f32 answers bad arguments for this env with a status
instead of crashing (before the env existed it answered 5, PPO_ERR_UNSUPPORTED, to every one of them)."""
import ctypes as C
import os
import re

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()


def test_header_declares_the_env():
    m = re.findall(r"\bPPO_ENV_MOUNTAINCAR_CONTINUOUS\s*=\s*(\d+)", HEADER)
    assert m == ["5"], m
    assert re.search(r"enum\s*\{[^}]*PPO_ENV_PENDULUM\s*=\s*4\s*,\s*PPO_ENV_MOUNTAINCAR_CONTINUOUS\s*=\s*5\s*\}", HEADER)
    assert re.search(r"#define\s+PPO_ABI_VERSION\s+5\b", HEADER)
    # the env block states the step; the two calls it adds to a Gaussian device env are named there
    block = HEADER[HEADER.index("/* PPO_ENV_MOUNTAINCAR_CONTINUOUS (new"):HEADER.index("enum { PPO_ENV_CARTPOLE")]
    for words in ("u * 0.0015f - 0.0025f * cosf(3.0f * p)", "p' >= 0.45f && v' >= 0.0f", "0.1f * (a * a)", "ppo_env_truncation_bootstrap", "ppo_evaluate", "obs_size = 2"):
        assert words in block, words


def test_binding_and_package_mirror_it():
    P = load_package()
    assert P.ENV_MOUNTAINCAR_CONTINUOUS == 5 == P.binding.ENV_MOUNTAINCAR_CONTINUOUS
    assert (P.ENV_CARTPOLE, P.ENV_MOUNTAINCAR, P.ENV_SYNTHETIC, P.ENV_HOST, P.ENV_PENDULUM) == (0, 1, 2, 3, 4)
    cfg = P.make_config(env_kind=P.ENV_MOUNTAINCAR_CONTINUOUS, dist_kind=P.DIST_GAUSSIAN, obs_size=2, head_dims=(1,), kernel_flags=P.KERNEL_GAUSS_FUSED,
                        max_episode_steps=999)
    assert (cfg.env_kind, cfg.dist_kind, cfg.obs_size, cfg.n_heads, cfg.head_dims[0], cfg.kernel_flags, cfg.max_episode_steps) == (5, 2, 2, 1, 1, 64, 999)


def test_abi_version_and_symbols_are_unchanged():
    P = load_package()
    lib = P.binding.lib()
    assert lib.ppo_abi_version() == 5 == P.binding.ABI_VERSION
    assert len(P.binding.ABI_SYMBOLS) == len(set(P.binding.ABI_SYMBOLS)) == 92   # the count in front of this env: it rides on existing calls


def test_bad_arguments_are_statuses():
    P = load_package()
    L = P.binding.lib()
    buf = (C.c_float * 8)()
    term = (C.c_int32 * 2)()
    # null pointers, a negative count: PPO_ERR_INVALID (1); n = 0: nothing to do.  None of them launches anything.
    assert L.ppo_env_transition_f32(5, None, buf, 1, buf, None, buf, term, None) == 1
    assert L.ppo_env_transition_f32(5, buf, None, 1, buf, None, buf, term, None) == 1
    assert L.ppo_env_transition_f32(5, buf, buf, 1, None, None, buf, term, None) == 1
    assert L.ppo_env_transition_f32(5, buf, buf, 1, buf, None, None, term, None) == 1
    assert L.ppo_env_transition_f32(5, buf, buf, 1, buf, None, buf, None, None) == 1
    assert L.ppo_env_transition_f32(5, buf, buf, -1, buf, None, buf, term, None) == 1
    assert L.ppo_env_transition_f32(5, buf, buf, 0, buf, None, buf, term, None) == 0
    assert L.ppo_env_transition_f32(5, buf, buf, 0, buf, buf, buf, term, None) == 0
    # an env kind nobody defined, and the envs with integer actions, are still PPO_ERR_UNSUPPORTED
    assert L.ppo_env_transition_f32(6, buf, buf, 0, buf, None, buf, term, None) == 5
    assert L.ppo_env_transition_f32(1, buf, buf, 0, buf, None, buf, term, None) == 5
