"""PPO_ENV_ACROBOT's surface without a GPU: the header declares the env kind (6) and states the step's formulas and the one accepted form, the binding and
the package mirror it, the state is 4 wide behind 6 observations, the facade headers exist, and the ABI version and the exported set are what they were (the
env rides on existing calls: two older tests hold the symbol count at 92, so the observation of a state comes from ppo_env_set_state_h, not a new symbol)."""
import ctypes as C
import os
import re
import subprocess

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()


def test_header_declares_the_env_and_states_the_step(tmp_path):
    # an enum of its own, written as the successor of the last env kind: older tests pin the first list's text (it ends at 5, and no other PPO_ENV_x = digit)
    assert re.search(r"enum\s*\{\s*PPO_ENV_ACROBOT\s*=\s*PPO_ENV_MOUNTAINCAR_CONTINUOUS\s*\+\s*1\s*\}", HEADER)
    exe = str(tmp_path / "acrobot_enum_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], check=True,
                   input=b'#include <stdio.h>\n#include "ppo_hip.h"\nint main(void) { printf("%d %d\\n", (int)PPO_ENV_ACROBOT, (int)PPO_ENV_MOUNTAINCAR_CONTINUOUS); return 0; }\n')
    assert subprocess.check_output([exe]).split() == [b"6", b"5"]
    assert re.search(r"#define\s+PPO_ABI_VERSION\s+5\b", HEADER)
    block = HEADER[HEADER.index("/* PPO_ENV_ACROBOT (new"):HEADER.index("enum { PPO_ENV_CARTPOLE")]
    for words in ("d1   = (0.25f + (1.25f + c2)) + 2.0f", "d2   = (0.25f + 0.5f * c2) + 1.0f", "phi2 = 4.9f * cosr((th1 + th2) - HALF_PI_F)",
                  "phi1 = (((-0.5f * (w2 * w2)) * s2 - (w2 * w1) * s2) + 14.7f * cosr(th1 - HALF_PI_F)) + phi2",
                  "dw2  = (((tau + (d2 / d1) * phi1) - (0.5f * (w1 * w1)) * s2) - phi2) / (1.25f - (d2 * d2) / d1)", "dw1  = -(d2 * dw2 + phi1) / d1",
                  "s'   = s + DT6 * (((k1 + 2.0f * k2) + 2.0f * k3) + k4)", "(-cosr(th1')) - cosr(th2' + th1') > 1.0f", "rint((double)x / TWO_PI_D)",
                  "|x| < 64.0f", "uniform(w.x | w.y | w.z | w.w, -0.1f, 0.1f)",
                  # the accepted form and what is refused
                  "PPO_DIST_CATEGORICAL", "head_dims[0] = 3", "obs_size = 6", "hidden = 64", "PPO_KERNEL_CAT_FUSED (required, never implied)",
                  "max_episode_steps >= 1", "cat_rollout_kernel", "cat_eval_kernel", "ppo_env_truncation_bootstrap", "does not hold the angles",
                  "PPO_BUF_ENV_STATE is [4, N]"):
        assert words in block, words


def test_binding_and_package_mirror_it():
    P = load_package()
    assert P.ENV_ACROBOT == 6 == P.binding.ENV_ACROBOT
    assert (P.ENV_CARTPOLE, P.ENV_MOUNTAINCAR, P.ENV_SYNTHETIC, P.ENV_HOST, P.ENV_PENDULUM, P.ENV_MOUNTAINCAR_CONTINUOUS) == (0, 1, 2, 3, 4, 5)
    cfg = P.make_config(env_kind=P.ENV_ACROBOT, dist_kind=P.DIST_CATEGORICAL, obs_size=6, head_dims=(3,), kernel_flags=P.KERNEL_CAT_FUSED, max_episode_steps=500)
    assert (cfg.env_kind, cfg.dist_kind, cfg.obs_size, cfg.n_heads, cfg.head_dims[0], cfg.kernel_flags, cfg.max_episode_steps) == (6, 0, 6, 1, 3, 256, 500)


def test_abi_version_and_symbols_are_unchanged():
    P = load_package()
    lib = P.binding.lib()
    assert lib.ppo_abi_version() == 5 == P.binding.ABI_VERSION
    assert len(P.binding.ABI_SYMBOLS) == len(set(P.binding.ABI_SYMBOLS)) == 92
    assert "ppo_env_observation" not in P.binding.ABI_SYMBOLS and "ppo_env_observation" not in re.findall(r"\bppo_\w+\s*\(", HEADER)


def test_transition_answers_bad_arguments_with_a_status():
    P = load_package()
    L = P.binding.lib()
    buf = (C.c_float * 8)()
    act = (C.c_int64 * 2)()
    term = (C.c_int32 * 2)()
    # null pointers, a negative count: PPO_ERR_INVALID (1); n = 0: nothing to do.  None of them launches anything.
    assert L.ppo_env_transition(6, None, act, 1, buf, buf, term, None) == 1
    assert L.ppo_env_transition(6, buf, None, 1, buf, buf, term, None) == 1
    assert L.ppo_env_transition(6, buf, act, -1, buf, buf, term, None) == 1
    assert L.ppo_env_transition(6, buf, act, 0, buf, buf, term, None) == 0
    # the env takes integer actions: its _f32 twin still answers PPO_ERR_UNSUPPORTED
    assert L.ppo_env_transition_f32(6, buf, buf, 0, buf, None, buf, term, None) == 5


def test_facade_files_exist():
    host = os.path.join(ROOT, "ppo-libtorch_amd", "host")
    for rel in ("Environments/Acrobot.h", "Environments/Acrobot.cpp", "PPO/PPO_DiscreteAcrobot.h", "tests/host_acrobot_test.cpp"):
        assert os.path.isfile(os.path.join(host, rel)), rel
    assert "host_acrobot_test" in open(os.path.join(host, "Makefile")).read()
    hdr = open(os.path.join(host, "PPO", "PPO_DiscreteAcrobot.h")).read()
    assert "PPO_ENV_ACROBOT" in hdr and "PPO_KERNEL_CAT_FUSED" in hdr
