"""PPO_KERNEL_ENV_GENERIC's surface without a GPU: the header defines the flag on bit 9 beside the other PPO_KERNEL_* values and describes it -- the two envs,
the refusals, the one-launch kernel --, the binding mirrors it, the facade reads its key, and the ABI version, the exported set and sizeof(ppo_config) are
what they were (the feature rides on one bit of kernel_flags: no symbol, no enumerator of an existing enum, no config field)."""
import ctypes as C
import os
import re
import subprocess

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()


def flat(text):
    return " ".join(text.replace(" *", " ").split())


def test_header_defines_the_flag_on_a_bit_of_its_own(tmp_path):
    m = re.search(r"^#define\s+PPO_KERNEL_ENV_GENERIC\s+(\d+)\b", HEADER, re.M)
    assert m and int(m.group(1)) == 512 == 1 << 9
    others = [int(v) for _, v in re.findall(r"(PPO_KERNEL_[A-Z_0-9]+)\s*=\s*(\d+)", HEADER)]
    others += [int(v) for v in re.findall(r"^#define\s+PPO_KERNEL_(?!ENV_GENERIC)[A-Z_0-9]+\s+(\d+)\b", HEADER, re.M)]
    assert sorted(others) == [1, 2, 4, 8, 16, 32, 64, 128, 256]
    exe = str(tmp_path / "flag_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], check=True,
                   input=b'#include <stdio.h>\n#include "ppo_hip.h"\nint main(void) { printf("%d %d %d\\n", (int)PPO_KERNEL_ENV_GENERIC, (int)PPO_ABI_VERSION, (int)sizeof(ppo_config)); return 0; }\n')
    flag, abi, size = (int(x) for x in subprocess.check_output([exe]).split())
    P = load_package()
    assert (flag, abi) == (512, 5) and size == C.sizeof(P.binding.Config)


def test_header_paragraph_names_envs_refusals_and_the_kernel():
    start = HEADER.index(" *   PPO_KERNEL_ENV_GENERIC ")
    para = flat(HEADER[start:HEADER.index("enum { PPO_KERNEL_ROLLOUT_VECTOR")])
    for words in ("PPO_ENV_CARTPOLE", "PPO_ENV_MOUNTAINCAR", "hidden 1 .. 2048", "n_hidden 1 .. 7", "PPO_DTYPE_BF16", "ppo_param_shapes",
                  # the env stays the unflagged context's
                  "PPO_BUF_ENV_STATE", "RESET_COUNT", "shared reset table", "ppo_env_set_state_h", "FIN_LEN / FIN_REW",
                  # the rollouts
                  "ppo_policy_act(step_index = rollout_steps + t) + ppo_env_step", "generic_env_rollout_kernel", "all T steps in ONE launch", "32 envs per workgroup",
                  "lanes 0 .. 31 of wave 0", "two critic launches",
                  # the refusals
                  "PPO_ERR_UNSUPPORTED", "any other env_kind", "PPO_KERNEL_GAUSS_FUSED or PPO_KERNEL_CAT_FUSED beside it", "PPO_DIST_GAUSSIAN",
                  "another engine never serves in the flag's place", "ppo_host_* / ppo_dev_* (PPO_ERR_STATE", "ppo_obs_norm_* / ppo_reward_norm_*", "ppo_evaluate",
                  "ppo_policy_act_greedy + ppo_env_transition", "ppo_env_truncation_bootstrap and ppo_env_truncations", "reference-shape critic",
                  "neither claimed nor tested"):
        assert words in para, words


def test_binding_mirrors_it():
    P = load_package()
    assert P.KERNEL_ENV_GENERIC == 512 == P.binding.KERNEL_ENV_GENERIC
    cfg = P.make_config(env_kind=P.ENV_MOUNTAINCAR, dist_kind=P.DIST_MASKED, obs_size=2, head_dims=(3,), hidden=256, n_hidden=4, compute_dtype=P.DTYPE_BF16,
                        kernel_flags=P.KERNEL_ENV_GENERIC)
    assert (cfg.env_kind, cfg.hidden, cfg.n_hidden, cfg.compute_dtype, cfg.kernel_flags) == (1, 256, 4, 1, 512)


def test_abi_version_and_symbols_are_unchanged():
    P = load_package()
    lib = P.binding.lib()
    assert lib.ppo_abi_version() == 5 == P.binding.ABI_VERSION
    assert len(P.binding.ABI_SYMBOLS) == len(set(P.binding.ABI_SYMBOLS)) == 92
    for name in P.binding.ABI_SYMBOLS:
        assert hasattr(lib, name), name


def test_facade_reads_the_key():
    host = os.path.join(ROOT, "ppo-libtorch_amd", "host")
    assert os.path.isfile(os.path.join(host, "tests", "host_env_generic_test.cpp"))
    assert "host_env_generic_test" in open(os.path.join(host, "Makefile")).read()
    algo = open(os.path.join(host, "PPO", "PPOAlgorithm.cpp")).read()
    assert '"network", "hidden_size"' in algo and "PPO_KERNEL_ENV_GENERIC" in algo
    for name in ("PPO_Discrete.h", "PPO_MultiDiscrete.h"):
        hdr = open(os.path.join(host, "PPO", name)).read()
        assert "hidden_size" in hdr and "PPO_KERNEL_ENV_GENERIC" in hdr and "Depth other than 2 and bf16 storage stay with the C-ABI" in hdr


def test_cost_tool_exists():
    tool = open(os.path.join(ROOT, "tools", "env_generic_cost.py")).read()
    assert "KERNEL_ENV_GENERIC" in tool and "ppo_policy_act" in tool and "ppo_env_step" in tool
