"""PPO_ENV_PENDULUM's surface without a GPU: the header declares the env kind (4) and the three _f32 calls, the built library exports them, the binding mirrors
them, the ABI version is still 5, and the stateless call answers bad arguments with a status instead of crashing."""
import ctypes as C
import os
import re
import subprocess

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
NEW = ("ppo_rollout_f32", "ppo_env_step_f32", "ppo_env_transition_f32")


def test_header_declares_the_env_and_the_calls():
    kinds = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"(PPO_ENV_[A-Z]+)\s*=\s*(\d+)", HEADER))
    assert kinds == {"PPO_ENV_CARTPOLE": 0, "PPO_ENV_MOUNTAINCAR": 1, "PPO_ENV_SYNTHETIC": 2, "PPO_ENV_HOST": 3, "PPO_ENV_PENDULUM": 4}
    assert re.search(r"#define\s+PPO_ABI_VERSION\s+5\b", HEADER)
    assert re.search(r"^PPO_API\s+ppo_status\s+ppo_rollout_f32\(ppo_ctx\*\s*\w+,\s*const float\*\s*forced_actions", HEADER, flags=re.M)
    assert re.search(r"^PPO_API\s+ppo_status\s+ppo_env_step_f32\(ppo_ctx\*\s*\w+,\s*const float\*\s*action[^)]*float\*\s*obs,\s*float\*\s*reward,\s*int32_t\*\s*done\);", HEADER, flags=re.M)
    assert re.search(r"^PPO_API\s+ppo_status\s+ppo_env_transition_f32\(int32_t\s+env_kind,\s*const float\*\s*state_in,\s*const float\*\s*action,\s*int64_t\s+n,\s*"
                     r"float\*\s*next_state,\s*float\*\s*obs_out,\s*float\*\s*reward,\s*int32_t\*\s*terminated,\s*void\*\s*stream\);", HEADER, flags=re.M)


def test_library_exports_the_calls():
    P = load_package()
    lib = P.binding.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", P.binding.LIB_PATH]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    for name in NEW:
        assert name in exported and hasattr(lib, name), name
    assert lib.ppo_abi_version() == 5 == P.binding.ABI_VERSION


def test_binding_mirrors_them():
    P = load_package()
    assert P.ENV_PENDULUM == 4 == P.binding.ENV_PENDULUM
    for name in NEW:
        assert P.binding.ABI_SYMBOLS.count(name) == 1
    assert hasattr(P.Context, "env_step_f32") and callable(P.env_transition_f32) and callable(P.binding.env_transition_f32)
    cfg = P.make_config(env_kind=P.ENV_PENDULUM, dist_kind=P.DIST_GAUSSIAN, obs_size=3, head_dims=(1,), kernel_flags=P.KERNEL_GAUSS_FUSED, max_episode_steps=200)
    assert (cfg.env_kind, cfg.dist_kind, cfg.obs_size, cfg.n_heads, cfg.head_dims[0], cfg.kernel_flags) == (4, 2, 3, 1, 1, 64)
    import inspect
    assert "forced_actions" in inspect.signature(P.Context.rollout).parameters


def test_bad_arguments_are_statuses():
    P = load_package()
    L = P.binding.lib()
    buf = (C.c_float * 8)()
    term = (C.c_int32 * 2)()
    # null pointers, a negative count: PPO_ERR_INVALID (1); an env with integer actions: PPO_ERR_UNSUPPORTED (5).  None of them launches anything.
    assert L.ppo_env_transition_f32(4, None, buf, 1, buf, None, buf, term, None) == 1
    assert L.ppo_env_transition_f32(4, buf, buf, -1, buf, None, buf, term, None) == 1
    assert L.ppo_env_transition_f32(0, buf, buf, 0, buf, None, buf, term, None) == 5
    assert L.ppo_env_transition_f32(4, buf, buf, 0, buf, None, buf, term, None) == 0   # n = 0: nothing to do
    assert L.ppo_rollout_f32(None, None) != 0 and L.ppo_env_step_f32(None, buf, buf, buf, term) != 0
