"""PPO_KERNEL_FUSED_MATRIX (include/ppo_hip.h) without a GPU: the macro's spelling, the binding's constant, ppo_ctx_create's refusals, which are decided in
front of the first device call, and the facade's TOML key (host/tests/host_matrix_cores_test, parse mode).  tests/test_gpu_fused_matrix.py runs the kernels."""
import os
import re
import subprocess

import pytest

from __graft_entry__ import ROOT, load_package

FLAG = 1 << 16


@pytest.fixture(scope="module")
def P():
    return load_package()


def test_header_and_binding(P):
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert re.search(r"^#define PPO_KERNEL_FUSED_MATRIX \(1 << 16\)$", src, re.M)
    assert P.KERNEL_FUSED_MATRIX == FLAG == P.binding.KERNEL_FUSED_MATRIX


def create_error(P, **kw):
    base = dict(env_kind=P.ENV_HOST, dist_kind=P.DIST_GAUSSIAN, obs_size=17, head_dims=(3,), num_envs=4, num_steps=4, num_minibatches=1,
                kernel_flags=P.KERNEL_GAUSS_FUSED | FLAG)
    base.update(kw)
    with pytest.raises(P.binding.PPOError) as e:
        P.Context(P.make_config(**base))
    return str(e.value)


CAT = dict(dist_kind=0, head_dims=(2,))
HOST_ONLY, ONE_FAMILY = "env_kind = PPO_ENV_HOST", "PPO_KERNEL_GAUSS_FUSED"   # the limit a refusal names: the env kind, or the family flag(s) it wants beside it
REFUSED = {
    "Pendulum": (dict(env_kind=4, obs_size=3, head_dims=(1,)), HOST_ONLY),
    "MountainCarContinuous": (dict(env_kind=5, obs_size=2, head_dims=(1,)), HOST_ONLY),
    "Acrobot": (dict(env_kind=6, obs_size=6, kernel_flags=256 | FLAG, dist_kind=0, head_dims=(3,)), HOST_ONLY),
    "Taxi": (dict(env_kind=8, obs_size=19, kernel_flags=256 | FLAG, dist_kind=1, head_dims=(6,)), HOST_ONLY),
    "FrozenLake": (dict(env_kind=10, obs_size=16, kernel_flags=256 | FLAG, dist_kind=0, head_dims=(4,)), HOST_ONLY),
    "FrozenLake8x8": (dict(env_kind=11, obs_size=64, kernel_flags=256 | FLAG, dist_kind=0, head_dims=(4,)), HOST_ONLY),
    "Blackjack": (dict(env_kind=13, obs_size=45, kernel_flags=256 | FLAG, **CAT), HOST_ONLY),
    "PPO_ENV_SYNTHETIC": (dict(env_kind=2, kernel_flags=256 | FLAG, **CAT), HOST_ONLY),
    "CartPole": (dict(env_kind=0, obs_size=4, kernel_flags=256 | FLAG, **CAT), HOST_ONLY),
    "MountainCar": (dict(env_kind=1, obs_size=2, kernel_flags=256 | FLAG, **CAT), HOST_ONLY),
    "no family flag": (dict(kernel_flags=FLAG), ONE_FAMILY),
    "both family flags": (dict(kernel_flags=64 | 256 | FLAG), "exactly one"),
    "beside PPO_KERNEL_ENV_GENERIC": (dict(env_kind=0, obs_size=4, kernel_flags=512 | FLAG, **CAT), "PPO_KERNEL_ENV_GENERIC"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refusals_name_the_flag_and_the_limit(P, case):
    kw, limit = REFUSED[case]
    msg = create_error(P, **kw)
    assert "status 5" in msg and "PPO_KERNEL_FUSED_MATRIX" in msg and limit in msg, msg


def test_an_unassigned_bit_beside_the_flag_stays_unknown(P):
    msg = create_error(P, kernel_flags=P.KERNEL_GAUSS_FUSED | FLAG | 2048)
    assert "status 1" in msg and "unknown bits in kernel_flags" in msg, msg


def test_the_facade_parses_matrix_cores(tmp_path):
    """host/tests/host_matrix_cores_test in its parse mode: PPO_Discrete reads the key from PPOConfig.toml and prints it; construction then throws"""
    host = os.path.join(ROOT, "ppo-libtorch_amd", "host")
    if not os.path.exists(os.path.join(host, "host_matrix_cores_test")):
        subprocess.check_call(["make", "-s", "-j", "4", "-C", host])
    r = subprocess.run([os.path.join(host, "host_matrix_cores_test"), "parse"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "parsed: matrix_cores = true" in r.stdout and "refusal:" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
