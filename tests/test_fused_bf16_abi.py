"""compute_dtype = PPO_DTYPE_BF16 beside PPO_KERNEL_FUSED_MATRIX (kernels_fused_matrix_bf16.hip) without a GPU: what ppo_ctx_create answers in front of the first
device call, and the facade's TOML key (host/tests/host_fused_bf16_test, parse mode).  The dtype is accepted on a PPO_ENV_HOST context with exactly one family
flag and the matrix flag at hidden 64 or 128 -- creation then gets as far as hipSetDevice (status 2 where no device exists) -- and every other bf16 request
is answered as before.  tests/test_gpu_fused_bf16.py runs the kernels."""
import os
import subprocess

import pytest

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX, WIDE, ENV_MATRIX = 1 << 16, 1 << 15, 1 << 17
CAT = dict(dist_kind=1, head_dims=(5, 3, 4))


@pytest.fixture(scope="module")
def P():
    return load_package()


def create_error(P, **kw):
    base = dict(env_kind=P.ENV_HOST, dist_kind=P.DIST_GAUSSIAN, obs_size=17, head_dims=(3,), hidden=128, num_envs=4, num_steps=4, num_minibatches=1,
                compute_dtype=P.DTYPE_BF16, kernel_flags=P.KERNEL_GAUSS_FUSED | MATRIX)
    base.update(kw)
    with pytest.raises(P.binding.PPOError) as e:
        P.Context(P.make_config(**base))
    return str(e.value)


@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("kw", [dict(), dict(obs_size=376, kernel_flags=64 | MATRIX | WIDE), dict(kernel_flags=256 | MATRIX, **CAT),
                                dict(obs_size=100, kernel_flags=256 | MATRIX | WIDE, **CAT)], ids=["gauss", "gauss wide", "cat", "cat wide"])
def test_bf16_beside_the_flag_passes_every_check_in_front_of_the_device(P, kw, hidden):
    msg = create_error(P, hidden=hidden, **kw)
    assert "status 2" in msg and "hipSetDevice" in msg, msg


def test_without_the_matrix_flag_bf16_is_answered_as_before(P):
    assert "dist_kind = PPO_DIST_GAUSSIAN is built for compute_dtype = PPO_DTYPE_F32; bf16 storage is not" in create_error(P, hidden=64, kernel_flags=64)
    assert "PPO_KERNEL_CAT_FUSED is built for compute_dtype = PPO_DTYPE_F32; bf16 storage is not" in create_error(P, hidden=64, kernel_flags=256, **CAT)
    # the matrix flag beside the other family's flag opens nothing either
    assert "dist_kind = PPO_DIST_GAUSSIAN is built for compute_dtype = PPO_DTYPE_F32; bf16 storage is not" in create_error(P, hidden=64, kernel_flags=256 | MATRIX)


def test_a_device_env_keeps_its_own_refusal(P):
    msg = create_error(P, env_kind=4, obs_size=3, head_dims=(1,), hidden=64, kernel_flags=64 | ENV_MATRIX)   # Pendulum beside PPO_KERNEL_ENV_MATRIX
    assert "status 5" in msg and "env_kind = PPO_ENV_PENDULUM is built for compute_dtype = PPO_DTYPE_F32; bf16 storage is not" in msg, msg


@pytest.mark.parametrize("hidden", [96, 256])
@pytest.mark.parametrize("family,kw", [("PPO_KERNEL_GAUSS_FUSED", dict()), ("PPO_KERNEL_CAT_FUSED", dict(kernel_flags=256 | MATRIX, **CAT))])
def test_other_widths_are_refused_with_the_reason(P, family, kw, hidden):
    msg = create_error(P, hidden=hidden, **kw)
    assert "status 5" in msg and all(w in msg for w in (family, "PPO_KERNEL_FUSED_MATRIX", "hidden = 64", "hidden = 128", "got hidden = %d" % hidden, "LDS",
                                                        "PPO_DTYPE_BF16")), msg


def test_the_facade_parses_bf16(tmp_path):
    """host/tests/host_fused_bf16_test in its parse mode: PPO_Discrete reads the key from PPOConfig.toml and prints it; construction then throws"""
    host = os.path.join(ROOT, "ppo-libtorch_amd", "host")
    if not os.path.exists(os.path.join(host, "host_fused_bf16_test")):
        subprocess.check_call(["make", "-s", "-j", "4", "-C", host])
    r = subprocess.run([os.path.join(host, "host_fused_bf16_test"), "parse"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "parsed: bf16 = true" in r.stdout and "refusal:" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
