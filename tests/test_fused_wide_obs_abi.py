"""PPO_KERNEL_FUSED_WIDE_OBS (include/ppo_hip.h) without a GPU: the macro's spelling, the binding's constant and ppo_ctx_create's refusals, which are decided
in front of the first device call.  tests/test_gpu_fused_wide_obs.py runs the kernels."""
import os
import re

import pytest

from __graft_entry__ import ROOT, load_package


@pytest.fixture(scope="module")
def P():
    return load_package()


def test_header_and_binding(P):
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert re.search(r"^#define PPO_KERNEL_FUSED_WIDE_OBS \(1 << 15\)$", src, re.M)
    assert re.search(r"#define PPO_ABI_VERSION 5\b", src)
    assert P.KERNEL_FUSED_WIDE_OBS == 1 << 15 == P.binding.KERNEL_FUSED_WIDE_OBS


def create_error(P, **kw):
    base = dict(env_kind=P.ENV_HOST, dist_kind=P.DIST_GAUSSIAN, obs_size=100, head_dims=(3,), num_envs=4, num_steps=4, num_minibatches=1,
                kernel_flags=P.KERNEL_GAUSS_FUSED | P.KERNEL_FUSED_WIDE_OBS)
    base.update(kw)
    with pytest.raises(P.binding.PPOError) as e:
        P.Context(P.make_config(**base))
    return str(e.value)


CAT = dict(dist_kind=0, head_dims=(2,))
REFUSED = {
    "a device env": dict(env_kind=4, obs_size=3, head_dims=(1,)),                                                      # PPO_ENV_PENDULUM
    "PPO_ENV_SYNTHETIC": dict(env_kind=2, kernel_flags=256 | 1 << 15, **CAT),
    "CartPole": dict(env_kind=0, obs_size=4, kernel_flags=256 | 1 << 15, **CAT),
    "MountainCar": dict(env_kind=1, obs_size=2, kernel_flags=256 | 1 << 15, **CAT),
    "no family flag": dict(kernel_flags=1 << 15),
    "beside PPO_KERNEL_ENV_GENERIC": dict(env_kind=0, obs_size=4, kernel_flags=512 | 1 << 15, **CAT),
    "obs_size 385, Gaussian": dict(obs_size=385),
    "obs_size 385, categorical": dict(obs_size=385, kernel_flags=256 | 1 << 15, **CAT),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refusals_name_the_flag_and_the_limit(P, case):
    msg = create_error(P, **REFUSED[case])
    assert "status 5" in msg and "PPO_KERNEL_FUSED_WIDE_OBS" in msg and "obs_size <= 384" in msg, msg
    if "385" in case:
        assert "obs_size = 385" in msg, msg


@pytest.mark.parametrize("bit", [2048, 4096, 16384])
def test_the_unassigned_bits_stay_unknown(P, bit):
    msg = create_error(P, kernel_flags=P.KERNEL_GAUSS_FUSED | P.KERNEL_FUSED_WIDE_OBS | bit)
    assert "status 1" in msg and "unknown bits in kernel_flags" in msg, msg


def test_without_the_flag_the_family_refuses_65_as_before(P):
    assert "PPO_KERNEL_GAUSS_FUSED is built for obs_size <= 64; got obs_size = 65" in create_error(P, obs_size=65, kernel_flags=P.KERNEL_GAUSS_FUSED)
    assert "PPO_KERNEL_CAT_FUSED is built for 1 <= obs_size <= 64; got obs_size = 65" in create_error(P, obs_size=65, kernel_flags=P.KERNEL_CAT_FUSED, **CAT)
