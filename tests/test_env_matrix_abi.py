"""PPO_KERNEL_ENV_MATRIX (include/ppo_hip.h) without a GPU: the macro's spelling, the binding's constant and ppo_ctx_create's answers, which are decided in
front of the first device call.  tests/test_gpu_env_matrix.py runs the kernels."""
import os
import re

import pytest

from __graft_entry__ import ROOT, load_package
from test_cut_state_abi import create

FLAG = 1 << 17
G, C = 64, 256   # PPO_KERNEL_GAUSS_FUSED, PPO_KERNEL_CAT_FUSED
# the seven envs in the form each accepts: env_kind -> (dist_kind, obs_size, actions, family flag)
FORMS = {4: (2, 3, 1, G), 5: (2, 2, 1, G), 6: (0, 6, 3, C), 8: (1, 19, 6, C), 10: (0, 16, 4, C), 11: (0, 64, 4, C), 13: (0, 45, 2, C)}


@pytest.fixture(scope="module")
def P():
    return load_package()


def env_kw(kind, flags):
    dist, obs, actions, family = FORMS[kind]
    return dict(env_kind=kind, dist_kind=dist, obs_size=obs, head_dims=(actions,), max_episode_steps=3, kernel_flags=family | FLAG | flags)


def test_header_and_binding(P):
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert re.search(r"^#define PPO_KERNEL_ENV_MATRIX \(1 << 17\)$", src, re.M)
    assert P.KERNEL_ENV_MATRIX == FLAG == P.binding.KERNEL_ENV_MATRIX and P.binding.ABI_VERSION == 5


REFUSED = {
    "PPO_ENV_HOST": (dict(env_kind=3, dist_kind=2, obs_size=17, head_dims=(3,), kernel_flags=G | FLAG), "PPO_KERNEL_FUSED_MATRIX"),
    "CartPole": (dict(env_kind=0, obs_size=4, kernel_flags=C | FLAG), "device envs of the fused 2 x 64 families only"),
    "MountainCar": (dict(env_kind=1, obs_size=2, head_dims=(3,), kernel_flags=C | FLAG), "device envs of the fused 2 x 64 families only"),
    "PPO_ENV_SYNTHETIC": (dict(env_kind=2, obs_size=16, kernel_flags=C | FLAG), "device envs of the fused 2 x 64 families only"),
    "no family flag, Pendulum": (dict(env_kw(4, 0), kernel_flags=FLAG), "needs PPO_KERNEL_GAUSS_FUSED"),
    "no family flag, Blackjack": (dict(env_kw(13, 0), kernel_flags=FLAG), "needs PPO_KERNEL_CAT_FUSED"),
    "beside PPO_KERNEL_ENV_GENERIC": (env_kw(6, 512), "excludes PPO_KERNEL_ENV_GENERIC"),
    "beside PPO_KERNEL_FUSED_MATRIX": (env_kw(8, 1 << 16), "PPO_KERNEL_FUSED_MATRIX"),
    "beside PPO_KERNEL_FUSED_WIDE_OBS": (env_kw(11, 1 << 15), "PPO_KERNEL_FUSED_WIDE_OBS"),
    "beside PPO_KERNEL_ENV_CUT_STATE": (env_kw(5, 1024), "excludes PPO_KERNEL_ENV_CUT_STATE"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refusals_name_the_flag_and_the_limit(P, case):
    kw, limit = REFUSED[case]
    st, msg = create(P, **kw)
    assert st == 5 and "PPO_KERNEL_ENV_MATRIX" in msg and limit in msg, (st, msg)


def test_bit_18_beside_the_flag_stays_unknown(P):
    st, msg = create(P, **env_kw(4, 1 << 18))
    assert st == 1 and "unknown bits in kernel_flags" in msg, (st, msg)


@pytest.mark.parametrize("kind", list(FORMS))
def test_each_env_accepts_the_flag(P, kind):
    """accepted: a live context on a machine with a GPU, or the end at hipSetDevice (status 2) without one; PPO_KERNEL_ENV_REWARD_NORM may stand beside it"""
    for beside in (0, P.KERNEL_ENV_REWARD_NORM):
        st, msg = create(P, **env_kw(kind, beside))
        assert st in (0, 2), (kind, beside, st, msg)
