"""hidden = 128 on the fused families (kernels_fused_matrix_h128.hip) without a GPU: what ppo_ctx_create answers in front of the first device call.  The
width is accepted on a PPO_ENV_HOST context with exactly one family flag and PPO_KERNEL_FUSED_MATRIX -- creation then gets as far as hipSetDevice (status 2
where no device exists, tests/refusal_grid.py) -- and nowhere else.  tests/test_gpu_fused_h128.py runs the kernels."""
import pytest

from __graft_entry__ import load_package

MATRIX, WIDE = 1 << 16, 1 << 15


@pytest.fixture(scope="module")
def P():
    return load_package()


def create_error(P, **kw):
    base = dict(env_kind=P.ENV_HOST, dist_kind=P.DIST_GAUSSIAN, obs_size=17, head_dims=(3,), hidden=128, num_envs=4, num_steps=4, num_minibatches=1,
                kernel_flags=P.KERNEL_GAUSS_FUSED | MATRIX)
    base.update(kw)
    with pytest.raises(P.binding.PPOError) as e:
        P.Context(P.make_config(**base))
    return str(e.value)


CAT = dict(dist_kind=1, head_dims=(5, 3, 4))


@pytest.mark.parametrize("kw", [dict(), dict(obs_size=376, kernel_flags=64 | MATRIX | WIDE), dict(kernel_flags=256 | MATRIX, **CAT),
                                dict(obs_size=100, kernel_flags=256 | MATRIX | WIDE, **CAT)], ids=["gauss", "gauss wide", "cat", "cat wide"])
def test_hidden_128_passes_every_check_in_front_of_the_device(P, kw):
    msg = create_error(P, **kw)
    assert "status 2" in msg and "hipSetDevice" in msg, msg


@pytest.mark.parametrize("hidden", [96, 256])
@pytest.mark.parametrize("family,kw", [("PPO_KERNEL_GAUSS_FUSED", dict()), ("PPO_KERNEL_CAT_FUSED", dict(kernel_flags=256 | MATRIX, **CAT))])
def test_other_widths_beside_the_flag_are_refused_with_the_reason(P, family, kw, hidden):
    msg = create_error(P, hidden=hidden, **kw)
    assert "status 5" in msg and all(w in msg for w in (family, "PPO_KERNEL_FUSED_MATRIX", "hidden = 64", "hidden = 128", "got hidden = %d" % hidden, "LDS")), msg


def test_without_the_flag_the_family_answers_as_before(P):
    assert "PPO_KERNEL_GAUSS_FUSED is built for hidden = 64; got hidden = 128" in create_error(P, kernel_flags=64)
    assert "PPO_KERNEL_CAT_FUSED is built for hidden = 64; got hidden = 128" in create_error(P, kernel_flags=256, **CAT)


def test_a_device_env_keeps_its_own_refusal(P):
    msg = create_error(P, env_kind=4, obs_size=3, head_dims=(1,), kernel_flags=64 | (1 << 17))   # Pendulum beside PPO_KERNEL_ENV_MATRIX
    assert "status 5" in msg and "PPO_ENV_PENDULUM is built for the 2 x 64 network" in msg and "got 2 x 128" in msg, msg
