"""The yardstick of tests/test_gpu_acrobot.py, checked on the CPU: the numpy model of the header's Acrobot step (tests/acrobot_model.py) in float32 against
the same model in float64 on set A (4096 rows: angles uniform in [-pi, pi], |w1| <= 2 pi, |w2| <= 4 pi, actions uniform).

The GPU test's bar per output is 8 x e_out, e_out the float32 model's worst deviation from float64 here.  This file holds three things about that bar:
it is a rounding-error bar (0 < e_out < 1e-4), wrong constants cannot pass it (a 1 % change of g moves more than half the rows beyond it in every state
output), and the rows left out of the exact reward / terminated comparison -- decided from the float64 values only -- are at most 1 % of the set."""
import numpy as np
import pytest

import acrobot_model as M


@pytest.fixture(scope="module")
def Y():
    return M.yardstick()


def test_float32_error_is_a_rounding_error(Y):
    print("e_out", Y["e_out"])
    assert Y["e_out"].shape == (4,)
    assert (Y["e_out"] > 0).all() and (Y["e_out"] < 1e-4).all(), Y["e_out"]


def test_a_wrong_constant_cannot_pass_the_bar(Y):
    wrong, _, _ = M.step(Y["st"], Y["act"], np.float64, g=9.8 * 1.01)
    moved = M.state_error(wrong, Y["ref"])
    print("median movement", np.median(moved, axis=0), "bar", 8 * Y["e_out"])
    beyond = (moved > 8 * Y["e_out"]).mean(axis=0)
    assert (beyond > 0.5).all(), beyond


def test_excluded_rows_are_few(Y):
    print("left out: by the wrap", Y["frac_wrap"], "per angle", Y["frac_wrap_each"], "by the margin", Y["frac_margin"])
    assert 1.0 - Y["keep"].mean() <= 0.01
    # the rest of the set terminates somewhere and not everywhere: the exact comparison has both cases
    t = Y["term"][Y["keep"]]
    assert 0 < t.sum() < t.size


def test_the_box_is_closed_under_the_step():
    """Set B (the 16 corners of the state box times the 3 actions, and 256 random rows at the full velocity range) stays finite and inside the box in the
    float32 model, which needs the header's large-argument rule: the stage angles pass 120 there."""
    st, act = M.set_b()
    ns, rew, term = M.step(st, act, np.float32)
    f = np.float32
    assert np.isfinite(ns).all()
    assert (np.abs(ns[:, :2]) <= f(np.pi)).all() and (np.abs(ns[:, 2]) <= f(M.MAX_W1)).all() and (np.abs(ns[:, 3]) <= f(M.MAX_W2)).all()
    assert set(np.unique(rew)) <= {f(0.0), f(-1.0)}


def test_near_upright_states_terminate_at_once():
    """What test_gpu_acrobot.py injects to get terminations at step 1 of a rollout."""
    st = np.tile(np.asarray([[3.0, 0.0, 0.0, 0.0]], np.float32), (3, 1))
    for dt in (np.float32, np.float64):
        _, rew, term = M.step(st, np.arange(3), dt)
        assert term.tolist() == [1, 1, 1] and rew.tolist() == [0.0, 0.0, 0.0]
