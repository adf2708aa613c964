"""PPO_DiscreteBlackjack of the C++ facade (a categorical policy on the device's Blackjack, PPO_ENV_BLACKJACK) on the GPU: host/tests/host_blackjack_test in a
fresh directory.  The host-side Blackjack class is checked alone first; then two iterations train, the rollout is none of the act launches, evaluate(8)
returns ppo_evaluate's numbers on the same context and prints nothing, the checkpoint loads into a fresh object with bit-equal parameters,
setBootstrapTruncated(true) throws the library's refusal, and the host-side class -- which computes on the CPU, its own Philox included -- steps every
(t, ace, show) x both actions x n in 4..11 x two keys to the numbers of ppo_env_transition."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ppo-libtorch_amd", "host", "host_blackjack_test")


def test_ppo_discrete_blackjack(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(EXE), EXE])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_blackjack_test ok" in r.stdout
    assert "host Blackjack alone: 19200 rows" in r.stdout
    assert "fused launches: act 0 " in r.stdout
    assert "evaluate: return mean" in r.stdout
    assert "bootstrap_truncated: " in r.stdout and "holds neither the card count nor the key" in r.stdout
    assert "host Blackjack against ppo_env_transition: 0 of 19200 rows differ" in r.stdout
