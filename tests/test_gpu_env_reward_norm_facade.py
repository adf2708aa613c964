"""`norm_reward = true` in [environment] of the C++ facade on a fused device-env class (PPO_KERNEL_ENV_REWARD_NORM; include/ppo_hip.h) on the GPU:
host/tests/host_env_reward_norm_test in a fresh directory.  PPO_Continuous (Pendulum) trains two iterations with the key, its context carries the flag, the
".rewnorm" file beside the checkpoint holds what ppo_reward_norm_get_h returns and loads into a fresh object; the same file without the key creates the context
without the flag, is refused the three calls as before and writes no statistics file.  Without a GPU: the six fused device-env classes ask for the flag, and the
classes that never did do not."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppo-libtorch_amd", "host")
EXE = os.path.join(HOST, "host_env_reward_norm_test")
DEVICE_ENV_CLASSES = ("PPO_Continuous", "PPO_ContinuousMountainCar", "PPO_DiscreteAcrobot", "PPO_MultiDiscreteTaxi", "PPO_DiscreteFrozenLake", "PPO_DiscreteBlackjack")


def test_the_six_device_env_classes_ask_for_the_flag_and_no_other_class_does():
    for name in DEVICE_ENV_CLASSES:
        src = open(os.path.join(HOST, "PPO", name + ".h")).read()
        assert src.index("getArgs();") < src.index("normRewardOnDeviceEnv();") < src.index("construct();"), name
    for name in ("PPO_Discrete", "PPO_MultiDiscrete", "PPO_HostEnv", "PPO_HostEnvBox"):
        assert "normRewardOnDeviceEnv" not in open(os.path.join(HOST, "PPO", name + ".h")).read(), name
    algo = open(os.path.join(HOST, "PPO", "PPOAlgorithm.cpp")).read()
    assert algo.count("normRewardOnDeviceEnv") == 1   # (a comment: PPO_Discrete's and PPO_MultiDiscrete's constructors live here and do not call it)
    make = algo[algo.index("void PPOAlgorithm::construct()"):algo.index("EvalResult PPOAlgorithm::evaluate(")]
    assert "if (m_env_norm_reward) c.kernel_flags |= PPO_KERNEL_ENV_REWARD_NORM;" in make
    assert make.index("ppo_ctx_create(") < make.index("ppo_reward_norm_enable(m_ctx, 1, 10.0f, 1e-8f)") < make.index("loadPolicyFromCheckpoint();")


@pytest.mark.gpu
def test_norm_reward_through_the_facade(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", HOST, "host_env_reward_norm_test"])
    r = subprocess.run([EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "host_env_reward_norm_test ok" in r.stdout
    assert "with norm_reward: count 4096 " in r.stdout and "without norm_reward: " in r.stdout
