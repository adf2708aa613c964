"""The C++ facade's observation normalisation (PPO_HostEnv::setNormObs / `norm_obs` in PPOConfig.toml; ppo-libtorch_amd/host/) and the statistics file
beside a checkpoint (ObsNormFile: "<agent file>.obsnorm", raw little-endian f64 O, count, mean[O], var[O]).

Without a GPU: the key is read where the other extension keys are, PPO_HostEnv has the setter and refuses env groups through the library's own call, the
checkpoint code writes and loads the file and never takes it for an agent file, and host/tests/host_obs_norm_test writes a file, checks its size and
layout and reads it back bit for bit.  On the GPU the same binary trains two updates of a toy env whose columns differ in scale by seven orders of
magnitude; the file it leaves beside the final model must hold count = (1 + 2 T) N."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppo-libtorch_amd", "host")
EXE = os.path.join(HOST, "host_obs_norm_test")
N, T, UPDATES = 16, 32, 2   # host/tests/host_obs_norm_test.cpp


def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-j", "4", "-C", HOST])
    return EXE


def test_facade_sources_have_the_key_the_setter_and_the_file():
    algo = open(os.path.join(HOST, "PPO", "PPOAlgorithm.cpp")).read()
    assert re.search(r'B\("environment", "norm_obs", m_norm_obs\)', algo)
    assert algo.index('"env_groups"') < algo.index('"norm_obs"') < algo.index('"seed"')   # in [environment], beside env_groups
    hdr = open(os.path.join(HOST, "PPO", "PPOAlgorithm.h")).read()
    assert re.search(r"bool m_norm_obs = false;", hdr) and "struct ObsNormFile" in hdr
    host = open(os.path.join(HOST, "PPO", "PPO_HostEnv.h")).read()
    assert "void setNormObs(bool on)" in host and "ppo_obs_norm_enable" in host
    # the refusal with env groups is the library's: the facade asks ppo_host_rollout_begin_groups and throws what it says
    body = host[host.index("void refuseGroupsWithNormObs"):]
    assert "ppo_host_rollout_begin_groups" in body[:body.index("\n    }\n")]
    # saved with every checkpoint through get, loaded through set when present, and skipped by the newest-file rule
    save = algo[algo.index("void PPOAlgorithm::saveCheckpoint"):algo.index("static std::string newestFile")]
    assert "ppo_obs_norm_get_h" in save and "ObsNormFile::pathFor(agentFile)" in save
    assert save.index("ppo_obs_norm_get_h") < save.index("ppo::pt::writeAgent")   # written before the agent file: never the newest file of its directory
    newest = algo[algo.index("static std::string newestFile"):algo.index("static bool flattenFor")]
    assert '".obsnorm"' in newest
    load = algo[algo.index("void PPOAlgorithm::loadPolicyFromCheckpoint"):]
    assert "ppo_obs_norm_set_h" in load and "fs::exists(side)" in load
    # the .pt archives are written as before: the container knows nothing of the statistics
    assert "obs_norm" not in open(os.path.join(HOST, "Utils", "TorchArchive.cpp")).read().lower()


def test_statistics_file_round_trip(tmp_path):
    r = subprocess.run([exe(), "sidecar", str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OBS_NORM_SIDECAR_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.gpu
def test_obs_norm_facade_on_gpu(tmp_path):
    r = subprocess.run([exe(), "train"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OBS_NORM_FACADE_OK" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    assert "group" in r.stdout   # the refusal's text was printed
    side = tmp_path / "Models" / ("PPO_Agent_%d_steps.pt.obsnorm" % (N * T * UPDATES))
    assert side.stat().st_size == 8 * (2 + 2 * 4)
    raw = np.fromfile(str(side), "<f8")
    assert raw[0] == 4 and raw[1] == (1 + UPDATES * T) * N
    mean, var = raw[2:6], raw[6:10]
    assert np.isfinite(mean).all() and (var >= 0).all() and abs(mean[3] - 10002) < 3
