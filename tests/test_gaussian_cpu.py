"""Diagonal-Gaussian policies without a GPU: the header declares the four new entry points and the binding lists them, DIST_GAUSSIAN == 2, and the float64
oracle that tests/test_gpu_gaussian.py holds the kernels to states torch.distributions.Normal's own formulas."""
import math
import os
import re

import numpy as np
import torch

from __graft_entry__ import ROOT, load_package

NEW = ["ppo_host_act_f32", "ppo_dev_act_f32", "ppo_policy_act_f32", "ppo_gaussian"]


def test_header_declares_the_new_symbols_and_the_binding_lists_them():
    P = load_package()
    hdr = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    declared = set(re.findall(r"^PPO_API\s+[\w\s\*]+?\b(ppo_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW:
        assert name in declared, name
        assert name in P.binding.ABI_SYMBOLS, name
    assert sorted(P.binding.ABI_SYMBOLS) == sorted(declared)
    assert re.search(r"PPO_DIST_GAUSSIAN\s*=\s*2\b", hdr)
    assert re.search(r"#define\s+PPO_ABI_VERSION\s+5\b", hdr)
    assert "clip" in hdr[hdr.index("PPO_DIST_GAUSSIAN"):][:3000].lower()   # the header says whose business clipping is


def test_dist_gaussian_constant_and_wrappers():
    P = load_package()
    assert P.DIST_GAUSSIAN == 2 and (P.DIST_CATEGORICAL, P.DIST_MASKED) == (0, 1)
    for m in ("host_act_f32", "dev_act_f32", "policy_act_f32"):
        assert callable(getattr(P.Context, m))
    assert callable(P.gaussian)
    cfg = P.make_config(env_kind=P.ENV_HOST, dist_kind=P.DIST_GAUSSIAN, obs_size=7, head_dims=(5,))
    assert (cfg.dist_kind, cfg.n_heads, cfg.head_dims[0]) == (2, 1, 5)


def test_oracle_formulas_equal_torch_normal():
    import test_gpu_gaussian as G
    gen = torch.Generator().manual_seed(0)
    for n, D in ((1, 1), (127, 3), (129, 17), (300, 32)):
        mu = torch.randn(n, D, dtype=torch.float64, generator=gen)
        log_std = torch.rand(D, dtype=torch.float64, generator=gen) * 3 - 2
        a = mu + torch.exp(log_std) * (torch.rand(n, D, dtype=torch.float64, generator=gen) * 8 - 4)
        dist = torch.distributions.Normal(mu, torch.exp(log_std).expand(n, D))
        assert torch.allclose(G.gauss_logprob(mu, log_std, a), dist.log_prob(a).sum(-1), rtol=1e-13, atol=1e-12)
        assert torch.allclose(G.gauss_entropy(mu, log_std), dist.entropy().sum(-1), rtol=1e-13, atol=1e-12)
    assert abs(G.HALF_LOG_2PI - 0.9189385332046727) < 1e-15
    # the parameter order the oracle assumes: critic layers, actor layers, log_std last
    shp = G.tensor_shapes(11, 64, 2, 3)
    assert shp == [(64, 11), (64,), (64, 64), (64,), (1, 64), (1,), (64, 11), (64,), (64, 64), (64,), (3, 64), (3,), (3,)]
    assert len(G.tensor_shapes(5, 96, 3, 17)) == 17
    # the initial reward of the bandit the learning test derives its threshold from: -(E|obs|^2 + D) = -(2/3 + 2)
    assert math.isclose(-(2.0 / 3.0 + 2.0), -2.6667, abs_tol=1e-4)


def test_oracle_loss_gradients_by_hand():
    """the two gradient formulas the kernel implements, against autograd of the oracle's loss on one clipped-nowhere batch"""
    import test_gpu_gaussian as G
    rng = np.random.default_rng(0)
    n, D = 9, 3
    mu = torch.tensor(rng.normal(0, 1, (n, D)), requires_grad=True)
    log_std = torch.tensor(rng.uniform(-1, 0.5, D), requires_grad=True)
    a = torch.tensor(rng.normal(0, 1, (n, D)))
    lp = G.gauss_logprob(mu, log_std, a)
    w = torch.tensor(rng.normal(0, 1, n))
    (w * lp).sum().backward()
    z = ((a - mu) * torch.exp(-log_std)).detach()
    assert torch.allclose(mu.grad, w[:, None] * z * torch.exp(-log_std.detach()), atol=1e-12)
    assert torch.allclose(log_std.grad, (w[:, None] * (z * z - 1)).sum(0), atol=1e-12)
