"""PPO_KERNEL_CAT_FUSED without a GPU: the five shapes of tests/cat_fused_shapes.py hold, at every list, every condition tests/test_grad_oracle_cpu.py puts
on a shape -- checked with the two oracles alone, before any kernel meets them -- and the binding carries the flag.

Measured with the committed seeds (C oracle f32 against float64, worst tensor over the four lists): 1.1e-6 at most."""
import numpy as np
import pytest

import cat_fused_shapes as S
import grad_oracle as G
from __graft_entry__ import load_package


@pytest.mark.parametrize("name", list(S.CAT_SHAPES))
def test_the_shapes_hold_the_oracle_conditions(name):
    s, b = S.CAT_SHAPES[name], S.batch(name)
    assert s["hidden"] == 64 and s["n_hidden"] == 2 and s["lists"] == (576, 225, 65, 2)
    assert [idx.size for idx in b["lists"]] == list(s["lists"])
    if s["masked"]:
        share, choice = G.single_action_rows(b["masks"], s["heads"]), float(G.choice_rows(b["masks"], s["heads"]).mean())
        print("%s: %.1f%% of rows have a head with one allowed action, %.1f%% a head of width >= 2 with >= 2 allowed actions" % (name, 100 * share, 100 * choice))
        assert share >= 0.01 and choice >= 0.10
    # what ref_index_lists promises of a two-row list
    two = b["lists"][s["lists"].index(2)]
    assert abs(b["d_logp"][two[0]]) < 0.1 and abs(b["d_values"][two[0]]) < 0.1 and abs(b["d_logp"][two[1]]) > 0.3 and abs(b["d_values"][two[1]]) > 0.3
    assert not G.shape_hp(s)["norm_adv"] or abs(float(b["adv"][two[0]]) - float(b["adv"][two[1]])) >= 0.5, (name, b["adv"][two])
    assert not s["masked"] or G.choice_rows(b["masks"][two[:1]], s["heads"])[0], name
    worst = 0.0
    for k, idx in enumerate(b["lists"]):
        (g64, s64, rows), (gc, sc) = S.oracle_step(name, k)
        d = G.tensor_distance(gc, g64, b["shapes"])
        for (_, net_i, layer, kind, v), di in zip(G.split(g64, b["shapes"]), d):
            print("%-32s M=%3d  %-14s max|g| %.3e  C oracle f32 vs float64 %.2e" % (name, idx.size, G.tensor_name(net_i, layer, kind), np.abs(v).max(), di))
            assert np.abs(v).max() > 0, (name, idx.size, G.tensor_name(net_i, layer, kind))          # every tensor carries a gradient
        for key in G.STAT_NAMES:
            assert abs(s64[key] - sc[key]) <= 1e-5 * max(1.0, abs(s64[key])), (name, idx.size, key, s64[key], sc[key])
        assert d.max() <= 1e-4, (name, idx.size, d)                        # above this the two oracles disagree about the formula
        worst = max(worst, float(d.max()))
        if idx.size >= 40:   # the conditions that make the step exercise PPO's branches (two rows cannot hold shares)
            clip = G.BASE_HP["clip_coef"]
            assert 0.2 <= s64["clipfrac"] <= 0.8, (name, idx.size, s64["clipfrac"])
            v_share = float((np.abs(rows["dv"]) > clip).mean())
            assert 0.2 <= v_share <= 0.8, (name, idx.size, v_share)
            assert (rows["l1"] > rows["l2"]).any() and (rows["l1"] < rows["l2"]).any(), (name, idx.size)
            if s["masked"]:
                assert G.single_action_rows(b["masks"][idx], s["heads"]) >= 0.01, (name, idx.size)
    print("MEASURED %r: %.1e" % (name, worst))


def test_binding_carries_the_flag():
    P = load_package()
    assert P.KERNEL_CAT_FUSED == 256 and P.binding.KERNEL_CAT_FUSED == S.CAT_FUSED
    assert P.make_config(kernel_flags=P.KERNEL_CAT_FUSED).kernel_flags == 256
    assert hasattr(P.Context, "cat_fused_launches")
    assert len(P.binding.ABI_SYMBOLS) == len(set(P.binding.ABI_SYMBOLS))   # the counts ride on ppo_gauss_fused_launches: no symbol of their own
    assert P.binding.ABI_VERSION == 5
