"""The element-by-element rule of tests/bf16_layers.py, held on the CPU before a kernel meets it (tests/test_gpu_bf16_layers.py) -- no GPU, no library.

On grad_oracle.stand_in_batch of every bf16 entry of grad_oracle.SHAPES, both nets, every hidden layer, the first 200 rows; the inputs of layer l >= 1 are the
rule's own expected activations of layer l - 1, so every arithmetic is judged on the same exact inputs:

  two correct f32 arithmetics must pass check_layer with no mismatch on a safe element:
    (a) the oracle's order: sequential from the bias, one f32 addition per product, then the C library's f32 tanh;
    (b) blocks of 16 products summed exactly, the block sums added in f32, the bias last, then tanh_mufu's formula (bf16_layers.tanh_mufu_f32);
  the safe share of every (shape, net, layer) is at least bf16_layers.SAFE_SHARE_MIN = 0.60 (a condition: a rule that judged few elements would hold little);
  four wrong arithmetics must each FAIL check_layer on every (shape, net, layer): a store that truncates, a tanh that is 1e-4 off, a sum that drops the last 8
    elements of the contraction, and one column's bias omitted (the column with the largest |bias|: 0.02-normal biases include some of 1e-4, which move
    nothing at 200 rows);
  tanh_mufu's formula with an exact exp2 and reciprocal stays within E_TANH / 2 of the float64 tanh over 10^6 points of [-9, 9].
"""
import numpy as np
import pytest

import bf16_layers as B
import grad_oracle as G

BF16_SHAPES = [n for n, s in G.SHAPES.items() if s["dtype"] == 1]
ROWS = 200


def f32_to_bf16(x):
    """an f32 array rounded to bf16, nearest even, as float64"""
    assert x.dtype == np.float32
    return B.bf16_rne(x.astype(np.float64))


def z_sequential(H, W, b, k_end=None):
    """acc = b; acc += h[k] w[k] for k = 0 .. K - 1, every step in f32 (the products of two bf16 numbers are exact in f32)"""
    H, W = H.astype(np.float32), W.astype(np.float32)
    acc = np.broadcast_to(np.asarray(b, np.float32).reshape(1, -1), (H.shape[0], W.shape[0])).copy()
    for k in range(H.shape[1] if k_end is None else k_end):
        acc = (acc + H[:, k:k + 1] * W[None, :, k]).astype(np.float32)
    return acc


def z_blocks_of_16(H, W, b):
    """every 16 products summed exactly (float64 holds the sum of 16 sixteen-bit products), the block sums added in f32, the bias last"""
    acc = np.zeros((H.shape[0], W.shape[0]), np.float32)
    for k0 in range(0, H.shape[1], 16):
        acc = (acc + (H[:, k0:k0 + 16] @ W[:, k0:k0 + 16].T).astype(np.float32)).astype(np.float32)
    return (acc + np.asarray(b, np.float32).reshape(1, -1)).astype(np.float32)


@pytest.fixture(scope="module")
def layers():
    """per shape name: [(net, layer, H_in, W_f32, b_f32)], built once and left unchanged"""
    out = {}
    for name in BF16_SHAPES:
        s = G.SHAPES[name]
        d = G.stand_in_batch(s)
        t = {(net, layer, kind): v for _, net, layer, kind, v in G.split(d["params"], d["shapes"])}
        rows = []
        for net in (0, 1):
            H = B.bf16_rne(d["obs"][:ROWS].astype(np.float64))
            for layer in range(s["n_hidden"]):
                W, b = t[net, layer, "w"], t[net, layer, "b"].reshape(-1)
                rows.append((net, layer, H, W, b))
                H = B.layer_expectation(H, W, b).expected
        out[name] = rows
    return out


@pytest.mark.parametrize("name", BF16_SHAPES)
def test_two_correct_arithmetics_agree_on_every_safe_element(layers, name):
    for net, layer, H, W, b in layers[name]:
        Wb = B.bf16_rne(W.astype(np.float64))
        a_seq = f32_to_bf16(np.tanh(z_sequential(H, Wb, b)))
        a_blk = f32_to_bf16(B.tanh_mufu_f32(z_blocks_of_16(H, Wb, b)))
        for what, a in (("sequential, tanhf", a_seq), ("blocks of 16, bias last, tanh_mufu", a_blk)):
            c = B.check_layer(a, H, W, b)
            print("%-45s %-12s K %3d %-36s safe %.3f flips among unsafe %d of %d" %
                  (name, G.tensor_name(net, layer, "w")[:-2], H.shape[1], what, c["safe_share"], c["unsafe_flips"], c["n"] - c["safe"]))
            assert c["safe_mismatch"] == 0 and c["unsafe_bad"] == 0, (name, net, layer, what, c)
            assert c["safe_share"] >= B.SAFE_SHARE_MIN, (name, net, layer, c)


@pytest.mark.parametrize("name", BF16_SHAPES)
def test_four_wrong_arithmetics_fail(layers, name):
    for net, layer, H, W, b in layers[name]:
        Wb = B.bf16_rne(W.astype(np.float64))
        t = np.tanh(z_sequential(H, Wb, b))
        b_less = b.copy()
        b_less[np.argmax(np.abs(b))] = 0.0
        wrong = {
            "a truncating store": B.bf16_trunc(t.astype(np.float64)),
            "tanh + 1e-4": f32_to_bf16((t + np.float32(1e-4)).astype(np.float32)),
            "the last 8 of the contraction dropped": f32_to_bf16(np.tanh(z_sequential(H, Wb, b, k_end=H.shape[1] - 8))),
            "one column's bias omitted": f32_to_bf16(np.tanh(z_sequential(H, Wb, b_less))),
        }
        for what, a in wrong.items():
            exp = B.layer_expectation(H, W, b)
            c = B.count_layer(a, exp)
            print("%-45s %-12s %-40s mismatches on safe elements %5d of %5d" % (name, G.tensor_name(net, layer, "w")[:-2], what, c["safe_mismatch"], c["safe"]))
            with pytest.raises(B.LayerMismatch):
                B.check_layer(a, H, W, b)


def test_tanh_mufu_formula_within_half_of_e_tanh():
    x = np.linspace(-9.0, 9.0, 10 ** 6).astype(np.float32)
    err = np.abs(B.tanh_mufu_f32(x).astype(np.float64) - np.tanh(x.astype(np.float64)))
    print("tanh_mufu's formula, exact exp2 and reciprocal: max |error| %.3e at x = %.6f (E_TANH / 2 = %.1e)" % (err.max(), x[np.argmax(err)], B.E_TANH / 2))
    assert err.max() <= B.E_TANH / 2


def test_bf16_rounding_and_neighbours():
    """bf16_rne against the bit trick of the oracle (u + 0x7fff + lsb) on f32 inputs, ties included; the neighbours across a power of two and at zero"""
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(100000).astype(np.float32), (rng.integers(0, 1 << 16, 4096).astype(np.uint32) << 16 | 0x8000).view(np.float32),
                        np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0 ** -126, 2.0 ** -127, 2.0 ** -133], np.float32)])
    x = x[np.isfinite(x) & (np.abs(x) < 3e38)]
    u = x.view(np.uint32).astype(np.uint64)
    want = (((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32)).view(np.float32)
    assert np.array_equal(B.bf16_rne(x.astype(np.float64)), want.astype(np.float64))
    assert B.bf16_rne(1.0 + 2.0 ** -8 + 2.0 ** -40) == 1.0 + 2.0 ** -7      # float64 just above a tie: up (through f32 it would land on the tie and go to even)
    lo, hi = B.bf16_neighbours(np.array([1.0, -1.0, 0.0, -0.0, 1.0 + 2.0 ** -7, 2.0 ** -126, 0.75]))
    assert np.array_equal(lo, [1 - 2.0 ** -8, -1 - 2.0 ** -7, -2.0 ** -133, -2.0 ** -133, 1.0, 2.0 ** -126 - 2.0 ** -133, 0.75 - 2.0 ** -8])
    assert np.array_equal(hi, [1 + 2.0 ** -7, -1 + 2.0 ** -8, 2.0 ** -133, 2.0 ** -133, 1.0 + 2.0 ** -6, 2.0 ** -126 + 2.0 ** -133, 0.75 + 2.0 ** -8])
    # every bf16 value of a stretch of bit patterns: the neighbours are the adjacent patterns
    pats = np.arange(0x0001, 0x7f7f, dtype=np.uint32)
    v = (pats << 16).view(np.float32).astype(np.float64)
    lo, hi = B.bf16_neighbours(v[1:-1])
    assert np.array_equal(lo, v[:-2]) and np.array_equal(hi, v[2:])
