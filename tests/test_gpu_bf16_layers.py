"""The generic engine's bf16 FORWARD, every hidden layer element by element, by the rule of tests/bf16_layers.py (derived from float64 and the number formats
alone; tests/test_bf16_layers_cpu.py holds the rule).  tests/test_gpu_generic.py's bf16 forward bars (TOL[1]: 2e-3 / 4e-3 on a row's log-prob and value)
stay the end-to-end check; they are fences at 3 x what was measured, and a store that truncates, a tanh 1e-4 off or a lost k chunk passes them.

How a hidden unit is read without a new symbol: PROBE NETWORKS.  For a shape s, grad_oracle.make_params(P, s) gives real weights.  For depth d = 1 .. n_hidden a
context with n_hidden = d, plain categorical, head_dims (2,), carries the source's hidden layers 0 .. d - 1 of both nets and SELECTOR heads for one unit j:
the critic's head weight is one-hot(j) with bias 0, so value = h_j exactly (1.0 is a bf16 number, every other term is a zero); the actor's head has row 0 =
one-hot(j), row 1 = 0, biases 0, so logits = [h_j, 0] and the log-prob of action a is -softplus(-h_j) (a = 0) or -softplus(h_j) (a = 1).  j walks over ALL
hidden units (set_params; a new context per unit for the rollout, whose synthetic observations follow the context's step counter).

Entry points, the same 200 rows each (40 envs x 5 steps of the synthetic env: three 64-row tiles and 8 rows):
  get_value                      critic units from the value
  policy_act (action = zeros)    critic units from its value, actor units from its log-prob
  rollout (40 envs x 5 steps)    critic units from VALUES, actor units from LOGPROBS with ACTIONS (the sampled ones), inputs from OBS: generic_rollout_kernel
PPO_KERNEL_GENERIC_CLASSIC and PPO_KERNEL_GENERIC_SPLIT_HEAD are read in gen_fwd_bwd alone (api.hip): they change no launch of gen_values, gen_policy or
gen_rollout, so no shape is run under them here.

The check.  Layer d - 1 of the depth-d context is bf16_layers.layer_expectation(H_in, W, b) with H_in = bf16_rne(obs) for d = 1 and, for d >= 2, the LIBRARY'S
OWN H_{d-1} from the depth d - 1 context at the same entry point and net (teacher forcing by observation): every layer is judged on exact inputs, nothing
cascades.
Critic: the values themselves through bf16_layers.count_layer -- a safe element is `expected` bit for bit, any other is `expected` or the neighbour beyond
the midpoint it is near.
Actor: |log-prob - float64 log-prob at expected| <= 4e-6 (the suite's f32 forward bar; one bf16 step at |h| >= 2^-6 moves the log-prob by >= 3.3e-5) on safe
elements with |expected| >= 2^-6.  Every other element (|expected| < 2^-6, about 1 %, counts as unsafe) is decoded: expected if that explains the log-prob
within 4e-6, else the bf16 value nearest the log-prob's inverse, which must explain it within 4e-6 and lie in bf16_layers' [allowed_lo, allowed_hi].  The
decoded units are the actor's H_d for the next depth; where a neighbour of the decoded value is within 8e-6 as well (|h| < 2^-8 or so: a bf16 step there is
below what a log-prob resolves), H_AMBIGUOUS = 3.2e-5 goes into layer_expectation's H_err, so the next layer's margins cover it.
The safe share of every (shape, entry, net, layer) must reach bf16_layers.SAFE_SHARE_MIN on the library's data as on the stand-in data.  Printed per (shape, entry, net, layer): safe share, mismatches on safe elements, flips among the others.

Shapes (entries of grad_oracle.SHAPES, the smallest that reach each path):
  obs120 h48x2     fused (generic_forward_kernel), pitch 128, mostly padding
  obs132 h160x3    fused, pitch 256, ragged second block, three layers: the top activation sits in the other LDS tile
  obs376 h256x4    configs[4]'s network
  obs120 h128x1    one hidden layer
  obs130 h160x3    obs % 4 != 0: launch_to_bf16_pad and the launch_matmul_bf16 chain for get_value / policy_act
  obs24 h257x2     ld_h 384: the product kernels

Run time.  One case per (shape, entry, layer); the cases of a (shape, entry) run bottom up and share what they walked (judged), since layer d's inputs are
layer d - 1's outputs over ALL units -- which is also why no unit is skipped anywhere.  Measured on an MI355X: get_value and policy_act 1.1 s for the four
layers of obs376 h256x4 together; the rollout, one context per unit, 1.0 .. 3.7 s per layer at 256 units and under 1 s per layer elsewhere.
"""
import ctypes as C
import time

import numpy as np
import pytest

import bf16_layers as B
import grad_oracle as G
import oracle as O
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

N_ENVS, N_STEPS = 40, 5
ROWS = N_ENVS * N_STEPS
LOGP_BAR = 4e-6          # the suite's f32 forward bar (tests/test_gpu_generic.py TOL[0]), on the log-prob of a two-logit head
H_MIN = 2.0 ** -6        # below it one bf16 step moves the log-prob by less than 3.3e-5: such actor elements count as unsafe
H_AMBIGUOUS = 2 * LOGP_BAR / 0.25   # |d log-prob / d h| = sigmoid(-+h) > 0.25 for |h| <= 1.09: every h whose log-prob is within 2 LOGP_BAR of the one seen lies this close
SHAPES = ["bf16 obs120 h48x2 (2,3) masked", "bf16 obs132 h160x3 (3,3,3,2) masked", "bf16 obs376 h256x4 (3,3,3,2) masked",
          "bf16 obs120 h128x1 (4,) plain value loss", "bf16 obs130 h160x3 (3,3,3,2) masked", "bf16 obs24 h257x2 (2,3) masked"]
NETS = ("critic", "actor")


@pytest.fixture(scope="module")
def P():
    return load_package()


_SOURCES = {}


def source(P, name):
    """the shape's real weights per (net, layer, kind) and the 200 observation rows, made once per shape and left unchanged"""
    if name not in _SOURCES:
        s = G.SHAPES[name]
        net = O.Net.make(s["obs"], list(s["heads"]), hidden=s["hidden"], n_hidden=s["n_hidden"])
        tensors = {(n, layer, kind): v.copy() for _, n, layer, kind, v in G.split(G.make_params(P, s), O.param_shapes(net))}
        obs = np.concatenate([O.synthetic_obs(s["seed"], np.arange(N_ENVS), t, s["obs"]) for t in range(N_STEPS)])
        _SOURCES[name] = (tensors, obs)
    return _SOURCES[name]


class Probe:
    """the flat parameters of a depth-d probe network (the library's order: critic layers, then actor layers) with selector heads that move to unit j"""

    def __init__(self, s, tensors, d):
        self.hidden = s["hidden"]
        parts, at, self.head = [], 0, []
        for net in (0, 1):
            for layer in range(d):
                parts += [tensors[net, layer, "w"].ravel(), tensors[net, layer, "b"].ravel()]
            at = sum(p.size for p in parts)
            self.head.append(at)                    # row 0 of this net's head weight
            out = 1 if net == 0 else 2
            parts += [np.zeros(out * self.hidden, np.float32), np.zeros(out, np.float32)]
        self.flat = np.concatenate(parts).astype(np.float32)
        self.j = None

    def select(self, j):
        for at in self.head:
            if self.j is not None:
                self.flat[at + self.j] = 0.0
            self.flat[at + j] = 1.0
        self.j = j
        return self.flat


def probe_context(P, s, d):
    sp = dict(s, heads=(2,), masked=False, n_hidden=d)
    return G.context(P, sp, 0, num_envs=N_ENVS, num_steps=N_STEPS, total_timesteps=8 * ROWS)


def walk_direct(P, s, tensors, d, obs):
    """get_value and policy_act of the depth-d probe over all units, on device arrays allocated once (the binding's own methods allocate per call)"""
    ctx = probe_context(P, s, d)
    probe = Probe(s, tensors, d)
    assert ctx.P == probe.flat.size, (ctx.P, probe.flat.size)
    L, chk, n = P.binding.lib(), P.binding._check, obs.shape[0]
    d_obs, d_forced = ctx.dev(obs, np.float32), ctx.dev(np.zeros((n, 1)), np.int64)
    d_a, d_lp, d_en, d_v, d_v2 = ctx.empty((n, 1), np.int64), ctx.empty(n, np.float32), ctx.empty(n, np.float32), ctx.empty(n, np.float32), ctx.empty(n, np.float32)
    out = {k: np.empty((n, s["hidden"]), np.float32) for k in ("get_value", "policy_act value", "policy_act logp")}
    for j in range(s["hidden"]):
        ctx.set_params(probe.select(j))
        chk(L.ppo_get_value(ctx.h, d_obs.ptr, C.c_int64(n), d_v.ptr), ctx.h)
        chk(L.ppo_policy_act(ctx.h, d_obs.ptr, None, d_forced.ptr, C.c_int64(n), C.c_int64(0), d_a.ptr, d_lp.ptr, d_en.ptr, d_v2.ptr), ctx.h)
        out["get_value"][:, j], out["policy_act value"][:, j], out["policy_act logp"][:, j] = d_v.download(), d_v2.download(), d_lp.download()
        if j == 0:
            assert not d_a.download().any()
    ctx.close()
    return {"get_value": {0: (out["get_value"], None)}, "policy_act": {0: (out["policy_act value"], None), 1: (out["policy_act logp"], np.zeros((n, 1), np.int64))}}


def walk_rollout(P, s, tensors, d, obs):
    """rollout of the depth-d probe over all units.  The synthetic env's observations follow the context's step counter, which only counts up, so every unit
    gets a context of its own: the same 200 rows each time (asserted)."""
    probe = Probe(s, tensors, d)
    values, logp = np.empty((ROWS, s["hidden"]), np.float32), np.empty((ROWS, s["hidden"]), np.float32)
    actions = np.empty((ROWS, s["hidden"]), np.int64)
    for j in range(s["hidden"]):
        ctx = probe_context(P, s, d)
        ctx.set_params(probe.select(j))
        ctx.env_reset()
        ctx.rollout()
        values[:, j], logp[:, j], actions[:, j] = ctx.read("VALUES", (ROWS,)), ctx.read("LOGPROBS", (ROWS,)), ctx.read("ACTIONS", (ROWS,))
        if j in (0, s["hidden"] - 1):
            assert np.array_equal(ctx.read("OBS", (ROWS, s["obs"])).view(np.uint32), obs.view(np.uint32)), j
        ctx.close()
    assert ((actions == 0) | (actions == 1)).all()
    return {"rollout": {0: (values, None), 1: (logp, actions)}}


def actor_layer(logp, actions, exp):
    """An actor layer from the log-probs of the selector head: (counts, decoded H, H_err).  The decoded unit is expected where expected explains the log-prob
    within LOGP_BAR, else the bf16 value nearest the log-prob's inverse; it must explain the log-prob within LOGP_BAR and lie in [allowed_lo, allowed_hi]."""
    sign = np.where(actions == 0, -1.0, 1.0)                      # log p(0) = -softplus(-h), log p(1) = -softplus(h)
    seen = np.asarray(logp, np.float64)
    away = lambda h: np.abs(seen - (-np.logaddexp(0.0, sign * h)))   # noqa: E731
    with np.errstate(all="ignore"):
        inverse = sign * np.log(np.expm1(-seen))
    fits = away(exp.expected) <= LOGP_BAR
    H = np.where(fits, exp.expected, B.bf16_rne(np.where(np.isfinite(inverse), inverse, 0.0)))
    ok = np.isfinite(inverse) & (away(H) <= LOGP_BAR) & (H >= exp.allowed_lo) & (H <= exp.allowed_hi)
    lo, hi = B.bf16_neighbours(H)
    H_err = np.where((away(lo) <= 2 * LOGP_BAR) | (away(hi) <= 2 * LOGP_BAR), H_AMBIGUOUS, 0.0)
    safe = exp.safe & (np.abs(exp.expected) >= H_MIN)
    counts = dict(n=int(safe.size), safe=int(safe.sum()), safe_share=float(safe.mean()), safe_mismatch=int((safe & ~fits).sum()),
                  unsafe_flips=int((~safe & ok & ~fits).sum()), unsafe_bad=int((~safe & ~ok).sum()))
    return counts, H, H_err


_JUDGED = {}


def judged(P, name, entry, d):
    """Layer d - 1 of (shape, entry) walked and judged ONCE: {(entry point, net): dict(H, H_err, counts, K, bad)}, kept for the depth above (its inputs) and
    for the case of the same depth.  The depths below are walked first if no earlier case has."""
    if (name, entry, d) in _JUDGED:
        return _JUDGED[name, entry, d]
    s = G.SHAPES[name]
    tensors, obs = source(P, name)
    below = judged(P, name, entry, d - 1) if d > 1 else None
    assert below is None or not any(r["bad"] for r in below.values()), "a layer that failed is no input for the one above it"
    out = {}
    for point, nets in (walk_rollout if entry == "rollout" else walk_direct)(P, s, tensors, d, obs).items():
        for net, (seen, actions) in nets.items():
            H_in, H_err = (below[point, net]["H"], below[point, net]["H_err"]) if below else (B.bf16_rne(obs.astype(np.float64)), None)
            exp = B.layer_expectation(H_in, tensors[net, d - 1, "w"], tensors[net, d - 1, "b"], H_err)
            if actions is None:
                c, H, err, worst = B.count_layer(seen, exp), seen.astype(np.float64), None, B.offenders(seen, exp)
            else:
                (c, H, err), worst = actor_layer(seen, actions, exp), []
            bad = [(point, NETS[net], d - 1, c, worst)] if c["safe_mismatch"] or c["unsafe_bad"] or not c["safe_share"] >= B.SAFE_SHARE_MIN else []
            out[point, net] = dict(H=H, H_err=err, counts=c, K=H_in.shape[1], bad=bad)
    _JUDGED[name, entry, d] = out
    return out


CASES = [(name, entry, d) for name in SHAPES for entry in ("get_value and policy_act", "rollout") for d in range(1, G.SHAPES[name]["n_hidden"] + 1)]


@pytest.mark.parametrize("name,entry,d", CASES, ids=["%s-%s-layer %d" % (n, e, d - 1) for n, e, d in CASES])
def test_hidden_layer_element_by_element(P, name, entry, d):
    """One case per (shape, entry, layer), so that each stays at a few seconds (a rollout case makes one context per hidden unit: 2 s at 256 units); the
    cases of a (shape, entry) run bottom up and share what they walked.  The top layer's case prints the (shape, entry) summary."""
    t0 = time.time()
    res = judged(P, name, entry, d)
    for (point, net), r in res.items():
        c = r["counts"]
        print("LAYERS %-42s %-10s %-6s layer %d K %3d: safe share %.3f, mismatches on safe elements %d, flips among the others %d of %d" %
              (name, point, NETS[net], d - 1, r["K"], c["safe_share"], c["safe_mismatch"], c["unsafe_flips"], c["n"] - c["safe"]))
    bad = [b for r in res.values() for b in r["bad"]]
    assert not bad, bad
    if d == G.SHAPES[name]["n_hidden"]:
        points = sorted({point for k in range(1, d + 1) for point, _ in judged(P, name, entry, k)})
        for point in points:
            cs = [r["counts"] for k in range(1, d + 1) for (pt, _), r in judged(P, name, entry, k).items() if pt == point]
            print("LAYERS %-42s %-10s all layers: lowest safe share %.3f, mismatches on safe elements %d, flips among the others %d" %
                  (name, point, min(c["safe_share"] for c in cs), sum(c["safe_mismatch"] for c in cs), sum(c["unsafe_flips"] for c in cs)))
    print("LAYERS %-42s %-24s layer %d: %.1f s" % (name, entry, d - 1, time.time() - t0))
