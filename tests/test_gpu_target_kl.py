"""Early stop of an update at a target KL (include/ppo_hip.h: ppo_target_kl_set / ppo_early_stop_read; csrc/kernels_earlystop.hip) on the GPU.

The oracle is the library's own arithmetic with the feature off: permutations are keyed (seed, update, epoch), the advantage sums are per minibatch slot and
the AdamW coefficients per applied step, so a context with update_epochs = j and no target IS "epochs 0 .. j - 1" of a context with update_epochs = 4, and
a 4-epoch context that stops behind epoch j must equal it bit for bit: parameters, both moments, every ppo_stats field (anneal_lr = 0, so that nothing
else depends on the epoch count).  Shapes: the smallest that reach every optimizer kernel --
  ref                 CartPole, 64 envs x 32 steps, 4 minibatches (reduce + clip_adamw_sumsq_kernel)
  ref-selftest        the same with KERNEL_COMM_SELFTEST (three launches, clip_adamw_kernel, collectives issued)
  gen-f32 / gen-bf16 / gen-bf16-classic
                      ENV_SYNTHETIC, obs 6, heads (3, 2), 3 x 32 (the network tests/test_gpu_generic.py trains behind heads (3, 2)), 50 envs x 12 steps,
                      4 minibatches of 150 rows: gen_adamw_kernel, gen_opt_fused_kernel, and the classic four-launch tail
  gauss               ENV_HOST, DIST_GAUSSIAN, obs 5, D 3, 3 x 96, 16 envs x 8 steps, 2 minibatches; both contexts are fed the same seeded numpy stream
Every context lives for one test; a run (iterations of one configuration with the feature off) is computed once per module and shared."""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

LR = 3e-3
SHAPES = ["ref", "ref-selftest", "gen-f32", "gen-bf16", "gen-bf16-classic", "gauss"]


@pytest.fixture(scope="module")
def P():
    return load_package()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def config(P, shape, epochs):
    common = dict(update_epochs=epochs, seed=7, total_timesteps=1 << 30, learning_rate=LR, anneal_lr=False)
    if shape.startswith("ref"):
        return P.make_config(num_envs=64, num_steps=32, num_minibatches=4, kernel_flags=P.KERNEL_COMM_SELFTEST if shape == "ref-selftest" else 0, **common)
    if shape.startswith("gen"):
        return P.make_config(env_kind=P.ENV_SYNTHETIC, dist_kind=P.DIST_MASKED, obs_size=6, head_dims=(3, 2), hidden=32, n_hidden=3, num_envs=50, num_steps=12,
                             num_minibatches=4, max_episode_steps=9, ent_coef=0.01, compute_dtype=P.DTYPE_F32 if shape == "gen-f32" else P.DTYPE_BF16,
                             kernel_flags=P.KERNEL_GENERIC_CLASSIC if shape == "gen-bf16-classic" else 0, **common)
    assert shape == "gauss"
    return P.make_config(env_kind=P.ENV_HOST, dist_kind=P.DIST_GAUSSIAN, obs_size=5, head_dims=(3,), hidden=96, n_hidden=3, num_envs=16, num_steps=8,
                         num_minibatches=2, max_episode_steps=1000, ent_coef=0.01, **common)


class Driver:
    """One context and what feeds it: iteration() = rollout + advantages + update, enqueued the way the context kind does it."""

    def __init__(self, P, shape, epochs, target=None):
        self.P, self.shape = P, shape
        self.ctx = P.Context(config(P, shape, epochs))
        self.ctx.init_orthogonal(11)
        self.nmb = self.ctx.cfg.num_minibatches
        if target is not None:
            self.ctx.target_kl_set(target)
        if shape == "gauss":
            self.rng = np.random.default_rng(5)   # the same stream for every context of this shape
            self.ctx.host_env_reset(self.rng.normal(0, 1, (16, 5)))
        else:
            self.ctx.env_reset()

    def rollout_only(self):
        """the rollout and the advantages, without the update (device envs only)"""
        self.ctx.rollout()
        self.ctx.calc_advantage()

    def iteration(self):
        ctx = self.ctx
        if self.shape == "gauss":
            ctx.host_rollout_begin()
            for _ in range(8):
                ctx.host_act_f32()   # the env ignores the action: both contexts see the same observations whatever they sample
                ctx.host_observe(self.rng.normal(0, 1, (16, 5)), self.rng.normal(0, 1, 16), self.rng.random(16) < 0.1)
            ctx.host_rollout_end()
        else:
            ctx.train_iteration()

    def state(self):
        ctx = self.ctx
        st = ctx.stats()
        m, v, step = ctx.get_optimizer()
        return dict(params=ctx.get_params(), m=m, v=v, step=step, stats=st)

    def close(self):
        self.ctx.close()


def assert_same_state(a, b, what):
    for k in ("params", "m", "v"):
        assert np.array_equal(bits(a[k]), bits(b[k])), "%s: %s differ in %d of %d words" % (what, k, int((bits(a[k]) != bits(b[k])).sum()), a[k].size)
    assert a["step"] == b["step"], (what, a["step"], b["step"])
    for k, x in a["stats"].items():
        y = b["stats"][k]
        assert np.float64(x).tobytes() == np.float64(y).tobytes(), "%s: ppo_stats.%s %r != %r" % (what, k, x, y)


_runs = {}


def plain_run(P, shape, epochs, iterations):
    """States after each of `iterations` iterations of a context that never sets a target (the oracle); computed once, shared, never modified."""
    key = (shape, epochs, iterations)
    if key not in _runs:
        d = Driver(P, shape, epochs)
        out = []
        for _ in range(iterations):
            d.iteration()
            out.append(d.state())
        assert d.ctx.early_stop()["epochs_run"] == epochs and d.ctx.early_stop()["stopped"] == 0
        assert d.ctx.early_stop()["epochs_total"] == epochs * iterations
        d.close()
        _runs[key] = out
    return _runs[key]


@pytest.mark.parametrize("shape", SHAPES)
def test_stops_after_first_epoch_every_update(P, shape):
    """E = 4 with a target every epoch exceeds == E = 1, after each of 3 iterations: also the proof that the AdamW coefficient table follows the APPLIED
    step count across updates (a table that started at 4 nmb instead of nmb in iteration 2 would change every parameter)."""
    target = 1e-12
    ref = plain_run(P, shape, 1, 3)
    for it in range(3):   # the precondition, from the run with the feature off
        print(shape, "E=1 iteration", it, "approx_kl %.9g" % ref[it]["stats"]["approx_kl"])
        assert ref[it]["stats"]["approx_kl"] > target
    d = Driver(P, shape, 4, target)
    assert d.ctx.target_kl_get() == target
    for it in range(3):
        d.iteration()
        es = d.ctx.early_stop()
        got = d.state()
        assert_same_state(got, ref[it], "%s iteration %d" % (shape, it))
        assert got["stats"]["optimizer_steps"] == (it + 1) * d.nmb and got["step"] == (it + 1) * d.nmb
        assert es == dict(epochs_run=1, stopped=1, kl_at_stop=ref[it]["stats"]["approx_kl"], epochs_total=it + 1), es
    d.close()


@pytest.mark.parametrize("shape", ["ref", "gen-bf16"])
def test_stops_at_the_epoch_the_sequence_says(P, shape):
    """kl_j = the approx_kl an E = j context reports after one iteration (feature off).  A target between kl_1 and kl_2 stops an E = 4 context behind
    epoch 2, not 1: it equals the E = 2 context.  Measured sequences: DESIGN.md section 6c."""
    runs = [plain_run(P, shape, j, 1)[0] for j in (1, 2, 3, 4)]
    kl = [r["stats"]["approx_kl"] for r in runs]
    print(shape, "kl_1..kl_4 =", " ".join("%.9g" % k for k in kl))
    assert kl[0] < kl[1], kl   # precondition (change the learning rate or the seed if it fails, never the feature)
    target = (kl[0] + kl[1]) / 2
    d = Driver(P, shape, 4, target)
    d.iteration()
    es = d.ctx.early_stop()
    assert_same_state(d.state(), runs[1], shape)
    assert es == dict(epochs_run=2, stopped=1, kl_at_stop=kl[1], epochs_total=2), es
    d.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_a_target_never_reached_changes_nothing(P, shape):
    ref = plain_run(P, shape, 4, 2)
    d = Driver(P, shape, 4, 1e30)
    for it in range(2):
        d.iteration()
        assert_same_state(d.state(), ref[it], "%s target 1e30, iteration %d" % (shape, it))
    es = d.ctx.early_stop()
    assert (es["epochs_run"], es["stopped"], es["epochs_total"]) == (4, 0, 8), es
    d.close()
    d = Driver(P, shape, 4, 0.5)   # set, then off again before any update: off is off
    d.ctx.target_kl_set(0)
    assert d.ctx.target_kl_get() == 0.0
    for it in range(2):
        d.iteration()
        assert_same_state(d.state(), ref[it], "%s target set and cleared, iteration %d" % (shape, it))
    es = d.ctx.early_stop()
    assert (es["epochs_run"], es["stopped"], es["kl_at_stop"], es["epochs_total"]) == (4, 0, 0.0, 8), es
    d.close()


@pytest.mark.parametrize("shape", ["ref", "gauss"])
def test_stop_does_not_leak(P, shape):
    """A stop is raised and cleared inside one ppo_update, and nothing of it reaches the stand-alone step DIRECTLY behind it -- no read of the statistics,
    the optimizer state or the outcome in between, any of which would bring the host's step count up to date first.  The step is applied, with the
    AdamW coefficient of applied step nmb + 1: parameters, moments and statistics equal, bit for bit, those of an E = 1 context with no target that
    takes the same stand-alone step on the same rows.  Reading the statistics raises no error: the STOP bit is not one, and it is cleared."""
    a, b = Driver(P, shape, 4, 1e-12), Driver(P, shape, 1)
    idx = np.arange(a.ctx.B // a.nmb, dtype=np.int32)[::-1].copy()
    for d in (a, b):
        d.iteration()
        d.ctx.minibatch_forward_backward(idx)
        d.ctx.optimizer_step()
    sa, sb = a.state(), b.state()
    assert sb["step"] == b.nmb + 1 and sb["stats"]["optimizer_steps"] == b.nmb + 1
    assert_same_state(sa, sb, shape + ": stand-alone step behind a stopped update")
    es = a.ctx.early_stop()
    assert (es["epochs_run"], es["stopped"], es["epochs_total"]) == (1, 1, 1), es
    one = plain_run(P, shape, 1, 3)[0]   # the state in front of the stand-alone step: it did change the parameters
    assert int((bits(sa["params"]) != bits(one["params"])).sum()) > sa["params"].size // 2
    a.close()
    b.close()


ROLLOUT_BUFS = ("OBS", "ACTIONS", "LOGPROBS", "REWARDS", "DONES", "VALUES", "ADVANTAGES", "RETURNS")


def test_checkpoint_sees_applied_steps(P):
    """ppo_optimizer_get_h behind a stopped update returns the applied steps.  That checkpoint -- parameters, moments, step -- goes into an E = 1 context;
    both then run one more update, with the same target, on the same rollout (the PPO_BUF_* arrays copied across), and agree bit for bit on everything the
    update produces.  The E = 1 context has run one iteration of its own first, so that its update counter -- the key of the permutations -- is the
    E = 4 context's; everything else of its state is replaced or does not enter the update."""
    shape, target = "ref", 1e-12
    a, b = Driver(P, shape, 4, target), Driver(P, shape, 1, target)
    a.iteration()
    b.iteration()
    m, v, step = a.ctx.get_optimizer()
    assert step == a.nmb
    b.ctx.set_params(a.ctx.get_params() * np.float32(1.0))
    b.ctx.set_optimizer(m, v, step)
    assert b.ctx.get_optimizer()[2] == a.nmb
    a.rollout_only()
    b.rollout_only()   # b's own rollout is overwritten with a's
    for name in ROLLOUT_BUFS:
        b.ctx.write(name, a.ctx.read(name))
    a.ctx.update()
    b.ctx.update()
    sa, sb = a.state(), b.state()
    assert sa["step"] == 2 * a.nmb and sb["step"] == 2 * a.nmb
    ea, eb = a.ctx.early_stop(), b.ctx.early_stop()
    assert (ea["epochs_run"], ea["stopped"], ea["epochs_total"]) == (1, 1, 2) and ea == eb, (ea, eb)
    for k in ("params", "m", "v"):
        assert np.array_equal(bits(sa[k]), bits(sb[k])), k
    for k in ("pg_loss", "v_loss", "entropy_loss", "approx_kl", "loss", "clipfrac_last", "clipfrac_mean", "total_norm", "explained_variance", "optimizer_steps",
              "updates", "learning_rate"):
        assert np.float64(sa["stats"][k]).tobytes() == np.float64(sb["stats"][k]).tobytes(), k
    a.close()
    b.close()


def test_arguments(P):
    d = Driver(P, "ref", 4)
    L = P.binding.lib()
    assert d.ctx.early_stop() == dict(epochs_run=0, stopped=0, kl_at_stop=0.0, epochs_total=0)
    assert d.ctx.target_kl_get() == 0.0
    d.ctx.target_kl_set(0.015)
    assert d.ctx.target_kl_get() == 0.015
    for bad in (-1e-3, float("nan"), float("inf"), float("-inf")):
        assert L.ppo_target_kl_set(d.ctx.h, C.c_double(bad)) == 1, bad
        assert d.ctx.target_kl_get() == 0.015
    assert L.ppo_early_stop_read(d.ctx.h, None, None, None, None) == 0   # any output may be NULL
    assert d.ctx.early_stop() == dict(epochs_run=0, stopped=0, kl_at_stop=0.0, epochs_total=0)
    d.ctx.target_kl_set(0)
    assert d.ctx.target_kl_get() == 0.0
    d.close()
