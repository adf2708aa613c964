"""Env groups of caller-stepped environments (include/ppo_hip.h, "Env groups": ppo_host_rollout_begin_groups / ppo_host_group_act /
ppo_host_group_actions / ppo_host_group_observe): the rollout taken group by group, in any interleaving, is the ungrouped rollout bit for bit.

The yardstick is tests/test_gpu_host_env.py's: context A trains on its own device env (ppo_train_iteration); context B is a PPO_ENV_HOST context driven by
the group calls, each group's envs stepped by a device-env context of its own configured as a shard of the global batch (num_envs = n_g, env_offset =
bounds[g], global_num_envs = N: env_reset / env_step reproduce the global envs' rows).  After every iteration every buffer of BUFS, the parameters, the
AdamW state and stats() of B are A's.  The generic engine has no device env a caller could step, so there the grouped context is compared with an
UNGROUPED PPO_ENV_HOST context fed the same pre-drawn transitions.
"""
import ctypes

import numpy as np
import pytest

from __graft_entry__ import load_package
from test_gpu_beyond_first_trip import ACT16_CAP, FUSED_CAP, VECTOR_CAP, assert_past_the_cap
from test_gpu_host_env import BUFS, NumpyFin, assert_same_state, bits
from test_gpu_matmul import DB_MAX_ROWS

pytestmark = pytest.mark.gpu

RAGGED = [0, 7, 50, 96]   # boundaries off the 16-row tile


@pytest.fixture(scope="module")
def P():
    return load_package()


# ---- interleavings: a list of (op, g) that is legal group by group (act -> actions -> observe, T times) ----
def order_lockstep(G, T):
    out = []
    for _ in range(T):
        out += [("act", g) for g in range(G)] + [("actions", g) for g in range(G)] + [("observe", g) for g in range(G)]
    return out


def order_pipeline(G, T):
    """act of the next group is enqueued before the actions of this one are read (G >= 2)"""
    assert G >= 2
    out = [("act", 0)]
    for k in range(T * G):
        if k + 1 < T * G:
            out.append(("act", (k + 1) % G))
        out += [("actions", k % G), ("observe", k % G)]
    return out


def order_sequential(G, T):
    """one group runs the whole rollout before the next starts"""
    return [(op, g) for g in range(G) for _ in range(T) for op in ("act", "actions", "observe")]


def order_random(G, T, seed=1234):
    rng = np.random.default_rng(seed)
    left = [3 * T] * G
    out = []
    while any(left):
        g = int(rng.choice([k for k in range(G) if left[k]]))
        out.append((("act", "actions", "observe")[(3 * T - left[g]) % 3], g))
        left[g] -= 1
    return out


ORDERS = dict(lockstep=order_lockstep, pipeline=order_pipeline, sequential=order_sequential, random=order_random)


class ShardEnvs:
    """One device-env context per group, each a shard of the global batch of N envs."""

    def __init__(self, P, bounds, fin_groups=(), **cfg):
        N = bounds[-1]
        self.bounds = bounds
        self.ctx = [P.Context(P.make_config(**dict(cfg, num_envs=bounds[g + 1] - bounds[g], env_offset=bounds[g], global_num_envs=N)))
                    for g in range(len(bounds) - 1)]
        self.fin = {g: NumpyFin(bounds[g + 1] - bounds[g]) for g in fin_groups}   # these groups report their finished episodes themselves

    def reset(self):
        return np.concatenate([c.env_reset() for c in self.ctx])

    def step(self, g, t, act):
        obs, rew, done = self.ctx[g].env_step(act)
        if g in self.fin:
            return (obs, rew, done) + self.fin[g].step(rew, done)
        return obs, rew, done

    def close(self):
        for c in self.ctx:
            c.close()


class ReplayEnvs:
    """Transitions drawn once, [T, N, ...] per iteration: any interleaving replays them."""

    def __init__(self, bounds, obs, rew, done):
        self.bounds, self.obs, self.rew, self.done = bounds, obs, rew, done

    def step(self, g, t, act):
        b0, b1 = self.bounds[g], self.bounds[g + 1]
        return self.obs[t, b0:b1], self.rew[t, b0:b1], self.done[t, b0:b1]


def grouped_iteration(b, envs, bounds, order, masks=None, seen=None):
    """masks: None or [T, N, A]; seen: dict that receives the actions [T, N, H] as the group calls returned them"""
    G = len(bounds) - 1
    b.host_rollout_begin(bounds)
    t_of, acts = [0] * G, [None] * G
    for op, g in order:
        b0, b1 = bounds[g], bounds[g + 1]
        if op == "act":
            b.host_group_act(g, None if masks is None else masks[t_of[g], b0:b1])
        elif op == "actions":
            acts[g] = b.host_group_actions(g)
            if seen is not None:
                seen[t_of[g], b0:b1] = acts[g]
        else:
            b.host_group_observe(g, *envs.step(g, t_of[g], acts[g]))
            t_of[g] += 1
    assert t_of == [b.T] * G
    b.host_rollout_end()


def run_against_device(P, env_kind, bounds, T, order="lockstep", iters=3, vector=False, fin_groups=(), params_hook=None, masked=False, **kw):
    N = bounds[-1]
    flags = P.KERNEL_ROLLOUT_VECTOR if vector else 0
    base = dict(num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2, seed=5, total_timesteps=N * T * 5, kernel_flags=flags, **kw)
    if env_kind == P.ENV_MOUNTAINCAR:
        base.update(obs_size=2, head_dims=(3,), dist_kind=P.DIST_MASKED if masked else P.DIST_CATEGORICAL)
    a = P.Context(P.make_config(env_kind=env_kind, **base))
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    envs = ShardEnvs(P, bounds, fin_groups, env_kind=env_kind, **base)
    a.init_orthogonal(11)
    params = a.get_params()
    if params_hook is not None:
        params_hook(params)
    a.set_params(params)
    b.set_params(params)
    obs0 = a.env_reset()
    shard_obs0 = envs.reset()
    assert np.array_equal(bits(obs0), bits(shard_obs0))   # the shards are the global envs' rows
    b.host_env_reset(shard_obs0)
    masks = np.ones((T, N, b.A), np.uint8) if masked else None   # MountainCar::getActionMask: every action valid
    dones = 0
    for it in range(iters):
        a.train_iteration()
        seen = np.full((T, N, b.H), -1, np.int64)
        grouped_iteration(b, envs, bounds, ORDERS[order](len(bounds) - 1, T), masks, seen)
        st = assert_same_state(a, b, tag=(order, it))
        assert np.array_equal(seen, a.read("ACTIONS", (T, N, b.H)).astype(np.int64)), (order, it)
        dones += int(a.read("DONES").sum())
    assert dones > 0   # at least one episode ended: auto-resets and the finished-episode statistics were exercised
    out = (a.profile_read()["vector_fallback_launches"], b.profile_read()["vector_fallback_launches"], st)
    a.close()
    b.close()
    envs.close()
    return out


EIGHT = [0, 12, 24, 36, 48, 60, 72, 84, 96]


@pytest.mark.parametrize("vector", [False, True])
@pytest.mark.parametrize("bounds", [[0, 48, 96], RAGGED, [0, 1, 7], EIGHT], ids=["halves", "ragged", "n7", "eight"])
def test_grouped_cartpole_reproduces_train_iteration(P, bounds, vector):
    fa, fb, st = run_against_device(P, P.ENV_CARTPOLE, bounds, 24, vector=vector, max_episode_steps=20)
    assert fa == fb == 0 and st["updates"] == 3


@pytest.mark.parametrize("vector", [False, True])
@pytest.mark.parametrize("order", ["pipeline", "sequential", "random"])
def test_grouped_cartpole_any_interleaving(P, order, vector):
    """each interleaving on the ragged three-group layout (lockstep is the layout test above)"""
    run_against_device(P, P.ENV_CARTPOLE, RAGGED, 24, order=order, vector=vector, max_episode_steps=20)


@pytest.mark.parametrize("vector", [False, True])
def test_grouped_mountaincar_masked(P, vector):
    run_against_device(P, P.ENV_MOUNTAINCAR, [0, 9, 25, 40], 20, order="pipeline", vector=vector, masked=True, max_episode_steps=25, gamma=0.99,
                       ent_coef=0.01)


def test_grouped_finished_episodes_given_by_one_group_only(P):
    """group 1 passes fin_len / fin_rew (kept in numpy), groups 0 and 2 leave them to the context's running sums, in the same rollout"""
    _, _, st = run_against_device(P, P.ENV_CARTPOLE, [0, 10, 21, 33], 24, order="random", fin_groups=(1,), max_episode_steps=15)
    assert st["ep_count"] > 0


def test_grouped_weights_outside_rollout16_range(P):
    """An actor output weight of 300: the whole grouped rollout takes the vector form, and the fall-back is counted once per ROLLOUT as in the device
    rollout, not once per group."""
    def hook(p):
        p[-130] = 300.0
    fa, fb, _ = run_against_device(P, P.ENV_CARTPOLE, [0, 7, 30, 48], 16, order="pipeline", params_hook=hook, max_episode_steps=12)
    assert fb == fa and fb >= 3


def test_begin_without_groups_is_the_ungrouped_rollout(P):
    """the other door into the same room: host_rollout_begin() and the ungrouped calls still equal A"""
    N, T = 96, 24
    base = dict(num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2, seed=5, total_timesteps=N * T * 5, max_episode_steps=20)
    a = P.Context(P.make_config(**base))
    env = P.Context(P.make_config(**base))
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    a.init_orthogonal(11)
    b.set_params(a.get_params())
    a.env_reset()
    b.host_env_reset(env.env_reset())
    for it in range(3):
        a.train_iteration()
        b.host_rollout_begin()
        for _ in range(T):
            b.host_observe(*env.env_step(b.host_act()))
        b.host_rollout_end()
        assert_same_state(a, b, tag=it)
    for c in (a, b, env):
        c.close()


def test_actions_of_an_earlier_group_survive_a_later_groups_read(P):
    """group_act(0); group_act(1); group_actions(1) first: group_actions(0) still returns group 0's rows, and both are the ungrouped rollout's"""
    N, T = 96, 8
    bounds = [0, 37, 96]
    base = dict(num_envs=N, num_steps=T, num_minibatches=2, update_epochs=1, seed=9, total_timesteps=N * T * 4, max_episode_steps=20)
    env = P.Context(P.make_config(**base))
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    u = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    b.init_orthogonal(2)
    u.set_params(b.get_params())
    obs0 = env.env_reset()
    b.host_env_reset(obs0)
    u.host_env_reset(obs0)
    u.host_rollout_begin()
    want = u.host_act()
    b.host_rollout_begin(bounds)
    b.host_group_act(0)
    b.host_group_act(1)
    got1 = b.host_group_actions(1)
    got0 = b.host_group_actions(0)
    assert got0.shape == (37, 1) and got1.shape == (59, 1)
    assert np.array_equal(got0, want[:37]) and np.array_equal(got1, want[37:])
    for c in (env, b, u):
        c.close()


# ---- generic engine: grouped against ungrouped on the same pre-drawn transitions ----
def run_generic_against_ungrouped(P, bounds, T, order, masked, iters=2, **cfg):
    N = bounds[-1]
    base = dict(num_envs=N, num_steps=T, num_minibatches=2, total_timesteps=N * T * 4, **cfg)
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    u = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    b.init_orthogonal(4)
    u.set_params(b.get_params())
    rng = np.random.default_rng(21)
    O = b.O
    obs0 = rng.standard_normal((N, O)).astype(np.float32)
    b.host_env_reset(obs0)
    u.host_env_reset(obs0)
    dones = 0
    for it in range(iters):
        obs = rng.standard_normal((T, N, O)).astype(np.float32)
        rew = rng.uniform(-1, 1, (T, N)).astype(np.float32)
        done = (rng.random((T, N)) < 0.1).astype(np.int32)
        masks = None
        if masked:
            masks = (rng.random((T, N, b.A)) < 0.7).astype(np.uint8)
            off = 0
            for h in range(b.H):   # every head keeps a valid action
                masks[..., off] = 1
                off += b.cfg.head_dims[h]
        u.host_rollout_begin()
        want = np.empty((T, N, b.H), np.int64)
        for t in range(T):
            want[t] = u.host_act(None if masks is None else masks[t])
            u.host_observe(obs[t], rew[t], done[t])
        u.host_rollout_end()
        seen = np.full((T, N, b.H), -1, np.int64)
        grouped_iteration(b, ReplayEnvs(bounds, obs, rew, done), bounds, ORDERS[order](len(bounds) - 1, T), masks, seen)
        assert np.array_equal(seen, want), (order, it)
        assert_same_state(u, b, tag=(order, it))
        dones += int(done.sum())
    assert dones > 0
    b.close()
    u.close()


@pytest.mark.parametrize("order", ["pipeline", "random"])
def test_grouped_generic_f32(P, order):
    """obs 6, heads (3, 2): the generic engine in f32"""
    run_generic_against_ungrouped(P, [0, 7, 33, 50], 12, order, False, obs_size=6, head_dims=(3, 2), update_epochs=2, seed=3, max_episode_steps=9)


@pytest.mark.parametrize("order", ["pipeline", "random"])
def test_grouped_generic_bf16_masked(P, order):
    """bf16 at configs[4]'s widths (obs 376, 4 x 256, heads (3, 3, 3, 2), masked)"""
    run_generic_against_ungrouped(P, [0, 5, 37, 64], 4, order, True, obs_size=376, head_dims=(3, 3, 3, 2), hidden=256, n_hidden=4,
                                  compute_dtype=P.DTYPE_BF16, dist_kind=P.DIST_MASKED, update_epochs=1, seed=7)


def test_grouped_obs8_reference_network(P):
    """obs 8 with the reference's 2 x 64 network: the reference-shape act kernels in the vector form"""
    run_generic_against_ungrouped(P, [0, 3, 20, 32], 16, "pipeline", False, obs_size=8, head_dims=(4,), update_epochs=2, seed=3)


@pytest.mark.parametrize("vector", [False, True])
def test_grouped_reference_shape_random_masks(P, vector):
    """obs 2, one head of 3, masked, on the reference-shape act kernels with masks that differ from row to row and step to step: a group's mask rows are
    its own (the staged mask is offset by the group's first row on both sides of the host link)"""
    run_generic_against_ungrouped(P, [0, 9, 25, 40], 12, "pipeline", True, obs_size=2, head_dims=(3,), dist_kind=P.DIST_MASKED, update_epochs=2, seed=5,
                                  kernel_flags=P.KERNEL_ROLLOUT_VECTOR if vector else 0)


# ---- batches past a launcher's grid cap or launch threshold, cut into groups that stay under it (tests/test_gpu_beyond_first_trip.py has the caps) ----
def groups_under_whole_over(bounds, cap):
    """the ungrouped call over bounds[-1] rows gives workgroup 0 a second tile, every group's call is one tile per workgroup"""
    assert_past_the_cap(bounds[-1], cap)
    return all(hi - lo <= cap[0] * cap[1] for lo, hi in zip(bounds, bounds[1:]))


def test_grouped_generic_f32_across_the_gemm_threshold(P):
    """obs 6, heads (3, 2), f32, 8320 envs in two groups of 4160: the ungrouped side runs every layer product of ppo_host_act at 8320 rows (gemm_kernel's
    two-workgroup loop, weight planes), each group at 4160 rows (the double-buffered loop) -- the header's promise that env groups reproduce the ungrouped
    rollout bit for bit, at the one launch choice of gen_forward that follows the row count (tests/test_gpu_matmul.py holds the loops to each other on
    plain operands)."""
    bounds = [0, 4160, 8320]
    assert bounds[-1] > DB_MAX_ROWS and all(hi - lo <= DB_MAX_ROWS for lo, hi in zip(bounds, bounds[1:]))
    run_generic_against_ungrouped(P, bounds, 2, "pipeline", False, iters=1, obs_size=6, head_dims=(3, 2), update_epochs=1, seed=3, max_episode_steps=9)


def test_grouped_cat_fused_past_the_grid_cap(P):
    """PPO_KERNEL_CAT_FUSED, obs 17, heads (5, 3, 4), masked, 65 605 envs in groups of 32 768 and 32 837: the ungrouped ppo_host_act is ONE launch of
    cat_act_kernel whose workgroups 0 and 1 walk a second tile (sampled actions, the per-tile OBS / MASKS / DONES stores); the groups' launches stay on the
    first trip and carry their row origin.  ppo_host_rollout_end's critic batch is 3 x 65 605 = 196 815 rows: four trips of gauss_values_kernel."""
    bounds = [0, 32768, 65605]
    assert groups_under_whole_over(bounds, FUSED_CAP)
    assert 3 * bounds[-1] > 3 * FUSED_CAP[0] * FUSED_CAP[1]
    run_generic_against_ungrouped(P, bounds, 2, "pipeline", True, iters=1, obs_size=17, head_dims=(5, 3, 4), dist_kind=P.DIST_MASKED, update_epochs=1, seed=3,
                                  kernel_flags=P.KERNEL_CAT_FUSED)


@pytest.mark.parametrize("case", ["cartpole", "cartpole_vector", "mountaincar_masked", "mountaincar_masked_vector"])
def test_grouped_reference_shape_past_the_grid_cap(P, case):
    """The reference-shape act kernels as ppo_host_act launches them (HOST = true: the row's OBS / MASKS / ACTIONS stores and the commit of the previous
    step in the same launch), ungrouped over more rows than the grid has workgroups against groups under the cap: 65 557 rows of policy_act16_kernel
    (4096 workgroups x 16 rows), 8197 rows of policy_act_kernel under PPO_KERNEL_ROLLOUT_VECTOR (8192 one-row workgroups)."""
    vector = case.endswith("_vector")
    bounds, cap = ([0, 4100, 8197], VECTOR_CAP) if vector else ([0, 32768, 65557], ACT16_CAP)
    assert groups_under_whole_over(bounds, cap)
    masked = case.startswith("mountaincar")
    cfg = dict(obs_size=2, head_dims=(3,), dist_kind=P.DIST_MASKED) if masked else dict(obs_size=4, head_dims=(2,))
    run_generic_against_ungrouped(P, bounds, 2, "pipeline", masked, iters=1, update_epochs=1, seed=5, kernel_flags=P.KERNEL_ROLLOUT_VECTOR if vector else 0, **cfg)


@pytest.mark.parametrize("case", ["cartpole", "cartpole_vector", "mountaincar_masked_vector"])
def test_device_rollout_of_many_envs_against_shard_stepped_groups(P, case):
    """ppo_train_iteration on 65 557 envs (rollout16_kernel: 4098 tiles of 16 envs; the critic batch of 3 x 65 557 rows walks values_mfma_kernel's capped
    grid several times) and, in the vector form, on 8197 envs (rollout2_kernel), against a caller-stepped context whose groups are stepped by shard contexts.
    A time limit of one step ends every episode at once, so the auto-reset and the finished-episode rows of every tile are exercised in T = 2 steps."""
    vector = case.endswith("_vector")
    bounds, cap = ([0, 4100, 8197], VECTOR_CAP) if vector else ([0, 32768, 65557], ACT16_CAP)
    assert groups_under_whole_over(bounds, cap)   # the env counts of test_grouped_reference_shape_past_the_grid_cap (the rollout launches themselves are uncapped)
    if case.startswith("mountaincar"):
        fa, fb, st = run_against_device(P, P.ENV_MOUNTAINCAR, bounds, 2, order="pipeline", iters=1, vector=vector, masked=True, max_episode_steps=1, gamma=0.99,
                                        ent_coef=0.01)
    else:
        fa, fb, st = run_against_device(P, P.ENV_CARTPOLE, bounds, 2, iters=1, vector=vector, max_episode_steps=1)
    assert fa == fb == 0 and st["updates"] == 1 and st["ep_count"] > 0


def test_given_finished_episodes_that_differ_from_the_running_sums(P):
    """Group 1 of three reports finished episodes 1000 steps longer and 1000 richer than the context's running sums would say; groups 0 and 2 report
    nothing.  FIN_LEN / FIN_REW must hold the given numbers on exactly group 1's rows -- the boundary rows on both sides end an episode at step T - 1,
    which only the one commit launch of ppo_host_rollout_end sees -- and everything equals an ungrouped context given the same numbers for every row."""
    bounds, T = RAGGED, 8
    N = bounds[-1]
    base = dict(num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2, seed=5, total_timesteps=N * T * 4)
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    u = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    b.init_orthogonal(4)
    u.set_params(b.get_params())
    rng = np.random.default_rng(8)
    obs0 = rng.uniform(-0.05, 0.05, (N, 4)).astype(np.float32)
    b.host_env_reset(obs0)
    u.host_env_reset(obs0)
    in_g1 = np.zeros(N, bool)
    in_g1[bounds[1]:bounds[2]] = True
    run = NumpyFin(N)   # the running sums as the context keeps them
    for it in range(2):
        obs = rng.uniform(-0.05, 0.05, (T, N, 4)).astype(np.float32)
        rew = rng.uniform(0, 1, (T, N)).astype(np.float32)
        done = (rng.random((T, N)) < 0.15).astype(np.int32)
        done[T - 1, [0, bounds[1] - 1, bounds[1], bounds[2] - 1, bounds[2], N - 1]] = 1
        fin_len, fin_rew = np.zeros((T, N), np.int32), np.zeros((T, N), np.float32)
        for t in range(T):
            fl, fr = run.step(rew[t], done[t])
            d = done[t] != 0
            fin_len[t] = np.where(d & in_g1, fl + 1000, fl)
            fin_rew[t] = np.where(d & in_g1, fr + np.float32(1000), fr).astype(np.float32)
        u.host_rollout_begin()
        for t in range(T):
            u.host_act()
            u.host_observe(obs[t], rew[t], done[t], fin_len[t], fin_rew[t])
        u.host_rollout_end()
        class Given(ReplayEnvs):   # group 1 passes its numbers, the others none
            def step(self, g, t, act):
                out = ReplayEnvs.step(self, g, t, act)
                b0, b1 = self.bounds[g], self.bounds[g + 1]
                return out + (fin_len[t, b0:b1], fin_rew[t, b0:b1]) if g == 1 else out
        grouped_iteration(b, Given(bounds, obs, rew, done), bounds, order_random(3, T, seed=77 + it))
        assert np.array_equal(b.read("FIN_LEN", (T, N)), fin_len), it
        assert np.array_equal(bits(b.read("FIN_REW", (T, N))), bits(fin_rew)), it
        assert fin_len[T - 1, bounds[1]] > 1000 and 0 < fin_len[T - 1, bounds[1] - 1] < 1000 and 0 < fin_len[T - 1, bounds[2]] < 1000
        st = assert_same_state(u, b, tag=("given", it))
    assert st["ep_count"] > 0 and st["ep_len_mean"] > 100   # the given lengths reached the statistics
    b.close()
    u.close()


# ---- one group of all N rows: the slice where the group calls and the whole-batch calls must be the same rollout ----
def _one_group_cases(P):
    """case -> (device env that steps both sides, or None for pre-drawn transitions; masked; config)"""
    return dict(
        cartpole_mfma=(P.ENV_CARTPOLE, False, dict(max_episode_steps=2)),
        cartpole_vector=(P.ENV_CARTPOLE, False, dict(max_episode_steps=2, kernel_flags=P.KERNEL_ROLLOUT_VECTOR)),
        mountaincar_masked=(P.ENV_MOUNTAINCAR, True, dict(obs_size=2, head_dims=(3,), dist_kind=P.DIST_MASKED, max_episode_steps=2)),
        generic_f32=(None, False, dict(obs_size=6, head_dims=(3, 2))),
        generic_bf16_masked=(None, True, dict(obs_size=376, head_dims=(3, 3, 3, 2), hidden=256, n_hidden=4, compute_dtype=P.DTYPE_BF16,
                                              dist_kind=P.DIST_MASKED)))


@pytest.mark.parametrize("N", [7, 33])   # a partial wave; one wave and a tail
@pytest.mark.parametrize("case", ["cartpole_mfma", "cartpole_vector", "mountaincar_masked", "generic_f32", "generic_bf16_masked"])
def test_one_group_of_all_rows_is_the_ungrouped_rollout(P, case, N):
    """bounds [0, N]: one iteration through the group calls and one through ppo_host_act / ppo_host_observe, from the same parameters and seed, leave
    the same bits in every rollout buffer (ACTIONS, LOGPROBS, OBS, DONES, REWARDS, MASKS among BUFS) and in the parameters after the update"""
    T, bounds = 4, [0, N]
    env_kind, masked, cfg = _one_group_cases(P)[case]
    base = dict(num_envs=N, num_steps=T, num_minibatches=2, update_epochs=1, seed=5, total_timesteps=N * T * 4, **cfg)
    u = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    u.init_orthogonal(4)
    b.set_params(u.get_params())
    rng = np.random.default_rng(31)
    masks = None
    if masked:
        masks = (rng.random((T, N, u.A)) < 0.7).astype(np.uint8)
        off = 0
        for h in range(u.H):   # every head keeps a valid action
            masks[..., off] = 1
            off += u.cfg.head_dims[h]
    if env_kind is None:
        obs0 = rng.standard_normal((N, u.O)).astype(np.float32)
        done = (rng.random((T, N)) < 0.2).astype(np.int32)
        done[1, 0] = 1
        envs = [ReplayEnvs(bounds, rng.standard_normal((T, N, u.O)).astype(np.float32), rng.uniform(-1, 1, (T, N)).astype(np.float32), done)] * 2
    else:
        envs = [ShardEnvs(P, bounds, env_kind=env_kind, **base) for _ in range(2)]   # each side steps envs of its own with its own actions
        obs0 = envs[0].reset()
        assert np.array_equal(bits(obs0), bits(envs[1].reset()))
    u.host_env_reset(obs0)
    b.host_env_reset(obs0)
    u.host_rollout_begin()
    want = np.empty((T, N, u.H), np.int64)
    for t in range(T):
        want[t] = u.host_act(None if masks is None else masks[t])
        u.host_observe(*envs[0].step(0, t, want[t]))
    u.host_rollout_end()
    seen = np.full((T, N, u.H), -1, np.int64)
    grouped_iteration(b, envs[1], bounds, order_lockstep(1, T), masks, seen)
    assert np.array_equal(seen, want), (case, N)
    assert_same_state(u, b, tag=(case, N))
    assert int(u.read("DONES").sum()) > 0   # an episode ended inside the rollout: the commit's reset rows were exercised
    for c in [u, b] + [e for e in envs if isinstance(e, ShardEnvs)]:
        c.close()


# ---- errors: host-side state checks only ----
def test_group_call_errors_leave_the_context_unchanged(P):
    N, T = 16, 8
    bounds = [0, 5, 16]
    base = dict(num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2, seed=5, total_timesteps=N * T * 4, max_episode_steps=6)
    a = P.Context(P.make_config(**base))
    b = P.Context(P.make_config(env_kind=P.ENV_HOST, **base))
    envs = ShardEnvs(P, bounds, **base)
    a.init_orthogonal(3)
    b.set_params(a.get_params())
    L = P.binding.lib()
    STATE, INVALID = 3, 1   # PPO_ERR_STATE, PPO_ERR_INVALID

    def status(fn, *args, **kw):
        with pytest.raises(P.binding.PPOError) as e:
            fn(*args, **kw)
        msg = str(e.value)
        return int(msg.split("status ")[1].split(":")[0]), msg

    z = np.zeros
    p = lambda x: ctypes.c_void_p(x.ctypes.data)
    b2, b10, act_buf = np.array([0, 16], np.int32), np.arange(0, 20, 2, dtype=np.int32), z(N, np.int64)
    fl5, fr5 = z(5, np.int32), z(5, np.float32)
    # device-env contexts: PPO_ERR_STATE
    for fn, args in ((a.host_rollout_begin, ([0, 8, 16],)), (a.host_group_act, (0,)), (a.host_group_actions, (0,)),
                     (a.host_group_observe, (0, z((N, 4)), z(N), z(N)))):
        assert status(fn, *args)[0] == STATE
    a.env_reset()
    b.host_env_reset(envs.reset())
    # no rollout open
    assert status(b.host_group_act, 0)[0] == STATE
    assert status(b.host_group_actions, 0)[0] == STATE
    assert status(b.host_group_observe, 0, z((N, 4)), z(N), z(N))[0] == STATE
    # bad n_groups / bounds / null: PPO_ERR_INVALID, and no rollout is opened by them
    assert L.ppo_host_rollout_begin_groups(b.h, 0, p(b2)) == INVALID
    assert L.ppo_host_rollout_begin_groups(b.h, P.binding.MAX_HOST_GROUPS + 1, p(b10)) == INVALID
    assert L.ppo_host_rollout_begin_groups(b.h, 2, None) == INVALID
    for bad in ([1, 5, 16], [0, 5, 15], [0, 5, 17], [0, 5, 5, 16], [0, 9, 5, 16], [0, 16, 16]):
        assert status(b.host_rollout_begin, bad)[0] == INVALID, bad
    assert status(b.host_group_act, 0)[0] == STATE                            # still no rollout open
    # group calls on a rollout opened without groups
    b.host_rollout_begin()
    assert status(b.host_group_act, 0)[0] == STATE
    assert status(b.host_group_actions, 0)[0] == STATE
    assert status(b.host_group_observe, 0, z((N, 4)), z(N), z(N))[0] == STATE
    assert status(b.host_rollout_begin, bounds)[0] == STATE                   # begin while open
    for t in range(T):   # (take that rollout to its end with the ungrouped calls: one more iteration that must equal A)
        act = b.host_act()
        b.host_observe(*(np.concatenate(x) for x in zip(*(envs.step(g, t, act[bounds[g]:bounds[g + 1]]) for g in range(2)))))
    b.host_rollout_end()
    a.train_iteration()
    assert_same_state(a, b, tag="ungrouped")
    # a grouped rollout
    b.host_rollout_begin(bounds)
    assert status(b.host_rollout_begin, bounds)[0] == STATE                   # begin while open, both doors
    assert status(b.host_rollout_begin)[0] == STATE
    assert status(b.host_env_reset, z((N, 4)))[0] == STATE
    code, msg = status(b.host_act)                                            # the ungrouped calls on a grouped rollout
    assert code == STATE and "group" in msg
    assert status(b.host_observe, z((N, 4)), z(N), z(N))[0] == STATE
    for g in (-1, 2, 8):                                                      # g out of range
        assert status(b.host_group_act, g)[0] == INVALID
        assert L.ppo_host_group_actions(b.h, g, p(act_buf)) == INVALID
        assert status(b.host_group_observe, g, z((N, 4)), z(N), z(N))[0] == INVALID
    assert status(b.host_group_actions, 0)[0] == STATE                        # actions before act
    code, msg = status(b.host_group_observe, 1, z((11, 4)), z(11), z(11))     # observe before act
    assert code == STATE and "group 1" in msg and "step 0" in msg, msg
    assert status(b.host_rollout_end)[0] == STATE                             # end before any step
    b.host_group_act(0)
    code, msg = status(b.host_group_act, 0)                                   # act twice
    assert code == STATE and "group 0" in msg and "step 0" in msg, msg
    assert status(b.host_group_observe, 0, z((5, 4)), z(5), z(5))[0] == STATE     # observe before the actions were read
    assert L.ppo_host_group_actions(b.h, 0, None) == INVALID                  # null pointers
    act0 = b.host_group_actions(0)
    assert status(b.host_group_actions, 0)[0] == STATE                        # actions twice
    o5, r5, d5 = envs.step(0, 0, act0)
    assert L.ppo_host_group_observe(b.h, 0, None, p(r5), p(d5), None, None) == INVALID
    assert L.ppo_host_group_observe(b.h, 0, p(o5), p(r5), p(d5), p(fl5), None) == INVALID   # fin_len without fin_rew
    assert L.ppo_host_group_observe(b.h, 0, p(o5), p(r5), p(d5), None, p(fr5)) == INVALID
    b.host_group_observe(0, o5, r5, d5)
    assert status(b.host_rollout_end)[0] == STATE                             # end before every group is done
    # group 0 to the end of the rollout, group 1 not started
    for t in range(1, T):
        b.host_group_act(0)
        b.host_group_observe(0, *envs.step(0, t, b.host_group_actions(0)))
    code, msg = status(b.host_group_act, 0)                                   # act beyond T
    assert code == STATE and "group 0" in msg, msg
    code, msg = status(b.host_rollout_end)
    assert code == STATE and "group 1" in msg, msg
    for t in range(T):
        b.host_group_act(1)
        b.host_group_observe(1, *envs.step(1, t, b.host_group_actions(1)))
    b.host_rollout_end()
    assert status(b.host_group_act, 0)[0] == STATE                            # the rollout is closed
    a.train_iteration()
    assert_same_state(a, b, tag="grouped")
    # ... and a further plain grouped iteration
    a.train_iteration()
    grouped_iteration(b, envs, bounds, order_pipeline(2, T))
    assert_same_state(a, b, tag="after errors")
    a.close()
    b.close()
    envs.close()
