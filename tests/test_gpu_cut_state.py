"""PPO_KERNEL_ENV_CUT_STATE (include/ppo_hip.h; ppo-libtorch_amd/csrc/kernels_gauss_fused.hip: the KEEP instantiations of gauss_rollout_kernel / cat_rollout_kernel,
step_episode_keep, cut_state_fold_kernel) on the GPU through the C-ABI: the one-launch rollout of a fused device env keeps the state a time limit cut an episode
off in, and ppo_env_truncation_bootstrap folds the critic's value of that state's observation into the reward -- on the five envs whose observation does not
hold the state too.  Every comparison is exact: bits, or integers.  Without the flag's bit none of the flagged contexts can be created ("unknown bits in
kernel_flags").

Shapes: N = 70 (one full rollout workgroup and a ragged one), T = 7 (490 samples: a ragged second fold workgroup; T is no multiple of a limit of 2 or 3, so
cut-offs fall on different t in consecutive rollouts); three consecutive rollouts per case, so episodes span rollout boundaries and the record holds columns
of earlier rollouts that the fold must not read."""
import numpy as np
import pytest

from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

N, T, SEED, ROLLOUTS = 70, 7, 5, 3
ROLLOUT_BUFS = ("OBS", "DONES", "ACTIONS", "LOGPROBS", "REWARDS", "FIN_LEN", "FIN_REW", "NEXT_OBS", "NEXT_DONE", "VALUES", "NEXT_VALUE", "MASKS")
ENV_BUFS = ("ENV_STATE", "EP_LEN", "EP_REW", "RESET_COUNT")
EPISODE_STATS = ("ep_rew_mean", "ep_len_mean", "ep_count")


@pytest.fixture(scope="module")
def P():
    return load_package()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def envs(P):
    """name -> (env_kind, dist_kind, obs_size, actions, family flag, Gaussian)"""
    g, c = P.KERNEL_GAUSS_FUSED, P.KERNEL_CAT_FUSED
    return {
        "pendulum": (P.ENV_PENDULUM, P.DIST_GAUSSIAN, 3, 1, g, True),
        "mcc": (P.ENV_MOUNTAINCAR_CONTINUOUS, P.DIST_GAUSSIAN, 2, 1, g, True),
        "acrobot": (P.ENV_ACROBOT, P.DIST_CATEGORICAL, 6, 3, c, False),
        "taxi_masked": (P.ENV_TAXI, P.DIST_MASKED, 19, 6, c, False),
        "taxi_categorical": (P.ENV_TAXI, P.DIST_CATEGORICAL, 19, 6, c, False),
        "frozenlake": (P.ENV_FROZENLAKE, P.DIST_CATEGORICAL, 16, 4, c, False),
        "frozenlake8x8": (P.ENV_FROZENLAKE8X8, P.DIST_CATEGORICAL, 64, 4, c, False),
        "blackjack": (P.ENV_BLACKJACK, P.DIST_CATEGORICAL, 45, 2, c, False),
    }


def make_ctx(P, env, max_steps, flagged, params=None, n=N, t=T):
    kind, dist, obs, actions, family, gauss = envs(P)[env]
    cfg = P.make_config(env_kind=kind, dist_kind=dist, obs_size=obs, head_dims=(actions,), num_envs=n, num_steps=t, num_minibatches=2, update_epochs=2,
                        max_episode_steps=max_steps, seed=SEED, total_timesteps=8 * n * t, learning_rate=1e-3, anneal_lr=True, gamma=0.99, gae_lambda=0.95,
                        ent_coef=0.01, kernel_flags=family | (P.KERNEL_ENV_CUT_STATE if flagged else 0))
    ctx = P.Context(cfg)
    if params is None:
        # the flat vector ends with the actor's output layer W3 [A, 64], b3 [A] (and log_std [1] on a Gaussian policy): scaled, so that every action keeps
        # a probability the draws show and the Gaussian's mean moves with the observation
        ctx.init_orthogonal(11)
        params = ctx.get_params()
        if gauss:
            params[-66:-2] *= 30.0
            params[-1] = 0.3
        else:
            params[-(actions * 65):-actions] *= 30.0
    ctx.set_params(params)
    ctx.env_reset()
    return ctx


def read_all(ctx, names=ROLLOUT_BUFS + ENV_BUFS):
    return {k: ctx.read(k) for k in names}


# ---------------------------------------------------------------------------------------------------------
# a. the envs that already fold: the old fold against the new one
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["mcc", "taxi_masked", "taxi_categorical"])
def test_fold_from_the_record_equals_the_fold_from_obs(P, env):
    old = make_ctx(P, env, 3, False)
    new = make_ctx(P, env, 3, True, old.get_params())
    old.env_truncation_bootstrap(True)
    new.env_truncation_bootstrap(True)
    for r in range(ROLLOUTS):
        old.rollout()
        new.rollout()
        a, b = read_all(old), read_all(new)
        for k in a:
            assert same(a[k], b[k]), (r, k)
        (i0, v0), (i1, v1) = old.env_truncations(), new.env_truncations()
        print("rollout %d: %d events" % (r, i0.size))
        assert i0.size > 0 and np.array_equal(i0, i1) and same(v0, v1), r
        assert old.gauss_fused_launches() == new.gauss_fused_launches()
    old.close()
    new.close()


# ---------------------------------------------------------------------------------------------------------
# b. the five new envs against a stepwise replay
# ---------------------------------------------------------------------------------------------------------
def replay_rollout(P, b, env, step0, forced, obs):
    """T x { policy_act(obs, step_index), env_step } on the unflagged context b from the observation `obs`, reading the env's state in front of every step.
    -> per sample: state [T, N, S], action [T, N], reward, done, the episode's length and return behind the step; and the observation behind the last step"""
    gauss = envs(P)[env][5]
    out = {k: [] for k in ("state", "action", "reward", "done", "len", "ret")}
    for t in range(T):
        state, ep_len, ep_rew, _ = b.env_get_state()
        kw = {} if forced is None else {"action": forced[t]}
        if gauss:
            act = b.policy_act_f32(obs, step_index=step0 + t, **kw)[0]
            obs, rew, done = b.env_step_f32(act)
        else:
            mask = None
            if b.cfg.dist_kind == P.DIST_MASKED:
                raise AssertionError("the replayed envs form no mask")
            act = b.policy_act(obs, mask, step_index=step0 + t, **kw)[0]
            obs, rew, done = b.env_step(act)
        for k, v in (("state", state), ("action", act.reshape(N)), ("reward", rew), ("done", done), ("len", ep_len + 1), ("ret", (ep_rew + rew).astype(np.float32))):
            out[k].append(v.copy())
    return {k: np.stack(v) for k, v in out.items()}, obs


def final_observations(P, ctx, scratch, env, state, action):
    """the env's own transition on (state, action): -> (the final observation, terminated)"""
    kind, gauss = envs(P)[env][0], envs(P)[env][5]
    if gauss:
        _, obs, _, term = P.env_transition_f32(ctx, kind, state, action.reshape(-1, 1))
        return obs, term
    ns, _, term = P.env_transition(ctx, kind, state, action)
    rows = np.repeat(ns[:1], scratch.N, axis=0)   # the scratch context has room for every sample of a rollout
    rows[:len(ns)] = ns
    scratch.env_set_state(rows)
    return scratch.read("NEXT_OBS", (scratch.N, scratch.O))[:len(ns)], term


CASES = [("pendulum", 3, False), ("pendulum", 1, False), ("acrobot", 3, False), ("frozenlake", 2, True), ("frozenlake8x8", 2, False), ("blackjack", 1, False),
         ("blackjack", 2, False)]


@pytest.mark.parametrize("env,max_steps,force", CASES, ids=["%s-limit%d%s" % (e, m, "-forced" if f else "") for e, m, f in CASES])
def test_fold_against_a_stepwise_replay(P, env, max_steps, force):
    """REWARDS[i] = f32(r + f32(gamma * V(final observation))) exactly where the limit cut episode i off and the env did not terminate, the raw reward
    elsewhere; the event list is exactly those (i, v); everything else the rollout leaves is the unflagged rollout's."""
    a = make_ctx(P, env, max_steps, True)
    params = a.get_params()
    b = make_ctx(P, env, max_steps, False, params)      # stepped through the API
    plain = make_ctx(P, env, max_steps, False, params)  # the unflagged rollout: the raw buffers and the episode statistics
    scratch = make_ctx(P, env, max_steps, False, params, n=N * T, t=1)
    a.env_truncation_bootstrap(True)
    gamma = np.float32(a.cfg.gamma)
    rng = np.random.default_rng(17)
    n_actions = envs(P)[env][3]
    folded_total = ended_total = 0
    obs = b.read("NEXT_OBS", (N, b.O))   # the reset's; the stepwise calls hand the observation on themselves
    for r in range(ROLLOUTS):
        forced = rng.integers(0, n_actions, (T, N, 1)) if force else None
        a.rollout(forced)
        plain.rollout(forced)
        rep, obs = replay_rollout(P, b, env, r * T, forced, obs)
        got, raw = read_all(a), read_all(plain)
        for k in got:
            if k != "REWARDS":
                assert same(got[k], raw[k]), (r, k)
        assert same(raw["ACTIONS"].reshape(T, N), rep["action"].astype(raw["ACTIONS"].dtype)) and same(raw["REWARDS"].reshape(T, N), rep["reward"]), r
        done = rep["done"] != 0
        fin_len = np.where(done, rep["len"], 0).astype(np.int32)
        assert same(got["FIN_LEN"].reshape(T, N), fin_len) and same(got["FIN_REW"].reshape(T, N), np.where(done, rep["ret"], np.float32(0)).astype(np.float32)), r
        sa, sp = a.stats(), plain.stats()
        assert all(sa[k] == sp[k] for k in EPISODE_STATS), (r, sa, sp)
        # the samples at the limit, their final observation and whether the env itself terminated there
        at = np.flatnonzero(fin_len.reshape(-1) == max_steps)
        fobs, term = final_observations(P, a, scratch, env, rep["state"].reshape(T * N, -1)[at], rep["action"].reshape(-1)[at])
        keep = term == 0
        v = a.get_value(fobs[keep]) if keep.any() else np.empty(0, np.float32)
        want = rep["reward"].reshape(-1).copy()
        want[at[keep]] = (want[at[keep]] + (gamma * v).astype(np.float32)).astype(np.float32)
        assert same(got["REWARDS"], want), (r, np.flatnonzero(bits(got["REWARDS"]) != bits(want))[:8])
        idx, val = a.env_truncations()
        assert np.array_equal(idx, at[keep].astype(np.int32)) and same(val, v), r
        print("%s limit %d rollout %d: %d at the limit, %d folded, %d terminated there" % (env, max_steps, r, at.size, keep.sum(), (~keep).sum()))
        folded_total += int(keep.sum())
        ended_total += int((~keep).sum())
    # an input without the branch cannot pass silently
    assert folded_total > 0
    if env in ("frozenlake", "blackjack"):
        assert ended_total > 0, "no sample reached the limit and terminated on the same step"
    if env == "pendulum":
        assert ended_total == 0
        if max_steps == 1:
            assert folded_total == ROLLOUTS * T * N   # every sample is an event: 256 kept rows in the first fold workgroup, four tiles
    for c in (a, b, plain, scratch):
        c.close()


# ---------------------------------------------------------------------------------------------------------
# c. off is off
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,max_steps", [("pendulum", 3), ("acrobot", 3), ("blackjack", 2)])
def test_off_is_off(P, env, max_steps):
    plain = make_ctx(P, env, max_steps, False)
    params = plain.get_params()
    never, back, on = (make_ctx(P, env, max_steps, True, params) for _ in range(3))
    back.env_truncation_bootstrap(True)
    back.env_truncation_bootstrap(False)
    on.env_truncation_bootstrap(True)
    for r in range(ROLLOUTS):
        for c in (plain, never, back, on):
            c.rollout()
        want = read_all(plain)
        for c in (never, back):
            got = read_all(c)
            for k in want:
                assert same(got[k], want[k]), (r, k)
            assert c.env_truncations()[0].size == 0
            assert c.gauss_fused_launches() == plain.gauss_fused_launches()
        assert on.env_truncations()[0].size > 0
        assert on.gauss_fused_launches() == plain.gauss_fused_launches()   # the fold is none of the counted launches
    # on after off rollouts: the events of the next rollout only (the record holds three rollouts' columns by now)
    never.env_truncation_bootstrap(True)
    never.rollout()
    on.rollout()
    (i0, v0), (i1, v1) = never.env_truncations(), on.env_truncations()
    assert i0.size > 0 and np.array_equal(i0, i1) and same(v0, v1)
    assert (never.read("FIN_LEN")[i0] == max_steps).all() and same(never.read("REWARDS"), on.read("REWARDS"))
    never.env_truncation_bootstrap(False)
    never.rollout()
    assert never.env_truncations()[0].size == 0
    for c in (plain, never, back, on):
        c.close()


# ---------------------------------------------------------------------------------------------------------
# d. the refusals that remain
# ---------------------------------------------------------------------------------------------------------
def test_refusals_that_remain(P):
    ctx = make_ctx(P, "pendulum", 3, True)
    o, r, d = np.zeros((N, 3), np.float32), np.zeros(N, np.float32), np.zeros(N, np.int32)
    d_o, d_r, d_d, d_a = ctx.dev(o), ctx.dev(r), ctx.dev(d), ctx.dev(np.zeros((N, 1), np.float32))
    calls = [
        (5, "ppo_evaluate is not built for PPO_ENV_PENDULUM", lambda: ctx.evaluate(4, 1)),
        (3, "device environment", lambda: ctx.host_env_reset(o)),
        (3, "device environment", lambda: ctx.host_rollout_begin()),
        (3, "device environment", lambda: ctx.host_act_f32()),
        (3, "device environment", lambda: ctx.host_observe(o, r, d)),
        (3, "device environment", lambda: ctx.host_rollout_end()),
        (3, "device environment", lambda: ctx.host_truncations()),
        (3, "device environment", lambda: ctx.dev_env_reset(d_o)),
        (3, "device environment", lambda: ctx.dev_act_f32(d_a)),
        (3, "device environment", lambda: ctx.dev_observe(d_o, d_r, d_d)),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_enable(1)),
        (5, "PPO_ENV_HOST", lambda: ctx.obs_norm_get()),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_enable(1)),
        (5, "PPO_ENV_HOST", lambda: ctx.reward_norm_get()),
        (1, "on must be 0 or 1", lambda: ctx.env_truncation_bootstrap(2)),
    ]
    for status, word, call in calls:
        with pytest.raises(P.binding.PPOError) as e:
            call()
        assert "status %d:" % status in str(e.value) and word in str(e.value), str(e.value)
    ctx.env_truncation_bootstrap(True)
    ctx.rollout()
    assert ctx.env_truncations()[0].size > 0
    ctx.close()
    # the dispatch does not leak: without the flag the pinned refusal stands
    plain = make_ctx(P, "pendulum", 3, False)
    for call in (lambda: plain.env_truncation_bootstrap(True), lambda: plain.env_truncations()):
        with pytest.raises(P.binding.PPOError) as e:
            call()
        assert "status 5:" in str(e.value) and "does not hold theta" in str(e.value), str(e.value)
    plain.close()


def test_ctx_create_refuses_the_flag_elsewhere(P):
    for kw in (dict(), dict(env_kind=P.ENV_MOUNTAINCAR, obs_size=2, head_dims=(3,)), dict(env_kind=P.ENV_HOST), dict(kernel_flags=P.KERNEL_ENV_GENERIC)):
        d = dict(num_envs=8, num_steps=4, kernel_flags=0)
        d.update(kw)
        d["kernel_flags"] |= P.KERNEL_ENV_CUT_STATE
        with pytest.raises(P.binding.PPOError) as e:
            P.Context(P.make_config(**d))
        assert "status 5:" in str(e.value) and "PPO_KERNEL_ENV_CUT_STATE" in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------
# e. one train iteration
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["pendulum", "acrobot"])
def test_train_iteration(P, env):
    ctx = make_ctx(P, env, 3, True)
    ctx.env_truncation_bootstrap(True)
    ctx.train_iteration()
    st = ctx.stats()
    assert all(np.isfinite(st[k]) for k in ("loss", "pg_loss", "v_loss", "explained_variance", "ep_rew_mean")), st
    idx, val = ctx.env_truncations()
    assert idx.size > 0 and np.isfinite(val).all()
    ctx.close()
