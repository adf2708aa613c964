"""The calls whose status and message are pinned word for word (tests/golden/ctx_create_refusals.json, tests/golden/device_env_refusals.json): the grid of
ppo_ctx_create configs and the context-level refusals of the fused device envs.  tools/record_ctx_create_refusals.py and tools/record_device_env_refusals.py
write the two files from these functions; tests/test_ctx_create_refusals_cpu.py and tests/test_gpu_device_env_refusals.py replay them."""
import itertools

import numpy as np

WORD_MAX = (1 << 24) - 1   # FROZENLAKE_WORD_MAX, BLACKJACK_WORD_MAX


def fused_envs(P):
    """kind -> (name, obs width, state width) of the envs of the fused 2 x 64 family"""
    return {P.ENV_PENDULUM: ("PPO_ENV_PENDULUM", 3, 2), P.ENV_MOUNTAINCAR_CONTINUOUS: ("PPO_ENV_MOUNTAINCAR_CONTINUOUS", 2, 2),
            P.ENV_ACROBOT: ("PPO_ENV_ACROBOT", 6, 4), P.ENV_TAXI: ("PPO_ENV_TAXI", 19, 4), P.ENV_FROZENLAKE: ("PPO_ENV_FROZENLAKE", 16, 4),
            P.ENV_FROZENLAKE8X8: ("PPO_ENV_FROZENLAKE8X8", 64, 4), P.ENV_BLACKJACK: ("PPO_ENV_BLACKJACK", 45, 4)}


def base_configs(P):
    """env_kind 0..14 -> (the kind's accepted form, the upper bound of its max_episode_steps or None); the unassigned kinds take Blackjack's form"""
    cat, masked, gauss = P.DIST_CATEGORICAL, P.DIST_MASKED, P.DIST_GAUSSIAN
    jack = dict(dist_kind=cat, obs_size=45, head_dims=(2,), kernel_flags=P.KERNEL_CAT_FUSED, max_episode_steps=100)
    forms = {
        P.ENV_CARTPOLE: (dict(dist_kind=cat, obs_size=4, head_dims=(2,), kernel_flags=0, max_episode_steps=500), None),
        P.ENV_MOUNTAINCAR: (dict(dist_kind=cat, obs_size=2, head_dims=(3,), kernel_flags=0, max_episode_steps=200), None),
        P.ENV_SYNTHETIC: (dict(dist_kind=cat, obs_size=4, head_dims=(2,), kernel_flags=0, max_episode_steps=500), None),
        P.ENV_HOST: (dict(dist_kind=cat, obs_size=4, head_dims=(2,), kernel_flags=0, max_episode_steps=500), None),
        P.ENV_PENDULUM: (dict(dist_kind=gauss, obs_size=3, head_dims=(1,), kernel_flags=P.KERNEL_GAUSS_FUSED, max_episode_steps=200), 290),
        P.ENV_MOUNTAINCAR_CONTINUOUS: (dict(dist_kind=gauss, obs_size=2, head_dims=(1,), kernel_flags=P.KERNEL_GAUSS_FUSED, max_episode_steps=999), None),
        P.ENV_ACROBOT: (dict(dist_kind=cat, obs_size=6, head_dims=(3,), kernel_flags=P.KERNEL_CAT_FUSED, max_episode_steps=500), None),
        P.ENV_TAXI: (dict(dist_kind=masked, obs_size=19, head_dims=(6,), kernel_flags=P.KERNEL_CAT_FUSED, max_episode_steps=200), None),
        P.ENV_FROZENLAKE: (dict(dist_kind=cat, obs_size=16, head_dims=(4,), kernel_flags=P.KERNEL_CAT_FUSED, max_episode_steps=100), WORD_MAX),
        P.ENV_FROZENLAKE8X8: (dict(dist_kind=cat, obs_size=64, head_dims=(4,), kernel_flags=P.KERNEL_CAT_FUSED, max_episode_steps=200), WORD_MAX),
        P.ENV_BLACKJACK: (jack, WORD_MAX),
    }
    return {k: forms.get(k, (jack, WORD_MAX)) for k in range(15)}


def perturbations(P, base, bound):
    """[(group, label, fields)]: every single change of one config field; two changes of one group exclude each other"""
    width = base["head_dims"][0]
    out = [("dist", "dist%d" % d, dict(dist_kind=d)) for d in (0, 1, 2)]
    out += [("heads", "width%d" % (width + 1), dict(head_dims=(width + 1,))), ("heads", "two_heads", dict(head_dims=(width, width)))]
    out += [("hidden", "hidden32", dict(hidden=32)), ("n_hidden", "n_hidden3", dict(n_hidden=3)), ("dtype", "bf16", dict(compute_dtype=P.DTYPE_BF16))]
    out += [("flags", "flags%d" % f, dict(kernel_flags=f))
            for f in (0, P.KERNEL_GAUSS_FUSED, P.KERNEL_CAT_FUSED, P.KERNEL_ENV_GENERIC, P.KERNEL_GAUSS_FUSED | P.KERNEL_CAT_FUSED)]
    out += [("steps", "steps%d" % s, dict(max_episode_steps=s)) for s in (0, -3) + ((bound + 1,) if bound is not None else ())]
    out += [("obs", "obs%d" % o, dict(obs_size=o)) for o in sorted({base["obs_size"] + 1, 4})]
    return out


def ctx_create_grid(P):
    """(case id, config fields) of the base config of every kind, every single perturbation and every pair of them"""
    for kind, (base, bound) in base_configs(P).items():
        yield "k%d" % kind, dict(base, env_kind=kind)
        ps = perturbations(P, base, bound)
        for _, label, fields in ps:
            yield "k%d %s" % (kind, label), dict(base, env_kind=kind, **fields)
        for (g0, l0, f0), (g1, l1, f1) in itertools.combinations(ps, 2):
            if g0 != g1:
                yield "k%d %s %s" % (kind, l0, l1), dict(base, env_kind=kind, **f0, **f1)


def ctx_create_cases(P):
    """case id -> (status, message) of ppo_ctx_create over the grid.  A refused config is answered before the device is touched; an accepted one ends at
    hipSetDevice with status 2 where there is no GPU, and is a live context, closed at once, where there is one"""
    import ctypes as C
    L = P.binding.lib()
    out = {}
    for case, fields in ctx_create_grid(P):
        cfg = P.make_config(num_envs=8, num_steps=4, num_minibatches=2, update_epochs=1, **fields)
        h = C.c_void_p()
        st = L.ppo_ctx_create(C.byref(cfg), C.byref(h))
        msg = L.ppo_last_error(None)
        if h.value:
            L.ppo_ctx_destroy(h)
        assert case not in out, case
        out[case] = (int(st), msg.decode() if msg else "")
    return out


def by_message(cases, keep=lambda status: True):
    """{case: (status, message)} -> [{status, message, cases}], each distinct answer once"""
    groups = {}
    for case, (st, msg) in cases.items():
        if keep(st):
            groups.setdefault((st, msg), []).append(case)
    return [dict(status=st, message=msg, cases=cs) for (st, msg), cs in groups.items()]


def by_case(recorded):
    return {case: (g["status"], g["message"]) for g in recorded for case in g["cases"]}


# ---- the refusals that need a live context: one context per fused kind, N = 8, T = 4; nothing launches a rollout ----
def _answer(P, call):
    try:
        call()
        return "ok"
    except P.binding.PPOError as e:   # "ppo_hip status <n>: <message>"
        return "PPOError: %s" % e


def _bad_states(name):
    """(label, word index, value): one out-of-range value per state word"""
    if name == "PPO_ENV_TAXI":
        return [("row5", 0, 5), ("col-1", 1, -1), ("pass4.5", 2, 4.5), ("dest4", 3, 4)]
    if name.startswith("PPO_ENV_FROZENLAKE"):
        cells = 64 if name.endswith("8X8") else 16
        return [("cell%d" % cells, 0, cells), ("j-1", 1, -1), ("k0_2^24", 2, WORD_MAX + 1), ("k1_half", 3, 0.5)]
    if name == "PPO_ENV_BLACKJACK":
        return [("hand704", 0, 704), ("hand_t1", 0, 1 + 64), ("hand_show0", 0, 12 + 32), ("n-1", 1, -1), ("k0_2^24", 2, WORD_MAX + 1), ("k1_half", 3, 0.5)]
    return []


def device_env_cases(P):
    """case id -> the answer of each pinned call, on one context per fused kind"""
    out = {}
    N, T = 8, 4
    for kind, (name, obs, state) in fused_envs(P).items():
        base, _ = base_configs(P)[kind]
        ctx = P.Context(P.make_config(env_kind=kind, num_envs=N, num_steps=T, num_minibatches=2, update_epochs=2, seed=5, total_timesteps=4 * N * T, **base))
        try:
            ctx.init_orthogonal(11)
            ctx.env_reset()
            st = ctx.env_get_state()[0]
            out["%s state_shape" % name] = "%s want %s" % (list(st.shape), [N, state])
            out["%s truncation_bootstrap" % name] = _answer(P, lambda: ctx.env_truncation_bootstrap(True))
            out["%s truncations" % name] = _answer(P, ctx.env_truncations)
            if base["dist_kind"] == P.DIST_GAUSSIAN:
                out["%s env_step" % name] = _answer(P, lambda: ctx.env_step(np.zeros((N, 1), np.int64)))
                out["%s rollout_forced_i64" % name] = _answer(P, lambda: ctx.rollout(np.zeros((T, N, 1), np.int64)))
            else:
                out["%s env_step_f32" % name] = _answer(P, lambda: ctx.env_step_f32(np.zeros((N, ctx.A), np.float32)))
            if name == "PPO_ENV_PENDULUM":
                out["%s evaluate" % name] = _answer(P, lambda: ctx.evaluate(4, 3))
            out["%s set_state same" % name] = _answer(P, lambda: ctx.env_set_state(state=st))   # the library and the binding agree on [N, STATE]
            for label, word, value in _bad_states(name):
                bad = st.copy()
                bad[N - 3, word] = value
                out["%s set_state %s" % (name, label)] = _answer(P, lambda: ctx.env_set_state(state=bad))
            assert np.array_equal(ctx.env_get_state()[0], st), "%s: a refused ppo_env_set_state_h changed the state" % name
        finally:
            ctx.close()
    return out
