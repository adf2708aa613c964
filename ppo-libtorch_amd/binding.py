"""ctypes binding of libppo_hip.so (include/ppo_hip.h) -- the thin host layer tests and bench.py drive.

Pure ctypes + numpy: device memory is allocated through the C-ABI itself (ppo_device_alloc / ppo_memcpy_*), so no
PyTorch is needed on the single-GPU path.  There is NO CPU fallback: if the HIP library is missing or the GPU
cannot be reached, every entry point raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PPO_HIP_LIBRARY: another build of the SAME C-ABI (tools/ab.sh times variant builds side by side without copying over the shipped file);
# it must export every symbol of include/ppo_hip.h like the shipped library or lib() raises
LIB_PATH = os.environ.get("PPO_HIP_LIBRARY") or os.path.join(_HERE, "libppo_hip.so")

MAX_HEADS = 8
ENV_CARTPOLE, ENV_MOUNTAINCAR, ENV_SYNTHETIC, ENV_HOST, ENV_PENDULUM = 0, 1, 2, 3, 4   # ENV_PENDULUM: Pendulum-v1 on the device, DIST_GAUSSIAN + KERNEL_GAUSS_FUSED only
ENV_ACROBOT = 6   # Acrobot-v1 on the device: DIST_CATEGORICAL, heads (3,), obs 6, state [4], KERNEL_CAT_FUSED required; rollout in one launch, evaluate
ENV_TAXI = 8   # Taxi-v3 on the device: DIST_MASKED or DIST_CATEGORICAL, heads (6,), obs 19 (one-hot), state [4], KERNEL_CAT_FUSED required; masks via read("MASKS")
# FrozenLake-v1 / FrozenLake8x8-v1 (slippery) on the device: DIST_CATEGORICAL, heads (4,), obs 16 / 64 (one-hot of the cell), state [4] = (cell, j, k0, k1) -- the
# state carries the key the env's slip is drawn from; KERNEL_CAT_FUSED required
ENV_FROZENLAKE, ENV_FROZENLAKE8X8 = 10, 11
# Blackjack-v1 (infinite deck, natural = False, sab = False) on the device: DIST_CATEGORICAL, heads (2,), obs 45 (three one-hot groups), state [4] = (hand, n, k0,
# k1) with hand = t + 32 * ace + 64 * show -- the state carries the key and the index of the next card; KERNEL_CAT_FUSED required
ENV_BLACKJACK = 13
ENV_MOUNTAINCAR_CONTINUOUS = 5   # MountainCarContinuous-v0 on the device, in the same one form; obs = state [2]; also env_truncation_bootstrap and evaluate
MM_EPI_NONE, MM_EPI_BIAS, MM_EPI_BIAS_TANH, MM_EPI_DTANH = 0, 1, 2, 3
MM_F32X3, MM_BF16 = 0, 1
DIST_CATEGORICAL, DIST_MASKED, DIST_GAUSSIAN = 0, 1, 2   # DIST_GAUSSIAN: f32 actions [.., D], the *_f32 calls (include/ppo_hip.h PPO_DIST_GAUSSIAN)
DTYPE_F32, DTYPE_BF16 = 0, 1
KERNEL_ROLLOUT_VECTOR, KERNEL_UPDATE_VECTOR, KERNEL_UPDATE_ONE_WAVE, KERNEL_COMM_SELFTEST, KERNEL_GENERIC_CLASSIC, KERNEL_GENERIC_SPLIT_HEAD, KERNEL_GAUSS_FUSED, KERNEL_SEPARATE_LAUNCHES = 1, 2, 4, 8, 16, 32, 64, 128   # ppo_config.kernel_flags (include/ppo_hip.h PPO_KERNEL_*)
KERNEL_CAT_FUSED = 256   # categorical / masked policies of a 2 x 64 f32 ENV_HOST context on the fused kernel family (include/ppo_hip.h PPO_KERNEL_CAT_FUSED)
KERNEL_ENV_GENERIC = 512   # ENV_CARTPOLE / ENV_MOUNTAINCAR on a network of any width and depth, f32 or bf16 (include/ppo_hip.h PPO_KERNEL_ENV_GENERIC)
# the fused device envs (ENV_PENDULUM .. ENV_BLACKJACK), next to the env's family flag: the rollout keeps the state a time limit cut an episode off in, and
# env_truncation_bootstrap / env_truncations are served on every one of them (include/ppo_hip.h PPO_KERNEL_ENV_CUT_STATE)
KERNEL_ENV_CUT_STATE = 1024
# the same envs, next to the family flag: reward_norm_enable / reward_norm_get / reward_norm_set are served on their one-launch rollouts (bits 11 and 12 stay
# unassigned; include/ppo_hip.h PPO_KERNEL_ENV_REWARD_NORM)
KERNEL_ENV_REWARD_NORM = 1 << 13
ABI_VERSION = 5
COMM_ID_BYTES = 128
COMM_HANDLE_BYTES = 64

BUF = dict(OBS=0, ACTIONS=1, LOGPROBS=2, REWARDS=3, DONES=4, VALUES=5, MASKS=6, ADVANTAGES=7, RETURNS=8, NEXT_OBS=9,
           NEXT_DONE=10, NEXT_VALUE=11, PARAMS=12, GRADS=13, EXP_AVG=14, EXP_AVG_SQ=15, ENV_STATE=16, EP_LEN=17, EP_REW=18,
           RESET_COUNT=19, PERM=20, FIN_LEN=21, FIN_REW=22)
_BUF_DTYPE = dict(OBS=np.float32, ACTIONS=np.int32, LOGPROBS=np.float32, REWARDS=np.float32, DONES=np.float32,
                  VALUES=np.float32, MASKS=np.uint8, ADVANTAGES=np.float32, RETURNS=np.float32, NEXT_OBS=np.float32,
                  NEXT_DONE=np.int32, NEXT_VALUE=np.float32, PARAMS=np.float32, GRADS=np.float32, EXP_AVG=np.float32,
                  EXP_AVG_SQ=np.float32, ENV_STATE=np.float32, EP_LEN=np.int32, EP_REW=np.float32, RESET_COUNT=np.int32,
                  PERM=np.int32, FIN_LEN=np.int32, FIN_REW=np.float32)

MAX_HOST_GROUPS = 8   # PPO_HOST_MAX_GROUPS

# every symbol include/ppo_hip.h declares (tests/test_abi_symbols.py checks the built library exports exactly these)
ABI_SYMBOLS = [
    "ppo_abi_version", "ppo_ctx_create", "ppo_ctx_destroy", "ppo_last_error", "ppo_sync", "ppo_stream", "ppo_get_config",
    "ppo_buffer", "ppo_device_alloc", "ppo_device_free", "ppo_memcpy_h2d", "ppo_memcpy_d2h", "ppo_param_count",
    "ppo_param_shapes", "ppo_params_init_orthogonal", "ppo_params_set_h", "ppo_params_get_h", "ppo_optimizer_set_h",
    "ppo_optimizer_get_h", "ppo_get_value", "ppo_policy_act", "ppo_categorical", "ppo_categorical_sample", "ppo_matmul", "ppo_env_transition",
    "ppo_cartpole_reset_stream_h", "ppo_env_reset", "ppo_env_step", "ppo_env_set_state_h", "ppo_env_get_state_h",
    "ppo_rollout", "ppo_calc_advantage", "ppo_gae", "ppo_gae_fast", "ppo_nstep_returns", "ppo_generate_permutations",
    "ppo_minibatch_forward_backward", "ppo_allreduce_grads", "ppo_optimizer_step", "ppo_update", "ppo_train_iteration",
    "ppo_read_stats", "ppo_set_learning_rate", "ppo_profile_enable", "ppo_profile_read", "ppo_comm_unique_id", "ppo_comm_init",
    "ppo_comm_init_local", "ppo_comm_exchange_handle", "ppo_comm_init_exchange", "ppo_comm_exchange_timeouts",
    "ppo_comm_set_wait_limit", "ppo_stats_snapshot", "ppo_stats_snapshot_read",
    "ppo_host_env_reset", "ppo_host_rollout_begin", "ppo_host_act", "ppo_host_observe", "ppo_host_rollout_end",
    "ppo_host_rollout_begin_groups", "ppo_host_group_act", "ppo_host_group_actions", "ppo_host_group_observe",
    "ppo_policy_act_greedy", "ppo_evaluate",
    "ppo_host_observe_truncated", "ppo_host_group_observe_truncated", "ppo_host_truncations", "ppo_bootstrap_rewards",
    "ppo_dev_env_reset", "ppo_dev_act", "ppo_dev_observe",
    "ppo_obs_norm_enable", "ppo_obs_norm_get_h", "ppo_obs_norm_set_h", "ppo_obs_norm_apply",
    "ppo_reward_norm_enable", "ppo_reward_norm_get_h", "ppo_reward_norm_set_h",
    "ppo_env_truncation_bootstrap", "ppo_env_truncations",
    "ppo_host_act_f32", "ppo_dev_act_f32", "ppo_policy_act_f32", "ppo_gaussian",
    "ppo_target_kl_set", "ppo_target_kl_get", "ppo_early_stop_read",
    "ppo_gauss_fused_launches",
    "ppo_rollout_f32", "ppo_env_step_f32", "ppo_env_transition_f32",
]


class Config(C.Structure):
    """ppo_config: the m_* hyper-parameters of PPO_Discrete (reference PPO/PPO_Discrete.h:52-85)."""
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("env_kind", C.c_int32), ("dist_kind", C.c_int32),
                ("obs_size", C.c_int32), ("n_heads", C.c_int32), ("head_dims", C.c_int32 * MAX_HEADS), ("hidden", C.c_int32),
                ("n_hidden", C.c_int32), ("num_envs", C.c_int32), ("num_steps", C.c_int32), ("num_minibatches", C.c_int32),
                ("update_epochs", C.c_int32), ("max_episode_steps", C.c_int32), ("use_gae", C.c_int32), ("norm_adv", C.c_int32),
                ("clip_vloss", C.c_int32), ("anneal_lr", C.c_int32), ("seed", C.c_int64), ("total_timesteps", C.c_int64),
                ("env_offset", C.c_int64), ("global_num_envs", C.c_int64), ("learning_rate", C.c_float), ("gamma", C.c_float),
                ("gae_lambda", C.c_float), ("clip_coef", C.c_float), ("ent_coef", C.c_float), ("vf_coef", C.c_float),
                ("max_grad_norm", C.c_float), ("compute_dtype", C.c_int32), ("kernel_flags", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("pg_loss", C.c_double), ("v_loss", C.c_double), ("entropy_loss", C.c_double), ("approx_kl", C.c_double),
                ("loss", C.c_double), ("clipfrac_last", C.c_double), ("clipfrac_mean", C.c_double), ("total_norm", C.c_double),
                ("explained_variance", C.c_double), ("learning_rate", C.c_double), ("ep_len_mean", C.c_double),
                ("ep_rew_mean", C.c_double), ("ep_count", C.c_int64), ("global_step", C.c_int64), ("optimizer_steps", C.c_int64),
                ("updates", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Profile(C.Structure):
    _fields_ = [("fwd_bwd_launches", C.c_int64), ("gae_launches", C.c_int64), ("rollout_launches", C.c_int64),
                ("optimizer_launches", C.c_int64), ("reduce_launches", C.c_int64), ("fwd_bwd_ms", C.c_double), ("gae_ms", C.c_double),
                ("rollout_ms", C.c_double), ("optimizer_ms", C.c_double), ("reduce_ms", C.c_double), ("phase_cycles", C.c_double * 24),
                ("allreduce_launches", C.c_int64), ("allreduce_ms", C.c_double), ("vector_fallback_launches", C.c_int64)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "phase_cycles"}
        d["phase_cycles"] = list(self.phase_cycles)
        return d


class EvalStats(C.Structure):
    """ppo_eval_stats: the summary of one ppo_evaluate run."""
    _fields_ = [("episodes", C.c_int64), ("env_steps", C.c_int64), ("return_mean", C.c_double), ("return_std", C.c_double),
                ("return_min", C.c_double), ("return_max", C.c_double), ("length_mean", C.c_double), ("length_min", C.c_int64),
                ("length_max", C.c_int64), ("truncated", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def make_config(env_kind=ENV_CARTPOLE, dist_kind=DIST_CATEGORICAL, obs_size=4, head_dims=(2,), num_envs=8, num_steps=32,
                num_minibatches=4, update_epochs=10, max_episode_steps=500, use_gae=True, norm_adv=True, clip_vloss=True,
                anneal_lr=True, seed=2, total_timesteps=100000, env_offset=0, global_num_envs=0, learning_rate=1e-3, gamma=0.98,
                gae_lambda=0.95, clip_coef=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, device=0, hidden=64, n_hidden=2,
                compute_dtype=0, kernel_flags=0):
    """Defaults = Environments/CartPoleRecommendedSettings.toml of the reference with action_size = 2."""
    c = Config()
    c.struct_size = C.sizeof(Config)
    c.device, c.env_kind, c.dist_kind, c.obs_size = device, env_kind, dist_kind, obs_size
    c.n_heads = len(head_dims)
    for i, d in enumerate(head_dims):
        c.head_dims[i] = d
    c.hidden, c.n_hidden = hidden, n_hidden
    c.num_envs, c.num_steps, c.num_minibatches, c.update_epochs = num_envs, num_steps, num_minibatches, update_epochs
    c.max_episode_steps = max_episode_steps
    c.use_gae, c.norm_adv, c.clip_vloss, c.anneal_lr = int(use_gae), int(norm_adv), int(clip_vloss), int(anneal_lr)
    c.seed, c.total_timesteps, c.env_offset, c.global_num_envs = seed, total_timesteps, env_offset, global_num_envs
    c.learning_rate, c.gamma, c.gae_lambda, c.clip_coef = learning_rate, gamma, gae_lambda, clip_coef
    c.ent_coef, c.vf_coef, c.max_grad_norm = ent_coef, vf_coef, max_grad_norm
    c.compute_dtype = compute_dtype
    c.kernel_flags = kernel_flags   # KERNEL_*: include/ppo_hip.h PPO_KERNEL_*
    return c


_lib = None


def lib():
    """Loads the HIP library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libppo_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback for the hot path)")
        L = C.CDLL(LIB_PATH)
        L.ppo_last_error.restype = C.c_char_p
        L.ppo_last_error.argtypes = [C.c_void_p]
        L.ppo_stream.restype = C.c_void_p
        L.ppo_param_count.restype = C.c_int64
        L.ppo_ctx_destroy.restype = None
        L.ppo_host_observe_truncated.argtypes = [C.c_void_p] * 8
        L.ppo_host_group_observe_truncated.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7
        L.ppo_host_truncations.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int64]
        L.ppo_bootstrap_rewards.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]
        L.ppo_dev_env_reset.argtypes = [C.c_void_p] * 3
        L.ppo_dev_act.argtypes = [C.c_void_p] * 4
        L.ppo_dev_observe.argtypes = [C.c_void_p] * 9
        L.ppo_obs_norm_enable.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_float]
        L.ppo_obs_norm_get_h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double)]
        L.ppo_obs_norm_set_h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double]
        L.ppo_obs_norm_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.ppo_reward_norm_enable.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_float]
        L.ppo_reward_norm_get_h.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p, C.c_int64]
        L.ppo_reward_norm_set_h.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double]
        L.ppo_env_truncation_bootstrap.argtypes = [C.c_void_p, C.c_int32]
        L.ppo_env_truncations.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int64]
        L.ppo_host_act_f32.argtypes = [C.c_void_p] * 2
        L.ppo_dev_act_f32.argtypes = [C.c_void_p] * 3
        L.ppo_policy_act_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32] + [C.c_void_p] * 4
        L.ppo_gaussian.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 4
        L.ppo_target_kl_set.argtypes = [C.c_void_p, C.c_double]
        L.ppo_target_kl_get.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.ppo_early_stop_read.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.ppo_gauss_fused_launches.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 3
        L.ppo_rollout_f32.argtypes = [C.c_void_p] * 2
        L.ppo_env_step_f32.argtypes = [C.c_void_p] * 5
        L.ppo_env_transition_f32.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5
        for name in ABI_SYMBOLS:
            getattr(L, name)  # AttributeError if the build lacks a declared symbol
        if L.ppo_abi_version() != ABI_VERSION:
            raise RuntimeError("libppo_hip.so ABI version mismatch")
        _lib = L
    return _lib


class PPOError(RuntimeError):
    pass


def _check(status, ctx=None):
    if status != 0:
        msg = lib().ppo_last_error(ctx)
        raise PPOError("ppo_hip status %d: %s" % (status, msg.decode() if msg else "?"))


class DeviceArray:
    """A typed device allocation made through the C-ABI (freed with the context or explicitly)."""

    def __init__(self, ctx, shape, dtype):
        self.ctx, self.shape, self.dtype = ctx, tuple(int(s) for s in np.atleast_1d(shape)), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        _check(lib().ppo_device_alloc(ctx.h, C.c_size_t(self.nbytes), C.byref(p)), ctx.h)
        self.ptr = C.c_void_p(p.value)
        ctx._arrays.append(self)

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.nbytes == self.nbytes, (host.shape, self.shape)
        _check(lib().ppo_memcpy_h2d(self.ctx.h, self.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(self.nbytes)), self.ctx.h)
        return self

    def download(self):
        out = np.empty(self.shape, self.dtype)
        if self.nbytes:
            _check(lib().ppo_memcpy_d2h(self.ctx.h, out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(self.nbytes)), self.ctx.h)
        return out

    def free(self):
        if self.ptr is not None and self.ctx.h:
            lib().ppo_device_free(self.ctx.h, self.ptr)
        self.ptr = None


class Context:
    """One ppo_ctx: a PPO_Discrete / PPO_MultiDiscrete instance living on one GPU."""

    def __init__(self, cfg):
        self.cfg = cfg
        self._arrays = []
        h = C.c_void_p()
        st = lib().ppo_ctx_create(C.byref(cfg), C.byref(h))
        if st != 0:
            msg = lib().ppo_last_error(None)
            raise PPOError("ppo_ctx_create status %d: %s" % (st, msg.decode() if msg else "?"))
        self.h = h
        self.T, self.N, self.O, self.H = cfg.num_steps, cfg.num_envs, cfg.obs_size, cfg.n_heads
        self.A = sum(cfg.head_dims[i] for i in range(cfg.n_heads))
        self.B = self.T * self.N
        # width of the env state (Pendulum: theta, theta_dot behind 3 observations; Acrobot: two angles and two velocities behind 6; Taxi: 4 integers behind 19;
        # FrozenLake: cell, step count and key behind 16 / 64; Blackjack: hand, card index and key behind 45)
        self.S = 2 if cfg.env_kind == ENV_PENDULUM else (4 if cfg.env_kind in (ENV_ACROBOT, ENV_TAXI, ENV_FROZENLAKE, ENV_FROZENLAKE8X8, ENV_BLACKJACK) else self.O)
        self.P = int(lib().ppo_param_count(self.h))

    def close(self):
        if getattr(self, "h", None):
            for a in self._arrays:
                a.free()
            lib().ppo_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- plumbing
    def dev(self, host, dtype=None):
        host = np.ascontiguousarray(host, dtype=dtype)
        return DeviceArray(self, host.shape, host.dtype).upload(host)

    def empty(self, shape, dtype):
        return DeviceArray(self, shape, dtype)

    def sync(self):
        _check(lib().ppo_sync(self.h), self.h)

    def stream(self):
        return lib().ppo_stream(self.h)

    def buffer_ptr(self, name):
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().ppo_buffer(self.h, BUF[name], C.byref(p), C.byref(n)), self.h)
        return p, n.value

    def _buf_dtype(self, name):
        # a Gaussian context keeps f32 actions [T,N,D] in PPO_BUF_ACTIONS
        return np.float32 if name == "ACTIONS" and self.cfg.dist_kind == DIST_GAUSSIAN else _BUF_DTYPE[name]

    def read(self, name, shape=None):
        p, n = self.buffer_ptr(name)
        out = np.empty(n // np.dtype(self._buf_dtype(name)).itemsize, self._buf_dtype(name))
        _check(lib().ppo_memcpy_d2h(self.h, out.ctypes.data_as(C.c_void_p), p, C.c_size_t(n)), self.h)
        return out.reshape(shape) if shape is not None else out

    def write(self, name, host):
        p, n = self.buffer_ptr(name)
        host = np.ascontiguousarray(host, dtype=self._buf_dtype(name))
        assert host.nbytes == n, (name, host.nbytes, n)
        _check(lib().ppo_memcpy_h2d(self.h, p, host.ctypes.data_as(C.c_void_p), C.c_size_t(n)), self.h)

    # ---- Agent
    def set_params(self, p):
        p = np.ascontiguousarray(p, np.float32)
        _check(lib().ppo_params_set_h(self.h, p.ctypes.data_as(C.c_void_p), C.c_int64(p.size)), self.h)

    def get_params(self):
        p = np.empty(self.P, np.float32)
        _check(lib().ppo_params_get_h(self.h, p.ctypes.data_as(C.c_void_p), C.c_int64(self.P)), self.h)
        return p

    def init_orthogonal(self, seed):
        _check(lib().ppo_params_init_orthogonal(self.h, C.c_int64(seed)), self.h)

    def param_shapes(self):
        shapes = np.empty((33, 2), np.int64)   # up to 2 nets x 8 layers x {weight, bias}, and a Gaussian policy's log_std
        n = C.c_int32()
        _check(lib().ppo_param_shapes(self.h, shapes.ctypes.data_as(C.c_void_p), C.byref(n)), self.h)
        return shapes[:n.value]

    def set_optimizer(self, m, v, step):
        m, v = np.ascontiguousarray(m, np.float32), np.ascontiguousarray(v, np.float32)
        _check(lib().ppo_optimizer_set_h(self.h, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), C.c_int64(m.size),
                                         C.c_int64(step)), self.h)

    def get_optimizer(self):
        m, v = np.empty(self.P, np.float32), np.empty(self.P, np.float32)
        step = C.c_int64()
        _check(lib().ppo_optimizer_get_h(self.h, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), C.c_int64(self.P),
                                         C.byref(step)), self.h)
        return m, v, step.value

    def get_value(self, obs):
        """Agent::getValue (reference Agent.cpp:107-109)."""
        obs = np.ascontiguousarray(obs, np.float32).reshape(-1, self.O)
        d_obs, d_v = self.dev(obs), self.empty(obs.shape[0], np.float32)
        _check(lib().ppo_get_value(self.h, d_obs.ptr, C.c_int64(obs.shape[0]), d_v.ptr), self.h)
        return d_v.download()

    def policy_act(self, obs, mask=None, action=None, step_index=0):
        """Agent::getActionAndValueDiscrete / getActionAndValueMasked (reference Agent.cpp:117-170)."""
        obs = np.ascontiguousarray(obs, np.float32).reshape(-1, self.O)
        n = obs.shape[0]
        d_obs = self.dev(obs)
        d_mask = self.dev(mask, np.uint8) if mask is not None else None
        d_forced = self.dev(np.asarray(action).reshape(n, self.H), np.int64) if action is not None else None
        d_a, d_lp, d_en, d_v = self.empty((n, self.H), np.int64), self.empty(n, np.float32), self.empty(n, np.float32), self.empty(n, np.float32)
        _check(lib().ppo_policy_act(self.h, d_obs.ptr, d_mask.ptr if d_mask else None, d_forced.ptr if d_forced else None, C.c_int64(n),
                                    C.c_int64(step_index), d_a.ptr, d_lp.ptr, d_en.ptr, d_v.ptr), self.h)
        return d_a.download(), d_lp.download(), d_en.download(), d_v.download()

    def policy_act_f32(self, obs, action=None, step_index=0, greedy=False):
        """ppo_policy_act_f32 (DIST_GAUSSIAN contexts): action f32 [n,D] forced, or None to sample (greedy: the mean).
        Returns (action f32 [n,D], logprob, entropy, value)."""
        obs = np.ascontiguousarray(obs, np.float32).reshape(-1, self.O)
        n = obs.shape[0]
        tmp = [self.dev(obs)]
        if action is not None:
            tmp.append(self.dev(np.asarray(action, np.float32).reshape(n, self.A)))
        out = [self.empty((n, self.A), np.float32), self.empty(n, np.float32), self.empty(n, np.float32), self.empty(n, np.float32)]
        try:
            _check(lib().ppo_policy_act_f32(self.h, tmp[0].ptr, tmp[1].ptr if action is not None else None, C.c_int64(n), C.c_int64(step_index),
                                            C.c_int32(1 if greedy else 0), *(x.ptr for x in out)), self.h)
            return tuple(x.download() for x in out)
        finally:
            for x in tmp + out:
                x.free()

    def policy_act_greedy(self, obs, mask=None):
        """Categorical::mode through the Agent (reference Categorical.cpp:139-141, Agent.cpp:117-170): the deterministic action per head, with the
        log-prob / entropy / value ppo_policy_act gives for it.  Returns (action i64 [n,H], logprob, entropy, value)."""
        obs = np.ascontiguousarray(obs, np.float32).reshape(-1, self.O)
        n = obs.shape[0]
        d_obs = self.dev(obs)
        d_mask = self.dev(np.asarray(mask).reshape(n, self.A), np.uint8) if mask is not None else None
        d_a, d_lp, d_en, d_v = self.empty((n, self.H), np.int64), self.empty(n, np.float32), self.empty(n, np.float32), self.empty(n, np.float32)
        _check(lib().ppo_policy_act_greedy(self.h, d_obs.ptr, d_mask.ptr if d_mask else None, C.c_int64(n), d_a.ptr, d_lp.ptr, d_en.ptr, d_v.ptr), self.h)
        out = d_a.download(), d_lp.download(), d_en.download(), d_v.download()
        for x in (d_obs, d_mask, d_a, d_lp, d_en, d_v):
            if x is not None:
                x.free()
        return out

    def evaluate(self, n_episodes, seed, greedy=True):
        """ppo_evaluate: n_episodes whole episodes of the context's device env (CartPole, MountainCar, ENV_MOUNTAINCAR_CONTINUOUS) under the current policy in
        one launch.
        Returns (stats dict, returns f32 [n], lengths i32 [n])."""
        n = int(n_episodes)
        d_r = self.empty(max(n, 1), np.float32)
        d_l = self.empty(max(n, 1), np.int32)
        st = EvalStats()
        try:
            _check(lib().ppo_evaluate(self.h, C.c_int64(n), C.c_int64(seed), C.c_int32(1 if greedy else 0), d_r.ptr, d_l.ptr, C.byref(st)), self.h)
            return st.as_dict(), d_r.download()[:n], d_l.download()[:n]
        finally:
            d_r.free()
            d_l.free()

    # ---- Environments
    def env_reset(self):
        """PPO_Discrete::initEnvs (reference PPO_Discrete.cpp:365-402)."""
        _check(lib().ppo_env_reset(self.h), self.h)
        return self.read("NEXT_OBS", (self.N, self.O))

    def env_step(self, action):
        """PPO_Discrete::stepEnvs (reference PPO_Discrete.cpp:413-483)."""
        d_a = self.dev(np.asarray(action).reshape(self.N, self.H), np.int64)
        d_o, d_r, d_d = self.empty((self.N, self.O), np.float32), self.empty(self.N, np.float32), self.empty(self.N, np.int32)
        _check(lib().ppo_env_step(self.h, d_a.ptr, d_o.ptr, d_r.ptr, d_d.ptr), self.h)
        return d_o.download(), d_r.download(), d_d.download()

    def env_step_f32(self, action):
        """ppo_env_step_f32 (ENV_PENDULUM, ENV_MOUNTAINCAR_CONTINUOUS): action f32 [N,D], the raw action (the env clips its own copy).  Returns (obs [N,O], reward [N], done i32 [N])."""
        tmp = [self.dev(np.asarray(action, np.float32).reshape(self.N, self.A)), self.empty((self.N, self.O), np.float32), self.empty(self.N, np.float32),
               self.empty(self.N, np.int32)]
        try:
            _check(lib().ppo_env_step_f32(self.h, *(x.ptr for x in tmp)), self.h)
            return tuple(x.download() for x in tmp[1:])
        finally:
            for x in tmp:
                x.free()

    def env_set_state(self, state=None, ep_len=None, ep_rew=None, reset_count=None):
        def p(a, dt):
            return None if a is None else np.ascontiguousarray(a, dt)
        s, l, r, k = p(state, np.float32), p(ep_len, np.int32), p(ep_rew, np.float32), p(reset_count, np.int32)
        _check(lib().ppo_env_set_state_h(self.h, *(x.ctypes.data_as(C.c_void_p) if x is not None else None for x in (s, l, r, k))), self.h)

    def env_get_state(self):
        s, l = np.empty((self.N, self.S), np.float32), np.empty(self.N, np.int32)
        r, k = np.empty(self.N, np.float32), np.empty(self.N, np.int32)
        _check(lib().ppo_env_get_state_h(self.h, *(x.ctypes.data_as(C.c_void_p) for x in (s, l, r, k))), self.h)
        return s, l, r, k

    def env_truncation_bootstrap(self, on=True):
        """ppo_env_truncation_bootstrap: with the switch on, a rollout of the context's own env (CartPole, MountainCar, ENV_MOUNTAINCAR_CONTINUOUS) folds gamma * V(final observation)
        into REWARDS where the time limit cut an episode off.  Off by default.  A context created with KERNEL_ENV_CUT_STATE is served on every fused device env
        (ENV_PENDULUM, ENV_ACROBOT, the two ENV_FROZENLAKE kinds and ENV_BLACKJACK too, which refuse the call without the flag): the fold then reads the
        state the rollout kept at each cut-off sample instead of rebuilding it from OBS."""
        _check(lib().ppo_env_truncation_bootstrap(self.h, int(on)), self.h)

    def env_truncations(self):
        """The truncation events of the last rollout: (flat indices t * N + n ascending i32 [K], folded-in values V(final obs) f32 [K])."""
        k = C.c_int64()
        _check(lib().ppo_env_truncations(self.h, C.byref(k), None, None, C.c_int64(0)), self.h)
        idx, val = np.empty(k.value, np.int32), np.empty(k.value, np.float32)
        if k.value:
            _check(lib().ppo_env_truncations(self.h, C.byref(k), idx.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), C.c_int64(idx.size)), self.h)
        return idx, val

    # ---- caller-stepped environments (ENV_HOST contexts: include/ppo_hip.h ppo_host_*)
    def host_env_reset(self, obs):
        """initEnvs for the caller's envs: obs f32 [N,O] = every env's reset observation."""
        obs = np.ascontiguousarray(obs, np.float32).reshape(self.N, self.O)
        _check(lib().ppo_host_env_reset(self.h, obs.ctypes.data_as(C.c_void_p)), self.h)

    def host_rollout_begin(self, groups=None):
        """Opens a rollout.  groups: None = the ungrouped calls (host_act / host_observe); an int G = G equal contiguous env groups (the remainder to the
        last); a sequence = the row boundaries [0, ..., N].  Grouped rollouts are driven by host_group_act / host_group_actions / host_group_observe."""
        if groups is None:
            _check(lib().ppo_host_rollout_begin(self.h), self.h)
            self.host_bounds = None
            return
        if isinstance(groups, (int, np.integer)):
            G = int(groups)
            if G < 1 or G > self.N:
                raise ValueError("groups = %d for %d envs" % (G, self.N))
            bounds = [g * (self.N // G) for g in range(G)] + [self.N]
        else:
            bounds = [int(b) for b in groups]
        b = np.ascontiguousarray(bounds, np.int32)
        _check(lib().ppo_host_rollout_begin_groups(self.h, C.c_int32(len(bounds) - 1), b.ctypes.data_as(C.c_void_p)), self.h)
        self.host_bounds = bounds

    def _group_rows(self, g):
        b = getattr(self, "host_bounds", None)
        if b is None or not 0 <= g < len(b) - 1:
            return self.N   # the library refuses the call; any shape will do
        return b[g + 1] - b[g]

    def host_group_act(self, g, mask=None):
        """Enqueues step t_g of group g (commit of its staged step, act, stores) and returns; mask u8 [n_g,A] or None."""
        n = self._group_rows(g)
        m = np.ascontiguousarray(mask, np.uint8).reshape(n, self.A) if mask is not None else None
        _check(lib().ppo_host_group_act(self.h, C.c_int32(g), m.ctypes.data_as(C.c_void_p) if m is not None else None), self.h)

    def host_group_actions(self, g):
        """Waits for group g's act only and returns its actions i64 [n_g,H]."""
        out = np.empty((self._group_rows(g), self.H), np.int64)
        _check(lib().ppo_host_group_actions(self.h, C.c_int32(g), out.ctypes.data_as(C.c_void_p)), self.h)
        return out

    def host_group_observe(self, g, obs, reward, done, fin_len=None, fin_rew=None, truncated=None, final_obs=None):
        """host_observe for group g's rows (arrays [n_g, ...])."""
        n = self._group_rows(g)
        o = np.ascontiguousarray(obs, np.float32).reshape(n, self.O)
        r = np.ascontiguousarray(reward, np.float32).reshape(n)
        d = np.ascontiguousarray(done, np.int32).reshape(n)
        fl = np.ascontiguousarray(fin_len, np.int32).reshape(n) if fin_len is not None else None
        fr = np.ascontiguousarray(fin_rew, np.float32).reshape(n) if fin_rew is not None else None
        args = [o, r, d, fl, fr]
        fn = lib().ppo_host_group_observe
        if truncated is not None or final_obs is not None:
            fn = lib().ppo_host_group_observe_truncated
            args.append(np.ascontiguousarray(truncated, np.int32).reshape(n) if truncated is not None else None)
            args.append(np.ascontiguousarray(final_obs, np.float32).reshape(n, self.O) if final_obs is not None else None)
        _check(fn(self.h, C.c_int32(g), *(x.ctypes.data_as(C.c_void_p) if x is not None else None for x in args)), self.h)

    def host_act(self, mask=None):
        """Step t of the rollout: returns the sampled actions i64 [N,H] (host)."""
        out = np.empty((self.N, self.H), np.int64)
        m = np.ascontiguousarray(mask, np.uint8).reshape(self.N, self.A) if mask is not None else None
        _check(lib().ppo_host_act(self.h, m.ctypes.data_as(C.c_void_p) if m is not None else None, out.ctypes.data_as(C.c_void_p)), self.h)
        return out

    def host_act_f32(self):
        """Step t of the rollout of a DIST_GAUSSIAN context: the raw samples f32 [N,D] (host); clipping to the env's bounds is the caller's."""
        out = np.empty((self.N, self.A), np.float32)
        _check(lib().ppo_host_act_f32(self.h, out.ctypes.data_as(C.c_void_p)), self.h)
        return out

    def host_observe(self, obs, reward, done, fin_len=None, fin_rew=None, truncated=None, final_obs=None):
        """The caller's envs' outputs for the step just acted on (obs already the reset observation where done; done includes truncation).
        truncated i32 [N] / final_obs f32 [N,O] (ppo_host_observe_truncated): where the episode that ended was cut off by a time limit, and the
        observation it ended on; the rollout's end then bootstraps the value there instead of treating the state as terminal."""
        o = np.ascontiguousarray(obs, np.float32).reshape(self.N, self.O)
        r = np.ascontiguousarray(reward, np.float32).reshape(self.N)
        d = np.ascontiguousarray(done, np.int32).reshape(self.N)
        fl = np.ascontiguousarray(fin_len, np.int32).reshape(self.N) if fin_len is not None else None
        fr = np.ascontiguousarray(fin_rew, np.float32).reshape(self.N) if fin_rew is not None else None
        args = [o, r, d, fl, fr]
        fn = lib().ppo_host_observe
        if truncated is not None or final_obs is not None:
            fn = lib().ppo_host_observe_truncated
            args.append(np.ascontiguousarray(truncated, np.int32).reshape(self.N) if truncated is not None else None)
            args.append(np.ascontiguousarray(final_obs, np.float32).reshape(self.N, self.O) if final_obs is not None else None)
        _check(fn(self.h, *(x.ctypes.data_as(C.c_void_p) if x is not None else None for x in args)), self.h)

    # ---- caller-stepped environments on the device (include/ppo_hip.h ppo_dev_*): every array stays on the GPU, every call only enqueues
    @staticmethod
    def _dev_ptr(a):
        """A device array argument: None, a DeviceArray, an int / c_void_p, or any object with data_ptr() (a torch tensor)."""
        if a is None:
            return None
        if isinstance(a, DeviceArray):
            return a.ptr
        if isinstance(a, C.c_void_p):
            return a
        if hasattr(a, "data_ptr"):
            return C.c_void_p(int(a.data_ptr()))
        return C.c_void_p(int(a))

    def _dev_stream(self, stream):
        """None = the context's own stream (no hand-over events); an int / c_void_p (0 = the null stream); an object with .cuda_stream (torch.cuda.Stream)."""
        if stream is None:
            return C.c_void_p(self.stream())
        if isinstance(stream, C.c_void_p):
            return stream
        return C.c_void_p(int(getattr(stream, "cuda_stream", stream)))

    def dev_env_reset(self, obs, stream=None):
        """initEnvs from a device array: obs f32 [N,O] = every env's reset observation."""
        _check(lib().ppo_dev_env_reset(self.h, self._dev_ptr(obs), self._dev_stream(stream)), self.h)

    def dev_act(self, action, mask=None, stream=None):
        """Step t of the rollout: the sampled actions go to the device array action i64 [N,H], valid for work enqueued on `stream` after the call."""
        _check(lib().ppo_dev_act(self.h, self._dev_ptr(mask), self._dev_ptr(action), self._dev_stream(stream)), self.h)

    def dev_act_f32(self, action, stream=None):
        """dev_act for a DIST_GAUSSIAN context: the raw samples go to the device array action f32 [N,D]."""
        _check(lib().ppo_dev_act_f32(self.h, self._dev_ptr(action), self._dev_stream(stream)), self.h)

    def dev_observe(self, obs, reward, done, fin_len=None, fin_rew=None, truncated=None, final_obs=None, stream=None):
        """The envs' outputs for the step just acted on, as device arrays (obs f32 [N,O], reward f32 [N], done i32 [N], ...), consumed in stream order.
        truncated i32 [N] / final_obs f32 [N,O]: one more launch folds gamma * V(final_obs[n]) into the step's reward where truncated[n] and done[n] are both
        set.  Served on the reference's 2 x 64 shapes (obs 2, 4, 8) and on KERNEL_GAUSS_FUSED / KERNEL_CAT_FUSED contexts (any obs_size up to 64); any other
        network refuses the flags with status 5."""
        _check(lib().ppo_dev_observe(self.h, *(self._dev_ptr(x) for x in (obs, reward, done, fin_len, fin_rew, truncated, final_obs)),
                                     self._dev_stream(stream)), self.h)

    # ---- observation normalisation of caller-stepped envs (include/ppo_hip.h ppo_obs_norm_*)
    def obs_norm_enable(self, mode=1, clip=10.0, eps=1e-8):
        """mode 0 off, 1 update the running statistics with every batch of observations and normalise, 2 normalise with frozen statistics."""
        _check(lib().ppo_obs_norm_enable(self.h, int(mode), float(clip), float(eps)), self.h)

    def obs_norm_get(self):
        """-> (mean f64 [O], var f64 [O], count)"""
        mean, var, count = np.empty(self.O, np.float64), np.empty(self.O, np.float64), C.c_double()
        _check(lib().ppo_obs_norm_get_h(self.h, mean.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p), C.c_int64(self.O), C.byref(count)), self.h)
        return mean, var, count.value

    def obs_norm_set(self, mean, var, count):
        mean, var = np.ascontiguousarray(mean, np.float64).ravel(), np.ascontiguousarray(var, np.float64).ravel()
        if mean.size != var.size:
            raise ValueError("mean has %d entries, var %d" % (mean.size, var.size))
        _check(lib().ppo_obs_norm_set_h(self.h, mean.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p), C.c_int64(mean.size), float(count)), self.h)

    def obs_norm_apply(self, obs, out=None, stream=None):
        """The apply step with the current statistics, no update.  obs: a host array [n,O] (returns the normalised host array) or a device array
        (DeviceArray, pointer, object with data_ptr(): then `out`, default obs itself, receives the result, enqueued on `stream`, and is returned)."""
        if isinstance(obs, np.ndarray):
            host = np.ascontiguousarray(obs, np.float32).reshape(-1, self.O)
            d = self.dev(host)
            try:
                _check(lib().ppo_obs_norm_apply(self.h, d.ptr, C.c_int64(host.shape[0]), d.ptr, self._dev_stream(None)), self.h)
                self.sync()
                return d.download()
            finally:
                d.free()
        if out is None:
            out = obs
        n = getattr(obs, "nbytes", None)
        n = n // (4 * self.O) if n is not None else int(obs.numel()) // self.O
        _check(lib().ppo_obs_norm_apply(self.h, self._dev_ptr(obs), C.c_int64(n), self._dev_ptr(out), self._dev_stream(stream)), self.h)
        return out

    # ---- reward normalisation of caller-stepped envs, and of the fused device envs under KERNEL_ENV_REWARD_NORM (include/ppo_hip.h ppo_reward_norm_*)
    def reward_norm_enable(self, mode=1, clip=10.0, eps=1e-8):
        """mode 0 off, 1 update the running statistics of the discounted return with every step and divide the rewards by its standard deviation,
        2 divide with frozen statistics.  On a fused device env created with KERNEL_ENV_REWARD_NORM the T steps of a rollout are normalised behind its
        one launch, with the bits the per-step path leaves."""
        _check(lib().ppo_reward_norm_enable(self.h, int(mode), float(clip), float(eps)), self.h)

    def reward_norm_get(self, returns=False):
        """-> (mean, var, count), or (mean, var, count, ret f64 [N]) with returns=True"""
        mean, var, count = C.c_double(), C.c_double(), C.c_double()
        ret = np.empty(self.N, np.float64) if returns else None
        _check(lib().ppo_reward_norm_get_h(self.h, C.byref(mean), C.byref(var), C.byref(count), ret.ctypes.data_as(C.c_void_p) if returns else None,
                                           C.c_int64(self.N)), self.h)
        return (mean.value, var.value, count.value, ret) if returns else (mean.value, var.value, count.value)

    def reward_norm_set(self, mean, var, count):
        _check(lib().ppo_reward_norm_set_h(self.h, float(mean), float(var), float(count)), self.h)

    def host_truncations(self):
        """The truncation events of the last closed rollout: (flat indices t * N + n ascending i32 [K], folded-in values V(final obs) f32 [K])."""
        k = C.c_int64()
        _check(lib().ppo_host_truncations(self.h, C.byref(k), None, None, C.c_int64(0)), self.h)
        idx, val = np.empty(k.value, np.int32), np.empty(k.value, np.float32)
        if k.value:
            _check(lib().ppo_host_truncations(self.h, C.byref(k), idx.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), C.c_int64(idx.size)), self.h)
        return idx, val

    def bootstrap_rewards(self, final_obs, index, gamma, rewards, want_values=True):
        """ppo_bootstrap_rewards: rewards[index[k]] += gamma * Critic(final_obs[k]) on the device.  rewards: a PPO_BUF name or a device pointer
        (DeviceArray / c_void_p).  Returns the values f32 [K] (None unless want_values), after waiting for the launch."""
        final_obs = np.ascontiguousarray(final_obs, np.float32).reshape(-1, self.O)
        index = np.ascontiguousarray(index, np.int32).ravel()
        K = index.size
        assert final_obs.shape[0] == K, (final_obs.shape, K)
        ptr = self.buffer_ptr(rewards)[0] if isinstance(rewards, str) else getattr(rewards, "ptr", rewards)
        tmp = [self.dev(final_obs), self.dev(index)] if K else []
        d_v = self.empty(K, np.float32) if want_values and K else None
        try:
            _check(lib().ppo_bootstrap_rewards(self.h, tmp[0].ptr if K else None, tmp[1].ptr if K else None, C.c_int64(K), C.c_float(gamma), ptr,
                                               d_v.ptr if d_v is not None else None), self.h)
            self.sync()
            return (d_v.download() if d_v is not None else np.empty(0, np.float32)) if want_values else None
        finally:
            for x in tmp + ([d_v] if d_v is not None else []):
                x.free()

    def host_rollout_end(self):
        """Values, advantages and the update of the rollout (enqueued)."""
        _check(lib().ppo_host_rollout_end(self.h), self.h)

    # ---- rollout / advantages / update
    def rollout(self, forced_actions=None):
        """ppo_rollout; on a DIST_GAUSSIAN context with forced actions ppo_rollout_f32 (f32 [T,N,D]); an integer array there is passed to ppo_rollout, which
        refuses it."""
        if forced_actions is not None and self.cfg.dist_kind == DIST_GAUSSIAN and np.asarray(forced_actions).dtype.kind == "f":
            d = self.dev(np.asarray(forced_actions, np.float32).reshape(self.T, self.N, self.A))
            try:
                _check(lib().ppo_rollout_f32(self.h, d.ptr), self.h)
            finally:
                d.free()
            return
        d = self.dev(np.asarray(forced_actions).reshape(self.T, self.N, -1), np.int64) if forced_actions is not None else None
        _check(lib().ppo_rollout(self.h, d.ptr if d else None), self.h)

    def calc_advantage(self):
        _check(lib().ppo_calc_advantage(self.h), self.h)
        return self.read("ADVANTAGES", (self.T, self.N)), self.read("RETURNS", (self.T, self.N))

    def generate_permutations(self):
        _check(lib().ppo_generate_permutations(self.h), self.h)
        return self.read("PERM", (self.cfg.update_epochs, self.B))

    def minibatch_forward_backward(self, idx):
        d = self.dev(idx, np.int32)
        _check(lib().ppo_minibatch_forward_backward(self.h, d.ptr, C.c_int64(d.shape[0])), self.h)
        return self.read("GRADS")

    def optimizer_step(self):
        _check(lib().ppo_optimizer_step(self.h), self.h)

    def set_learning_rate(self, lr):
        _check(lib().ppo_set_learning_rate(self.h, C.c_double(lr)), self.h)

    def target_kl_set(self, target_kl):
        """Early stop at a target KL (ppo_hip.h: ppo_target_kl_set): 0 = off; takes effect at the next update."""
        _check(lib().ppo_target_kl_set(self.h, float(target_kl)), self.h)

    def target_kl_get(self):
        out = C.c_double(0.0)
        _check(lib().ppo_target_kl_get(self.h, C.byref(out)), self.h)
        return out.value

    def early_stop(self):
        """The last update's outcome (ppo_early_stop_read); waits for that update only."""
        run, stopped, kl, total = C.c_int32(0), C.c_int32(0), C.c_double(0.0), C.c_int64(0)
        _check(lib().ppo_early_stop_read(self.h, C.byref(run), C.byref(stopped), C.byref(kl), C.byref(total)), self.h)
        return {"epochs_run": run.value, "stopped": stopped.value, "kl_at_stop": kl.value, "epochs_total": total.value}

    def update(self):
        _check(lib().ppo_update(self.h), self.h)

    def train_iteration(self):
        _check(lib().ppo_train_iteration(self.h), self.h)

    def stats(self):
        s = Stats()
        _check(lib().ppo_read_stats(self.h, C.byref(s)), self.h)
        return s.as_dict()

    def stats_snapshot(self):
        """Enqueue a statistics snapshot behind the work enqueued so far (ppo_hip.h); read it later with stats_snapshot_read()."""
        _check(lib().ppo_stats_snapshot(self.h), self.h)

    def stats_snapshot_read(self):
        s = Stats()
        _check(lib().ppo_stats_snapshot_read(self.h, C.byref(s)), self.h)
        return s.as_dict()

    def profile_enable(self, on=1):
        """0 = off, 1 = every instrumented launch, 2 = only the dominant kernel (1 launch in 8) and the GAE scan, 4 = the same with 1 launch in 41."""
        _check(lib().ppo_profile_enable(self.h, C.c_int32(int(on))), self.h)

    def gauss_fused_launches(self):
        """ppo_gauss_fused_launches: (act, value, update) launches of the fused 2 x 64 kernels (KERNEL_GAUSS_FUSED, or KERNEL_CAT_FUSED: cat_fused_launches) since
        creation; (0, 0, 0) with neither flag."""
        a, v, u = C.c_int64(), C.c_int64(), C.c_int64()
        _check(lib().ppo_gauss_fused_launches(self.h, C.byref(a), C.byref(v), C.byref(u)), self.h)
        return a.value, v.value, u.value

    def cat_fused_launches(self):
        """(act, value, update) launches of the KERNEL_CAT_FUSED kernels since creation; (0, 0, 0) without the flag.  The library keeps one set of counters for
        the fused kernel family and ppo_gauss_fused_launches reads it for either flag (the flags exclude each other): this is that call on a flagged context."""
        if not self.cfg.kernel_flags & KERNEL_CAT_FUSED:
            return 0, 0, 0
        return self.gauss_fused_launches()

    def profile_read(self):
        p = Profile()
        _check(lib().ppo_profile_read(self.h, C.byref(p)), self.h)
        return p.as_dict()

    def comm_init(self, unique_id, rank, nranks):
        buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        _check(lib().ppo_comm_init(self.h, buf, C.c_int32(rank), C.c_int32(nranks)), self.h)


def _comm_init_local(self, group_id, rank, nranks):
    _check(lib().ppo_comm_init_local(self.h, C.c_int64(group_id), C.c_int32(rank), C.c_int32(nranks)), self.h)


Context.comm_init_local = _comm_init_local


def _comm_exchange_handle(self):
    """IPC handle of this context's exchange buffer (one-shot direct exchange; ppo_hip.h)."""
    buf = (C.c_char * COMM_HANDLE_BYTES)()
    _check(lib().ppo_comm_exchange_handle(self.h, buf), self.h)
    return bytes(buf)


def _comm_init_exchange(self, handles, rank, nranks):
    blob = b"".join(handles)
    assert len(blob) == nranks * COMM_HANDLE_BYTES
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    _check(lib().ppo_comm_init_exchange(self.h, buf, C.c_int32(rank), C.c_int32(nranks)), self.h)


def _comm_exchange_timeouts(self):
    n = C.c_int32()
    _check(lib().ppo_comm_exchange_timeouts(self.h, C.byref(n)), self.h)
    return n.value


def _comm_set_wait_limit(self, seconds):
    """How long a direct-exchange kernel waits for a peer before it gives up (default 30 s; ppo_hip.h)."""
    _check(lib().ppo_comm_set_wait_limit(self.h, C.c_double(seconds)), self.h)


Context.comm_set_wait_limit = _comm_set_wait_limit
Context.comm_exchange_handle = _comm_exchange_handle
Context.comm_init_exchange = _comm_init_exchange
Context.comm_exchange_timeouts = _comm_exchange_timeouts


def comm_unique_id():
    buf = (C.c_char * COMM_ID_BYTES)()
    st = lib().ppo_comm_unique_id(buf)
    if st != 0:
        raise PPOError("ppo_comm_unique_id failed: %s" % lib().ppo_last_error(None).decode())
    return bytes(buf)


# ---- stateless entry points (need a context only for device memory plumbing)
def gae(ctx, rewards, values, dones, next_value, next_done, gamma, gae_lambda, nstep=False, fast=False):
    """PPO_Discrete::calcAdvantage on caller buffers (reference PPO_Discrete.cpp:274-331).  fast: the associative scan (ppo_gae_fast; not bit-identical)."""
    rewards = np.ascontiguousarray(rewards, np.float32)
    T, N = rewards.shape
    d = [ctx.dev(rewards), ctx.dev(values, np.float32), ctx.dev(dones, np.float32), ctx.dev(np.ravel(next_value), np.float32),
         ctx.dev(np.ravel(next_done), np.int32)]
    adv, ret = ctx.empty((T, N), np.float32), ctx.empty((T, N), np.float32)
    if nstep:
        st = lib().ppo_nstep_returns(*(x.ptr for x in d), C.c_int64(T), C.c_int64(N), C.c_float(gamma), adv.ptr, ret.ptr, C.c_void_p(ctx.stream()))
    else:
        fn = lib().ppo_gae_fast if fast else lib().ppo_gae
        st = fn(*(x.ptr for x in d), C.c_int64(T), C.c_int64(N), C.c_float(gamma), C.c_float(gae_lambda), adv.ptr, ret.ptr, C.c_void_p(ctx.stream()))
    _check(st, ctx.h)
    ctx.sync()
    out = adv.download(), ret.download()
    for x in d + [adv, ret]:
        x.free()
    return out


def gae_launch(ctx, d_rewards, d_values, d_dones, d_next_value, d_next_done, T, N, gamma, gae_lambda, d_adv, d_ret, fast=False):
    """Enqueues the scan on device arrays that already live in HBM (no copies, no synchronisation)."""
    _check((lib().ppo_gae_fast if fast else lib().ppo_gae)(d_rewards.ptr, d_values.ptr, d_dones.ptr, d_next_value.ptr, d_next_done.ptr, C.c_int64(T), C.c_int64(N), C.c_float(gamma),
                         C.c_float(gae_lambda), d_adv.ptr, d_ret.ptr, C.c_void_p(ctx.stream())), ctx.h)


def env_transition(ctx, env_kind, state, action):
    """ppo_env_transition: state f32 [n,S] (S = 4 for ENV_CARTPOLE, ENV_ACROBOT, ENV_TAXI, both ENV_FROZENLAKE kinds and ENV_BLACKJACK, 2 for ENV_MOUNTAINCAR), action i64 [n].  Returns (next_state, reward,
    terminated).  The observation of an ENV_ACROBOT state is what ppo_env_set_state_h leaves in NEXT_OBS."""
    state = np.ascontiguousarray(state, np.float32)
    n, O = state.shape
    d_s, d_a = ctx.dev(state), ctx.dev(np.ravel(action), np.int64)
    d_ns, d_r, d_t = ctx.empty((n, O), np.float32), ctx.empty(n, np.float32), ctx.empty(n, np.int32)
    _check(lib().ppo_env_transition(C.c_int32(env_kind), d_s.ptr, d_a.ptr, C.c_int64(n), d_ns.ptr, d_r.ptr, d_t.ptr, C.c_void_p(ctx.stream())), ctx.h)
    ctx.sync()
    return d_ns.download(), d_r.download(), d_t.download()


def env_transition_f32(ctx, env_kind, state, action, want_obs=True):
    """ppo_env_transition_f32 (ENV_PENDULUM, ENV_MOUNTAINCAR_CONTINUOUS): state f32 [n,2], action f32 [n,1] raw.  Returns (next_state, obs or None, reward,
    terminated); obs is [n,3] for ENV_PENDULUM and [n,2] (the next state) for ENV_MOUNTAINCAR_CONTINUOUS."""
    state = np.ascontiguousarray(state, np.float32)
    n, S = state.shape
    O = 3 if env_kind == ENV_PENDULUM else S
    tmp = [ctx.dev(state), ctx.dev(np.asarray(action, np.float32).reshape(n, -1)), ctx.empty((n, S), np.float32), ctx.empty((n, O), np.float32),
           ctx.empty(n, np.float32), ctx.empty(n, np.int32)]
    try:
        _check(lib().ppo_env_transition_f32(C.c_int32(env_kind), tmp[0].ptr, tmp[1].ptr, C.c_int64(n), tmp[2].ptr, tmp[3].ptr if want_obs else None, tmp[4].ptr,
                                            tmp[5].ptr, C.c_void_p(ctx.stream())), ctx.h)
        ctx.sync()
        return tmp[2].download(), (tmp[3].download() if want_obs else None), tmp[4].download(), tmp[5].download()
    finally:
        for x in tmp:
            x.free()


def categorical(ctx, dist_kind, logits, mask=None, value=None):
    logits = np.ascontiguousarray(logits, np.float32)
    n, A = logits.shape
    d_l = ctx.dev(logits)
    d_m = ctx.dev(mask, np.uint8) if mask is not None else None
    d_v = ctx.dev(np.ravel(value), np.int64) if value is not None else None
    o = dict(m_logits=ctx.empty((n, A), np.float32), m_probs=ctx.empty((n, A), np.float32), log_prob=ctx.empty(n, np.float32),
             entropy=ctx.empty(n, np.float32), mode=ctx.empty(n, np.int64))
    _check(lib().ppo_categorical(C.c_int32(dist_kind), d_l.ptr, d_m.ptr if d_m else None, d_v.ptr if d_v else None, C.c_int64(n), C.c_int32(A),
                                 o["m_logits"].ptr, o["m_probs"].ptr, o["log_prob"].ptr, o["entropy"].ptr, o["mode"].ptr,
                                 C.c_void_p(ctx.stream())), ctx.h)
    ctx.sync()
    return {k: v.download() for k, v in o.items()}


def gaussian(ctx, mean, log_std, value=None, seed=0, row_offset=0, step_index=0):
    """ppo_gaussian: the diagonal Gaussian alone.  mean [n,D], log_std [D]; value [n,D] -> its log-prob, None -> a sample keyed by
    (seed, row_offset + row, step_index, d).  Returns dict(sample, log_prob, entropy)."""
    mean = np.ascontiguousarray(mean, np.float32)
    n, D = mean.shape
    tmp = [ctx.dev(mean), ctx.dev(np.ravel(log_std), np.float32)]
    if value is not None:
        tmp.append(ctx.dev(np.asarray(value, np.float32).reshape(n, D)))
    o = dict(sample=ctx.empty((n, D), np.float32), log_prob=ctx.empty(n, np.float32), entropy=ctx.empty(n, np.float32))
    try:
        _check(lib().ppo_gaussian(tmp[0].ptr, tmp[1].ptr, tmp[2].ptr if value is not None else None, C.c_int64(n), C.c_int32(D), C.c_int64(seed),
                                  C.c_int64(row_offset), C.c_int64(step_index), o["sample"].ptr, o["log_prob"].ptr, o["entropy"].ptr,
                                  C.c_void_p(ctx.stream())), ctx.h)
        ctx.sync()
        return {k: v.download() for k, v in o.items()}
    finally:
        for x in tmp + list(o.values()):
            x.free()


def matmul_launch(ctx, trans_a, trans_b, M, N, K, d_a, lda, d_b, ldb, d_c, ldc, epilogue=MM_EPI_NONE, d_aux=None, ld_aux=0, precision=MM_F32X3):
    """Enqueues ppo_matmul on device arrays (no copies, no synchronisation)."""
    _check(lib().ppo_matmul(C.c_int32(int(trans_a)), C.c_int32(int(trans_b)), C.c_int64(M), C.c_int64(N), C.c_int64(K), d_a.ptr, C.c_int64(lda), d_b.ptr,
                            C.c_int64(ldb), d_c.ptr, C.c_int64(ldc), C.c_int32(epilogue), d_aux.ptr if d_aux is not None else None, C.c_int64(ld_aux),
                            C.c_int32(precision), C.c_void_p(ctx.stream())), ctx.h)


def matmul(ctx, a, b, trans_a=False, trans_b=False, epilogue=MM_EPI_NONE, aux=None, precision=MM_F32X3):
    """c[M, N] = epilogue(sum_k A(m, k) B(n, k)) with A = a or a^T, B = b or b^T as stored (see ppo_matmul in ppo_hip.h)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if trans_a:
        K, M = a.shape
    else:
        M, K = a.shape
    N = b.shape[1] if trans_b else b.shape[0]
    assert (b.shape[0] if trans_b else b.shape[1]) == K
    d_a, d_b, d_c = ctx.dev(a), ctx.dev(b), ctx.empty((M, N), np.float32)
    d_x = ctx.dev(aux, np.float32) if aux is not None else None
    matmul_launch(ctx, trans_a, trans_b, M, N, K, d_a, a.shape[1], d_b, b.shape[1], d_c, N, epilogue, d_x, N if epilogue == MM_EPI_DTANH else 0, precision)
    ctx.sync()
    out = d_c.download()
    for x in (d_a, d_b, d_c) + ((d_x,) if d_x is not None else ()):
        x.free()
    return out


def cartpole_reset_stream(seed, n_resets):
    out = np.empty((n_resets, 4), np.float32)
    st = lib().ppo_cartpole_reset_stream_h(C.c_int64(seed), C.c_int64(n_resets), out.ctypes.data_as(C.c_void_p))
    if st != 0:
        raise PPOError("ppo_cartpole_reset_stream_h failed")
    return out
