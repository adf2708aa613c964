"""Time-limit truncations of caller-stepped environments (include/ppo_hip.h, "Time-limit truncations") without a GPU: the header declares the four
calls, the binding lists them, the scripted env the GPU tests step has both kinds of episode end, and the reward fold is the partial-episode bootstrap:
GAE on r + gamma V(final obs) equals GAE with the bootstrap term written out at the truncations.

Also home of the scripted env (ScriptedEnv) that tests/test_gpu_host_truncation.py drives: action-independent, so every count is known on the CPU.
"""
import inspect
import re
import os

import numpy as np

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ppo_hip.h")
CALLS = ["ppo_host_observe_truncated", "ppo_host_group_observe_truncated", "ppo_host_truncations", "ppo_bootstrap_rewards"]


class Transitions:
    """One rollout of stepEnvs outputs, [T, N, ...]: obs (already the reset observation where done), rew, done, trunc (subset of done) and final (the
    observation the step itself produced: the last one of the episode where done)."""

    def __init__(self, obs, rew, done, trunc, final):
        self.obs, self.rew, self.done, self.trunc, self.final = obs, rew, done, trunc, final

    def events(self):
        """flat indices t * N + n of the truncations, ascending"""
        return np.flatnonzero(self.trunc.ravel()).astype(np.int32)


class ScriptedEnv:
    """Env n, step k (1-based) of its current episode: obs[e] = f32(sin(0.37 n + 0.11 k + 0.5 e + 0.013 episode_no)), reward f32(0.5 + 0.01 n);
    n % 3 == 0 terminates at k == 4 + n % 5, every other env is truncated at k == 5 + n % 4; the reset observation is the k = 0 formula."""

    def __init__(self, N, O):
        self.N, self.O = N, O
        self.n = np.arange(N)
        self.k = np.zeros(N, np.int64)
        self.ep = np.zeros(N, np.int64)

    def _obs(self):
        e = np.arange(self.O)
        return np.sin(0.37 * self.n[:, None] + 0.11 * self.k[:, None] + 0.5 * e[None, :] + 0.013 * self.ep[:, None]).astype(np.float32)

    def reset(self):
        self.k[:] = 0
        return self._obs()

    def step(self):
        """-> next_obs, reward, done, truncated, final_obs"""
        self.k += 1
        final = self._obs()
        term = (self.n % 3 == 0) & (self.k == 4 + self.n % 5)
        trunc = (self.n % 3 != 0) & (self.k == 5 + self.n % 4)
        done = term | trunc
        self.k[done] = 0
        self.ep[done] += 1
        obs = self._obs()   # rows that did not end: k unchanged, the same numbers as final
        rew = (0.5 + 0.01 * self.n).astype(np.float32)
        return obs, rew, done.astype(np.int32), trunc.astype(np.int32), final

    def rollout(self, T):
        steps = [self.step() for _ in range(T)]
        return Transitions(*(np.stack([s[i] for s in steps]) for i in range(5)))


def test_header_declares_the_truncation_calls():
    src = open(HDR).read()
    assert re.search(r"#define PPO_ABI_VERSION 5\b", src)   # additions only
    for name in CALLS:
        assert re.search(r"PPO_API\s+ppo_status\s+%s\s*\(" % name, src), name
    assert "PPO_Discrete.cpp:443-452" in src   # the truncation-as-termination the calls replace


def test_binding_lists_the_truncation_calls():
    P = load_package()
    for name in CALLS:
        assert name in P.binding.ABI_SYMBOLS, name
    for meth in ("host_observe", "host_group_observe"):
        params = inspect.signature(getattr(P.Context, meth)).parameters
        assert "truncated" in params and "final_obs" in params, meth
    assert callable(P.Context.host_truncations) and callable(P.Context.bootstrap_rewards)


def test_scripted_env_has_both_kinds_of_episode_end():
    for N, T in ((33, 24), (7, 24)):
        tr = ScriptedEnv(N, 4).rollout(T)
        K, terminations = int(tr.trunc.sum()), int((tr.done & ~tr.trunc.astype(bool)).sum())
        assert K > 0 and terminations > 0, (N, T, K, terminations)
        assert not (tr.trunc & ~tr.done).any()
        assert len(tr.events()) == K
        # where an episode ended the next observation is the reset one, elsewhere it is the step's own
        same = (tr.obs == tr.final).all(axis=2)
        assert same[tr.done == 0].all() and not same[tr.done != 0].any()


def test_gae_on_folded_rewards_is_the_explicit_bootstrap():
    """5 x 3: delta_t = r_t + gamma V(next) (1 - done_next) - V_t.  At a truncation done_next = 1 cuts the chain and the bootstrap; the explicit form puts
    gamma V(final obs) back into delta_t and leaves the chain cut.  Folding f32(gamma V(final)) into r_t first is the same arithmetic up to the association of
    one sum, so the two agree to the f32 rounding of the scan's own steps."""
    import oracle as O
    rng = np.random.default_rng(5)
    T, N, gamma, lam = 5, 3, np.float32(0.98), np.float32(0.95)
    rew = rng.uniform(0.5, 1.5, (T, N)).astype(np.float32)
    val = rng.standard_normal((T, N)).astype(np.float32)
    nv = rng.standard_normal(N).astype(np.float32)
    done_after = np.zeros((T, N), bool)     # the episode ended with step t
    done_after[1, 0] = done_after[3, 1] = done_after[4, 2] = done_after[2, 2] = True
    trunc = np.zeros((T, N), bool)
    trunc[1, 0] = trunc[4, 2] = True         # one inside the rollout, one at t = T - 1; (3, 1) and (2, 2) are terminations
    v_final = rng.standard_normal((T, N)).astype(np.float32)
    dones = np.zeros((T, N), np.float32)     # m_dones[t]: the episode ended with step t - 1
    dones[1:] = done_after[:-1]
    next_done = done_after[-1].astype(np.int32)
    folded = np.where(trunc, rew + (gamma * v_final).astype(np.float32), rew).astype(np.float32)
    adv, ret = O.gae(folded, val, dones, nv, next_done, float(gamma), float(lam))
    # the explicit form, in f64
    want = np.zeros((T, N))
    last = np.zeros(N)
    for t in reversed(range(T)):
        nonterminal = 1.0 - (next_done if t == T - 1 else dones[t + 1])
        nextv = nv if t == T - 1 else val[t + 1]
        delta = rew[t] + float(gamma) * nextv * nonterminal + np.where(trunc[t], float(gamma) * v_final[t].astype(np.float64), 0.0) - val[t]
        last = delta + float(gamma) * float(lam) * nonterminal * last
        want[t] = last
    # bound from the f32 format: a step of the f32 scan rounds at most 6 times (two products and a sum in delta, its difference, two products and a sum in
    # the chain -- the last product's error scaled by < 1), each by half an ULP of an operand no larger than `top`, and errors pass down the chain scaled by
    # gamma * lambda < 1: T steps * 6 roundings * ulp(top) / 2, plus one such rounding for the fold and one for returns = advantages + values
    top = np.float32(max(np.abs(want).max(), np.abs(want + val).max(), np.abs(folded).max(), np.abs(val).max()))
    bound = (T * 6 + 2) * float(np.spacing(top)) / 2
    assert np.abs(adv - want).max() <= bound, (np.abs(adv - want).max(), bound)
    assert np.abs(ret - (want + val)).max() <= bound, (np.abs(ret - (want + val)).max(), bound)
    # and the fold changes the advantages at and in front of the truncations only
    adv0, _ = O.gae(rew, val, dones, nv, next_done, float(gamma), float(lam))
    changed = adv0.view(np.uint32) != adv.view(np.uint32)
    assert changed[1, 0] and changed[4, 2] and not changed[:, 1].any() and not changed[2:, 0].any() and not changed[:3, 2].any()
