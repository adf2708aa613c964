"""PPO_ENV_BLACKJACK's surface without a GPU: the header declares the env kind (13, as a sum, in an enum of its own) and states the env -- cards, state, step,
the dealer's bound, reset, observation, the accepted form, the refusals -- the binding and the package mirror it, the facade files and the tools exist, and the
ABI version and the exported set are what they were (the env rides on existing calls).  Fails without the feature: the header has no PPO_ENV_BLACKJACK."""
import ctypes as C
import os
import re
import subprocess

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()


def test_header_declares_the_env_and_states_it(tmp_path):
    assert re.search(r"enum\s*\{\s*PPO_ENV_BLACKJACK\s*=\s*PPO_ENV_TAXI\s*\+\s*5\s*\}", HEADER)
    assert not re.search(r"PPO_ENV_BLACKJACK\w*\s*=\s*\d", HEADER)
    exe = str(tmp_path / "blackjack_enum_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], check=True,
                   input=b'#include <stdio.h>\n#include "ppo_hip.h"\nint main(void) { printf("%d %d %d\\n", (int)PPO_ENV_BLACKJACK, (int)PPO_ENV_FROZENLAKE8X8, '
                         b'(int)PPO_ENV_TAXI); return 0; }\n')
    assert subprocess.check_output([exe]).split() == [b"13", b"11", b"8"]
    assert re.search(r"#define\s+PPO_ABI_VERSION\s+5\b", HEADER)
    # the block stands behind the PPO_ENV_FROZENLAKE8X8 enum line and in front of the distributions' text: nothing of FrozenLake's block moved
    lake_enum = HEADER.index("enum { PPO_ENV_FROZENLAKE8X8 = PPO_ENV_TAXI + 3 }")
    start = HEADER.index("/* PPO_ENV_BLACKJACK (new; value 13)")
    end = HEADER.index("PPO_DIST_CATEGORICAL reproduces", start)
    assert lake_enum < start < HEADER.index("enum { PPO_ENV_BLACKJACK = ") < end
    block = " ".join(HEADER[start:end].replace("\n *", " ").split())   # the comment as running text: a phrase may stand across a line break
    for words in ("natural = False, sab = False", "infinite deck", "THE STATE CARRIES THE RANDOMNESS", "NUMBER OF DRAWS DEPENDS ON THE DATA",
                  "pure function of (state, action)", "card(word) = min(1 + ((uint64(word) * 13) >> 32), 10)", "[1..10, 10, 10, 10]", "probability 4/13",
                  "card(w[i & 3])", "philox4x32_10(key = (k0, k1); counter = (i >> 2, 0, 0, 0x21))", "philox4x32_10(k0, k1, c0, c1, c2, c3)",
                  "tag 0x21 is used by no other draw", "card 2 is the dealer's showing card", "card 3 the dealer's hidden card",
                  "State (hand, n, k0, k1)", "hand = t + 32 * ace + 64 * show", "t in 2..31", "show in 1..10", "(4 after a reset)",
                  "usable = ace && t + 10 <= 21", "sum = t + 10 * usable", "PPO_BUF_ENV_STATE is f32 [4, N]", "clamped into 0..1: 0 stick, 1 hit",
                  "nothing is drawn and the state is unchanged", "c = card n; t += c; ace |= (c == 1); n' = min(n + 1, 2^24 - 1)",
                  "dt = show + card 3", "dt + (dace && dt + 10 <= 21 ? 10 : 0) < 17", "Dealer's score = 0 if dt > 21", "held at 2^24 - 1",
                  "at most 10 cards", "never a `while` on data", "philox4x32_10(seed; e, k, 0, 1)", "k0 = w.x >> 8, k1 = w.y >> 8",
                  "t = card 0 + card 1, ace = either is 1, show = card 2, n = 4", "Global env 0 takes reset 1", "obs_size 45",
                  "Tuple(Discrete(32), Discrete(11), Discrete(2))", "sum at [0..31], 32 + show at [32..42], 43 + usable at [43..44]",
                  "neither n nor the key", "1..16 777 215", "at most 20 steps", "-1, 0 or +1", "PPO_ERR_INVALID and changes nothing", "a NaN becomes 0",
                  "hand into 0..703", "saturated, not truncated",
                  # the accepted form, the launches, the refusals, and why 13
                  "dist_kind = PPO_DIST_CATEGORICAL", "PPO_DIST_MASKED is refused", "head_dims[0] = 2", "obs_size = 45", "hidden = 64",
                  "PPO_KERNEL_CAT_FUSED (required, never implied)", "1 <= max_episode_steps <= 16 777 215", "ppo_env_transition(13, state [n, 4], action i64 [n], ...)",
                  "cat_rollout_kernel", "79 808 bytes", "cat_eval_kernel", "ppo_env_truncation_bootstrap and ppo_env_truncations",
                  "which the stored observation does not hold", "Sharding is neither claimed nor tested", "value 12 stays unassigned"):
        assert words in block, words


def test_binding_and_package_mirror_it():
    P = load_package()
    assert P.ENV_BLACKJACK == 13 == P.binding.ENV_BLACKJACK
    assert (P.ENV_CARTPOLE, P.ENV_MOUNTAINCAR, P.ENV_SYNTHETIC, P.ENV_HOST, P.ENV_PENDULUM, P.ENV_MOUNTAINCAR_CONTINUOUS, P.ENV_ACROBOT, P.ENV_TAXI,
            P.ENV_FROZENLAKE, P.ENV_FROZENLAKE8X8) == (0, 1, 2, 3, 4, 5, 6, 8, 10, 11)
    cfg = P.make_config(env_kind=P.ENV_BLACKJACK, dist_kind=P.DIST_CATEGORICAL, obs_size=45, head_dims=(2,), kernel_flags=P.KERNEL_CAT_FUSED, max_episode_steps=100)
    assert (cfg.env_kind, cfg.dist_kind, cfg.obs_size, cfg.n_heads, cfg.head_dims[0], cfg.kernel_flags, cfg.max_episode_steps) == (13, 0, 45, 1, 2, 256, 100)


def test_abi_version_and_symbols_are_unchanged():
    P = load_package()
    lib = P.binding.lib()
    assert lib.ppo_abi_version() == 5 == P.binding.ABI_VERSION
    assert len(P.binding.ABI_SYMBOLS) == len(set(P.binding.ABI_SYMBOLS)) == 92
    for name in P.binding.ABI_SYMBOLS:
        assert "blackjack" not in name.lower()
    cfg = P.make_config()
    assert cfg.struct_size == C.sizeof(type(cfg))


def test_transition_answers_bad_arguments_with_a_status():
    P = load_package()
    L = P.binding.lib()
    buf = (C.c_float * 8)()
    act = (C.c_int64 * 2)()
    term = (C.c_int32 * 2)()
    # null pointers, a negative count: PPO_ERR_INVALID (1); n = 0: nothing to do.  None of them launches anything.
    assert L.ppo_env_transition(13, None, act, 1, buf, buf, term, None) == 1
    assert L.ppo_env_transition(13, buf, None, 1, buf, buf, term, None) == 1
    assert L.ppo_env_transition(13, buf, act, 1, None, buf, term, None) == 1
    assert L.ppo_env_transition(13, buf, act, -1, buf, buf, term, None) == 1
    assert L.ppo_env_transition(13, buf, act, 0, buf, buf, term, None) == 0
    assert L.ppo_env_transition_f32(13, buf, buf, 0, buf, None, buf, term, None) == 5


def test_facade_files_and_tools_exist():
    host = os.path.join(ROOT, "ppo-libtorch_amd", "host")
    for rel in ("Environments/Blackjack.h", "Environments/Blackjack.cpp", "PPO/PPO_DiscreteBlackjack.h", "tests/host_blackjack_test.cpp"):
        assert os.path.isfile(os.path.join(host, rel)), rel
    mk = open(os.path.join(host, "Makefile")).read()
    assert "host_blackjack_test" in mk and "Environments/Blackjack.cpp" in mk
    hdr = open(os.path.join(host, "PPO", "PPO_DiscreteBlackjack.h")).read()
    assert "PPO_ENV_BLACKJACK" in hdr and "PPO_DIST_CATEGORICAL" in hdr and "fused_categorical" in hdr and "m_action_size = 2" in hdr
    for rel in ("tools/blackjack_cost.py", "tools/blackjack_curve.py"):
        assert os.path.isfile(os.path.join(ROOT, rel)), rel
    readme = open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "blackjack_cost.py" in readme and "blackjack_curve.py" in readme
