"""Kernel-argument preloading (gfx940 and later): the leading scalar parameters of a kernel arrive in user SGPRs at wave launch instead of being fetched by
the wave's first s_load from the cold kernel-argument segment.  csrc/Makefile compiles the headline kernels' files with
-amdgpu-kernarg-preload-count=16; a by-value struct parameter is never preloaded, so a kernel's SIGNATURE decides what it gets.  Nothing in the source
guarantees it stays that way (a struct moved to the front, a flag lost from the Makefile): this test reads .amdhsa_user_sgpr_kernarg_preload_length out of
the kernel descriptors of the SHIPPED library and holds it to the dword count of each kernel's leading parameters, and it holds the two optimizer kernels
and the update kernel to what the preload is for: no wait for scalar memory between the entry point and the first global load."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "ppo-libtorch_amd", "libppo_hip.so")
OBJDUMP = os.path.join(LLVM, "llvm-objdump")

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(OBJDUMP)), reason="needs the built library and llvm-objdump")

MAX_PRELOAD = 14   # 16 user SGPRs less the kernel-argument segment pointer

# size in dwords (= alignment in dwords) of a parameter: p pointer, l 64-bit integer, i / f 32-bit integer / float
DWORDS = {"p": 2, "l": 2, "i": 1, "f": 1}

# kernel (substring of the demangled-free symbol: the source name) -> its LEADING parameters, in signature order, up to the first one that no longer fits
# into 14 dwords or is a by-value struct.  Names as in the signatures (csrc/kernels_*.hip).
LEADING = {
    "reduce_grads_sumsq_kernel": [("slab", "p"), ("grads", "p"), ("partial", "p"), ("stat_slab", "p"), ("nb0", "i"), ("nb1", "i"), ("P", "i"),
                                  ("net_off0", "i"), ("net_off1", "i"), ("Pmax", "i")],
    "clip_adamw_sumsq_kernel": [("grads", "p"), ("p_src", "p"), ("m_src", "p"), ("v_src", "p"), ("partial", "p"), ("coef", "p"), ("P", "i")],
    "fwd_bwd_mfma_ws_kernel": [("idx", "p"), ("rec_critic", "p"), ("rec_actor", "p"), ("params", "p"), ("M", "i"), ("nb0", "i"), ("nb1", "i")],
    "fwd_bwd_mfma_kernel": [("idx", "p"), ("rec_critic", "p"), ("rec_actor", "p"), ("params", "p"), ("M", "i"), ("nb0", "i"), ("nb1", "i")],
    "fwd_bwd_kernel": [("idx", "p"), ("rec_critic", "p"), ("rec_actor", "p"), ("params", "p"), ("M", "i"), ("nb0", "i"), ("nb1", "i")],
    "rollout16_kernel": [("params", "p"), ("env_state", "p"), ("ep_len_p", "p"), ("ep_rew_p", "p"), ("reset_count", "p"), ("next_done", "p"), ("N", "i"),
                         ("n_tiles", "i")],
    "values_mfma_kernel": [("P", "p"), ("obs0", "p"), ("n0", "l"), ("out0", "p"), ("obs1", "p"), ("n1", "l"), ("out1", "p")],
    "gae_kernel": [("rewards", "p"), ("values", "p"), ("dones", "p"), ("next_value", "p"), ("next_done", "p"), ("T", "i"), ("N", "i"), ("gamma", "f"),
                   ("lambda", "f")],
    "gae_pipe_kernel": [("rewards", "p"), ("values", "p"), ("dones", "p"), ("next_value", "p"), ("next_done", "p"), ("T", "i"), ("N", "i"),
                        ("gamma", "f"), ("lambda", "f")],
    "pack_records_kernel": [("obs", "p"), ("actions", "p"), ("n_heads", "i"), ("masks", "p"), ("A", "i"), ("logprobs", "p"), ("advantages", "p")],
    "perm_adv_stats_kernel": [("adv", "p"), ("perm", "p"), ("B", "l"), ("MB", "l"), ("n_mb_per_epoch", "i"), ("seed", "l"), ("update_index", "l")],
    "adv_norm_kernel": [("stats", "p"), ("n", "i"), ("per_epoch", "i"), ("B", "l"), ("MB", "l"), ("explicit_M", "l"), ("world", "i"), ("out", "p")],
    "episode_count_kernel": [("fin_len", "p"), ("N", "i"), ("row_counts", "p"), ("group_bits", "p")],
    "episode_push_kernel": [("fin_len", "p"), ("fin_rew", "p"), ("T", "i"), ("N", "i"), ("row_counts", "p"), ("group_bits", "p"), ("ring", "p"),
                            ("step_base", "l")],
}
HEAD_CHAIN = ("reduce_grads_sumsq_kernel", "clip_adamw_sumsq_kernel", "fwd_bwd_mfma_ws_kernel")


def leading_dwords(params):
    """Dwords the parameters occupy at the head of the kernel-argument segment, alignment padding included."""
    off = 0
    for _, t in params:
        n = DWORDS[t]
        off = (off + n - 1) // n * n + n
    return off


def source_name(symbol):
    """_ZN12_GLOBAL__N_123clip_adamw_sumsq_kernelEPKf... -> clip_adamw_sumsq_kernel; _Z15adv_norm_kernelPK7AdvStat... -> adv_norm_kernel."""
    m = re.match(r"^_ZN12_GLOBAL__N_1(\d+)", symbol) or re.match(r"^_Z(\d+)", symbol)
    if not m:
        return symbol
    n = int(m.group(1))
    return symbol[m.end():m.end() + n]


@pytest.fixture(scope="module")
def code_objects():
    """[(descriptors, functions)] of the library's gfx950 code objects: {symbol: preload length}, {symbol: [instruction, ...]}."""
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        lib = os.path.join(tmp, "lib.so")
        shutil.copy(LIB, lib)
        subprocess.run([OBJDUMP, "--offloading", lib], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tmp)
        for co in sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if "amdgcn" in f):
            kd = subprocess.run([OBJDUMP, "-d", "-j", ".rodata", co], check=True, capture_output=True, text=True).stdout
            desc, name = {}, None
            for line in kd.splitlines():
                m = re.match(r"^\.amdhsa_kernel (\S+)", line)
                if m:
                    name = m.group(1)
                m = re.match(r"^\s+\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", line)
                if m and name:
                    desc[name] = int(m.group(1))
            if not any(source_name(s) in LEADING for s in desc):
                continue
            dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
            funcs, name = {}, None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
                if m:
                    name = m.group(1)
                    funcs[name] = []
                    continue
                if name is not None and line.strip():
                    m = re.search(r"//\s*([0-9A-Fa-f]+):", line)
                    funcs[name].append((int(m.group(1), 16) if m else -1, line.split("//")[0].strip()))
            out.append((desc, funcs))
    return out


def test_the_table_counts_dwords_with_alignment():
    assert leading_dwords([("a", "p"), ("n", "i"), ("b", "p")]) == 6          # the int is followed by one dword of padding
    assert leading_dwords(LEADING["clip_adamw_sumsq_kernel"]) == 13
    assert all(leading_dwords(p) <= MAX_PRELOAD for p in LEADING.values())


@pytest.mark.parametrize("kernel", sorted(LEADING))
def test_leading_parameters_are_preloaded(code_objects, kernel):
    want = leading_dwords(LEADING[kernel])
    seen = 0
    for desc, _ in code_objects:
        for sym, got in desc.items():
            if source_name(sym) != kernel:
                continue
            seen += 1
            assert got != 0 and got == want, (sym, got, want)
    assert seen >= 1, "no instantiation of %s in the shipped library" % kernel


def heads(insts, at, entry):
    """Walks from the entry to the first global load on BOTH sides of every branch on the scalar condition code -- how these kernels pick a workgroup's job
    (critic / actor body of the update kernel, gradient / loss-sum workgroup of the reduction) -- so that each body's head is held, not only the one laid out
    first.  Branches on vcc / exec are followed on their fall-through only: their other side SKIPS the head's loads (lanes past the end; the update kernel's
    gradient waves, which request no batch rows and start with the weights, whose offsets are in the struct), it does not lead to another head.
    Returns (paths that reached a global load, the scalar-memory waits met on the way)."""
    seen, todo, ends, waits = set(), [entry], 0, []
    while todo:
        i = todo.pop()
        while i not in seen and i < len(insts):
            seen.add(i)
            addr, t = insts[i]
            op = t.split()[0] if t else ""
            if op.startswith("global_load"):
                ends += 1
                break
            if op == "s_endpgm":
                break
            if op == "s_waitcnt" and "lgkmcnt" in t:
                waits.append("%x: %s" % (addr, t))
                break
            if op == "s_branch" or op.startswith("s_cbranch"):
                off = int(t.split()[1])
                target = at[addr + 4 + 4 * (off - 65536 if off >= 32768 else off)]
                if op == "s_branch":
                    i = target
                    continue
                if op.startswith("s_cbranch_scc"):
                    todo.append(target)
            i += 1
    return ends, waits


@pytest.mark.parametrize("kernel", HEAD_CHAIN)
def test_no_scalar_memory_wait_in_front_of_the_first_global_load(code_objects, kernel):
    """A preloading kernel starts with the compatibility prologue for firmware that does not preload (s_loads of the leading arguments, a wait, a branch,
    padded to 256 bytes); the dispatcher enters it BEHIND that prologue.  From there to the first global load no s_waitcnt may name lgkmcnt: the loads'
    addresses come from the preloaded registers, and what is fetched from the argument struct is waited for behind them.

    fwd_bwd_mfma_ws_kernel holds this by construction: it reads its argument struct through a pointer formed BEHIND the first batch-row loads
    (kernels_update_mfma.hip: mg_args_behind_here).  With the struct's scalar loads hoisted to the entry, the register allocator gave the wave index the dead
    dword of one of them and the wait for that load stood in front of the row load (profiles/NOTES.md, "Kernel-argument preloading")."""
    seen = 0
    for _, funcs in code_objects:
        for sym, insts in funcs.items():
            if source_name(sym) != kernel:
                continue
            seen += 1
            body = [t for _, t in insts]
            at = {a: i for i, (a, _) in enumerate(insts)}
            br = next(i for i, l in enumerate(body[:16]) if l.startswith("s_branch"))
            assert any(l.startswith("s_load_dword") for l in body[:br]), sym
            entry = br + 1
            while body[entry].startswith(("s_nop", "s_code_end")):
                entry += 1
            ends, waits = heads(insts, at, entry)
            assert ends >= (2 if kernel != "clip_adamw_sumsq_kernel" else 1), (sym, ends)   # two kinds of workgroup in the update kernel and in the reduction
            assert waits == [], (sym, waits)
    assert seen >= 1
