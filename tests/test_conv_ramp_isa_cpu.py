"""The ramp of the fp16-pair convolution kernels, read off the shipped ISA (medfusion_amd.build.lint_isa -> csrc/build/lint/conv_f16x2.s): between
the first LDS-DMA instruction and the first barrier of every matrix-kernel instantiation nothing but the kernel's own counted waits may wait for
memory, the kernel argument is not fetched in a chain of dependent scalar round trips, and the main loop holds no SGPR-spill lane moves and no
scratch access.  profiles/ramp_round_trips.txt has the counts of the parent commit next to the ones asserted here."""
import re
from pathlib import Path

import pytest

KERNELS = ("conv_f16x2_kernel", "conv_halo_kernel", "conv_group_kernel")
N_INSTANTIATIONS = 40
# `s_load` -> `s_waitcnt lgkmcnt(0)` pairs on the worst path from the entry to the first DMA.  The largest count over all instantiations of this
# tree -- 1 in the plain and halo kernels (the whole ramp block in one burst), 2 in the grouped ones (the workgroup count `na` that selects
# the body, then that body's burst) -- is an upper bound: a change that brings dependent kernel-argument round trips back fails here.
MAX_SCALAR_WAITS = 2
# the same count in the parent commit (its ISA, same flags): the new count must be lower for every instantiation
PARENT_SCALAR_WAITS = {
    "conv_f16x2_kernel<128,256,2,4,3,1>": 8, "conv_f16x2_kernel<128,256,2,4,3,3>": 11, "conv_f16x2_kernel<256,128,4,2,3,1>": 9, "conv_f16x2_kernel<256,128,4,2,3,3>": 10,
    "conv_f16x2_kernel<128,128,2,4,3,1>": 9, "conv_f16x2_kernel<128,128,2,4,3,3>": 10, "conv_f16x2_kernel<128,128,4,2,3,1>": 8, "conv_f16x2_kernel<128,128,4,2,3,3>": 8,
    "conv_f16x2_kernel<256,64,4,2,3,1>": 9, "conv_f16x2_kernel<256,64,4,2,3,3>": 9, "conv_f16x2_kernel<128,64,4,2,3,1>": 6, "conv_f16x2_kernel<128,64,4,2,3,3>": 6,
    "conv_f16x2_kernel<64,256,1,8,3,1>": 9, "conv_f16x2_kernel<64,256,1,8,3,3>": 10, "conv_f16x2_kernel<128,128,2,2,2,1>": 9, "conv_f16x2_kernel<128,128,2,2,2,3>": 10,
    "conv_f16x2_kernel<128,128,2,2,3,1>": 10, "conv_f16x2_kernel<128,128,2,2,3,3>": 9, "conv_f16x2_kernel<64,128,2,2,3,1>": 9, "conv_f16x2_kernel<64,128,2,2,3,3>": 9,
    "conv_f16x2_kernel<128,64,2,2,3,1>": 10, "conv_f16x2_kernel<128,64,2,2,3,3>": 9, "conv_halo_kernel<256,128,4,2,6,1>": 9, "conv_halo_kernel<256,128,4,2,6,3>": 9,
    "conv_halo_kernel<256,128,4,2,7,1>": 9, "conv_halo_kernel<256,128,4,2,7,3>": 9, "conv_halo_kernel<128,128,2,4,4,1>": 8, "conv_halo_kernel<128,128,2,4,4,3>": 8,
    "conv_halo_kernel<128,128,2,4,5,1>": 8, "conv_halo_kernel<128,128,2,4,5,3>": 8, "conv_group_kernel<64,128,2,2,3,3>": 12, "conv_group_kernel<128,64,2,2,3,64,128,2,2,3,3>": 10,
    "conv_group_kernel<128,128,4,2,3,128,64,4,2,3,3>": 12, "conv_group_kernel<128,128,4,2,3,64,256,1,8,3,3>": 11, "conv_group_kernel<256,128,4,2,7,128,64,4,2,3,3>": 12, "conv_group_kernel<256,128,4,2,7,64,256,1,8,3,3>": 12,
    "conv_group_kernel<128,128,2,4,3,128,64,4,2,3,3>": 11, "conv_group_kernel<128,128,2,4,3,64,256,1,8,3,3>": 11, "conv_group_kernel<128,256,2,4,3,128,64,4,2,3,3>": 11, "conv_group_kernel<128,256,2,4,3,64,256,1,8,3,3>": 11,
}

_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_BRANCH = re.compile(r"^\s*s_c?branch\S*\s+(\.LBB\d+_\d+)")
_INSTR = re.compile(r"^\s+([a-z]\w+)")
_DMA = re.compile(r"^\s*buffer_load_dwordx4\b.*\blds\b")
_NOT_RAMP = ("global_store", "buffer_store", "flat_store", "global_atomic", "buffer_atomic", "flat_atomic", "ds_")
_LANE = re.compile(r"^\s*v_(readlane|writelane)_b32")


def demangled(sym: str) -> str:
    """_ZN4mfc217conv_f16x2_kernelILi128ELi128E...  ->  conv_f16x2_kernel<128,128,...> (group kernels: the two tiles in order)"""
    name = next(k for k in KERNELS if k in sym)
    return name + "<" + ",".join(re.findall(r"Li(\d+)E", sym)) + ">"


def kernel_bodies(text: str) -> dict:
    """symbol -> the lines of its body, for every instantiation of the three matrix kernels"""
    out, cur, sym = {}, None, None
    for ln in text.splitlines():
        if cur is None:
            m = re.match(r"^(_ZN4mfc2\w+):", ln)
            if m and any(k in m.group(1) for k in KERNELS):
                sym, cur = m.group(1), []
        elif ln.startswith(".Lfunc_end"):
            out[sym] = cur
            cur = None
        else:
            cur.append(ln)
    return out


def _own(lines):
    """per line: does it sit between ;;#ASMSTART and ;;#ASMEND (= written in the source, not placed by the compiler)?"""
    own, inside = [], False
    for ln in lines:
        s = ln.strip()
        if s.startswith(";;#ASMSTART"):
            inside = True
        own.append(inside)
        if s.startswith(";;#ASMEND"):
            inside = False
    return own


def _is_instr(ln):
    s = ln.strip()
    return bool(_INSTR.match(ln)) and not s.startswith((";", "."))


def _main_loops(lines):
    """(first, last) line of every main loop: the smallest backward-branch spans that hold matrix instructions, DMA and a barrier -- one per
    convolution body (two in a grouped kernel)"""
    labels = {m.group(1): i for i, ln in enumerate(lines) for m in [_LABEL.match(ln)] if m}
    spans = []
    for i, ln in enumerate(lines):
        m = _BRANCH.match(ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            a = labels[m.group(1)]
            span = lines[a:i + 1]
            if any("v_mfma" in x for x in span) and any(_DMA.match(x) for x in span) and any(x.strip().startswith("s_barrier") for x in span):
                spans.append((a, i))
    return [s for s in spans if not any(t != s and s[0] <= t[0] and t[1] <= s[1] for t in spans)]   # innermost only


def _ramps(lines):
    """(start, first DMA, first barrier) of every convolution body of the kernel (a grouped kernel holds two).  The ramp is the one stretch of a
    body between two barriers (or the kernel's entry / an s_endpgm and a barrier) that issues DMA and no matrix instruction."""
    marks = [-1] + [i for i, ln in enumerate(lines) if ln.strip().startswith(("s_barrier", "s_endpgm"))]
    out = []
    for lo, hi in zip(marks, marks[1:]):
        if not lines[hi].strip().startswith("s_barrier"):
            continue
        seg = range(lo + 1, hi)
        dma = [i for i in seg if _DMA.match(lines[i])]
        if dma and not any("v_mfma" in lines[i] for i in seg):
            out.append((lo + 1, dma[0], hi))
    return out


def _scalar_waits_on_path(lines, first_dma) -> int:
    """The largest number of `s_waitcnt lgkmcnt(0)` that follow at least one s_load (= scalar round trips a wave sits out) on any path from the
    kernel's entry to the DMA instruction at line `first_dma`.  Text order would add up the two bodies of a grouped kernel, whose ramps the
    block placement interleaves; a path belongs to one body.  Blocks are visited in text order over forward edges only (the ramp has no
    loops), and a path does not pass through code that is not ramp: a barrier, a matrix instruction, a store, an LDS access."""
    starts = sorted({0} | {i for i, ln in enumerate(lines) if _LABEL.match(ln)} | {i + 1 for i, ln in enumerate(lines) if _BRANCH.match(ln) or ln.strip().startswith("s_endpgm")})
    starts = [i for i in starts if i < len(lines)]
    block_of = {}
    for k, a in enumerate(starts):
        for i in range(a, starts[k + 1] if k + 1 < len(starts) else len(lines)):
            block_of[i] = k
    labels = {m.group(1): block_of[i] for i, ln in enumerate(lines) for m in [_LABEL.match(ln)] if m}
    best = {(0, False): 0}    # (block, a scalar load is pending) -> waits so far
    target = block_of[first_dma]
    result = None
    for k, a in enumerate(starts):
        end = starts[k + 1] if k + 1 < len(starts) else len(lines)
        for pending in (False, True):
            if (k, pending) not in best:
                continue
            n, pend, ok, succ = best[(k, pending)], pending, True, []
            for i in range(a, end):
                s = lines[i].strip()
                if k == target and i == first_dma:
                    result = n if result is None else max(result, n)
                    ok = False
                    break
                if s.startswith(("s_barrier", "v_mfma") + _NOT_RAMP):
                    ok = False
                    break
                if s.startswith("s_load"):
                    pend = True
                elif s.startswith("s_waitcnt") and "lgkmcnt(0)" in s and pend:
                    n, pend = n + 1, False
                m = _BRANCH.match(lines[i])
                if m:
                    if labels.get(m.group(1), -1) > k:
                        succ.append(labels[m.group(1)])
                    if s.startswith("s_branch"):
                        ok = False      # (no fall-through)
                    break
                if s.startswith("s_endpgm"):
                    ok = False
                    break
            if ok and k + 1 < len(starts):
                succ.append(k + 1)
            for t in succ:
                best[(t, pend)] = max(best.get((t, pend), -1), n)
    assert result is not None, "the first DMA is not reachable from the entry through ramp code"
    return result


def ramp_report(lines) -> dict:
    """the worst body of the kernel for every count"""
    own = _own(lines)
    loops, ramps = _main_loops(lines), _ramps(lines)
    assert loops and ramps, "no main loop / no ramp found"
    rep = dict(bodies=len(ramps), compiler_vm_waits=0, load_then_wait=0, scalar_waits=0, lane_moves=sum(1 for x in lines if _LANE.match(x)),
               lane_moves_loop=sum(1 for a, b in loops for x in lines[a:b + 1] if _LANE.match(x)),
               scratch_loop=sum(1 for a, b in loops for x in lines[a:b + 1] if re.match(r"^\s*scratch_", x)),
               loop_labels=[lines[a].split(":")[0] for a, _ in loops])
    for start, first_dma, first_bar in ramps:
        # (1) compiler-placed vmcnt waits between the first DMA and the first barrier
        comp_vm = sum(1 for i in range(first_dma, first_bar) if "s_waitcnt" in lines[i] and "vmcnt" in lines[i] and not own[i])
        # (2) a global load followed within three instructions by a full VMEM wait
        instrs = [i for i in range(first_dma, first_bar) if _is_instr(lines[i])]
        load_then_wait = sum(1 for k, i in enumerate(instrs) if lines[i].strip().startswith("global_load")
                             and any("s_waitcnt" in lines[j] and "vmcnt(0)" in lines[j] for j in instrs[k + 1:k + 4]))
        # (3) s_load -> lgkmcnt(0) pairs ahead of the first DMA, on the worst path from the kernel's entry to it
        scalar_waits = _scalar_waits_on_path(lines, first_dma)
        for key, val in (("compiler_vm_waits", comp_vm), ("load_then_wait", load_then_wait), ("scalar_waits", scalar_waits)):
            rep[key] = max(rep[key], val)
    return rep


def report(path) -> dict:
    return {demangled(sym): ramp_report(body) for sym, body in kernel_bodies(Path(path).read_text()).items()}


@pytest.fixture(scope="module")
def isa():
    from medfusion_amd import build as B
    assert B.lint_isa() == []
    rep = report(B.OBJ / "lint" / "conv_f16x2.s")
    assert len(rep) == N_INSTANTIATIONS, sorted(rep)
    return rep


def test_no_compiler_memory_wait_between_the_first_dma_and_the_first_barrier(isa):
    bad = {k: v["compiler_vm_waits"] for k, v in isa.items() if v["compiler_vm_waits"]}
    assert not bad, bad


def test_no_load_directly_followed_by_a_full_wait_in_the_ramp(isa):
    bad = {k: v["load_then_wait"] for k, v in isa.items() if v["load_then_wait"]}
    assert not bad, bad


def test_kernel_argument_is_not_fetched_in_a_chain_of_scalar_round_trips(isa):
    counts = {k: v["scalar_waits"] for k, v in isa.items()}
    print("s_load -> lgkmcnt(0) pairs ahead of the first DMA (parent, now):", {k: (PARENT_SCALAR_WAITS[k], v) for k, v in counts.items()})
    assert set(counts) == set(PARENT_SCALAR_WAITS)
    worse = {k: (PARENT_SCALAR_WAITS[k], v) for k, v in counts.items() if v >= PARENT_SCALAR_WAITS[k]}
    assert not worse, worse
    assert max(counts.values()) <= MAX_SCALAR_WAITS, counts


def test_main_loop_has_no_lane_moves_and_no_scratch(isa):
    bad = {k: (v["lane_moves_loop"], v["scratch_loop"]) for k, v in isa.items() if v["lane_moves_loop"] or v["scratch_loop"]}
    assert not bad, bad
