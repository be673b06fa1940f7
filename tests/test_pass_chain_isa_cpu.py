"""The memory-bound passes around the convolutions -- wino_tail_kernel and wino_input_kernel (csrc/winograd.h), gn_apply_part_kernel
(csrc/groupnorm.hip) -- read off the shipped ISA (medfusion_amd.build.lint_isa -> csrc/build/lint/conv_f16x2.s, groupnorm.s): what depends on
nothing is requested at the kernel's entry, nothing that the statistics do not feed is fetched behind them, no wait stands behind a store,
nothing spills.  profiles/pass_round_trips.txt has the counts of the parent commit (MF_PASS_CHAIN=1) next to the ones asserted here.

Conventions of the checks:
  * a path runs over forward edges only (fall-through and branches to later labels), blocks in text order -- the method of
    tests/test_conv_ramp_isa_cpu.py; a loop's latch, which the block placement may put in front of its header, is reached by a backward
    branch and lies on no such path;
  * scalar loads from the kernel-argument segment (the base register pair of the kernel's first s_load) are argument fetches from the 64-byte
    lines the entry already read, not uniform DATA fetched late: check (b) counts scalar loads from any other base;
  * "a wait behind a store": vmcnt retires in order, so `s_waitcnt vmcnt(N)` behind S stores with no load in between waits for a store exactly
    when N < S.  N >= S leaves every one of the stores in flight (the wait is for an older load -- the loop of the tail that keeps one round of
    residual rows ahead ends in one); the plain count of waits that follow a store, whatever N, is printed next to it.
"""
import re
from pathlib import Path

import pytest

TAIL = "_ZN3mfw16wino_tail_kernelENS_9WinoTailPE"
INPUT = "_ZN3mfw17wino_input_kernelEPKvPKfPvPfiiii"
APPLY = "_ZN12_GLOBAL__N_120gn_apply_part_kernelILb1ELi{u}ELb{f}EEE"     # <SPLIT = true, U, FIXED_C>
# .vgpr_count of the parent commit's gn_apply_part_kernel<true, U> (same flags): occupancy must not be lower
PARENT_APPLY_VGPRS = {4: 106, 2: 78, 1: 60}

_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_BRANCH = re.compile(r"^\s*s_c?branch\S*\s+(\.LBB\d+_\d+)")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")


def body(text: str, prefix: str):
    """the lines of the one kernel whose symbol starts with `prefix`, and its metadata entry"""
    lines, cur, found = text.splitlines(), None, []
    for ln in lines:
        if cur is None:
            m = re.match(r"^(_Z\w+):", ln)
            if m and m.group(1).startswith(prefix):
                cur = []
        elif ln.startswith(".Lfunc_end"):
            found.append(cur)
            cur = None
        else:
            cur.append(ln)
    assert len(found) == 1, (prefix, len(found))
    meta = {}
    i = next(i for i, ln in enumerate(lines) if ".name:" in ln and prefix in ln)
    for ln in lines[i:i + 20]:
        m = re.match(r"^\s+\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", ln)
        if m:
            meta[m.group(1)] = int(m.group(2))
    return found[0], meta


def op(ln: str) -> str:
    s = ln.strip()
    return "" if not s or s.startswith((";", ".")) else s.split()[0]


def first_m_load(lines) -> int:
    """line of the first of 16 global_load_dwordx4 in a row (no other vector memory instruction, no wait for one in between): the M burst"""
    run = []
    for i, ln in enumerate(lines):
        o = op(ln)
        if o == "global_load_dwordx4":
            run.append(i)
            if len(run) == 16:
                return run[0]
        elif o.startswith(("global_", "buffer_", "flat_")) or (o == "s_waitcnt" and "vmcnt" in ln):
            run = []
    raise AssertionError("no burst of 16 global_load_dwordx4")


def late_loads(lines):
    """check (b): (line, text) of every wait, on a forward path from the kernel's first barrier to the first global_store on that path, for a
    global load or a scalar load (not of the kernel argument) issued on that path behind the barrier"""
    karg = next(re.search(r"(s\[\d+:\d+\]),\s*\S+\s*$", ln).group(1) for ln in lines if op(ln).startswith("s_load"))
    starts = sorted({0} | {i for i, ln in enumerate(lines) if _LABEL.match(ln)} | {i + 1 for i, ln in enumerate(lines) if _BRANCH.match(ln) or op(ln) == "s_endpgm"})
    starts = [i for i in starts if i < len(lines)]
    block_of = {}
    for k, a in enumerate(starts):
        for i in range(a, starts[k + 1] if k + 1 < len(starts) else len(lines)):
            block_of[i] = k
    labels = {m.group(1): block_of[i] for i, ln in enumerate(lines) for m in [_LABEL.match(ln)] if m}
    bar = next(i for i, ln in enumerate(lines) if op(ln) == "s_barrier")
    bad, seen = [], set()
    todo = [(block_of[bar], bar + 1, False, False)]     # (block, first line, a vector load is pending, a scalar load is pending)
    while todo:
        k, a, pv, ps = todo.pop()
        if (k, a, pv, ps) in seen:
            continue
        seen.add((k, a, pv, ps))
        end = starts[k + 1] if k + 1 < len(starts) else len(lines)
        fall = True
        for i in range(a, end):
            o, ln = op(lines[i]), lines[i]
            if o.startswith("global_store"):
                fall = False
                break
            if o.startswith("global_load"):
                pv = True
            elif o.startswith(("s_load", "s_buffer_load")) and not re.search(re.escape(karg) + r",\s*\S+\s*$", ln):
                ps = True
            elif o == "s_waitcnt":
                if pv and "vmcnt" in ln:
                    bad.append((i, ln.strip()))
                    pv = False
                if ps and "lgkmcnt" in ln:
                    bad.append((i, ln.strip()))
                    ps = False
            m = _BRANCH.match(ln)
            if m:
                if labels.get(m.group(1), -1) > k:
                    t = labels[m.group(1)]
                    todo.append((t, starts[t], pv, ps))
                if o == "s_branch":
                    fall = False
                break
            if o == "s_endpgm":
                fall = False
                break
        if fall and k + 1 < len(starts):
            todo.append((k + 1, starts[k + 1], pv, ps))
    return sorted(set(bad))


def _cfg(lines):
    """(first lines of the blocks, successors of every block -- backward edges included)"""
    starts = sorted({0} | {i for i, ln in enumerate(lines) if _LABEL.match(ln)} | {i + 1 for i, ln in enumerate(lines) if _BRANCH.match(ln) or op(ln) == "s_endpgm"})
    starts = [i for i in starts if i < len(lines)]
    label_block = {}
    for k, a in enumerate(starts):
        m = _LABEL.match(lines[a])
        if m:
            label_block[m.group(1)] = k
    succ = []
    for k, a in enumerate(starts):
        end = starts[k + 1] if k + 1 < len(starts) else len(lines)
        last = next((i for i in range(end - 1, a - 1, -1) if op(lines[i])), None)
        out = []
        if last is not None:
            m = _BRANCH.match(lines[last])
            if m:
                out.append(label_block[m.group(1)])
            if op(lines[last]) not in ("s_branch", "s_endpgm") and k + 1 < len(starts):
                out.append(k + 1)
        elif k + 1 < len(starts):
            out.append(k + 1)
        succ.append(out)
    return starts, succ


def store_waits(lines, back_edges=True):
    """check (c): (waits that wait for a store, waits that merely follow one) -- see the module docstring.  `stores behind the last load` is the
    largest count over all paths of the control-flow graph that reach the wait (loops included; capped at 64).  back_edges=False: forward
    edges only -- for a loop whose exit test and back edge share a block (`if (jw >= per4) break; load the next round`: the compiler branches
    to the latch from both sides and tests the same condition again there), where the graph alone holds a path from the stores to the
    header that no execution takes; round_loads_precede_the_back_edge covers the back edge of such a loop."""
    starts, succ = _cfg(lines)
    if not back_edges:
        succ = [[t for t in out if t > k] for k, out in enumerate(succ)]
    entry = {0: 0}      # block -> stores behind the last load at its first line, the worst path
    todo = [0]
    for_store, after_store = {}, {}
    while todo:
        k = todo.pop()
        stores = entry[k]
        end = starts[k + 1] if k + 1 < len(starts) else len(lines)
        for i in range(starts[k], end):
            o = op(lines[i])
            if o.startswith("global_load"):
                stores = 0
            elif o.startswith("global_store"):
                stores = min(stores + 1, 64)
            elif o == "s_waitcnt" and stores:
                m = _VMCNT.search(lines[i])
                if m:
                    after_store[i] = (i, lines[i].strip(), max(stores, after_store.get(i, (0, "", 0))[2]))
                    if int(m.group(1)) < stores:
                        for_store[i] = (i, lines[i].strip(), max(stores, for_store.get(i, (0, "", 0))[2]))
        for t in succ[k]:
            if entry.get(t, -1) < stores:
                entry[t] = stores
                todo.append(t)
    return sorted(for_store.values()), sorted(after_store.values())


def round_loads_precede_the_back_edge(lines) -> bool:
    """between the last global_store in front of the kernel's last backward branch (the end of the round loop's body) and that branch there is a
    global load: the wait at the top of the next round has the round's own loads between it and the stores"""
    seen, back = set(), []
    for i, ln in enumerate(lines):
        m = _LABEL.match(ln)
        if m:
            seen.add(m.group(1))
        b = _BRANCH.match(ln)
        if b and b.group(1) in seen:
            back.append(i)
    if not back:
        return False
    last_store = max(i for i in range(back[-1]) if op(lines[i]).startswith("global_store"))
    return any(op(lines[j]).startswith("global_load") for j in range(last_store, back[-1]))


def load_then_full_wait(lines):
    """global loads followed within three instructions by `s_waitcnt vmcnt(0)`"""
    ins = [i for i, ln in enumerate(lines) if op(ln)]
    return [(i, lines[i].strip()) for k, i in enumerate(ins) if op(lines[i]).startswith("global_load")
            and any(op(lines[j]) == "s_waitcnt" and "vmcnt(0)" in lines[j] for j in ins[k + 1:k + 4])]


def no_spill(lines, meta):
    assert not [ln for ln in lines if op(ln).startswith("scratch_")]
    assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, meta


@pytest.fixture(scope="module")
def isa():
    from medfusion_amd import build as B
    assert B.lint_isa() == []
    conv, gn = (B.OBJ / "lint" / "conv_f16x2.s").read_text(), (B.OBJ / "lint" / "groupnorm.s").read_text()
    out = {"tail": body(conv, TAIL), "input": body(conv, INPUT)}
    for u in (4, 2, 1):
        for f in (1, 0):
            out["apply", u, f] = body(gn, APPLY.format(u=u, f=f))
    return out


def test_tail_requests_everything_before_the_first_load_of_m(isa):
    """(a) no wait with a vmcnt field between the entry and the first load of M: the residual rows and the uniform data are in flight across phase 1"""
    lines, _ = isa["tail"]
    m0 = first_m_load(lines)
    early = [i for i in range(m0) if op(lines[i]).startswith("global_load")]
    waits = [(i, lines[i].strip()) for i in range(m0) if op(lines[i]) == "s_waitcnt" and "vmcnt" in lines[i]]
    print(f"tail: {len(early)} global loads and {len(waits)} vmcnt waits in front of the first load of M")
    assert len(early) >= 10 and not waits, waits      # (2 halves x 5 residual rows at least)


def test_tail_fetches_nothing_between_the_statistics_and_the_first_store(isa):
    """(b)"""
    assert late_loads(isa["tail"][0]) == []


def test_tail_never_waits_for_a_store(isa):
    """(c), and the barrier in front of phase 3 orders LDS only: no vmcnt wait between it and the first store of V"""
    lines, _ = isa["tail"]
    for_store, after_store = store_waits(lines)
    print(f"tail: waits that follow a store with no load in between (line, wait, stores behind the last load): {after_store}")
    assert for_store == []
    bars = [i for i, ln in enumerate(lines) if op(ln) == "s_barrier"]
    assert len(bars) == 2, bars
    nxt = next(i for i in range(bars[1], len(lines)) if op(lines[i]).startswith("global_store"))
    assert not [lines[i] for i in range(bars[1], nxt) if op(lines[i]) == "s_waitcnt" and "vmcnt" in lines[i]]


def test_tail_has_no_scratch_and_two_workgroups_per_cu(isa):
    """(d); <= 256 VGPRs: two 256-thread workgroups per CU at 64 KB of LDS each"""
    lines, meta = isa["tail"]
    no_spill(lines, meta)
    print("tail: .vgpr_count", meta["vgpr_count"])
    assert meta["vgpr_count"] <= 256, meta


@pytest.mark.parametrize("u", [4, 2, 1])
def test_apply_pass_fixed_channels(isa, u):
    """gn_apply_part_kernel<true, U, true> (every published width): (b), (c), (d); the records are waited for by a count that leaves every load
    requested behind them in flight; occupancy not below the parent's"""
    lines, meta = isa["apply", u, 1]
    assert late_loads(lines) == []
    for_store, after_store = store_waits(lines, back_edges=False)
    print(f"apply U={u}: waits that follow a store with no load in between: {after_store}; .vgpr_count {meta['vgpr_count']} (parent {PARENT_APPLY_VGPRS[u]})")
    assert for_store == [] and after_store == [] and round_loads_precede_the_back_edge(lines)
    no_spill(lines, meta)
    assert 512 // meta["vgpr_count"] >= 512 // PARENT_APPLY_VGPRS[u], meta     # waves per SIMD
    loads = [i for i, ln in enumerate(lines) if op(ln).startswith("global_load")]
    w = next(i for i, ln in enumerate(lines) if op(ln) == "s_waitcnt" and "vmcnt" in ln)
    behind = sum(1 for i in loads if loads[0] < i < w)
    n = int(_VMCNT.search(lines[w]).group(1))
    print(f"apply U={u}: first vmcnt wait is vmcnt({n}), {behind} loads requested behind the record")
    assert behind >= 3 * u and n == behind, (lines[w], behind)     # (x and the residual's two halves of every element of round 0 at least)


@pytest.mark.parametrize("u", [4, 2, 1])
def test_apply_pass_general_channels(isa, u):
    """gn_apply_part_kernel<true, U, false> (256 % (C / 4) != 0: the channel constants are fetched per element, behind the statistics by necessity):
    (c) and (d)"""
    lines, meta = isa["apply", u, 0]
    for_store, _ = store_waits(lines, back_edges=False)
    assert for_store == [] and round_loads_precede_the_back_edge(lines)
    no_spill(lines, meta)
    assert 512 // meta["vgpr_count"] >= 512 // PARENT_APPLY_VGPRS[u], meta


def test_input_transform_requests_its_patch_in_one_burst(isa):
    lines, meta = isa["input"]
    assert load_then_full_wait(lines) == []
    no_spill(lines, meta)
