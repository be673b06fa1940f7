"""Host-side planning of the Winograd form on the EXACT arithmetics (ABI 250; no GPU: the library only plans here).  Its 16 component GEMMs run on
mf_conv2d_f32 with the upsample = 3 descriptor {N = 16 n, Hin = 1, Win = T, 1x1} (csrc/conv_plan.h); the planner's rule for that descriptor
(csrc/conv.hip make_plan) is checked over a grid of every descriptor mf_wino_f32_ok admits, and each of its outcomes is pinned to a shape."""
import ctypes as C
import itertools
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest

from medfusion_amd import kernels as K
from medfusion_amd import lib as L

ROOT = Path(__file__).resolve().parents[1]
# tile id -> (BM, BN, BK): csrc/conv.hip kCfgs
TILES = {1: (128, 128, 32), 2: (128, 64, 32), 3: (64, 128, 32), 4: (64, 64, 32), 5: (128, 32, 32), 6: (64, 32, 32), 7: (128, 128, 32), 8: (128, 128, 32),
         9: (128, 256, 32), 10: (256, 128, 32), 23: (64, 128, 64), 24: (64, 64, 64), 27: (128, 128, 64), 28: (128, 128, 64)}
MF_EUNSUPPORTED = -2   # include/medfusion_hip.h
CHAIN = 96   # split modes: one truncating bf16-MFMA accumulation chain <= 96 chunks of 32 (test_planner_cpu.py, test_kernels_gpu.py)


def _direct(n, h, w, c1, c2, co, prec):
    return K.make_conv_desc(n, h, w, c1, c2, co, 3, 1, 1, 0, precision=prec)


def _gemm(n, h, w, c1, c2, co, prec, tile=0, sk=0):
    """the component-GEMM descriptor kernels.conv2d_wino_gn_apply_f32 builds for the 3x3 convolution (n, h, w, c1, c2, co)"""
    return K.make_conv_desc(16 * n, 1, (h // 2) * (w // 2), c1, c2, co, 1, 1, 0, 3, tile_hint=tile, splitk_hint=sk, precision=prec)


def _query(d):
    t, k = C.c_int32(), C.c_int32()
    rc = L.load().mf_conv2d_plan_query(C.byref(d), C.byref(t), C.byref(k))
    return rc, t.value, k.value


@pytest.mark.parametrize("prec", [0, 3])
def test_conv_out_hw_agrees_with_the_c_geometry(prec):
    """kernels.conv_out_hw sizes every output mf_conv2d_f32 writes.  The C side's rows M = N Hout Wout are visible without a GPU through the split-K
    workspace (sk slabs of M x Cout floats): nearest-x2 (1), the sub-pixel form (2) and the component GEMM of a Winograd convolution (3, a plain 1 x T
    1x1 -- until this was fixed the Python side took it for nearest-x2 and allocated M four times over)."""
    lib = L.load()
    for (n, h, w, c1, c2, co, k, stride, pad, ups), want in [
        ((2, 16, 16, 64, 0, 128, 3, 1, 1, 0), (16, 16)),
        ((2, 16, 12, 64, 32, 128, 3, 2, 1, 0), (8, 6)),
        ((2, 8, 8, 128, 0, 128, 1, 1, 0, 0), (8, 8)),
        ((2, 8, 6, 64, 0, 128, 3, 1, 1, 1), (16, 12)),
        ((2, 8, 8, 64, 0, 128, 3, 1, 1, 2), (16, 16)),
        ((64, 1, 16, 512, 0, 512, 1, 1, 0, 3), (1, 16)),        # n = 4, 8 x 8
        ((256, 1, 64, 512, 256, 256, 1, 1, 0, 3), (1, 64)),     # n = 16, 16 x 16, two sources
        ((1024, 1, 1, 128, 0, 64, 1, 1, 0, 3), (1, 1)),         # n = 64, 2 x 2: T = 1
    ]:
        d = K.make_conv_desc(n, h, w, c1, c2, co, k, stride, pad, ups, splitk_hint=2, precision=prec)
        assert K.conv_out_hw(d) == want, (n, h, w, ups, K.conv_out_hw(d), want)
        rc, tile, sk = _query(d)
        assert rc == 0 and tile > 0 and sk == 2, (n, h, w, ups, rc, tile, sk)
        ho, wo = want
        assert lib.mf_conv2d_workspace_bytes(C.byref(d)) == sk * n * ho * wo * co * 4, (n, h, w, ups)


def _sweep():
    hw = [(s, s) for s in (2, 4, 8, 16, 32, 64)] + [(2, 4), (4, 2), (8, 16), (16, 8), (8, 32), (32, 8), (16, 64), (64, 32)]
    cins = [(c, 0) for c in (32, 64, 96, 128, 256, 512, 1024, 1536, 2048, 3072, 4096, 6144, 8192)] + \
           [(256, 256), (512, 256), (1024, 512), (1024, 1024), (2048, 1024), (2048, 2048), (3072, 1024), (4096, 4096)]
    return itertools.product((1, 2, 3, 4, 8, 16, 32, 64), hw, cins, (64, 128, 192, 256, 512, 1024), (8, 24, 32), (0, 3))


def test_every_admitted_component_gemm_plans_within_its_invariants():
    """For every descriptor mf_wino_f32_ok admits: the component GEMM plans; the tile's rows divide a component (a tile never straddles two weight
    slabs); the split-K workspace is sk slabs of M x Cout floats (none for split-K 1); on the bf16-triplet arithmetic one accumulation chain is
    <= 96 chunks of 32.  Before the rule for upsample = 3 kept that cap, 2 468 of these planned a longer chain, e.g. (4, 8 x 8, 4096 -> 1024): 128.
    (G = 24 admits Cout 192, the only width here whose component GEMM the rule leaves to the generic planner.)"""
    lib = L.load()
    seen, long_k, bad = 0, 0, []
    for n, (h, w), (c1, c2), co, G, prec in _sweep():
        if not K.wino_f32_ok(_direct(n, h, w, c1, c2, co, prec), G):
            continue
        seen += 1
        g = _gemm(n, h, w, c1, c2, co, prec)
        rc, tile, sk = _query(g)
        rows = n * (h // 2) * (w // 2)
        key = (n, h, w, c1, c2, co, G, prec, tile, sk)
        if rc != 0 or tile not in TILES or not 1 <= sk <= 16:
            bad.append(("plan", key, rc))
            continue
        bm, bn, bk = TILES[tile]
        nk = (c1 + c2) // bk
        if rows % bm or co % bn:
            bad.append(("tile straddles a component", key))
        ws = lib.mf_conv2d_workspace_bytes(C.byref(g))
        if ws != (0 if sk == 1 else sk * 16 * rows * co * 4):
            bad.append(("workspace", key, ws))
        if sk > nk:
            bad.append(("empty split", key))
        if prec == 3:
            long_k += (c1 + c2) // 32 > CHAIN
            if math.ceil((c1 + c2) / 32 / sk) > CHAIN:
                bad.append(("chain", key))
    print(f"[planner] {seen} admitted descriptors ({long_k} with Cin / 32 > {CHAIN} on the bf16-triplet arithmetic), {len(bad)} violations")
    assert seen > 5000 and long_k > 500, (seen, long_k)
    assert not bad, (len(bad), bad[:10])


# (n, H, W, C1, C2, Cout) -> (tile, split-K) of the component GEMM on both exact arithmetics, as planned before the chain cap: every published shape
# (the 32 x 32, 16 x 16 and 8 x 8 levels of the UNet) at B = 4, 8, 16 -- the cap must not move any of them
PUBLISHED_PLANS = {
    (4, 32, 32, 256, 0, 256): (8, 1), (4, 32, 32, 256, 256, 256): (8, 1), (4, 16, 16, 256, 0, 512): (3, 1), (4, 16, 16, 512, 0, 512): (3, 1),
    (4, 16, 16, 512, 512, 512): (8, 2), (4, 16, 16, 512, 256, 256): (3, 1), (4, 16, 16, 256, 0, 256): (3, 1), (4, 8, 8, 512, 0, 1024): (3, 1),
    (4, 8, 8, 1024, 0, 1024): (3, 1), (4, 8, 8, 1024, 1024, 1024): (3, 1), (4, 8, 8, 1024, 512, 512): (3, 1), (4, 8, 8, 512, 0, 512): (3, 1),
    (8, 32, 32, 256, 0, 256): (9, 1), (8, 32, 32, 256, 256, 256): (9, 1), (8, 16, 16, 256, 0, 512): (8, 1), (8, 16, 16, 512, 0, 512): (8, 1),
    (8, 16, 16, 512, 512, 512): (8, 1), (8, 16, 16, 512, 256, 256): (3, 1), (8, 16, 16, 256, 0, 256): (3, 1), (8, 8, 8, 512, 0, 1024): (3, 1),
    (8, 8, 8, 1024, 0, 1024): (8, 2), (8, 8, 8, 1024, 1024, 1024): (8, 2), (8, 8, 8, 1024, 512, 512): (3, 1), (8, 8, 8, 512, 0, 512): (3, 1),
    (16, 32, 32, 256, 0, 256): (9, 1), (16, 32, 32, 256, 256, 256): (9, 1), (16, 16, 16, 256, 0, 512): (9, 1), (16, 16, 16, 512, 0, 512): (9, 1),
    (16, 16, 16, 512, 512, 512): (9, 1), (16, 16, 16, 512, 256, 256): (8, 1), (16, 16, 16, 256, 0, 256): (8, 1), (16, 8, 8, 512, 0, 1024): (8, 1),
    (16, 8, 8, 1024, 0, 1024): (8, 1), (16, 8, 8, 1024, 1024, 1024): (8, 1), (16, 8, 8, 1024, 512, 512): (8, 2), (16, 8, 8, 512, 0, 512): (3, 1),
}


@pytest.mark.parametrize("prec", [0, 3])
def test_published_component_gemm_plans_do_not_move(prec):
    for (n, h, w, c1, c2, co), want in PUBLISHED_PLANS.items():
        assert K.wino_f32_ok(_direct(n, h, w, c1, c2, co, prec), 32)
        assert K.conv_plan(_gemm(n, h, w, c1, c2, co, prec)) == want, (n, h, w, c1, c2, co, prec)


# one shape per outcome of the rule: (n, H, W, C1, C2, Cout) -> {precision: (tile, split-K)}
RULE_OUTCOMES = [
    ((16, 16, 16, 512, 0, 512), {0: (9, 1), 3: (9, 1)}),        # 128 x 256, one workgroup per CU without split-K
    ((16, 8, 8, 1024, 0, 1024), {0: (8, 1), 3: (8, 1)}),        # 128 x 128, the same
    ((8, 8, 8, 1024, 0, 1024), {0: (8, 2), 3: (8, 2)}),         # 128 x 128 with the K loop split in two
    ((4, 8, 8, 2048, 0, 1024), {0: (3, 1), 3: (3, 1)}),         # 64 x 128: rows per component = 64
    ((4, 8, 8, 4096, 0, 1024), {0: (3, 1), 3: (3, 2)}),         # ... with 128 chunks: the bf16-triplet chain is split to 64
    ((4, 8, 8, 2048, 2048, 1024), {0: (3, 1), 3: (3, 2)}),      # the same, two sources
    ((4, 8, 8, 8192, 0, 1024), {0: (3, 1), 3: (3, 4)}),         # 256 chunks -> 4 chains of 64
    ((4, 8, 8, 256, 0, 192), {0: (24, 1), 3: (4, 1)}),          # Cout % 128 != 0: no rule tile, the generic rule (BK = 64 where the channels allow)
    ((64, 2, 2, 64, 0, 64), {0: (24, 1), 3: (4, 1)}),           # T = 1: the smallest grid (one 64-row tile per component)
]


@pytest.mark.parametrize("case,want", RULE_OUTCOMES, ids=lambda c: "x".join(str(v) for v in c) if isinstance(c, tuple) else None)
def test_each_outcome_of_the_component_gemm_rule(case, want):
    lib = L.load()
    n, h, w, c1, c2, co = case
    for prec, (tile, sk) in want.items():
        assert K.wino_f32_ok(_direct(n, h, w, c1, c2, co, prec), co // 8), (case, prec)    # (8 channels per group)
        g = _gemm(n, h, w, c1, c2, co, prec)
        assert K.conv_plan(g) == (tile, sk), (case, prec, K.conv_plan(g))
        m = 16 * n * (h // 2) * (w // 2)
        assert lib.mf_conv2d_workspace_bytes(C.byref(g)) == (0 if sk == 1 else sk * m * co * 4), (case, prec)


def test_split_k_hint_keeps_the_rule_tile_and_is_taken_as_written():
    """d.splitk_hint > 0 on the component descriptor: the rule's tile stays, the hint is the split-K factor (no cap: a hint is the caller's call),
    the workspace follows it; a tile hint whose rows straddle two components is refused before anything launches"""
    lib = L.load()
    for (n, h, w, c1, c2, co), tile in [((4, 8, 8, 4096, 0, 1024), 3), ((16, 8, 8, 1024, 0, 1024), 8), ((16, 16, 16, 512, 0, 512), 9)]:
        m = 16 * n * (h // 2) * (w // 2)
        for prec in (0, 3):
            for sk in (1, 2, 4, 8, 16):
                g = _gemm(n, h, w, c1, c2, co, prec, sk=sk)
                assert K.conv_plan(g) == (tile, sk), ((n, h, w, c1, c2, co), prec, sk, K.conv_plan(g))
                assert lib.mf_conv2d_workspace_bytes(C.byref(g)) == (0 if sk == 1 else sk * m * co * 4)
    rc, _, _ = _query(_gemm(4, 8, 8, 1024, 0, 1024, 3, tile=8))      # 64 rows per component, a 128-row tile
    assert rc == MF_EUNSUPPORTED, rc
    rc, _, _ = _query(_gemm(4, 8, 8, 1024, 0, 1024, 3, tile=3))
    assert rc == 0


def test_the_generic_rule_never_straddles_a_component():
    """MF_WINO_F32_PLAN=0 (the A/B switch read once per process) hands the component GEMM to the generic rule; where that rule's tile would straddle
    two components, the planner takes the largest built tile whose rows divide one.  Run in a child process so the switch is read fresh."""
    code = (
        "import ctypes as C\n"
        "from medfusion_amd import kernels as K\n"
        "for n, h, c1, co, prec in [(4, 8, 2048, 1024, 3), (4, 8, 4096, 1024, 0), (4, 8, 4096, 1024, 3), (8, 8, 2048, 1024, 3)]:\n"
        "    g = K.make_conv_desc(16 * n, 1, (h // 2) ** 2, c1, 0, co, 1, 1, 0, 3, precision=prec)\n"
        "    print(n, h, c1, co, prec, *K.conv_plan(g))\n"
    )
    env = dict(os.environ, MF_WINO_F32_PLAN="0")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {tuple(int(v) for v in line.split()[:5]): tuple(int(v) for v in line.split()[5:]) for line in out.stdout.splitlines()}
    # (the generic rule picks a 128-row tile for all four; 64 rows per component at n = 4 -> the 64 x 128 tile; 128 rows at n = 8 -> its own tile stays)
    assert [got[k][0] for k in [(4, 8, 2048, 1024, 3), (4, 8, 4096, 1024, 0), (4, 8, 4096, 1024, 3)]] == [3, 3, 3], got
    assert TILES[got[(8, 8, 2048, 1024, 3)][0]][0] == 128, got
    for (n, h, c1, co, prec), (tile, sk) in got.items():
        assert n * (h // 2) ** 2 % TILES[tile][0] == 0, got
        assert prec != 3 or math.ceil(c1 / 32 / sk) <= CHAIN, got
