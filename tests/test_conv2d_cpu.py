"""The 2-D convolutions' edge cases without a GPU (tests/conv2d_cases.py): the references agree bit for bit, every exact case of every family
qualifies, the host rules restated in Python are the library's (its planner answers without a device), the case lists hold every tile, slice kind
and tile edge the GPU file relies on, no constant of the case file comes from a run, and the wrappers' size checks (kernels.check_conv2d)."""

import re
from pathlib import Path

import pytest
import torch

from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from tests import conv2d_cases as CC

CSRC = Path(__file__).resolve().parents[1] / "medfusion_amd" / "csrc"
EXTRA = [CC.COV_CASE] + [g[0] for g in CC.GROUP_SMALL]
LAYOUT = {"nchw": L.LAYOUT_NCHW, "nhwc": L.LAYOUT_NHWC}


def _desc(c, tile=0, sk=0, precision=5, lin="nhwc", lout="nhwc"):
    return K.make_conv_desc(c.N, c.H, c.W, c.C1, c.C2, c.Cout, c.k, c.stride, c.pad, c.ups, LAYOUT[lin], LAYOUT[lout], tile_hint=tile, splitk_hint=sk,
                            precision=precision)


# ------------------------------------------------------------------------------------------------ references
def test_the_reference_at_pad_0_stride_2_and_extents_of_1_by_hand():
    """hand-checked values of ref64 and gather64: a 1-D problem along W (H = 1, taps of the middle filter row), pad 0 and 1, stride 1 and 2 on an even
    and an odd extent, an extent of 1, and upsampled"""
    w = torch.zeros(1, 1, 3, 3)
    w[0, 0, 1] = torch.tensor([1.0, 2.0, 4.0])

    def by_hand(row, pad, stride):
        n = len(row)
        return [float(sum(wt * (row[o * stride - pad + t] if 0 <= o * stride - pad + t < n else 0) for t, wt in enumerate((1, 2, 4)))) for o in range((n + 2 * pad - 3) // stride + 1)]

    for row in ([1, 10, 100, 1000], [1, 10, 100, 1000, 10000], [7]):
        for pad, stride in ((1, 1), (1, 2)):
            c = CC.case("h", 1, (1, len(row)), 1, Cout=1, k=3, stride=stride, pad=pad)
            x = torch.tensor(row, dtype=torch.float64).view(1, 1, 1, -1)
            for f in (CC.ref64, CC.gather64):
                assert f(x, None, w, None, c).view(-1).tolist() == by_hand(row, pad, stride), (row, pad, stride, f.__name__)
    assert by_hand([1, 10, 100, 1000], 1, 2) == [42.0, 4210.0] and by_hand([1, 10, 100, 1000, 10000], 1, 2) == [42.0, 4210.0, 21000.0] and by_hand([7], 1, 2) == [14.0]
    # pad 0 needs three rows as well (the window must fit): a 3 x n image, the filter's middle row only
    for row, stride in (([1, 10, 100, 1000], 1), ([1, 10, 100, 1000], 2), ([1, 10, 100, 1000, 10000], 2)):
        c = CC.case("h0", 1, (3, len(row)), 1, Cout=1, k=3, stride=stride, pad=0)
        x = torch.zeros(1, 1, 3, len(row), dtype=torch.float64)
        x[0, 0, 1] = torch.tensor(row, dtype=torch.float64)
        for f in (CC.ref64, CC.gather64):
            assert f(x, None, w, None, c).view(-1).tolist() == by_hand(row, 0, stride), (row, stride, f.__name__)
    assert by_hand([1, 10, 100, 1000], 0, 2) == [421.0] and by_hand([1, 10, 100, 1000, 10000], 0, 2) == [421.0, 42100.0]
    # nearest x2: the row 1 10 reads as 1 1 10 10
    c = CC.case("hu", 1, (1, 2), 1, Cout=1, k=3, ups=2)
    x = torch.tensor([1.0, 10.0], dtype=torch.float64).view(1, 1, 1, 2)
    for f in (CC.ref64, CC.gather64, CC.subpixel64):
        assert f(x, None, w, None, c)[0, 0, 0].tolist() == by_hand([1, 1, 10, 10], 1, 1) == [6.0, 43.0, 61.0, 30.0], f.__name__


@pytest.mark.parametrize("c", CC.EXACT_CASES + EXTRA + [d.c for d in CC.DIRECT_CASES], ids=lambda c: c.name)
def test_gather64_equals_ref64_bit_for_bit_on_the_exact_operands(c):
    family, ratio = CC.variants(c)[0] if c.C1 % 32 == 0 else ("int8", None if c.C2 == 0 else "mixed")
    x1, x2, w, b, _ = CC.exact_operands(c, family, ratio)
    a, e = CC.ref64(x1, x2, w, None, c), CC.gather64(x1, x2, w, None, c)
    assert a.shape == e.shape == (c.N, c.Cout, *CC.out_hw(c)) and torch.equal(a, e)          # (the sums are exact in fp64)
    assert bool((a != 0).any())
    # with the bias the fp64 sum itself may round (a 2^-20 sample under a 2^20 bias): float32 of it is the same wherever the bias is added
    assert torch.equal(CC.ref64(x1, x2, w, b, c).float(), CC.want32(x1, x2, w, b, c)) and torch.equal(CC.gather64(x1, x2, w, b, c).float(), CC.want32(x1, x2, w, b, c))
    assert CC.geometry_ok(c) and K.conv_out_hw(_desc(c)) == CC.out_hw(c)
    if c.ups == 2:
        assert torch.equal(CC.subpixel64(x1, x2, w, None, c), a)          # the four phase filters of the sub-pixel form give the same sums


def test_pair_terms_and_split_bf16x3_restate_the_splits():
    x = torch.tensor([1.0 + 3 * 2.0 ** -13, -1.0 - 2.0 ** -13, 0.0, 1.0, 0.3, 127.0, -96.0])
    t0, t1, t2 = CC.split_bf16x3(x)
    assert torch.equal(t0 + t1 + t2, x.double())                              # 24 bits fit three bf16 terms
    assert t0[:4].tolist() == [1.0, -1.0, 0.0, 1.0] and t1[:4].tolist() == [3 * 2.0 ** -13, -2.0 ** -13, 0.0, 0.0] and t2[:4].abs().max() == 0
    assert t0[4] == 0.30078125 and t1[4] != 0 and t2[4] != 0                  # (a value with 24 significant bits uses all three)
    assert t0[5:].tolist() == [127.0, -96.0] and float(t1[5:].abs().max()) == 0
    s, hi, lo = CC.pair_terms(x[5:], 127.0)
    assert s == -8 and hi.tolist() == [127.0 * 256, -96.0 * 256] and float(lo.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ every exact case qualifies
@pytest.mark.parametrize("c", CC.EXACT_CASES, ids=lambda c: c.name)
def test_every_exact_case_qualifies(c):
    for family, ratio in CC.variants(c):
        x1, x2, w, b, units = CC.exact_operands(c, family, ratio)
        for t in (x1, x2, w, b):
            assert t is None or torch.equal(t.float().double(), t)          # fp32 values
        q = CC.exact_budget(c, x1, x2, w, b, units)
        print(f"[margin] {c.name} {family} ratio={ratio} density={CC.density(c):.3f}: lo.lo = {q['lolo']}, log2 sum|terms|/unit: hi.hi {q['bits_m']:.2f}, "
              f"cross {q['bits_x']:.2f}, all {q['bits_all']:.2f} (< 24)")
        assert q["lolo"] == 0.0 and q["unit_ok"], (family, ratio, q)
        assert q["bits_m"] < 24 and q["bits_x"] < 24 and q["bits_all"] < 24, (family, ratio, q)
        # the family's lo part is really there (none in int8), and both signs of the ratio occur in a mixed case
        lo_x = max(float(CC.pair_terms(x[n], float(x[n].abs().max()))[2].abs().max()) for x in (x1, x2) if x is not None for n in range(c.N))
        lo_w = max(float(CC.pair_terms(f, max(float(g.abs().max()) for g, _, _ in CC.kernel_forms(c, w)))[2].abs().max()) for f, _, _ in CC.kernel_forms(c, w))
        assert (lo_x > 0, lo_w > 0) == {"xlo": (True, False), "wlo": (False, True), "int8": (False, False)}[family]
        exps = CC.sample_exps(c, ratio)
        assert {e for e, _ in exps} == set(CC.SAMPLE_EXPS[:min(3, c.N)])
        if ratio == "mixed":
            assert {b2 - a for a, b2 in exps} == {20, -20}
        y0 = CC.ref64(x1, x2, w, None, c)
        assert torch.equal(y0.float().double(), y0)                            # the value before the bias is an fp32 value
        assert CC.bias_add_rounds_once(y0, b) and bool((b != 0).any())
        for n in range(c.N):                                                   # a sample's output is not all bias
            assert bool((y0[n] != 0).any()) or (c.H, c.W) == (1, 1)
        # the bf16 triplet mode (precision 3) is admitted on every family: the products it drops are zero
        assert CC.bf16x3_dropped(x1, x2, w) == 0.0
        for f, _, _ in CC.kernel_forms(c, w):
            assert CC.bf16x3_dropped(x1, x2, f) == 0.0
        if family == "int8":   # one bf16 term (precision 4) and one fp16 term (precision 6) hold the operands exactly
            xs = torch.cat([x1, x2], 1) if x2 is not None else x1
            assert torch.equal(xs.float().bfloat16().double(), xs) and all(torch.equal(f.float().bfloat16().double(), f) for f, _, _ in CC.kernel_forms(c, w))
            assert lo_x == 0 and lo_w == 0


@pytest.mark.parametrize("dc", CC.DIRECT_CASES, ids=lambda d: d.c.name)
def test_every_direct_case_qualifies_on_an_fp32_fma_chain(dc):
    c = dc.c
    ratio = None if c.C2 == 0 else "mixed"
    x1, x2, w, b, units = CC.exact_operands(c, "int8", ratio)
    s = CC.sabs64(x1, x2, w, c)
    for n in range(c.N):
        u = 2.0 ** units[n]
        assert float(s[n].max()) / u < 2.0 ** 24                               # every partial sum, in any order, is an integer below 2^24 units
        assert all(CC._is_multiple(t[n], u) for t in (x1, x2) if t is not None) and CC._is_multiple(b, u)
    assert CC._is_multiple(w, 1.0)
    y0 = CC.ref64(x1, x2, w, None, c)
    assert torch.equal(y0.float().double(), y0) and CC.bias_add_rounds_once(y0, b)
    assert not CC.igemm_ok(c) or c.Cout % 32                                   # really not an implicit-GEMM shape
    d = _desc(c, precision=0, lin=dc.lin, lout=dc.lout)
    assert not K.conv_is_igemm(d) and K.conv_plan(d) == (0, 0)


# ------------------------------------------------------------------------------------------------ the restated rules are the library's
ALL_PAIR = CC.EXACT_CASES + EXTRA


@pytest.mark.parametrize("c", ALL_PAIR, ids=lambda c: c.name)
def test_the_restated_pair_planner_is_the_librarys(c):
    lib = L.load()
    import ctypes as C
    ho, wo = CC.out_hw(c)
    m = c.N * ho * wo
    for prec in (5, 6):
        assert K.conv_f16x2_ok(_desc(c, precision=prec)) == CC.f16x2_ok(c), (c, prec)
    for sk in range(1, 10):   # next to tile hint 0 the planner takes a power-of-two split up to the channel groups, and refuses any other
        assert K.conv_f16x2_ok(_desc(c, 0, sk)) == CC.f16x2_ok(c, 0, sk), (c, sk)
        if CC.f16x2_ok(c, 0, sk):
            assert K.conv_plan(_desc(c, 0, sk))[1] == CC.slices(c, sk)[3]
    for tile, (bm, bn) in CC.F16X2_TILES.items():
        ok = CC.f16x2_ok(c, tile)
        assert K.conv_f16x2_ok(_desc(c, tile)) == ok, (c, tile)
        if not ok:
            continue
        for sk in range(1, (c.C1 + c.C2) // 32 + 2):
            d = _desc(c, tile, sk)
            cg, sw, per, eff = CC.slices(c, sk)
            assert K.conv_plan(d) == (tile, eff), (c, tile, sk)
            tiles = -(-m // bm) * (c.Cout // bn)
            tree = CC.tree_possible(c, sk)
            slabs = eff * m * c.Cout * 4 if eff > 1 else 0
            handoff = tiles * 2 * (eff - 1) * bm * bn * 4 if tree else 0
            assert lib.mf_conv2d_workspace_bytes(C.byref(d)) == max(slabs, handoff), (c, tile, sk)
            assert lib.mf_conv2d_f16x2_sync_words(C.byref(d)) == (tiles * (eff - 1) if tree else 0), (c, tile, sk)
            assert K.conv_pairs_out_ok(d) == (eff == 1 or tree)
            kinds = CC.slice_kinds(c, sk)
            assert len(kinds) == eff and (eff - 1) * per < cg <= eff * per         # no empty slice
            if c.C2 == 0:
                assert set(kinds) == {"before"}
    if c.ups == 2:
        assert K.subpixel_ok(_desc(c, precision=0)) == CC.subpixel_ok(c)


@pytest.mark.parametrize("c", CC.EXACT_IGEMM_CASES, ids=lambda c: c.name)
def test_the_restated_implicit_gemm_planner_is_the_librarys(c):
    assert K.conv_is_igemm(_desc(c, precision=0)) == CC.igemm_ok(c) is True
    for prec in (0, 3, 4):
        for tile in CC.IGEMM_CFGS:
            # (the plan query admits 128 x 32 in the split modes; only the launch refuses it: the restated list leaves it out)
            want = tile in CC.igemm_tiles(c, prec) or (prec != 0 and tile == 5 and tile in CC.igemm_tiles(c, 0))
            try:
                got = K.conv_plan(_desc(c, tile, 1, prec))[0] == tile
            except RuntimeError:
                got = False
            assert got == want, (c, prec, tile)
            if want:
                for sk in (1, 2, 3, 1000):
                    assert K.conv_plan(_desc(c, tile, sk, prec)) == (tile, CC.igemm_slices(c, tile, sk)[2]), (c, prec, tile, sk)
    for t in (23, 24, 27, 28):
        assert (t in CC.igemm_tiles(c, 0)) == (c.C1 % 64 == 0 and c.C2 % 64 == 0 and c.Cout % CC.IGEMM_BN[t] == 0 and (c.ups != 2 or (c.H * c.W) % CC.IGEMM_CFGS[t][0] == 0))


def test_what_the_restated_rule_refuses_the_library_refuses():
    """shapes off the paths: Cout % 64, the gather form of nearest x2, a sub-pixel source that no tile divides, pad 0 on a halo tile"""
    for c, why in ((CC.case("r1", 2, (5, 7), 32, Cout=96), "Cout % 64"), (CC.case("r2", 2, (5, 7), 32, ups=1), "upsample 1"),
                   (CC.case("r3", 2, (5, 6), 32, ups=2), "30 source pixels"), (CC.case("r4", 2, (8, 8), 32, Cout=64, ups=2), "64 source pixels, BN = 64 tiles have 128 rows"),
                   (CC.case("r5", 2, (8, 8), 48), "C1 % 32")):
        assert not CC.f16x2_ok(c) and not K.conv_f16x2_ok(_desc(c)), why
    c = CC.case("r6", 2, (8, 8), 32, Cout=128, pad=0)
    assert CC.f16x2_ok(c, 33) and K.conv_f16x2_ok(_desc(c, 33))
    for t in CC.HALO_HG:
        assert not CC.f16x2_ok(c, t) and not K.conv_f16x2_ok(_desc(c, t))
    assert CC.subpixel_ok(CC.case("r7", 2, (8, 8), 32, Cout=32, ups=2)) and K.subpixel_ok(_desc(CC.case("r7", 2, (8, 8), 32, Cout=32, ups=2), precision=0))
    assert not CC.subpixel_ok(CC.case("r3", 2, (5, 6), 32, ups=2)) and not K.subpixel_ok(_desc(CC.case("r3", 2, (5, 6), 32, ups=2), precision=0))


# ------------------------------------------------------------------------------------------------ census
def pair_combos(cases):
    """(case, tile, sk) of GPU test A on the pair path: every admitted tile x every distinct split, plus the planner's own plan"""
    return [(c.name, t, sk) for c in cases for t in CC.f16x2_tiles(c) for sk in CC.distinct_sks(c)] + [(c.name, 0, 0) for c in cases if CC.f16x2_ok(c)]


def igemm_combos(cases, prec):
    return [(c.name, t, sk) for c in cases for t in CC.igemm_tiles(c, prec) for sk in (1, 2, 3)] + [(c.name, 0, 0) for c in cases]


def test_the_lists_hold_every_tile_and_the_counts_are_these():
    total = 0
    seen = set()
    counted = {}
    for name, cases in (("GEOM", CC.GEOM_CASES), ("M_EDGE", CC.M_EDGE_CASES), ("COUT_EDGE", CC.COUT_EDGE_CASES), ("TWO_SOURCE", CC.TWO_SOURCE_CASES),
                        ("HALO", CC.HALO_CASES), ("SUBPIXEL", CC.SUBPIXEL_CASES), ("REDUCER", [CC.REDUCER_CASE])):
        combos = pair_combos(cases)
        assert len(cases) > 0 and len(combos) >= 4 * len(cases), name                 # (Cout = 64: three tiles and the planner's own)
        seen |= {t for _, t, _ in combos}
        total += len(combos)
        counted[name] = len(combos)
        print(f"[census] pair path {name}: {len(cases)} cases, {len(combos)} (case, tile, sk) combinations")
    assert seen == set(CC.TILES2) | {0}, sorted(set(CC.TILES2) - seen)
    print(f"[census] pair path: {total} combinations x the families of each case")
    # (what the restated rule yields on these lists: a case or a tile that drops out of a list shows up here, not as a shorter GPU run)
    assert counted == dict(GEOM=88, M_EDGE=145, COUT_EDGE=34, TWO_SOURCE=132, HALO=248, SUBPIXEL=53, REDUCER=34), counted
    for prec in (0, 3, 4):
        combos = igemm_combos(CC.EXACT_IGEMM_CASES, prec)
        want = set(CC.IGEMM_CFGS) if prec == 0 else set(CC.IGEMM_SPLIT_MODE_TILES)
        assert {t for _, t, _ in combos} == want | {0}, prec
        print(f"[census] implicit GEMM precision {prec}: {len(CC.EXACT_IGEMM_CASES)} cases, {len(combos)} combinations")
        assert len(combos) == {0: 1370, 3: 1112, 4: 1112}[prec]
    assert all(CC.igemm_ok(c) and not CC.pair_path_ok(c) for c in CC.COUT_IGEMM_CASES)
    # every tile whose BN divides Cout is admitted in COUT_EDGE (3 x 3 pad 1: no halo tile fits a 5 x 7 image)
    for c in CC.COUT_EDGE_CASES:
        assert set(CC.f16x2_tiles(c)) == {t for t, (_, bn) in CC.F16X2_TILES.items() if c.Cout % bn == 0 and t not in CC.HALO_HG}
    for c in CC.SUBPIXEL_CASES:
        assert set(CC.f16x2_tiles(c)) == {t for t, (bm, _) in CC.F16X2_TILES.items() if (c.H * c.W) % bm == 0 and t not in CC.HALO_HG} != set()
    assert {c.H * c.W for c in CC.SUBPIXEL_CASES} == {64, 128, 256}


def test_m_crosses_every_tile_edge():
    ms = {c.name: c.N * CC.out_hw(c)[0] * CC.out_hw(c)[1] for c in CC.M_EDGE_CASES}
    for bm in (64, 128, 256):
        for m in (bm - 1, bm, bm + 1):
            hit = [n for n, v in ms.items() if v == m]
            assert hit, (bm, m)
            print(f"[census] M = {m} (tile rows {bm}): {hit}")
    # k = 3 where a tile's last rows belong to the next sample: the image is smaller than every tile and the last tile is ragged
    for c in CC.M_EDGE_CASES:
        if c.k == 3:
            assert c.H * c.W < 64 and (c.N * c.H * c.W) % 64 != 0 and c.N * c.H * c.W > 64
    assert all(set(CC.f16x2_tiles(c)) >= {37, 53, 31, 32} for c in CC.M_EDGE_CASES)   # the 64-, 128- and 256-row tiles


def test_the_split_k_list_meets_the_source_switch_in_every_way_under_both_forms():
    for form in ("tree", "reducer"):
        hit = {}
        for c in CC.TWO_SOURCE_CASES:
            for sk in CC.distinct_sks(c):
                if sk > 1 and CC.tree_possible(c, sk) == (form == "tree"):
                    for kind in CC.slice_kinds(c, sk):
                        hit.setdefault(kind, []).append((c.name, sk))
        print(f"[slices] {form}: " + "; ".join(f"{kind}: {len(v)} plans, e.g. {v[0]}" for kind, v in sorted(hit.items())))
        for kind in ("before", "ends_at", "starts_at", "straddles", "after"):
            assert hit.get(kind), (form, kind)
    # the larger source comes first and second: by sample in the mixed families, by family in wlo
    for c in CC.TWO_SOURCE_CASES:
        assert {r for _, r in CC.variants(c)} == {"mixed", 20, -20}
        assert {e1 > e2 for e1, e2 in CC.sample_exps(c, "mixed")} == {True, False}
    assert max(CC.distinct_sks(CC.SK8_CASE)) == 8 and CC.slices(CC.SK8_CASE, 8) == (8, 4, 1, 8) and CC.density(CC.SK8_CASE) < 0.5
    c, sk = CC.BOUND_TWO_SOURCE
    assert "straddles" in CC.slice_kinds(c, sk)
    for t, sk in CC.COV_PLANS:
        assert sk < 2 or "straddles" in CC.slice_kinds(CC.COV_CASE, sk)
        assert CC.f16x2_ok(CC.COV_CASE, t)
    assert {t in CC.HALO_HG for t, _ in CC.COV_PLANS if t} == {True, False}


def test_the_reducer_case_gives_the_grid_stride_loop_a_second_trip():
    """splitk_reduce_kernel's launch in conv_f16x2_impl: bx = min(ceil(p4 / 256), cdiv(2048, N)) blocks of 256 threads per sample, p4 = Ho Wo Cout / 4"""
    c = CC.REDUCER_CASE
    ho, wo = CC.out_hw(c)
    p4 = ho * wo * c.Cout // 4
    bx = min(-(-p4 // 256), -(-2048 // c.N))
    assert bx * 256 < p4 <= 2 * bx * 256                                      # a second trip for some threads, no third
    assert CC.slices(c, CC.REDUCER_SK)[3] == 3 and not CC.tree_possible(c, CC.REDUCER_SK)
    src = (CSRC / "conv_f16x2.hip").read_text()
    assert "const int cap = cdiv(2048, d->N);" in src and "int bx = (int)((p4 + 255) / 256);" in src and "const long p4 = (long)HW * d->Cout / 4;" in src


def test_the_halo_list_holds_every_kind_for_both_tile_heights():
    hit = {}
    for c in CC.HALO_CASES:
        ts = [t for t in CC.HALO_HG if CC.f16x2_ok(c, t)]
        assert ts, c.name
        for t in ts:
            hit.setdefault((CC.F16X2_TILES[t][0], CC.halo_kind(c, t), c.C2 > 0), []).append((c.name, t))
    for k, v in sorted(hit.items()):
        print(f"[census] halo BM = {k[0]}, {k[1]}, two sources {k[2]}: {v}")
    for bm in (128, 256):
        for kind in ("images_per_tile", "one_image", "row_blocks"):
            assert (bm, kind, False) in hit or (bm, kind, True) in hit, (bm, kind)
        assert any(k[0] == bm and k[2] for k in hit)
    assert {t for v in hit.values() for _, t in v} == set(CC.HALO_HG)
    # ragged N: the last tile is partly empty and samples of three scales share a tile
    assert any(c.N * c.H * c.W % 128 and c.H * c.W < 128 and c.N >= 3 for c in CC.HALO_CASES)
    assert any(c.N * c.H * c.W % 256 and c.H * c.W < 256 and c.N >= 5 and CC.f16x2_ok(c, 62) for c in CC.HALO_CASES)
    # 4 x 4 where it fits: eight images in a 128-row tile of HG = 5 only
    c44 = [c for c in CC.HALO_CASES if (c.H, c.W) == (4, 4)][0]
    assert [t for t in CC.HALO_HG if CC.f16x2_ok(c44, t)] == [64]


def test_the_bound_cases_stay_inside_the_chain_the_bound_is_derived_for():
    for c in CC.BOUND_CASES + [CC.COV_CASE]:
        assert CC.chain_chunks(c) <= 96, c.name
    for c, a, b in CC.GROUP_SMALL:
        assert (a, b) in CC.GROUP_PAIRS and CC.f16x2_ok(c, a) and CC.f16x2_ok(c._replace(k=1, pad=0), b)
    assert {(a, b) for _, a, b in CC.GROUP_SMALL} == set(CC.GROUP_PAIRS)
    assert len(CC.BOUND_DIRECT) == 5
    for c in CC.NONFINITE_CASES + CC.GUARD_CASES:
        assert CC.f16x2_ok(c)
    assert CC.halo_kind(CC.NONFINITE_CASES[1], 63) == "images_per_tile" and CC.f16x2_ok(CC.NONFINITE_CASES[1], 63)


# ------------------------------------------------------------------------------------------------ no constant comes from a run
def test_no_constant_of_the_case_file_comes_from_a_run_of_the_kernels():
    """the tables are the sources' own, read here from the sources; the sizes are derived in the tests above; the rest is the issue's or conv3d's"""
    src = (CSRC / "conv_f16x2.hip").read_text()
    body = src[src.index("const Tile2 kTiles2[] = {"):src.index("inline size_t tile_lds")]
    tiles = {int(m[0]): tuple(int(v) for v in m[1:]) for m in re.findall(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}", body)}
    assert tiles == CC.TILES2
    conv = (CSRC / "conv.hip").read_text()
    body = conv[conv.index("const TileCfg kCfgs[] = {"):conv.index("int make_plan(")]
    cfgs = {int(m[0]): tuple(int(v) for v in m[1:]) for m in re.findall(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}", body)}
    assert cfgs == CC.IGEMM_CFGS
    body = src[src.index("int dispatch_group("):src.index("int tree_mode()")]
    assert {(int(a) // 100, int(a) % 100) for a in re.findall(r"case (\d{4}):", body)} == set(CC.GROUP_PAIRS)
    split_modes = conv[conv.index("if (d->precision == MF_CONV_BF16)") if "if (d->precision == MF_CONV_BF16)" in conv else 0:]
    for prec_mode in ("32, 5>", "32, 3>"):   # the launch switches of the bf16 and the bf16-triplet mode
        assert {int(t) for t in re.findall(r"case (\d+): rc = launch_igemm<\d+, \d+, \d, \d, " + prec_mode, split_modes)} == set(CC.IGEMM_SPLIT_MODE_TILES)
    assert CC.GUARD_FLOATS == 64 and CC.SAMPLE_EXPS == (0, 20, -20) and CC.LO_BITS == 13 and CC.RATIO_INSIDE == 80


# ------------------------------------------------------------------------------------------------ kernels.check_conv2d
def test_check_conv2d_compares_every_size_with_the_descriptor():
    d = K.make_conv_desc(2, 4, 5, 32, 64, 6, 3, 2, 1)
    ho, wo = K.conv_out_hw(d)
    assert (ho, wo) == (2, 3)
    x1, x2 = torch.zeros(2, 4, 5, 32), torch.zeros(2, 4, 5, 64)
    w, bias, out = torch.zeros(6, 3, 3, 96), torch.zeros(6), torch.zeros(2, ho, wo, 6)
    K.check_conv2d("t", x1, x2, w, bias, out, d)
    K.check_conv2d("t", x1, x2, w, None, None, d)
    K.check_conv2d("t", torch.zeros(2, 4, 5, 32, device="meta"), torch.zeros(2, 4, 5, 64, device="meta"), w, bias, out, d)
    bad = [
        ("x1 holds", dict(x1=torch.zeros(2, 4, 5, 31))), ("x1 holds", dict(x1=torch.zeros(1, 4, 5, 32))), ("x1 holds", dict(x1=x2)), ("x1 holds", dict(x1=None)),
        ("x2 holds", dict(x2=x1)), ("second source is missing", dict(x2=None)), ("bias", dict(bias=torch.zeros(5))), ("bias", dict(bias=torch.zeros(6, dtype=torch.float64))),
        ("bias", dict(bias=torch.zeros(12)[::2])), ("the weights hold", dict(w=torch.zeros(6, 3, 3, 64))), ("the weights hold", dict(w=torch.zeros(4, 6, 2, 2, 96))),
        ("not contiguous", dict(w=torch.zeros(6, 3, 96, 3).transpose(2, 3))), ("out", dict(out=torch.zeros(2, ho, wo, 5))), ("out", dict(out=torch.zeros(2, ho + 1, wo, 6))),
        ("out", dict(out=torch.zeros(2, ho, wo, 6, dtype=torch.float64))), ("out", dict(out=torch.zeros(2, ho, 6, wo).transpose(2, 3))),
    ]
    for msg, kw in bad:
        a = dict(x1=x1, x2=x2, w=w, bias=bias, out=out)
        a.update(kw)
        with pytest.raises(RuntimeError, match=msg):
            K.check_conv2d("t", a["x1"], a["x2"], a["w"], a["bias"], a["out"], d)
    d1 = K.make_conv_desc(2, 4, 5, 32, 0, 6, 1, 1, 0)
    with pytest.raises(RuntimeError, match="second source is given"):
        K.check_conv2d("t", x1, x1, torch.zeros(6, 32), bias, None, d1)
    # NCHW in and out: the same counts; the sub-pixel packing: 4 phases of 2 x 2 taps; the bf16 triplets: three terms
    dn = K.make_conv_desc(2, 4, 5, 8, 0, 6, 3, 1, 1, 0, L.LAYOUT_NCHW, L.LAYOUT_NCHW)
    K.check_conv2d("t", torch.zeros(2, 8, 4, 5), None, torch.zeros(6, 3, 3, 8), bias, torch.zeros(2, 6, 4, 5), dn)
    with pytest.raises(RuntimeError, match=r"x1 holds 280 values.*\(NCHW\) needs 320"):
        K.check_conv2d("t", torch.zeros(2, 7, 4, 5), None, torch.zeros(6, 3, 3, 8), bias, None, dn)
    du = K.make_conv_desc(2, 8, 8, 32, 0, 64, 3, 1, 1, 2)
    K.check_conv2d("t", torch.zeros(2, 8, 8, 32), None, torch.zeros(4, 64, 2, 2, 32), None, torch.zeros(2, 16, 16, 64), du)
    with pytest.raises(RuntimeError, match="sub-pixel packing"):
        K.check_conv2d("t", torch.zeros(2, 8, 8, 32), None, torch.zeros(64, 3, 3, 32), None, None, du)
    with pytest.raises(RuntimeError, match="out"):
        K.check_conv2d("t", torch.zeros(2, 8, 8, 32), None, torch.zeros(4, 64, 2, 2, 32), None, torch.zeros(2, 8, 8, 64), du)
    d3 = K.make_conv_desc(2, 4, 5, 32, 0, 64, 3, 1, 1, precision=3)
    K.check_conv2d("t", x1, None, torch.zeros(64, 3 * 288, dtype=torch.int16), None, None, d3)
    with pytest.raises(RuntimeError, match="three bf16 terms"):
        K.check_conv2d("t", x1, None, torch.zeros(64, 288, dtype=torch.int16), None, None, d3)
    # it is the first thing the three wrappers do: a wrong size raises before any device is asked for
    wh = (torch.zeros(6, 3, 3, 96, dtype=torch.int32), 1.0)
    with pytest.raises(RuntimeError, match="conv2d: out"):
        K.conv2d(x1, w, bias, d, x2=x2, out=torch.zeros(2, ho, wo, 5))
    with pytest.raises(RuntimeError, match="conv2d_f16x2: x2 holds"):
        K.conv2d_f16x2(x1, wh, bias, d, x2=x1)
    with pytest.raises(RuntimeError, match="conv2d_f16x2_pairs_out: bias"):
        K.conv2d_f16x2_pairs_out(x1, wh, torch.zeros(5), d, (1.0, 1.0), 0.0, x2=x2)
