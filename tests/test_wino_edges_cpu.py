"""The premises of tests/test_wino_edges_gpu.py without a GPU (tests/wino_cases.py): every exact case of every family is exact IN THE TRANSFORM
DOMAIN (no lo.lo product, a common unit, a sum budget below 2^24 units) and the four steps restated in plain fp32 give float32(ref64); the host
rules restated in Python are the library's (its planner answers without a device); the renumbering of the tail's workgroups is a bijection that
keeps an XCD's range contiguous; the case lists reach every path the GPU file relies on; the bound on real operands holds an fp32 restatement;
and the wrappers' size checks (kernels.check_wino)."""

import ctypes as C
import math

import pytest
import torch

from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from tests import conv2d_cases as CC
from tests import wino_cases as WC


def _desc(c, tile=0, sk=0, precision=5):
    return K.make_conv_desc(c.N, c.H, c.W, c.C1, c.C2, c.Cout, c.k, c.stride, c.pad, c.ups, tile_hint=tile, splitk_hint=sk, precision=precision)


# ------------------------------------------------------------------------------------------------ every exact case qualifies
@pytest.mark.parametrize("c", WC.EXACT_CASES + WC.RECORD_CASES + [cg[0] for cg in WC.F32_CASES], ids=lambda c: c.name)
def test_every_exact_case_qualifies_in_the_transform_domain(c):
    if c in [cg[0] for cg in WC.F32_CASES]:       # (the fp32 form has its own admission rule: 64 rows are enough whatever Cout)
        assert all(K.wino_f32_ok(_desc(c, precision=p), G) for p in (0, 3) for cc, G in WC.F32_CASES if cc == c)
    else:
        assert K.wino_ok(_desc(c)) and WC.wino_ok(c), c
    for family, ratio in WC.variants(c):
        x1, x2, w, b = WC.wino_operands(c, family, ratio)
        for t in (x1, x2, w, b):
            assert t is None or torch.equal(t.float().double(), t)                      # fp32 values
        q = WC.wino_budget(c, x1, x2, w, b)
        print(f"[margin] {c.name} {family} ratio={ratio} keep={WC.keep(c):.3f}: lo.lo = {q['lolo']}, log2 sum|U||V|/unit over an output's nine components "
              f"{max(q['bits']):.2f}, over all 16 {max(q['bits16']):.2f} (< 24); with |bias| {q['bits_with_bias']:.2f}")
        assert q["lolo"] == 0.0 and q["pair_ok"] and q["bias_ok"], (family, ratio, q)              # (a), (b)
        assert max(q["bits"]) < 24 and max(q["bits16"]) < 24, (family, ratio, q)                   # (c): even the loose sum over 16 fits
        assert [u for u in q["units"]] == [u - 2 for u in WC.direct_units(c, family, ratio)] or c.C2, (q["units"], WC.direct_units(c, family, ratio))
        if c.C2:   # a two-source sample's unit is never below the direct unit / 4 (a sparse source may leave it higher)
            assert all(u >= d - 2 for u, d in zip(q["units"], WC.direct_units(c, family, ratio)))
        # the family's lo part survives the thinning and the transforms (none in int8)
        u = WC.U64(w)
        lo_u = float(WC.pair_terms(u, float(u.abs().max()))[2].abs().max())
        lo_v = max(float(WC.pair_terms(WC.V64(x[n:n + 1]), 4.0 * float(x[n].abs().max()))[2].abs().max()) for x in (x1, x2) if x is not None for n in range(c.N))
        assert (lo_v > 0, lo_u > 0) == {"xlo": (True, False), "wlo": (False, True), "int8": (False, False)}[family], (family, lo_v, lo_u)
        assert {e for e, _ in CC.sample_exps(c, ratio)} == set(CC.SAMPLE_EXPS[:min(3, c.N)])
        # the reference alone meets the condition: the value before the bias is an fp32 value, the bias rounds once, and the four steps in fp32 torch
        # -- U once rounded, V, the 16 products summed over Cin, A^T M A + bias in the kernel's order -- return float32(ref64) bit for bit
        y0 = WC.ref64(x1, x2, w, None, c)
        assert torch.equal(y0.float().double(), y0) and CC.bias_add_rounds_once(y0, b) and bool((b != 0).any())
        assert all(bool((y0[n] != 0).any()) for n in range(c.N))
        assert torch.equal(WC.restate_fp32(x1, x2, w, b, c), WC.want32(x1, x2, w, b, c)), (c.name, family, ratio)
        assert torch.equal(WC.restate_fp32(x1, x2, w, None, c).double(), y0)


def test_the_transform_references_by_hand():
    """U64, V64 and output32 on a filter and a patch small enough to check by hand, and their composition against F.conv2d"""
    w = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    w[0, 0, 1, 1] = 1.0                                                   # the identity filter: G e11 G^T = outer((0, .5, -.5, 0), (0, .5, -.5, 0))
    col = torch.tensor([0, .5, -.5, 0], dtype=torch.float64)
    assert torch.equal(WC.U64(w).view(4, 4), torch.outer(col, col))
    x = torch.arange(1.0, 5.0, dtype=torch.float64).view(1, 1, 2, 2)     # one tile; the patch is x inside a ring of zeros
    v = WC.V64(x).view(4, 4)
    d = torch.zeros(4, 4, dtype=torch.float64)
    d[1:3, 1:3] = x[0, 0]
    assert torch.equal(v, WC.BT @ d @ WC.BT.T) and torch.equal(WC.V32(x.float()).view(4, 4).double(), v)
    assert v[0, 0] == d[0, 0] - d[2, 0] - d[0, 2] + d[2, 2] == 4.0 and v[1, 1] == 1 + 2 + 3 + 4
    c = WC.case("hand", 1, (2, 2), 1, Cout=1)
    m = (WC.U64(w).view(16, 1, 1) * WC.V64(x).view(16, 1, 1)).view(16, 1, 1, 1)
    assert torch.equal(WC.output32(m, None, c).double(), x)
    assert bool((WC.Vabs64(x) >= WC.V64(x).abs()).all())
    assert sorted(len(set(ks)) for ks in WC.OUT_COMPONENTS.values()) == [9, 9, 9, 9] and set().union(*WC.OUT_COMPONENTS.values()) == set(range(16))
    # which components an output reads, from A^T itself
    for (a, b), ks in WC.OUT_COMPONENTS.items():
        assert ks == [4 * i + j for i in range(4) for j in range(4) if WC.AT[a, i] != 0 and WC.AT[b, j] != 0]


# ------------------------------------------------------------------------------------------------ the restated rules are the library's
def _sweep():
    for n in (1, 2, 3, 4, 5, 8, 16, 64):
        for hw in ((2, 2), (2, 8), (4, 4), (8, 8), (6, 8), (7, 8), (16, 16), (16, 18), (32, 32)):
            for c1, c2 in ((32, 0), (64, 32), (48, 0), (256, 0), (1024, 1024)):
                for co in (32, 64, 128, 192, 256, 320, 512, 1024, 2048):
                    yield CC.case("s", n, hw, c1, c2, Cout=co, k=3)


def test_the_restated_host_rules_are_the_librarys():
    lib = L.load()
    n_ok = n_all = 0
    for c in _sweep():
        n_all += 1
        d = _desc(c)
        ok = WC.wino_ok(c)
        assert K.wino_ok(d) == ok, c
        n_ok += ok
        assert WC.wino_shape_ok(c) or not ok
        for tile in (31, 35, 36, 37, 52, 53, 54, 61, 63):
            if c.Cout % 64 == 0 and (tile not in WC.TILES or c.Cout % WC.TILES[tile][1] == 0):   # (a BN that does not divide Cout is an argument error)
                assert K.wino_ok(_desc(c, tile)) == WC.wino_ok(c, tile), (c, tile)
        for sk in (1, 2, 3, 4, 6, 8):
            assert K.wino_ok(_desc(c, 0, sk)) == WC.wino_ok(c, 0, sk), (c, sk)
            for tile in WC.wino_tiles(c)[:2]:
                assert K.wino_ok(_desc(c, tile, sk)) == WC.wino_ok(c, tile, sk), (c, tile, sk)
                if WC.wino_ok(c, tile, sk):
                    t, s = C.c_int32(), C.c_int32()
                    lib.mf_wino_plan_query(C.byref(_desc(c, tile, sk)), C.byref(t), C.byref(s))
                    eff = WC.slices(WC.gemm_case(c), sk)[3]
                    assert (t.value, s.value) == (tile, eff), (c, tile, sk)
                    assert lib.mf_wino_sync_words(C.byref(_desc(c, tile, sk))) == WC.sync_words(c, tile, eff), (c, tile, sk)
        for G in (1, 2, 4, 8, 16, 32, 64, 256, 512):
            assert K.wino_gn_parts(d, G) == WC.gn_parts(c, G), (c, G)
            assert K.wino_tail_ok(d, G) == WC.tail_ok(c, G), (c, G)
            for prec in (0, 3, 5):
                assert K.wino_f32_ok(_desc(c, precision=prec), G) == WC.f32_ok(c, G, prec), (c, G, prec)
    for bad in (dict(k=1, pad=0), dict(stride=2), dict(ups=2), dict(pad=0)):
        c = CC.case("b", 4, (8, 8), 32, Cout=128, **{"k": 3, **bad})
        assert not WC.wino_shape_ok(c) and not K.wino_ok(_desc(c)) and not WC.f32_ok(c, 8, 3) and not K.wino_f32_ok(_desc(c, precision=3), 8)
    for prec in (0, 3, 4, 6):
        c = WC.case("p", 4, (8, 8), 32, Cout=128)
        assert not WC.wino_shape_ok(c, prec) and not K.wino_ok(_desc(c, precision=prec))
    print(f"[sweep] {n_all} descriptors, {n_ok} on the Winograd path")
    assert 0 < n_ok < n_all


def test_the_issue_example_is_refused_and_the_record_cases_cover_the_rounds():
    """Cout = 64 has 128- and 256-row tiles only: (2, 66, 64, 32, 0, 64) has 2112 rows and is not a Winograd shape.  The record cases: idle tile lanes,
    one round, several whole rounds, a last part with fewer rounds, a ragged round, one tile per round"""
    e = WC.ISSUE_EXAMPLE_REFUSED
    assert not WC.wino_ok(e) and not K.wino_ok(_desc(e)) and (e.N * WC.tiles_of(e)) % 128 == 64
    got = {c.name: WC.output_rounds(c) for c in WC.RECORD_CASES}
    assert got == {"T<R": (4, 1, 1, 1), "one_round": (4, 4, 1, 4), "rounds_whole": (16, 33, 2, 32), "rounds_ragged": (16, 33, 2, 16), "ragged_round": (8, 1, 1, 3),
                   "R1": (1, 16, 1, 1)}, got
    for c in WC.RECORD_CASES:
        G = WC.RECORD_GROUPS[c.Cout]
        assert K.wino_gn_parts(_desc(c), G) == WC.gn_parts(c, G) == got[c.name][1] > 0


def test_the_4gb_refusal_of_the_input_transform():
    """mf_wino_input_f16x2 refuses before it launches anything when [16][N][T][C] x 4 bytes reaches 4 GB (the pointers are never read on the host)"""
    lib = L.load()
    for shape, refused in (((1024, 16, 16, 1024), True), ((1023, 16, 16, 1024), False), ((4, 256, 256, 1024), True), ((4, 256, 254, 1024), False)):
        assert WC.input_refused_4gb(*shape) == refused, shape
        if refused:
            assert lib.mf_wino_input_f16x2(4096, 4096, 4096, 4096, *shape, None) == -2, shape           # MF_EUNSUPPORTED


def test_the_renumbering_is_a_bijection_with_contiguous_ranges():
    for total in range(1, 601):
        image = [WC.xcd_renumber(lin, total) for lin in range(total)]
        assert sorted(image) == list(range(total)), total
        q, r = total >> 3, total & 7
        for xcd in range(8):
            mine = [image[lin] for lin in range(xcd, total, 8)]
            assert mine == list(range(mine[0], mine[0] + len(mine))) if mine else True, (total, xcd)
            assert len(mine) == q + (1 if xcd < r else 0)
    assert [WC.xcd_renumber(i, 10) for i in range(10)] == [0, 2, 4, 5, 6, 7, 8, 9, 1, 3]


# ------------------------------------------------------------------------------------------------ census
def test_the_cases_reach_every_path_the_gpu_file_relies_on():
    tails = {t.c.name: WC.tail_census(t.c, t.G, t.nslots) for t in WC.TAIL_CASES}
    for t in WC.TAIL_CASES:
        assert WC.tail_ok(t.c, t.G) and K.wino_tail_ok(_desc(t.c), t.G), t.c.name
    assert {v["nel"] for v in tails.values()} >= {8, 384, 1024, 1152} and tails["lds64k"]["lds"] == 64 * 1024 == tails["GN10"]["lds"]
    assert tails["nel8"]["idle_phase2"] and tails["nel8"]["idle_phase1"] and tails["nel8"]["padded_everywhere"]
    assert tails["nel1024"]["unrolled_only"] and not tails["nel1024"]["rest_loop"]
    assert tails["nel1152"]["ragged_rest"] and tails["nel1152f"]["ragged_rest"] and tails["lds64k"]["rest_loop"] and not tails["lds64k"]["ragged_rest"]
    assert {v["cq"] for v in tails.values()} >= {2, 4, 16, 32}
    assert tails["GN4"]["below_8"] and tails["GN4"]["remainder"] and tails["GN10"]["remainder"] and not tails["GN10"]["below_8"]
    assert (WC.TAIL_CASES[6].G * WC.TAIL_CASES[6].c.N, WC.TAIL_CASES[7].G * WC.TAIL_CASES[7].c.N) == (4, 10)
    assert any(not v["remainder"] for v in tails.values())
    assert {v["slots"] for v in tails.values()} == {"none", "one", "under_256", "256", "second_loop"} and {t.nslots for t in WC.TAIL_CASES} >= {1, 7, 256, 257, 600}
    # the one thread that reads the slot of the maximum sits in each of the four waves in some case (a wave left out of the maximum shows)
    readers = {n: WC.slot_reader(n, WC.SLOT_MAX_AT[n]) for n in sorted({t.nslots for t in WC.TAIL_CASES if t.nslots > 1})}
    assert readers == {7: (2, 2), 256: (255, 255), 257: (0, 0), 448: (191, 191), 600: (87, 87)} and {a // 64 for a, _ in readers.values()} == {0, 1, 2, 3}
    assert WC.slot_reader(7, 6) == (6, 255) and WC.slot_reader(1, 0) == (0, 255)          # (the last of fewer than 256 slots is read by every later thread)
    assert tails["H2"]["padded_everywhere"] and [t for t in WC.TAIL_CASES if t.c.name == "H2"][0].want_wino
    assert {t.res for t in WC.TAIL_CASES} == {None, "f32", "pairs", "slots"} and {t.act for t in WC.TAIL_CASES} == {0, 1}
    assert {t.affine for t in WC.TAIL_CASES} == {True, False} == {t.out_fp32 for t in WC.TAIL_CASES} == {t.want_wino for t in WC.TAIL_CASES} == {t.emb for t in WC.TAIL_CASES}
    # the output transform: R = 1 at Cin = 32, and the grid cap of the input transform
    assert any(256 // (c.Cout // 4) == 1 and c.C1 == 32 for c in WC.COUT_CASES + WC.RECORD_CASES)
    n, h, w, ch = WC.GRID_CAP_SHAPE
    assert WC.input_grid(n, h, w, ch) == (WC.INPUT_GRID_CAP, 2) and WC.input_grid(1, h, w, ch)[0] < WC.INPUT_GRID_CAP and not WC.input_refused_4gb(n, h, w, ch)
    assert (n - 1) * (h // 2) * (w // 2) * (ch // 4) <= WC.INPUT_GRID_CAP * 256 < n * (h // 2) * (w // 2) * (ch // 4)     # the smallest batch of that shape above it
    assert (WC.PACK_CASE[0] * WC.PACK_CASE[1]) % 256 != 0
    # rows of 64 five ways, 128 and 256; every tile that holds a component is met by some case; the K = 2048 case splits up to 64 inside the launch
    assert [c.N * WC.tiles_of(c) for c in WC.ROW_CASES] == [64] * 5 + [128, 256]
    assert set().union(*(WC.wino_tiles(c) for c in WC.EXACT_CASES)) == set(WC.TILES)
    assert WC.wino_sks(WC.K2048_CASE) == [1, 2, 4, 8, 16, 32, 64]
    kinds = {k for c in WC.TWO_SOURCE_CASES for sk in WC.wino_sks(c) for k in CC.slice_kinds(WC.gemm_case(c), sk)}
    assert kinds >= {"ends_at", "starts_at", "straddles", "after"}, kinds
    for c, G in WC.F32_CASES:
        assert all(WC.f32_ok(c, G, p) and K.wino_f32_ok(_desc(c, precision=p), G) for p in (0, 3))
    assert WC.F32_CASES[0][0].N * WC.tiles_of(WC.F32_CASES[0][0]) == 64 and {c.Cout // G for c, G in WC.F32_CASES} >= {4}
    for c, G in WC.F32_REFUSED:
        assert not any(WC.f32_ok(c, G, p) or K.wino_f32_ok(_desc(c, precision=p), G) for p in (0, 3)), c.name


_SMALL = WC.TAIL_CASES + [WC.Tail(c, WC.RECORD_GROUPS[c.Cout], None, 0, False, False, 0, True, False) for c in WC.RECORD_CASES]


@pytest.mark.parametrize("t", _SMALL, ids=lambda t: t.c.name)
def test_the_tail_operands_give_an_exact_y_and_exact_sums(t):
    """the tail cases and the GroupNorm-record cases on small_operands: y exact, and (without the bias) the fp32 sums of 16 values and of their
    squares that the kernels form before they go to fp64 exact as well"""
    c = t.c
    for bias in (True, False):
        x1, w, b = WC.small_operands(t.c, bias=bias)
        q = WC.wino_budget(c, x1, None, w, b)
        assert q["lolo"] == 0.0 and q["pair_ok"] and q["bias_ok"] and max(q["bits16"]) < 24 and q["bits_with_bias"] < 24, q
        assert q["units"] == [WC.tail_scale_exps(n) - 2 for n in range(c.N)]
        y = WC.ref64(x1, None, w, b, c)
        assert torch.equal(WC.restate_fp32(x1, None, w, b, c).double(), y)
        if not bias:
            assert WC.tail_sums_exact(y, c)
            mean = y.mean(dim=(1, 2, 3)) / torch.tensor([2.0 ** WC.tail_scale_exps(n) for n in range(c.N)], dtype=torch.float64)
            spread = y[0].std() / 2.0 ** WC.tail_scale_exps(0)
            assert bool((mean > 0.25 * spread).all()) and bool((mean < spread).all()), (mean, spread)      # a mean of about half the spread
    assert len({WC.tail_scale_exps(n) for n in range(c.N)}) == min(c.N, WC.TAIL_SCALES)
    gamma, beta, res, wide = WC.tail_side_operands(t)
    assert (res is not None) == (t.res is not None) and (wide is not None) == t.emb
    if t.nslots:
        sl = WC.slot_table(res, t.nslots)
        at = WC.SLOT_MAX_AT[t.nslots]
        assert torch.equal(sl.amax(dim=1), res.abs().amax(dim=(1, 2, 3))) and torch.equal(sl[:, at], sl.amax(dim=1))
        rest = torch.cat([sl[:, :at], sl[:, at + 1:]], 1)
        assert t.nslots == 1 or bool((rest.amax(dim=1) < sl[:, at]).all())


# ------------------------------------------------------------------------------------------------ the bound on real operands
@pytest.mark.parametrize("cancelling", [False, True])
@pytest.mark.parametrize("c", WC.REAL_CASES, ids=lambda c: c.name)
def test_the_real_bound_holds_an_fp32_restatement(c, cancelling):
    assert K.wino_ok(_desc(c)) and WC.wino_ok(c)
    x1, x2, w, b = WC.scaled_real_operands(c, cancelling=cancelling)
    y64 = WC.ref64(x1, x2, w, b, c)
    E = WC.real_bound(x1, x2, w, b, c)
    r = float(((WC.restate_fp32(x1, x2, w, b, c).double() - y64).abs() / E).max())
    s = WC.sabs_wino(x1, x2, w, c)
    print(f"[margin] {c.name} cancelling={cancelling}: fp32 restatement uses {r:.3f} of the bound (c = {WC.real_bound_c(c)} x 2^-24); "
          f"median |y| / sum |U||V| = {float((y64.abs() / s).median()):.1e}")
    assert r < 1.0
    assert 20 <= WC.real_bound_c(c) <= 40 and WC.real_bound_c(c, 4) == WC.real_bound_c(c) - 2 * ((c.C1 + c.C2) // 32 - -(-((c.C1 + c.C2) // 32) // 4)) + 4
    x = torch.cat([x1, x2], 1) if x2 is not None else x1
    assert bool((WC.sabs_wino(x1, x2, w, c, vabs=WC.Vabs64(x)) >= s).all())
    # algebra: the transform-domain form is the convolution
    m = torch.einsum("kntc,koc->knto", WC.V64(x), WC.U64(w))
    y = torch.einsum("ai,bj,ijnto->ntoab", WC.AT, WC.AT, m.view(4, 4, c.N, -1, c.Cout)).reshape(c.N, c.H // 2, c.W // 2, c.Cout, 2, 2).permute(0, 3, 1, 4, 2, 5)
    assert float((y.reshape(y64.shape) + b.view(1, -1, 1, 1) - y64).abs().max()) <= 1e-12 * float(y64.abs().max())


# ------------------------------------------------------------------------------------------------ the wrappers' size checks
def test_check_wino_compares_every_size_with_the_descriptor():
    c = WC.case("chk", 4, (8, 8), 32, 32, Cout=128)
    d = _desc(c)
    x1, x2 = torch.zeros(4, 8, 8, 32), torch.zeros(4, 8, 8, 32)
    u = torch.zeros(16, 128, 1, 1, 64, dtype=torch.int32)
    b = g = be = torch.zeros(128)
    res, wide = torch.zeros(4, 8, 8, 128), torch.zeros(4, 136)
    emb = wide[:, 8:]
    good = dict(x1=x1, x2=x2, u=u, bias=b, d=d, G=8, gamma=g, beta=be, residual=res, emb=emb, emb_stride=136)
    K.check_wino("t", **good)
    K.check_wino("t", x1, x2, u, None, d)
    for change, word in ((dict(x1=torch.zeros(4, 8, 8, 64)), "x1"), (dict(x1=torch.zeros(3, 8, 8, 32)), "x1"), (dict(x1=x1.permute(0, 2, 1, 3)), "x1"),
                         (dict(x2=None), "x2"), (dict(x2=torch.zeros(4, 8, 8, 64)), "x2"), (dict(x1=x1.double()), "x1"),
                         (dict(u=u[:15]), "weights"), (dict(u=u.float()), "weights"), (dict(u=torch.zeros(16, 128, 1, 1, 32, dtype=torch.int32)), "weights"),
                         (dict(bias=torch.zeros(64)), "bias"), (dict(gamma=torch.zeros(127)), "gamma"), (dict(beta=None), "gamma and beta"), (dict(G=7), "groups"),
                         (dict(residual=torch.zeros(4, 8, 8, 64)), "residual"), (dict(residual=res.permute(0, 2, 1, 3)), "residual"),
                         (dict(emb=wide[:, :128].t()), "embedding"), (dict(emb=wide[:3, 8:]), "embedding"), (dict(emb_stride=128), "emb_stride"),
                         (dict(emb=torch.zeros(4, 134)[:, 6:], emb_stride=134), "emb_stride")):
        with pytest.raises(RuntimeError, match=word):
            K.check_wino("t", **{**good, **change})
    with pytest.raises(RuntimeError, match="x2"):
        K.check_wino("t", x1, x2, u, None, _desc(WC.case("chk1", 4, (8, 8), 32, Cout=128)))
    # the fp32 forms: fp32 slabs on precision 0, three bf16 terms (opaque int16) on precision 3
    c1 = WC.case("chk32", 4, (8, 8), 32, Cout=64)
    K.check_wino("t", x1, None, torch.zeros(16, 64, 1, 1, 32), None, _desc(c1, precision=0))
    K.check_wino("t", x1, None, torch.zeros(16 * 64, 96, dtype=torch.int16), None, _desc(c1, precision=3))
    with pytest.raises(RuntimeError, match="weights"):
        K.check_wino("t", x1, None, torch.zeros(16, 64, 1, 1, 32), None, _desc(c1, precision=3))
    # the wrappers call it before anything touches a device
    with pytest.raises(RuntimeError, match="conv2d_wino_f16x2: x1"):
        K.conv2d_wino_f16x2(torch.zeros(4, 8, 8, 64), (u, 1.0), None, d, x2=x2)
    with pytest.raises(RuntimeError, match="conv2d_wino_gn_apply: the residual"):
        K.conv2d_wino_gn_apply(x1, (u, 1.0), None, d, None, None, 8, 1e-5, residual=torch.zeros(4, 8, 8, 64), x2=x2)
    with pytest.raises(RuntimeError, match="conv2d_wino_gn_apply_f32: the transformed weights"):
        K.conv2d_wino_gn_apply_f32(x1, torch.zeros(16, 64, 1, 1, 64), None, _desc(c1, precision=0), None, None, 8, 1e-5)


def test_no_constant_of_the_case_file_comes_from_a_run():
    """the numeric constants of wino_cases.py against the tables they restate (the rules themselves are held by the sweep against the library and by
    the bijection test)"""
    assert WC.INPUT_GRID_CAP == 256 * 16
    assert set(WC.TILES) == {31, 32, 33, 34, 35, 36, 37, 51, 52, 53, 54} and all(WC.TILES[t] == CC.F16X2_TILES[t] for t in WC.TILES)
    assert math.isclose(WC.keep(WC.case("k", 1, (2, 2), 32)), 0.5) and WC.RATIO == CC.LO_BITS
    # (B^T, G and A^T: test_the_real_bound_holds_an_fp32_restatement checks that the transform-domain form IS the convolution)
