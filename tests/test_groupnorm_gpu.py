"""The GroupNorm kernels (csrc/groupnorm.hip, csrc/gn_partial.h) against fp64 at the edges of their paths, in-process on the product dispatch.
Cases, restatement and the elementwise bound E: tests/groupnorm_cases.py (checked by tests/test_groupnorm_cpu.py, which also asserts which path
every case reaches).  Every output is compared element by element, per sample; the largest |got - fp64| / E of a case is printed as [measured].

a. statistics on exact-arithmetic inputs: records equal the fp64 sums, mean bit for bit, rstd within one ulp
b. the from-partials apply pass (gn_apply_part_kernel) within E, its pair mirror, its derived bound
c. the stats-fed passes (gn_apply_kernel, gn_apply_split_kernel) within E, across the 2048-workgroup cap
d. maxabs_rows    e. what the two apply entries refuse"""
import functools

import pytest
import torch

from tests import groupnorm_cases as GC
from tests import pass_chain_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import medfusion_amd  # noqa: F401  (loads libmedfusion_hip.so; raises if missing)
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=1)
def _on_device(case5, dev):
    """the inputs of a case on the device, with the fp64 statistics [N, G, 2] of y (computed once, shared by every variant)"""
    y, gamma, beta, r, wide = (t.to(dev) for t in GC.apply_inputs(case5))
    mean, var = GC.group_stats(y, case5[4])
    st64 = torch.stack([mean, 1.0 / torch.sqrt(var + GC.EPS)], dim=-1)
    return y, gamma, beta, r, GC.emb_of(wide), st64


def _bound_want(bconst, r, emb, n, dev, first=None):
    """bconst (or the measured bound of x) + bound(residual) + bound(embedding row), in fp32, in that order"""
    b = torch.full((n,), bconst, dtype=torch.float32, device=dev) if first is None else first
    b = b + (r.abs().amax(dim=(1, 2, 3)) if r is not None else torch.zeros((n,), device=dev))
    return b + (emb.abs().amax(dim=1) if emb is not None else torch.zeros((n,), device=dev))


def _check_mirror(K, got, shape, tm, E, tag):
    """the pair mirror and the derived bound of `got`; returns the per-sample ratios of what exists (fp32 output, or the decoded pairs)"""
    bound = got._mf_bound
    dec = GC.decode_pairs(got._mf_split, bound, shape)
    if K.pairs_only(got):
        ratios = GC.ratio_rows(dec, tm, E + 2.0 ** -22 * tm["out"].abs())
        top = dec.abs().amax(dim=(1, 2, 3))
    else:
        ratios = GC.ratio_rows(got, tm, E)
        assert torch.equal(got._mf_split, K.split_f16x2(got, bound)), tag
        top = got.double().abs().amax(dim=(1, 2, 3))
    assert bool((bound.double() >= top).all()), (tag, bound.tolist(), top.tolist())
    return ratios


# ---------------------------------------------------------------- a. statistics

@pytest.mark.parametrize("case", GC.STATS_CASES, ids=GC.case_id)
def test_statistics_are_exact_on_exact_inputs(dev, case):
    from medfusion_amd import kernels as K
    n, h, w, c, G = case
    x = GC.stats_inputs(case)
    rec_w, mean_w, rstd_w = GC.stats_expected(x, G)
    xd = x.to(dev)
    st = K.gn_stats(xd, G, GC.EPS).cpu()
    assert st.shape == (n, G, 2)
    assert torch.equal(st[..., 0].contiguous().view(torch.int32), mean_w.view(torch.int32)), case
    ulps = GC.ulp_distance(st[..., 1], rstd_w)
    print(f"[measured] gn_stats {GC.case_id(case)}: mean bit-exact, rstd within {ulps} ulp")
    assert ulps <= 1, case
    if case in GC.STATS_ONLY:
        return
    chunks = GC.stats_chunks(h * w)
    # (the records are written into uninitialised memory: leave NaN where the allocator will most likely put them)
    poison = torch.full((n, chunks, G, 2), float("nan"), dtype=torch.float64, device=dev)
    del poison
    rec, parts = K.gn_stats_partial(xd, G)
    assert parts == chunks and rec.shape == rec_w.shape
    rec_c = rec.cpu()
    assert torch.equal(rec_c, rec_w), (case, float((rec_c - rec_w).abs().max()))
    for k, size in enumerate(GC.stats_census(case)["chunk_sizes"]):
        if size == 0:
            assert bool((rec_c[:, k] == 0.0).all()), (case, k)
    st2 = K.gn_finalize(rec, parts, h * w, c, G, GC.EPS).cpu()
    assert torch.equal(st2.view(torch.int32), st.view(torch.int32)), case


# ---------------------------------------------------------------- b. the from-partials pass

@pytest.mark.parametrize("case", GC.APPLY_CASES, ids=GC.case_id)
def test_from_partials_apply_is_within_E(dev, case):
    from medfusion_amd import kernels as K
    n, h, w, c, G, parts = case
    hw, cpg = h * w, c // G
    y, gamma, beta, r0, emb, st64 = _on_device(case[:5], dev)
    rec = GC.cut_records(y, G, parts)
    assert rec.shape == (n, parts, G, 2) and rec.dtype == torch.float64 and rec.is_cuda
    runs = [(v, 1) for v in GC.variants(case)]
    if not GC.is_large(case):
        runs.append((("f32", True, True, True), 0))
    worst = (0.0, None)
    for (rkind, has_emb, affine, out_fp32), act in runs:
        tag = (case, rkind, has_emb, affine, out_fp32, act)
        ga, be = (gamma, beta) if affine else (None, None)
        e = emb if has_emb else None
        bconst = GC.bconst_of(ga, be, hw, cpg)
        got = K.gn_apply(y, K.GnPartials(rec, parts, GC.EPS), ga, be, G, act, PC._residual(rkind, r0, K, dev), e, e.stride(0) if has_emb else 0,
                         split=True, bconst=bconst, out_fp32=out_fp32)
        assert K.pairs_only(got) == (not out_fp32), tag
        tm = GC.ref_terms(y, G, ga, be, act, r0 if rkind else None, e, stats=st64)
        E = GC.bound_E(tm, res_pairs=rkind == "pairs")
        assert torch.equal(got._mf_bound, _bound_want(bconst, r0 if rkind else None, e, n, dev)), tag
        ratios = _check_mirror(K, got, y.shape, tm, E, tag)
        if max(ratios) > worst[0]:
            worst = (max(ratios), tag[1:])
        assert max(ratios) <= 1.0, (tag, ratios)
        del got, tm, E
    if not GC.is_large(case):      # the pass without the pair mirror (SPLIT = false)
        got = K.gn_apply(y, K.GnPartials(rec, parts, GC.EPS), gamma, beta, G, 1, r0.clone(), emb, emb.stride(0))
        assert getattr(got, "_mf_split", None) is None
        tm = GC.ref_terms(y, G, gamma, beta, 1, r0, emb, stats=st64)
        ratios = GC.ratio_rows(got, tm, GC.bound_E(tm))
        if max(ratios) > worst[0]:
            worst = (max(ratios), "plain")
        assert max(ratios) <= 1.0, (case, "plain", ratios)
    print(f"[measured] from-partials apply / E, case {GC.case_id(case)}: {worst[0]:.3f} at {worst[1]}")


# ---------------------------------------------------------------- c. the stats-fed passes

@pytest.mark.parametrize("case", GC.STATS_APPLY_CASES, ids=GC.case_id)
def test_stats_fed_apply_is_within_E(dev, case):
    from medfusion_amd import kernels as K
    n, h, w, c, G = case
    hw, cpg = h * w, c // G
    y, gamma, beta, r0, emb, st64 = _on_device(case, dev)
    stats = K.gn_stats(y, G, GC.EPS)
    # (the kernel's own statistics go into the restatement and test a holds them to fp64; here only: they are those of this tensor, sample by
    # sample and group by group -- fp32 sums of at most 16 elements per thread stay below 1e-5 of mean 0.5 / deviation 1, a neighbour's are far off)
    assert float(((stats.double() - st64).abs() / st64.abs()).max()) < 1e-4, case
    worst = (0.0, None)
    for split in (False, True):
        for affine, act, has_res, has_emb in ((True, 1, True, True), (True, 1, False, False), (False, 0, True, False)):
            tag = (case, split, affine, act, has_res, has_emb)
            ga, be = (gamma, beta) if affine else (None, None)
            e, r = (emb if has_emb else None), (r0.clone() if has_res else None)
            bconst = GC.bconst_of(ga, be, hw, cpg)
            got = K.gn_apply(y, stats, ga, be, G, act, r, e, e.stride(0) if has_emb else 0, split=split, bconst=bconst)
            tm = GC.ref_terms(y, G, ga, be, act, r, e, stats=stats)
            E = GC.bound_E(tm)
            if split:
                assert torch.equal(got._mf_bound, _bound_want(bconst, r, e, n, dev)), tag
                ratios = _check_mirror(K, got, y.shape, tm, E, tag)
            else:
                assert getattr(got, "_mf_split", None) is None, tag
                ratios = GC.ratio_rows(got, tm, E)
            if max(ratios) > worst[0]:
                worst = (max(ratios), tag[1:])
            assert max(ratios) <= 1.0, (tag, ratios)
    # no statistics: out = x + r + e under a MEASURED bound of x
    yc = y.clone()
    got = K.gn_apply(yc, None, None, None, G, 0, r0.clone(), emb, emb.stride(0), split=True)
    tm = GC.ref_terms(y, G, None, None, 0, r0, emb, normalise=False)
    assert torch.equal(got._mf_bound, _bound_want(0.0, r0, emb, n, dev, first=y.abs().amax(dim=(1, 2, 3)))), case
    ratios = _check_mirror(K, got, y.shape, tm, GC.bound_E(tm), (case, "stats=None"))
    if max(ratios) > worst[0]:
        worst = (max(ratios), "stats=None")
    assert max(ratios) <= 1.0, (case, "stats=None", ratios)
    print(f"[measured] stats-fed apply / E, case {GC.case_id(case)}: {worst[0]:.3f} at {worst[1]}")


# ---------------------------------------------------------------- d. maxabs_rows

@pytest.mark.parametrize("per_row", GC.MAXABS_PER_ROW)
def test_maxabs_rows_is_exact(dev, per_row):
    from medfusion_amd import kernels as K
    rows = 7
    x = torch.randn((rows, per_row), generator=torch.Generator().manual_seed(per_row)) * GC.scales(rows).view(rows, 1)
    for i in range(0, rows, 3):      # every third row holds its maximum in its LAST float4
        x[i, per_row - 1 - (i % 4)] = -3.0 * x[i].abs().max()
    x[4] = 0.0
    want = x.abs().amax(dim=1)
    assert float(want[4]) == 0.0 and all(int(x[i].abs().argmax()) >= per_row - 4 for i in range(0, rows, 3))
    got = K.maxabs_rows(x.to(dev))
    assert torch.equal(got.cpu(), want), (per_row, got.tolist(), want.tolist())


# ---------------------------------------------------------------- e. refusals

def test_apply_entries_refuse_what_they_cannot_run(dev):
    from medfusion_amd import kernels as K, lib as L

    def entries(x, G):
        n = x.shape[0]
        return (torch.zeros((n, G, 2), device=dev), K.GnPartials(torch.zeros((n, 1, G, 2), dtype=torch.float64, device=dev), 1, GC.EPS))

    def x_of(c):
        return torch.ones((1, 2, 2, c), device=dev)

    for st in entries(x_of(6), 3):            # C % 4 != 0
        with pytest.raises(RuntimeError, match="C=6|multiple of 4"):
            K.gn_apply(x_of(6), st, None, None, 3, 1)
    for st in entries(x_of(8), 3):            # C % G != 0
        with pytest.raises(RuntimeError, match="C=8 G=3"):
            K.gn_apply(x_of(8), st, None, None, 3, 1)
    with pytest.raises(RuntimeError, match="G <= 256"):      # more groups than the from-partials pass has threads for
        K.gn_apply(x_of(1028), entries(x_of(1028), 257)[1], None, None, 257, 1)
    for st in entries(x_of(8), 2):            # gamma without beta
        with pytest.raises(RuntimeError, match="gamma/beta"):
            K.gn_apply(x_of(8), st, torch.ones((8,), device=dev), None, 2, 1)
    # a pair mirror next to a residual whose bound nobody gives (the wrapper would measure it: the C entries themselves)
    lib = L.load()
    x, r = x_of(8), x_of(8)
    out, outs, ob = torch.empty_like(x), torch.empty(x.shape, dtype=torch.int32, device=dev), torch.empty((1,), device=dev)
    st, part = entries(x, 2)
    part.records[...] = 16.0      # (x = 1 over a group of 16 elements: sum = sum of squares = 16)
    rb = torch.ones((1,), device=dev)
    p = lambda t: None if t is None else t.data_ptr()

    def stats_fed(res_bound):
        return lib.mf_gn_apply_split_f32(p(x), p(st), None, None, p(r), None, 0, p(out), p(outs), None, p(res_bound), None, 2.0, p(ob), 1, 4, 8, 2, 1, K.stream())

    def from_partials(res_bound):
        return lib.mf_gn_apply_from_partials_pairs_f32(p(x), p(part.records), 1, GC.EPS, None, None, p(r), None, None, 0, p(out), p(outs), p(res_bound), None, 0,
                                                       None, 2.0, p(ob), 1, 4, 8, 2, 1, K.stream())

    for name, call in (("mf_gn_apply_split_f32", stats_fed), ("mf_gn_apply_from_partials_pairs_f32", from_partials)):
        with pytest.raises(RuntimeError, match="res_bound"):
            L.check(call(None), name)
        L.check(call(rb), name)      # (the same call with the bound is taken: the refusal was about the bound)
    torch.cuda.synchronize()
    assert float(ob[0]) == 3.0
