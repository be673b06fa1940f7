"""The yardstick of tests/test_groupnorm_gpu.py, checked without a GPU (tests/groupnorm_cases.py): the fp64 restatement against
torch.nn.functional.group_norm, the bound E against a plain fp32 evaluation (it must hold it, and must stay of the order of u |out|), the
exactness premise of the statistics inputs, and a census of the host dispatch: every path the cases are there for is reached by one of them."""
import pytest
import torch
import torch.nn.functional as F

from tests import groupnorm_cases as GC

ALL_APPLY = [c[:5] for c in GC.APPLY_CASES] + GC.STATS_APPLY_CASES
ALL_APPLY = sorted(set(ALL_APPLY), key=ALL_APPLY.index)


@pytest.mark.parametrize("case", ALL_APPLY, ids=GC.case_id)
def test_restatement_equals_group_norm_and_E_holds_an_fp32_chain(case):
    n, h, w, c, G = case
    y, gamma, beta, r, wide = GC.apply_inputs(case)
    emb = GC.emb_of(wide)
    nchw = lambda a: a.permute(0, 3, 1, 2)
    worst = 0.0
    forms = [(True, 1, True, True), (False, 0, False, False)] if GC.is_large(case) else \
        [(True, 1, True, True), (True, 1, False, False), (False, 1, True, False), (True, 0, True, True), (False, 0, False, False)]
    for affine, act, has_res, has_emb in forms:
        ga, be = (gamma, beta) if affine else (None, None)
        tm = GC.ref_terms(y, G, ga, be, act, r if has_res else None, emb if has_emb else None)
        gn = F.group_norm(nchw(y.double()), G, ga.double() if affine else None, be.double() if affine else None, GC.EPS)
        want = (gn * torch.sigmoid(gn) if act == 1 else gn)
        if has_res:
            want = want + nchw(r.double())
        if has_emb:
            want = want + emb.double()[:, :, None, None]
        for a, b in ((nchw(tm["t"]), gn), (nchw(tm["out"]), want)):   # per sample: the samples are 2^6 apart
            d = (a - b).abs().reshape(n, -1).amax(1) / b.abs().reshape(n, -1).amax(1)
            assert float(d.max()) <= 1e-12, (case, affine, act, float(d.max()))
        E = GC.bound_E(tm)
        got = GC.fp32_chain(y, G, ga, be, act, r if has_res else None, emb if has_emb else None)
        assert got.dtype == torch.float32
        ratio = max(GC.ratio_rows(got, tm, E))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (case, affine, act, has_res, has_emb, ratio)
        # E does not degenerate: nobody passes the GPU test by inflating it
        med = float((E / tm["out"].abs().clamp_min(1e-300)).median())
        assert med < 1e-5, (case, affine, act, med)
        if affine and act == 1 and has_res:
            med_full = med
    print(f"[measured] fp32 torch chain / E, case {GC.case_id(case)}: {worst:.3f}; median E / |out| {med_full:.2e}")


@pytest.mark.parametrize("case", GC.STATS_CASES, ids=GC.case_id)
def test_statistics_inputs_are_exact_in_fp32(case):
    n, h, w, c, G = case
    x = GC.stats_inputs(case)
    xi = x / GC.scales(n).view(n, 1, 1, 1)
    assert torch.equal(xi, xi.round()) and bool((xi != 0).any())
    assert GC.exact_premise(xi, G) < 2 ** 24
    rec, mean, rstd = GC.stats_expected(x, G)
    assert float((mean != 0).float().mean()) > 0.9 and bool(torch.isfinite(rstd).all())      # (a mean that is not zero)
    # a sequential fp32 sum of a whole group in two different orders equals the fp64 sum
    xg = x.reshape(n, h * w, G, c // G).permute(0, 2, 1, 3).reshape(n * G, -1)
    tot = rec.sum(dim=1).reshape(n * G, 2)
    m = xg.shape[1]
    orders = [torch.arange(m), torch.cat([torch.arange(k, m, 7) for k in range(min(7, m))])]
    for order in orders:
        assert sorted(order.tolist()) == list(range(m))
        v = xg[:, order]
        s, q = torch.zeros(n * G), torch.zeros(n * G)
        vt, v2t = v.t().contiguous(), (v * v).t().contiguous()
        for j in range(m):      # one fp32 addition per element, in this order
            s += vt[j]
            q += v2t[j]
        assert s.dtype == torch.float32 and q.dtype == torch.float32
        assert torch.equal(s.double(), tot[:, 0]) and torch.equal(q.double(), tot[:, 1]), case
    print(f"[measured] case {GC.case_id(case)}: max sum x^2 per group {GC.exact_premise(xi, G):.0f} < 2^24")


def _covered(rows, key, values):
    seen = {r[key] for r in rows}
    missing = [v for v in values if v not in seen]
    assert not missing, (key, missing, sorted(seen, key=str))


def test_path_census_statistics():
    cen = {c: GC.stats_census(c) for c in GC.STATS_CASES}
    rows = list(cen.values())
    assert all(r["lds_bytes"] <= 64 * 1024 and r["groups_per_slice"] >= 1 for r in rows)
    _covered(rows, "slices", [1, 2, 8])
    _covered(rows, "c4_iters", [1, 2])
    _covered(rows, "g_iters", [1, 5])
    _covered(rows, "cpg", [1, 3, 6])
    _covered(rows, "G", [1])
    _covered(rows, "empty_chunks", [0, 2])
    _covered(rows, "chunks", [1, 2, 16])
    assert cen[(2, 1, 1, 32, 8)]["chunk_sizes"] == [1]
    assert cen[(3, 1, 5, 24, 4)]["chunk_sizes"] == [3, 2] and cen[(3, 1, 5, 24, 4)]["C4"] == 6
    r = cen[(2, 1, 67, 96, 32)]
    assert (r["rowphases"], r["idle_threads"], r["chunks"], r["chunk_sizes"][13:]) == (10, 16, 16, [2, 0, 0])
    assert cen[(1, 4, 4, 512, 2)]["slices"] == 2 and cen[(1, 4, 4, 512, 2)]["slices_cpg_limited"]
    assert cen[(1, 4, 4, 512, 32)]["slices"] == 8
    r = cen[(2, 3, 3, 1028, 4)]
    assert (r["C4"], r["c4_iters"], r["c4_last_lanes"]) == (257, 2, 1)
    r = cen[(1, 5, 5, 2048, 1)]       # (with 32 groups the planner cuts 2048 channels into 8 slices of 256: one iteration)
    assert (r["slices"], r["c4_iters"], r["c4_last_lanes"]) == (1, 2, 256)
    assert cen[(1, 5, 5, 2048, 32)]["slices"] == 8 and cen[(1, 5, 5, 2048, 32)]["rowphases"] == 4
    r = cen[(1, 2, 2, 1028, 1028)]    # (1024 channels are cut into 8 slices of 128 groups: the loop over groups needs a width that cannot be sliced)
    assert (r["slices"], r["groups_per_slice"], r["g_iters"]) == (1, 1028, 5)
    assert cen[(1, 2, 2, 1024, 1024)]["groups_per_slice"] == 128
    r = cen[(1, 64, 64, 64, 8)]
    assert (max(r["chunk_sizes"]), r["px_per_thread"]) == (256, 16)


def test_path_census_apply():
    cen = {c: GC.apply_census(c) for c in GC.APPLY_CASES}
    rows = list(cen.values())
    _covered(rows, "U", [1, 2, 4])
    _covered(rows, "FIXED_C", [True, False])
    _covered(rows, "cpg_mod4", [0, 3])
    _covered(rows, "PPT", [1, 8, 32, 85, 256])
    _covered(rows, "records_per_thread", [1, 2, 4])
    _covered(rows, "rounds", [1, 2])
    _covered(rows, "capped", [True, False])
    assert cen[(2, 16, 16, 96, 8, 3)]["FIXED_C"] is False and cen[(2, 16, 16, 96, 32, 3)]["cpg"] == 3
    r = cen[(3, 5, 7, 24, 3, 1)]
    assert (r["PPT"], r["idle_record_threads"], r["parts"], r["ragged_tail"]) == (85, 1, 1, True)
    assert cen[(2, 8, 8, 1024, 256, 4)]["PPT"] == 1 and cen[(1, 32, 32, 64, 1, 16)]["PPT"] == 256
    assert cen[(2, 16, 16, 64, 8, 64)]["records_per_thread"] == 2
    assert cen[(2, 32, 32, 1024, 32, 9)]["U"] == 2 and cen[(4, 32, 32, 1024, 32, 9)]["U"] == 4
    r = cen[(1, 95, 97, 1024, 32, 16)]
    assert (r["U"], r["bps"], r["capped"], r["rounds"], r["ragged_last_round"]) == (4, 2048, True, 2, True)
    assert 95 * 97 * 256 == 2359040 == 2097152 + 261888
    # every case fits the entry's limits (G <= 256, C % 4 == 0, C % G == 0) and emits pairs (C % 8 == 0)
    assert all(c[4] <= 256 and c[3] % 8 == 0 and c[3] % c[4] == 0 for c in GC.APPLY_CASES)
    for c in GC.APPLY_CASES:
        assert len(GC.variants(c)) == (2 if GC.is_large(c) else 7)
    assert [c for c in GC.APPLY_CASES if GC.is_large(c)] == GC.APPLY_CASES[-3:]


def test_path_census_stats_fed_apply():
    cen = {c: GC.stats_apply_census(c) for c in GC.STATS_APPLY_CASES}
    _covered(list(cen.values()), "crosses_samples", [True, False])
    _covered(list(cen.values()), "cpg_mod4", [0, 2])
    r = cen[(9, 16, 16, 1024, 32)]
    assert (r["total4"], r["blocks"]) == (589824, 2048) and r["total4"] > 524288
    assert 524288 // (16 * 16 * 256) == 8      # the thread that started in sample 0 continues in sample 8
    assert all(c[3] % 8 == 0 for c in GC.STATS_APPLY_CASES)
    assert all(p % 4 == 0 for p in GC.MAXABS_PER_ROW)
