"""Nearest neighbours with indices, density / coverage and the copy audit on a real MI355X (medfusion_amd/fidelity.py, csrc/fidelity.hip) against
the kernel's own matrix bit for bit and against the fp64 restatement (tests/neighbour_cases.py): the selection is the stable sort of
pairwise_sqdist; the unrefined values are held to the DERIVED bound E_ij = (D + 8) 2^-24 (n_i + n_j) with no case left out, the indices to fp64
under the ambiguity rule; the refined values to 4 2^-24 relative (derived in neighbour_cases' header); counts and coverage to the matrix form
exactly and to fp64 within the ambiguous pairs; then the memory the fused search takes, the meter and the audit script."""
import functools
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import fidelity as F
from medfusion_amd import kernels as K
from tests import fidelity_cases as FC
from tests import neighbour_cases as NC
from tests.test_neighbours_cpu import _script

DEV = "cuda:0"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device(DEV)


def _misaligned(t):
    """the same values, contiguous, one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _random_banks(m, n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(m, d, generator=g) * 0.9 + 0.7, torch.randn(n, d, generator=g) * 1.3 + 0.5


SHAPES = {"q5": (5, 257, 260), "k16": (129, 16, 8), "d1": (17, 16, 1)}        # query rows, reference rows, D


@functools.lru_cache(maxsize=None)
def _banks(name):
    """(query, ref, pivot) on the device: a case's generated rows searched in its real rows, or a random shape"""
    if name in SHAPES:
        q, r = _random_banks(*SHAPES[name], seed=11)
    else:
        r, q = NC.case(name)
    q, r = q.to(DEV), r.to(DEV)
    return q, r, K.feat_colmean(r)


@functools.lru_cache(maxsize=None)
def _sorted_matrix(name):
    """the stable sort of the kernel's own matrix: (values, indices), computed once per case and left unchanged"""
    q, r, p = _banks(name)
    return torch.sort(M.pairwise_sqdist(q, r, pivot=p), dim=1, stable=True)


@functools.lru_cache(maxsize=None)
def _sorted_own(name):
    """the same of a bank against itself with +inf on the diagonal"""
    _, r, p = _banks(name)
    own = M.pairwise_sqdist(r, pivot=p)
    own.fill_diagonal_(float("inf"))
    return torch.sort(own, dim=1, stable=True)


# ------------------------------------------------------------------------------------------------ 1. selection, bit for bit
@pytest.mark.parametrize("splits", [1, 2, 16])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_selection_is_the_stable_sort_of_the_kernels_own_matrix(dev, k, splits):
    for name in ("c1", "c3", "q5", "k16", "d1"):
        q, r, p = _banks(name)
        want_v, want_i = _sorted_matrix(name)
        dist, index = M.nearest_neighbours(q, r, k, pivot=p, refine=False, squared=True, _splits=splits)
        assert dist.shape == index.shape == (q.shape[0], k) and dist.dtype == torch.float32 and index.dtype == torch.int64
        assert torch.equal(index, want_i[:, :k]), (name, k, splits)
        assert torch.equal(dist, want_v[:, :k]), (name, k, splits)
    assert torch.equal(M.nearest_neighbours(q, r, k, refine=False, squared=True)[1], index)       # the planner's own S, the pivot of ref
    assert torch.equal(M.nearest_neighbours(q, r, k, pivot=p, refine=False, _splits=splits)[0], torch.sqrt(dist))


@pytest.mark.parametrize("splits", [1, 2, 16])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_leave_one_out_selection_is_the_sort_with_an_infinite_diagonal(dev, k, splits):
    for name in ("c1", "c3", "d1"):
        _, r, p = _banks(name)
        if name == "d1":                                                      # 17 rows of the d1 queries' bank: k = 16 = N - 1
            r = _banks("d1")[0]
            p = K.feat_colmean(r)
            own = M.pairwise_sqdist(r, pivot=p)
            own.fill_diagonal_(float("inf"))
            want_v, want_i = torch.sort(own, dim=1, stable=True)
        else:
            want_v, want_i = _sorted_own(name)
        dist, index = M.nearest_neighbours(r, None, k, pivot=p, refine=False, squared=True, _splits=splits)
        assert torch.equal(index, want_i[:, :k]) and torch.equal(dist, want_v[:, :k]), (name, k, splits)
        assert not bool((index == torch.arange(r.shape[0], device=dev)[:, None]).any())
        assert bool(torch.isfinite(dist).all())


# ------------------------------------------------------------------------------------------------ 2. ties and duplicates
def test_ties_are_broken_by_the_smaller_index(dev):
    real, fake = FC.case("c0")
    ref, query = real.clone(), fake.clone()
    ref[200] = ref[3]
    ref[77] = ref[3]
    query[0] = ref[3]
    ref, query = ref.to(dev), query.to(dev)
    p = K.feat_colmean(ref)
    for splits in (1, 2, 3, 16):
        dist, index = M.nearest_neighbours(query, ref, 5, pivot=p, refine=False, squared=True, _splits=splits)
        assert index[0, :3].tolist() == [3, 77, 200], (splits, index[0].tolist())
        assert float(dist[0, 0]) == float(dist[0, 1]) == float(dist[0, 2]) < float(dist[0, 3])
        rd, ri = M.nearest_neighbours(query, ref, 5, pivot=p, squared=True, _splits=splits)
        assert ri[0, :3].tolist() == [3, 77, 200] and rd[0, :3].tolist() == [0.0, 0.0, 0.0] and float(rd[0, 3]) > 0
        # the bank against itself: a duplicated row finds its twin, never itself
        dist, index = M.nearest_neighbours(ref, None, 2, pivot=p, refine=False, squared=True, _splits=splits)
        assert index[3].tolist() == [77, 200] and index[77].tolist() == [3, 200] and index[200].tolist() == [3, 77]
        n3 = float(K.feat_norms(ref, p)[3])
        assert 0.0 <= float(dist[3, 0]) <= (96 + 8) * 2.0 ** -24 * 2 * n3
        rd, ri = M.nearest_neighbours(ref, None, 2, pivot=p, _splits=splits)
        assert ri[3].tolist() == [77, 200] and ri[200].tolist() == [3, 77] and rd[3].tolist() == [0.0, 0.0] and rd[77].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ 3. determinism
def test_the_two_load_paths_give_the_same_bits(dev):
    q, r, p = _banks("c0")                                                     # D = 96: sixteen-byte loads when aligned
    assert q.data_ptr() % 16 == 0 and r.data_ptr() % 16 == 0
    for kw in (dict(refine=False), dict(refine=True)):
        a = M.nearest_neighbours(q, r, 5, pivot=p, squared=True, **kw)
        for qq, rr, pp in ((_misaligned(q), r, p), (q, _misaligned(r), p), (q, r, _misaligned(p))):
            b = M.nearest_neighbours(qq, rr, 5, pivot=pp, squared=True, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a = M.nearest_neighbours(r, None, 5, pivot=p, refine=False, squared=True)
    b = M.nearest_neighbours(_misaligned(r), None, 5, pivot=p, refine=False, squared=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    r2 = M.knn_radii(r, 5, pivot=p, squared=True)
    nr, nq = K.feat_norms(r, p), K.feat_norms(q, p)
    a = K.manifold_counts(r, nr, r2, q, nq, p, 2)
    b = K.manifold_counts(_misaligned(r), nr, r2, _misaligned(q), nq, p, 2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_a_rows_result_does_not_depend_on_its_place(dev):
    q, r, p = _banks("c3")                                                     # 384 queries in 512 rows, D = 260
    for kw in (dict(refine=False), dict(refine=True)):
        dist, index = M.nearest_neighbours(q, r, 5, pivot=p, squared=True, **kw)
        assert all(torch.equal(a, b) for a, b in zip((dist, index), M.nearest_neighbours(q, r, 5, pivot=p, squared=True, **kw)))     # two calls
        for j in (0, 127, 128, 383):
            alone = M.nearest_neighbours(q[j:j + 1], r, 5, pivot=p, squared=True, **kw)
            assert torch.equal(alone[0][0], dist[j]) and torch.equal(alone[1][0], index[j]), j
        moved = M.nearest_neighbours(torch.roll(q, 131, 0), r, 5, pivot=p, squared=True, **kw)
        assert torch.equal(torch.roll(moved[0], -131, 0), dist) and torch.equal(torch.roll(moved[1], -131, 0), index)
        sub = M.nearest_neighbours(q[37:301], r, 5, pivot=p, squared=True, _splits=3, **kw)
        assert torch.equal(sub[0], dist[37:301]) and torch.equal(sub[1], index[37:301])


# ------------------------------------------------------------------------------------------------ 4. fp64, no case left out
@pytest.mark.parametrize("name", FC.ALL)
def test_unrefined_values_within_the_derived_bound_of_fp64(dev, name):
    q, r, p = _banks(name)
    D = q.shape[1]
    qt, rt = FC.centred(q.cpu(), p.cpu()), FC.centred(r.cpu(), p.cpu())
    d64 = FC.sqdist64(qt, rt)
    E = FC.bound(FC.norms(qt), FC.norms(rt), D)
    s64 = torch.sort(d64, dim=1, stable=True).values
    for k in (1, 5, 15):
        dist, index = (t.cpu() for t in M.nearest_neighbours(q, r, k, pivot=p, refine=False, squared=True))
        order = ((dist.double() - s64[:, :k]).abs() / E.max(dim=1).values[:, None]).max()
        own = ((d64.gather(1, index) - dist.double()).abs() / E.gather(1, index)).max()
        print(f"[measured] unrefined {name} k={k}: max |value_j - fp64 order statistic j| / max_i E = {float(order):.4f}, "
              f"max |fp64 d2(row, index_j) - value_j| / E = {float(own):.4f}")
        assert float(order) <= 1.0 and float(own) <= 1.0, (name, k)


# ------------------------------------------------------------------------------------------------ 5. fp64 indices under the ambiguity rule
@pytest.mark.parametrize("name", FC.ALL)
def test_indices_equal_fp64_on_unambiguous_rows(dev, name):
    q, r, p = _banks(name)
    D = q.shape[1]
    qt, rt = FC.centred(q.cpu(), p.cpu()), FC.centred(r.cpu(), p.cpu())
    for k, loo in ((1, False), (5, False), (5, True)):
        a, b = (rt, rt) if loo else (qt, rt)
        amb = NC.ambiguous_rows(a, b, D, k, leave_one_out=loo)
        assert int(amb.sum()) <= FC.AMBIGUOUS_CAP * a.shape[0], (name, k, loo, int(amb.sum()))          # a condition on the inputs, asserted first
        want = NC.nearest64(a, b, k, leave_one_out=loo)[1]
        got = M.nearest_neighbours(r if loo else q, None if loo else r, k, pivot=p, refine=False)[1].cpu()
        differ = (got != want).any(1)
        print(f"[measured] indices {name} k={k}{' leave-one-out' if loo else ''}: ambiguous rows {int(amb.sum())} of {a.shape[0]}, rows that differ from fp64 {int(differ.sum())}")
        assert torch.equal(got[~amb], want[~amb]), (name, k, loo)


# ------------------------------------------------------------------------------------------------ 6. refinement
@pytest.mark.parametrize("name", NC.ALL)
def test_refined_distances_within_four_ulps_of_fp64(dev, name):
    q, r, p = _banks(name)
    for k, loo in ((5, False), (1, True)):
        dist, index = M.nearest_neighbours(r if loo else q, None if loo else r, k, pivot=p, squared=True)
        x = (r if loo else q).cpu()
        want = NC.pair_d2_64(x, r.cpu(), index.cpu())
        got = dist.cpu().double()
        rel = ((got - want).abs() / want.clamp_min(1e-300)).max()
        print(f"[measured] refined {name} k={k}{' leave-one-out' if loo else ''}: max relative error against fp64 = {float(rel) / NC.U:.3f} x 2^-24 (bound 4)")
        assert bool(((got - want).abs() <= NC.REFINE_REL * want).all()), (name, k, loo)               # (want == 0 demands exactly 0)
        assert bool((dist[:, 1:] >= dist[:, :-1]).all())                                                # sorted again by the refined value
        cand = M.nearest_neighbours(r if loo else q, None if loo else r, k, pivot=p, refine=False)[1]
        assert torch.equal(index.sort(dim=1).values, cand.sort(dim=1).values)                           # the same candidate set


def test_an_index_outside_the_bank_never_reaches_memory(dev):
    q, r, _ = _banks("c2")
    index = torch.tensor([[-1, 0, r.shape[0] - 1, r.shape[0], 1 << 30]], dtype=torch.int32, device=dev).repeat(q.shape[0], 1).contiguous()
    out = K.pair_sqdist(q, r, index)
    inf = float("inf")
    assert bool((out[:, [0, 3, 4]] == inf).all()) and bool(torch.isfinite(out[:, 1:3]).all())
    want = NC.pair_d2_64(q.cpu(), r.cpu(), index[:, 1:3].cpu().long())
    assert bool(((out[:, 1:3].cpu().double() - want).abs() <= NC.REFINE_REL * want).all())


@pytest.mark.parametrize("name", list(NC.DROPPING))
def test_planted_copies_are_found_and_measured(dev, name):
    fake, train, p = _banks(name)
    D = train.shape[1]
    near_f, near_t = (list(v) for v in NC.PLANTED_NEAR)
    exact_f, exact_t = (list(v) for v in NC.PLANTED_EXACT)
    dist, index = M.nearest_neighbours(fake, train, NC.NEIGHBOURS, pivot=p, squared=True)
    assert dist[exact_f, 0].tolist() == [0.0, 0.0] and index[exact_f, 0].tolist() == exact_t
    assert index[near_f, 0].tolist() == near_t
    want = NC.pair_d2_64(fake.cpu(), train.cpu(), index.cpu())
    assert bool(((dist.cpu().double() - want).abs() <= NC.REFINE_REL * want).all())
    raw, raw_i = M.nearest_neighbours(fake, train, 1, pivot=p, refine=False, squared=True)
    assert raw_i[near_f, 0].tolist() == near_t                                 # the index is right; the unrefined distance is noise:
    nf, nt = K.feat_norms(fake, p).cpu().double(), K.feat_norms(train, p).cpu().double()
    for j, i in zip(near_f, near_t):
        E = (D + 8) * NC.U * float(nf[j] + nt[i])
        print(f"[measured] {name} near-copy {j} of training row {i}: fp64 d2 {float(want[j, 0]):.4e}, refined {float(dist[j, 0]):.4e}, "
              f"unrefined {float(raw[j, 0]):.4e} with its bound E = {E:.3e}")
        assert abs(float(raw[j, 0]) - float(want[j, 0])) <= E
    rep = M.memorization_report(train, fake, neighbours=NC.NEIGHBOURS)
    planted = near_f + exact_f
    others = [j for j in range(fake.shape[0]) if j not in planted]
    ratio = rep["copy_ratio"].cpu()
    print(f"[measured] {name} copy_ratio: largest planted {float(ratio[planted].max()):.5f}, smallest other {float(ratio[others].min()):.5f}")
    assert float(ratio[planted].max()) < 0.1 * float(ratio[others].min())
    assert ratio[exact_f].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ 7. density / coverage
@pytest.mark.parametrize("splits", [1, 2, 16])
@pytest.mark.parametrize("name", ["c1", "c3", "m4"])
def test_counts_and_coverage_are_the_comparison_on_the_kernels_own_matrix(dev, name, splits):
    fake, real, p = _banks(name)
    n, m = real.shape[0], fake.shape[0]
    r2 = M.knn_radii(real, NC.KNN_DC, pivot=p, squared=True)
    mat = M.pairwise_sqdist(real, fake, pivot=p)
    want = (mat < r2[:, None]).sum(0)
    nr, nf = K.feat_norms(real, p), K.feat_norms(fake, p)
    count, total = K.manifold_counts(real, nr, r2, fake, nf, p, splits)
    assert count.dtype == torch.int32 and total.dtype == torch.int64 and torch.equal(count.long(), want) and int(total) == int(want.sum()) > 0
    assert int(K.manifold_counts(real, nr, r2, fake, nf, p, splits, want_counts=False)[1]) == int(want.sum())
    covered = mat.min(1).values < r2
    out = M.density_coverage(real, fake, NC.KNN_DC, _splits=splits)
    assert out == {"density": int(want.sum()) / (NC.KNN_DC * m), "coverage": int(covered.sum()) / n, "n_real": n, "n_fake": m, "knn": NC.KNN_DC}
    assert out == M.density_coverage(real, fake, NC.KNN_DC)
    nearest = M.nearest_neighbours(real, fake, 1, pivot=p, refine=False, squared=True, _splits=splits)[0][:, 0]
    assert torch.equal(nearest < r2, covered)


@pytest.mark.parametrize("splits", [1, 2, 16])
def test_a_hit_is_a_nonzero_count(dev, splits):
    """the flag and the count are one kernel body over one tile: query j is inside some ball exactly when it is inside at least one"""
    like, wide = _random_banks(257 + 65, 65, 36, seed=29)
    ref, query = like[:257].to(dev), torch.cat([like[257:], wide]).to(dev)    # [257, 36]: 3 reference tiles, the last of one row; [130, 36]: 2 query
    p = K.feat_colmean(ref)                                                    # tiles, half of them drawn like the bank, half wider: in fp64 52 inside
    nr, nq = K.feat_norms(ref, p), K.feat_norms(query, p)
    r2 = M.knn_radii(ref, NC.KNN_DC, pivot=p, squared=True)
    hit, hits = K.manifold_hits(ref, nr, r2, query, nq, p, splits)
    count, _ = K.manifold_counts(ref, nr, r2, query, nq, p, splits)
    assert torch.equal(hit.bool(), count > 0) and int(hits) == int((count != 0).sum())
    assert 0 < int(hits) < 130                                                 # (both answers occur)


@pytest.mark.parametrize("name", NC.ALL + ("m4-", "m5-"))
def test_density_coverage_against_fp64_within_the_ambiguous_pairs(dev, name):
    fake, real, p = _banks(name)
    n, m, D = real.shape[0], fake.shape[0], real.shape[1]
    want = NC.density_coverage64(FC.centred(real.cpu(), p.cpu()), FC.centred(fake.cpu(), p.cpu()), D, NC.KNN_DC)
    amb_pairs, amb_rows = int(want["ambiguous_pairs"].sum()), want["ambiguous_rows"]
    assert amb_pairs <= 0.001 * n * m, (name, amb_pairs)                      # conditions on the inputs
    assert int(amb_rows.sum()) <= (0 if name in FC.ALL else FC.AMBIGUOUS_CAP * n)
    r2 = M.knn_radii(real, NC.KNN_DC, pivot=p, squared=True)
    count, total = K.manifold_counts(real, K.feat_norms(real, p), r2, fake, K.feat_norms(fake, p), p, F.plan_splits(m, n))
    covered = (M.nearest_neighbours(real, fake, 1, pivot=p, refine=False, squared=True)[0][:, 0] < r2).cpu()
    out = M.density_coverage(real, fake, NC.KNN_DC)
    print(f"[measured] {name} density {out['density']:.5f} (fp64 {want['density']:.5f}) coverage {out['coverage']:.5f} (fp64 {want['coverage']:.5f}); "
          f"ambiguous pairs {amb_pairs} of {n * m}, sum of counts differs by {abs(int(total) - int(want['count'].sum()))}; "
          f"ambiguous rows {int(amb_rows.sum())}, coverage decisions that differ {int((covered != want['covered']).sum())}")
    assert abs(int(total) - int(want["count"].sum())) <= amb_pairs
    assert bool(((count.cpu().long() - want["count"]).abs() <= want["ambiguous_pairs"].sum(0)).all())
    assert torch.equal(covered[~amb_rows], want["covered"][~amb_rows])
    assert out["density"] == int(total) / (NC.KNN_DC * m) and out["coverage"] == int(covered.sum()) / n
    if name.endswith("-"):                                                     # the recorded table (its density: one count, tests/test_neighbours_cpu.py)
        density, coverage, _ = NC.TABLE[name[:-1]]
        assert abs(int(total) - round(density * NC.KNN_DC * m)) <= amb_pairs + 1
        assert abs(int(covered.sum()) - round(coverage * n)) <= int(amb_rows.sum())


# ------------------------------------------------------------------------------------------------ 8. the report
@pytest.mark.parametrize("name", ["c0", "m4", "m5", "m4-"])
def test_memorization_report_against_fp64(dev, name):
    fake, train, _ = _banks(name)
    m = fake.shape[0]
    want = NC.memorization64(train.cpu(), fake.cpu(), NC.NEIGHBOURS)
    torch.manual_seed(3)
    state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    rep = M.memorization_report(train, fake, neighbours=NC.NEIGHBOURS)
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)       # nothing drawn
    for key, dtype in (("nearest_index", torch.int64), ("nearest_dist", torch.float32), ("train_gap", torch.float32), ("authentic", torch.bool),
                       ("copy_ratio", torch.float32)):
        assert rep[key].shape == (m,) and rep[key].dtype == dtype and rep[key].is_cuda, key
    assert isinstance(rep["authenticity"], float) and (rep["n_train"], rep["n_fake"], rep["neighbours"]) == (train.shape[0], m, NC.NEIGHBOURS)
    # a distance is sqrt of a d2 within 4 2^-24 relative: within 3 2^-24 relative itself (half of 4, the square root's own rounding)
    slack = 3 * NC.U * (want["nearest_dist"] + want["train_gap"])
    close = (want["nearest_dist"] - want["train_gap"]).abs() <= slack
    print(f"[measured] {name} authenticity {rep['authenticity']:.5f} (fp64 {want['authenticity']:.5f}); rows within the refinement bound of their gap: {int(close.sum())} of {m}")
    assert int(close.sum()) == 0                                               # none on the chosen inputs
    assert torch.equal(rep["nearest_index"].cpu(), want["nearest_index"])
    assert torch.equal(rep["authentic"].cpu(), want["authentic"]) and rep["authenticity"] == int(want["authentic"].sum()) / m
    assert bool(((rep["nearest_dist"].cpu().double() - want["nearest_dist"]).abs() <= 3 * NC.U * want["nearest_dist"]).all())
    assert bool(((rep["train_gap"].cpu().double() - want["train_gap"]).abs() <= 3 * NC.U * want["train_gap"]).all())
    # the ratio: 3u on either distance, the fp32 mean and the division a few u more (<= 8u = 5e-7), and a candidate within E of the k-th that the
    # selection on d2 exchanged for its neighbour moves the mean by at most E / (2 k d2_k) ~ 1e-6 on these inputs: 1e-5
    ok = ~torch.isnan(want["copy_ratio"])
    assert bool(((rep["copy_ratio"].cpu().double() - want["copy_ratio"])[ok].abs() <= 1e-5 * want["copy_ratio"][ok]).all())
    if name.endswith("-"):
        assert abs(rep["authenticity"] - NC.TABLE[name[:-1]][2]) < 5e-4


# ------------------------------------------------------------------------------------------------ 9. memory: the fusion is real
def test_nearest_neighbours_never_holds_the_matrix(dev):
    n = m = 4096
    ref, query = (t.to(dev) for t in FC.make(5, n, m, 64))
    K.Workspace.get(16 * m * 16 * 8, dev)                                      # the partial lists at S = 16: 8 MiB, part of the budget below
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    dist, index = M.nearest_neighbours(query, ref, 10, _splits=16)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(dev) - before + 16 * m * 16 * 8
    print(f"[measured] nearest_neighbours 4096 x 4096 x 64, k = 10: peak allocation above the inputs {extra / 2 ** 20:.2f} MiB (one fp32 matrix: 64 MiB)")
    assert extra < n * m * 4 // 4                                              # under a quarter of ONE materialised matrix: 16 MiB
    assert K.nn_workspace_bytes(K.make_fidelity_desc(n, m, 64, 10, 16)) == 16 * 4096 * 16 * 8
    raw = M.nearest_neighbours(query, ref, 10, refine=False, squared=True)     # 32 x 32 tiles, the planner's splits: the materialised form
    want = torch.sort(M.pairwise_sqdist(query, ref, pivot=K.feat_colmean(ref)), dim=1, stable=True)
    assert torch.equal(raw[0], want.values[:, :10]) and torch.equal(raw[1], want.indices[:, :10])
    assert torch.equal(index.sort(dim=1).values, raw[1].sort(dim=1).values) and bool((dist[:, 1:] >= dist[:, :-1]).all())


# ------------------------------------------------------------------------------------------------ 10. the meter and the script
def test_meter_switches_add_the_new_figures(dev):
    real, fake = (t.to(dev) for t in FC.case("c2"))
    meter = M.FidelityMeter(lambda t: t, knn=3)
    meter.update(real[:50], real=True)
    meter.update(fake, real=False)
    meter.update(real[50:], real=True)
    plain = meter.compute()
    assert set(plain) == {"precision", "recall", "n_real", "n_fake", "knn", "fd"}
    want = M.precision_recall(real, fake, 3)
    assert {key: plain[key] for key in want} == want and plain["fd"] == M.frechet_distance(real, fake)
    both = meter.compute(density_coverage=True, memorization=True)
    assert set(both) == set(plain) | {"density", "coverage", "authenticity", "memorization"} and {key: both[key] for key in plain} == plain
    dc = M.density_coverage(real, fake, 3)
    rep = M.memorization_report(real, fake, neighbours=10)
    assert (both["density"], both["coverage"], both["authenticity"]) == (dc["density"], dc["coverage"], rep["authenticity"])
    for key in ("nearest_index", "nearest_dist", "train_gap", "authentic", "copy_ratio"):
        assert torch.equal(both["memorization"][key], rep[key]), key
    assert set(meter.compute(density_coverage=True)) == set(plain) | {"density", "coverage"}


def test_nearest_train_script_lists_the_copies_first(dev, tmp_path):
    import numpy as np
    from PIL import Image
    g = np.random.default_rng(0)
    (tmp_path / "train").mkdir()
    (tmp_path / "fake").mkdir()
    train = g.integers(0, 256, (12, 16, 16), dtype=np.uint8)
    fake = g.integers(0, 256, (6, 16, 16), dtype=np.uint8)
    fake[4], fake[1] = train[7], train[2]                                      # two copies
    for i, a in enumerate(train):
        Image.fromarray(a).save(tmp_path / "train" / f"t{i:02d}.png")
    for i, a in enumerate(fake):
        Image.fromarray(a).save(tmp_path / "fake" / f"f{i:02d}.png")
    nt = _script("nearest_train")
    res = nt.main(["--train", str(tmp_path / "train"), "--fake", str(tmp_path / "fake"), "--features", "pixels", "--neighbours", "10", "--top", "4",
                   "--out", str(tmp_path / "out")])
    assert json.loads((tmp_path / "out" / "nearest_train.json").read_text())["top"] == res["top"] and len(res["top"]) == 4
    first = {(e["fake"].split("/")[-1], e["nearest"][0]["train"].split("/")[-1], e["nearest"][0]["dist"]) for e in res["top"][:2]}
    assert first == {("f01.png", "t02.png", 0.0), ("f04.png", "t07.png", 0.0)} and res["exact_copies"] == 2
    assert [e["fake"].split("/")[-1] for e in res["top"][:2]] == ["f01.png", "f04.png"]
    assert all(e["copy_ratio"] > 0.5 for e in res["top"][2:]) and not res["top"][0]["authentic"] and not res["top"][1]["authentic"]
    assert res["authenticity"] <= 4 / 6 and res["feature_width"] == 256 and res["n_train"] == 12
    sheet = np.asarray(Image.open(tmp_path / "out" / "nearest_train.png"))
    assert sheet.shape[:2] == (4 * 16, 4 * 16)
    assert np.array_equal(sheet[:16, :16, 0] if sheet.ndim == 3 else sheet[:16, :16], fake[1])
