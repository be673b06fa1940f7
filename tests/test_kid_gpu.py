"""Kernel distances on a real MI355X (medfusion_amd/fidelity.py, csrc/fidelity.hip) against the fp64 restatement and the DERIVED bounds of
tests/kid_cases.py: the kernel matrix elementwise with no case left out, the bit-identity of its elements across load paths, places and transposition,
the fused sums against the exact sum of the kernel's own matrix, gathered subsets against their materialised rows bit for bit, mmd2 and kid against
fp64 with the same index lists, determinism, the memory a call takes, and the meter and the script."""
import functools
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import fidelity as F
from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from tests import fidelity_cases as FC
from tests import kid_cases as KC
from tests.test_neighbours_cpu import _script
from tests.test_neighbours_gpu import _misaligned

DEV = "cuda:0"
KINDS = tuple(("poly", d) for d in KC.DEGREES) + (("rbf", 0),)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device(DEV)


@functools.lru_cache(maxsize=None)
def _banks(name):
    """(real, fake) of a case on the device"""
    return tuple(t.to(DEV) for t in KC.case(name))


@functools.lru_cache(maxsize=None)
def _rbf(name):
    """(gamma, pivot on the host) of a case's rbf runs: a bandwidth that keeps gamma d2 of order 1, and the pivot the library takes -- the fp64 column
    mean of real rounded to fp32 (a tie may fall either way: the restatement runs on the device's)"""
    real = KC.case(name)[0]
    pivot, want = K.feat_colmean(_banks(name)[0]).cpu(), FC.pivot_of(real)
    assert float((pivot - want).abs().max()) <= float(want.abs().max()) * 2.0 ** -23
    return KC.rbf_gamma(real), pivot


def _kw(name, kind, degree):
    """the keyword arguments of the library call and of the fp64 restatement for one kernel on one case"""
    if kind == "poly":
        return dict(kernel="poly", degree=degree), dict(kernel="poly", degree=degree)
    gamma, pivot = _rbf(name)
    return dict(kernel="rbf", gamma=gamma), dict(kernel="rbf", gamma=gamma, pivot=pivot)


def _exact_sum(t):
    """the exactly rounded sum of a tensor's entries as fp64 numbers (math.fsum: no summation error at all)"""
    return math.fsum(t.double().flatten().tolist())


def _desc(a, b, S=1, sa=None, sb=None, same=0, kind="poly", degree=3, gamma=None):
    return K.make_ksum_desc(a.shape[0], b.shape[0], a.shape[1], S, sa, sb, kernel=F.KERNELS[kind], degree=degree if kind == "poly" else 0,
                            gamma=KC.gamma_default(a.shape[1]) if gamma is None else gamma, coef0=1.0, same_bank=same)


def _operands(name, kind, *banks):
    """(pivot on the device, the norms of the banks) as the library forms them"""
    first = banks[0]
    if kind == "poly":
        return torch.zeros(first.shape[1], device=first.device), [None] * len(banks)
    c = _rbf(name)[1].to(first.device)
    return c, [K.feat_norms(b, c) for b in banks]


# ------------------------------------------------------------------------------------------------ 1. the matrix against fp64, elementwise
@pytest.mark.parametrize("name", KC.SHAPE_CASES + ("inception+64",))
def test_kernel_matrix_within_the_derived_bound_of_fp64(dev, name):
    x, y = _banks(name)
    for kind, degree in KINDS:
        lib_kw, ref_kw = _kw(name, kind, degree)
        for a, b, ah, bh in ((x, y, *KC.case(name)), (x, None, KC.case(name)[0], KC.case(name)[0])):
            got = M.kernel_matrix(a, b, **lib_kw)
            k, E = KC.kernel64(ah, bh, **ref_kw)
            assert got.shape == k.shape and got.dtype == torch.float32
            ratio = float(((got.cpu().double() - k).abs() / E).max())
            print(f"[measured] kernel_matrix {name} {tuple(k.shape)} D={ah.shape[1]} {kind}{degree or ''}: max |k - fp64| / E = {ratio:.4f}")
            assert ratio <= 1.0, (name, kind, degree)
    if name == "s0":                                                            # the scalars are honoured: another gamma and coef0, a pivot for poly
        got = M.kernel_matrix(x, y, degree=2, gamma=0.25, coef0=0.5)
        k, E = KC.kernel64(*KC.case(name), degree=2, gamma=0.25, coef0=0.5)
        assert float(((got.cpu().double() - k).abs() / E).max()) <= 1.0
        p = FC.pivot_of(KC.case(name)[0])
        got = M.kernel_matrix(x, y, degree=3, pivot=p.to(dev))
        xs, ys = (FC.centred(t, p).float() for t in KC.case(name))              # (exact: the centred rows ARE fp32 numbers)
        k, E = KC.kernel64(xs, ys, degree=3, gamma=KC.gamma_default(x.shape[1]))
        assert float(((got.cpu().double() - k).abs() / E).max()) <= 1.0


# ------------------------------------------------------------------------------------------------ 2. the bits of an element
def _padded(t, to):
    out = torch.zeros(t.shape[0], to, device=t.device)
    out[:, :t.shape[1]] = t
    return out


def test_the_two_load_paths_give_the_same_bits(dev):
    x, y = _banks("s2")                                                        # D = 36: sixteen-byte loads when aligned
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0 and x.shape[1] % 4 == 0
    for kind, degree in KINDS:
        kw = _kw("s2", kind, degree)[0]
        p = _operands("s2", kind, x)[0]
        a = M.kernel_matrix(x, y, pivot=p, **kw)
        for xx, yy, pp in ((_misaligned(x), y, p), (x, _misaligned(y), p), (x, y, _misaligned(p))):
            assert torch.equal(M.kernel_matrix(xx, yy, pivot=pp, **kw), a), (kind, degree)
    x, y = _banks("s0")                                                        # D = 33: element loads; three zero columns more: D = 36, sixteen-byte loads
    g = KC.gamma_default(33)
    for kind, degree in KINDS:
        kw = dict(_kw("s0", kind, degree)[0])
        kw.setdefault("gamma", g)
        p = _operands("s0", kind, x)[0]
        a = M.kernel_matrix(x, y, pivot=p, **kw)
        assert torch.equal(M.kernel_matrix(_padded(x, 36), _padded(y, 36), pivot=_padded(p[None], 36)[0], **kw), a), (kind, degree)
    # the fused sums: mmd2 through either path
    real, fake = _banks("mixture")                                             # D = 64
    for kw in (dict(), dict(kernel="rbf", gamma=_rbf("mixture")[0])):
        a = M.mmd2(real, fake, **kw)
        for rr, ff in ((_misaligned(real), fake), (real, _misaligned(fake)), (_misaligned(real), _misaligned(fake))):
            assert torch.equal(M.mmd2(rr, ff, **kw), a)


def test_an_element_does_not_depend_on_its_place_and_the_kernel_is_symmetric(dev):
    for name in ("s0", "s4"):
        x, y = _banks(name)
        for kind, degree in KINDS:
            kw = _kw(name, kind, degree)[0]
            p = _operands(name, kind, x)[0]
            full = M.kernel_matrix(x, y, pivot=p, **kw)
            assert torch.equal(M.kernel_matrix(y, x, pivot=p, **kw), full.t()), (name, kind, degree)          # k(i, j) == k(j, i)
            own = M.kernel_matrix(x, pivot=p, **kw)
            assert torch.equal(own, own.t())
            for i in (0, 127, 128):
                assert torch.equal(M.kernel_matrix(x[i:i + 1], y, pivot=p, **kw)[0], full[i]), (name, kind, i)
            moved = M.kernel_matrix(torch.roll(x, 5, 0), torch.roll(y, 131, 0), pivot=p, **kw)
            assert torch.equal(torch.roll(torch.roll(moved, -5, 0), -131, 1), full)
            assert torch.equal(M.kernel_matrix(x[3:100], y[120:], pivot=p, **kw), full[3:100, 120:])


# ------------------------------------------------------------------------------------------------ 3. the fused sums against the kernel's own matrix
def _check_sums(label, got, blocks, same, diag):
    """got [S] fp64 from the device; blocks: the S sub-matrices of the kernel's own fp32 matrix"""
    worst = 0.0
    for s, block in enumerate(blocks):
        want = _exact_sum(block) - (_exact_sum(block.diagonal()) if same and not diag else 0.0)
        bound = KC.sum_bound(block.double())
        ratio = abs(float(got[s]) - want) / bound
        worst = max(worst, ratio)
        assert ratio <= 1.0, (label, s, float(got[s]), want)
    print(f"[measured] fused sums {label}: max |sum - exact sum of the kernel's own matrix| / ((n - 1) 2^-53 sum |k|) = {worst:.2e}")


@pytest.mark.parametrize("kind,degree", [("poly", 3), ("poly", 1), ("rbf", 0)])
def test_fused_sums_equal_the_sum_of_the_kernels_own_matrix(dev, kind, degree):
    # one bank of 257 rows: three row tiles, a half grid with diagonal tiles
    x, _ = _banks("s4")
    kw = _kw("s4", kind, degree)[0]
    gamma = kw.get("gamma")
    c, (nx,) = _operands("s4", kind, x)
    own = M.kernel_matrix(x, pivot=c, **kw).cpu()
    for same, diag in ((1, False), (2, True)):
        got = K.kernel_sums(x, nx, None, x, nx, None, c, _desc(x, x, same=same, kind=kind, degree=degree, gamma=gamma)).cpu()
        _check_sums(f"{kind}{degree or ''} one bank of 257 rows, diagonal {'counted' if diag else 'left out'}", got, [own], True, diag)
    full = K.kernel_sums(x, nx, None, x, nx, None, c, _desc(x, x, kind=kind, degree=degree, gamma=gamma)).cpu()     # the same pairs over the FULL grid
    _check_sums(f"{kind}{degree or ''} one bank of 257 rows as two banks", full, [own], False, True)
    # two banks with tails in both axes
    x, y = _banks("s0")
    kw = _kw("s0", kind, degree)[0]
    gamma = kw.get("gamma")
    c, (nx, ny) = _operands("s0", kind, x, y)
    mat = M.kernel_matrix(x, y, pivot=c, **kw).cpu()
    got = K.kernel_sums(x, nx, None, y, ny, None, c, _desc(x, y, kind=kind, degree=degree, gamma=gamma)).cpu()
    _check_sums(f"{kind}{degree or ''} two banks 129 x 257", got, [mat], False, True)
    # S = 3 subsets of 128 and of 130 rows, gathered
    real, fake = _banks("mixture")
    kw = _kw("mixture", kind, degree)[0]
    gamma = kw.get("gamma")
    c, (nr, nf) = _operands("mixture", kind, real, fake)
    kxx, kxy = M.kernel_matrix(real, pivot=c, **kw).cpu(), M.kernel_matrix(real, fake, pivot=c, **kw).cpu()
    for size in (128, 130):
        ia, ib = F.draw_subsets(real.shape[0], fake.shape[0], 3, size, seed=size)
        da, db = ia.to(dev), ib.to(dev)
        got = K.kernel_sums(real, nr, da, real, nr, da, c, _desc(real, real, 3, size, size, same=1, kind=kind, degree=degree, gamma=gamma)).cpu()
        _check_sums(f"{kind}{degree or ''} 3 subsets of {size} of one bank", got, [kxx[a.long()][:, a.long()] for a in ia], True, False)
        got = K.kernel_sums(real, nr, da, fake, nf, db, c, _desc(real, fake, 3, size, size, kind=kind, degree=degree, gamma=gamma)).cpu()
        _check_sums(f"{kind}{degree or ''} 3 subsets of {size} of two banks", got, [kxy[a.long()][:, b.long()] for a, b in zip(ia, ib)], False, True)


# ------------------------------------------------------------------------------------------------ 4. gathered subsets, bit for bit
@pytest.mark.parametrize("kind,degree", [("poly", 3), ("rbf", 0)])
def test_a_gathered_subset_gives_the_bits_of_its_materialised_rows(dev, kind, degree):
    real, fake = _banks("mixture")
    gamma = _kw("mixture", kind, degree)[0].get("gamma")
    c, (nr, nf) = _operands("mixture", kind, real, fake)
    for size in (128, 130):
        ia, ib = (t.to(dev) for t in F.draw_subsets(real.shape[0], fake.shape[0], 3, size, seed=7))
        d = functools.partial(_desc, kind=kind, degree=degree, gamma=gamma)
        sxx = K.kernel_sums(real, nr, ia, real, nr, ia, c, d(real, real, 3, size, size, same=1))
        sxy = K.kernel_sums(real, nr, ia, fake, nf, ib, c, d(real, fake, 3, size, size))
        for s in range(3):
            xs, ys = real[ia[s].long()].contiguous(), fake[ib[s].long()].contiguous()
            ns, ms = (None, None) if kind == "poly" else (K.feat_norms(xs, c), K.feat_norms(ys, c))
            assert torch.equal(K.kernel_sums(xs, ns, None, xs, ns, None, c, d(xs, xs, same=1))[0], sxx[s]), (size, s)
            assert torch.equal(K.kernel_sums(xs, ns, None, ys, ms, None, c, d(xs, ys))[0], sxy[s]), (size, s)
    # an explicit identity list gives the bits of no list
    n, m = real.shape[0], fake.shape[0]
    ida, idb = torch.arange(n, dtype=torch.int32, device=dev)[None], torch.arange(m, dtype=torch.int32, device=dev)[None]
    assert torch.equal(K.kernel_sums(real, nr, ida, real, nr, ida, c, d(real, real, same=1)), K.kernel_sums(real, nr, None, real, nr, None, c, d(real, real, same=1)))
    assert torch.equal(K.kernel_sums(real, nr, ida, fake, nf, idb, c, d(real, fake)), K.kernel_sums(real, nr, None, fake, nf, None, c, d(real, fake)))
    # an index outside the bank is clamped into it before any load
    wild = torch.tensor([[-5, 0, n - 1, n, 1 << 30]], dtype=torch.int32, device=dev)
    tame = torch.tensor([[0, 0, n - 1, n - 1, n - 1]], dtype=torch.int32, device=dev)
    assert torch.equal(K.kernel_sums(real, nr, wild, fake, nf, wild, c, d(real, fake, 1, 5, 5)), K.kernel_sums(real, nr, tame, fake, nf, tame.clamp(max=m - 1), c, d(real, fake, 1, 5, 5)))
    if kind == "poly":                                                          # the public face of the same statement: one drawn subset is mmd2 of its rows
        for size in (128, 130):
            ia, ib = F.draw_subsets(n, m, 1, size, seed=3)
            one = M.kid(real, fake, subsets=1, subset_size=size, seed=3)
            assert one["kid_mean"] == float(M.mmd2(real[ia[0].long().to(dev)], fake[ib[0].long().to(dev)])) and one["kid_std"] == 0.0


# ------------------------------------------------------------------------------------------------ 5. the statistics against fp64
@pytest.mark.parametrize("name", ["mixture", "same", "inception", "s1"])
def test_mmd2_within_the_summed_bound_of_fp64(dev, name):
    real, fake = _banks(name)
    for kw_lib, kw_ref in (_kw(name, "poly", 3), _kw(name, "poly", 2), _kw(name, "rbf", 0)):
        for unbiased in (True, False):
            want, terms, bound = KC.mmd2_64(*KC.case(name), unbiased=unbiased, **kw_ref)
            got, got_terms = M.mmd2(real, fake, unbiased=unbiased, return_terms=True, **kw_lib)
            assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda and all(t.dim() == 0 and t.dtype == torch.float64 for t in got_terms.values())
            print(f"[measured] mmd2 {name} {kw_lib} unbiased={unbiased}: {float(got):.9e} (fp64 {want:.9e}), |error| / bound = {abs(float(got) - want) / bound:.4f}, "
                  f"bound / |figure| = {bound / abs(want):.2e}")
            assert abs(float(got) - want) <= bound, (name, kw_lib, unbiased)
            assert all(abs(float(got_terms[key]) - terms[key]) <= bound for key in terms)
            assert torch.equal(M.mmd2(real, fake, unbiased=unbiased, **kw_lib), got)
            if name == "mixture" and unbiased:
                assert bound < 0.1 * abs(want)                                  # about the fp64 reference: the case is informative


def test_the_offset_case_stays_within_its_rbf_bound_where_the_uncentred_formula_does_not(dev):
    real, fake = _banks("inception+64")
    rh, fh = KC.case("inception+64")
    gamma, pivot = _rbf("inception+64")
    want, _, bound = KC.mmd2_64(rh, fh, kernel="rbf", gamma=gamma, pivot=pivot)
    got = float(M.mmd2(real, fake, kernel="rbf", gamma=gamma))
    n, m = rh.shape[0], fh.shape[0]
    kxx, kyy, kxy = (torch.exp(-gamma * FC.plain_torch_sqdist(a, b)) for a, b in ((real, real), (fake, fake), (real, fake)))     # un-centred, fp32, on the device
    plain = float((kxx.double().sum() - kxx.double().diagonal().sum()) / (n * (n - 1)) + (kyy.double().sum() - kyy.double().diagonal().sum()) / (m * (m - 1))
                  - 2 * kxy.double().sum() / (n * m))
    k64, E = KC.kernel64(rh, fh, kernel="rbf", gamma=gamma, pivot=pivot)
    elementwise = float(((kxy.cpu().double() - k64).abs() / E).max())
    print(f"[measured] mmd2 inception+64 rbf: {got:.9e} (fp64 {want:.9e}), |error| / bound = {abs(got - want) / bound:.4f}; the un-centred fp32 formula: "
          f"statistic |error| / bound = {abs(plain - want) / bound:.2f}, elements max |k - fp64| / E = {elementwise:.1f}")
    assert abs(got - want) <= bound
    assert elementwise > 1.0                                                    # the un-centred elements leave the bound (the statistic averages some of it away)


@pytest.mark.parametrize("name", ["mixture", "same"])
def test_kid_within_the_summed_bound_of_fp64_with_the_same_lists(dev, name):
    real, fake = _banks(name)
    n, m = real.shape[0], fake.shape[0]
    for subsets, size, seed in ((3, 128, 0), (3, 130, 1), (5, 257, 2)):
        ia, ib = F.draw_subsets(n, m, subsets, size, seed)
        mean, std, values, e_mean, e_std = KC.kid64(*KC.case(name), ia, ib)
        got = M.kid(real, fake, subsets=subsets, subset_size=size, seed=seed)
        assert set(got) == {"kid_mean", "kid_std", "subsets", "subset_size", "n_real", "n_fake"}
        assert (got["subsets"], got["subset_size"], got["n_real"], got["n_fake"]) == (subsets, size, n, m)
        print(f"[measured] kid {name} {subsets} x {size}: mean {got['kid_mean']:.9e} (fp64 {mean:.9e}) |error| / bound = {abs(got['kid_mean'] - mean) / e_mean:.4f}; "
              f"std {got['kid_std']:.9e} (fp64 {std:.9e}) |error| / bound = {abs(got['kid_std'] - std) / e_std:.4f}; bound / |mean| = {e_mean / abs(mean):.2e}")
        assert abs(got["kid_mean"] - mean) <= e_mean and abs(got["kid_std"] - std) <= e_std, (name, subsets, size)
        if name == "mixture":
            assert e_mean < 0.1 * abs(mean) and mean > 3e-3
    full = M.kid(real, fake, subsets=None)
    want, _, bound = KC.mmd2_64(*KC.case(name), kernel="poly")
    assert full["kid_std"] is None and full["subsets"] is None and full["subset_size"] is None and abs(full["kid_mean"] - want) <= bound
    assert full["kid_mean"] == float(M.mmd2(real, fake))
    other = M.kid(real, fake, subsets=3, subset_size=128, degree=2, gamma=0.05, coef0=0.5)
    ia, ib = F.draw_subsets(n, m, 3, 128, 0)
    mean, std, _, e_mean, e_std = KC.kid64(*KC.case(name), ia, ib, degree=2, gamma=float(torch.tensor(0.05).float()), coef0=0.5)
    assert abs(other["kid_mean"] - mean) <= e_mean and abs(other["kid_std"] - std) <= e_std


# ------------------------------------------------------------------------------------------------ 6. determinism
def test_two_calls_give_the_same_bits_and_the_seed_decides_the_lists(dev):
    real, fake = _banks("mixture")
    torch.manual_seed(11)
    state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    a = M.kid(real, fake, subsets=4, subset_size=130, seed=9)
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(torch.cuda.get_rng_state(dev), dev_state)       # nothing drawn from torch's generators
    torch.manual_seed(12)
    assert M.kid(real, fake, subsets=4, subset_size=130, seed=9) == a
    b = M.kid(real, fake, subsets=4, subset_size=130, seed=10)
    assert not torch.equal(F.draw_subsets(300, 257, 4, 130, 9)[0], F.draw_subsets(300, 257, 4, 130, 10)[0]) and b["kid_mean"] != a["kid_mean"]
    for kw in (dict(), dict(unbiased=False), dict(kernel="rbf", gamma=_rbf("mixture")[0]), dict(degree=4)):
        first = M.mmd2(real, fake, **kw)
        assert all(torch.equal(M.mmd2(real, fake, **kw), first) for _ in range(3))
    assert torch.equal(M.kernel_matrix(real, fake), M.kernel_matrix(real, fake))


# ------------------------------------------------------------------------------------------------ 7. memory and synchronisation: the fusion is real
def test_kid_never_holds_a_matrix_and_mmd2_does_not_wait(dev):
    n = m = 2048
    real, fake = (t.to(dev) for t in KC.make("mixture", 5, n, m, 64))
    plan = M.plan_kid(n, m, 100, 1000)
    K.Workspace.get(plan["workspace_bytes"], dev)                              # the planned workspace: part of the budget below
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = M.kid(real, fake)                                                     # 100 x 1000
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(dev) - before
    slack = 64 << 10                                                            # the zero pivot, three [100] fp64 sums, the values and the allocator's 512-byte blocks
    print(f"[measured] kid 2048 x 2048 x 64, 100 x 1000: peak allocation above the inputs {extra / 2 ** 10:.1f} KiB + planned workspace "
          f"{plan['workspace_bytes'] / 2 ** 10:.1f} KiB (index lists {plan['index_bytes'] / 2 ** 10:.1f} KiB; one fp32 matrix of the full sets {n * m * 4 / 2 ** 20:.0f} MiB, "
          f"the materialised subsets {plan['matrix_bytes'] / 2 ** 20:.0f} MiB)")
    assert extra <= plan["index_bytes"] + slack
    assert extra + plan["workspace_bytes"] < n * m * 4 // 8 and extra + plan["workspace_bytes"] < 1000 * 1000 * 4      # nothing of N M 4 bytes, nor one subset's matrix
    assert out["kid_mean"] > 0 and out["subsets"] == 100 and out["subset_size"] == 1000
    # mmd2 enqueues and returns: no synchronising call of torch's inside it (the workspace and the library are warm)
    M.mmd2(real, fake)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        value, terms = M.mmd2(real, fake, return_terms=True)
        biased = M.mmd2(real, fake, kernel="rbf", gamma=0.05, unbiased=False)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert value.is_cuda and biased.is_cuda and float(value) > 0 and float(biased) > 0 and float(terms["kxy"]) > 0


# ------------------------------------------------------------------------------------------------ 8. the meter and the script
def test_meter_adds_the_kid_keys(dev):
    real, fake = (t.to(dev) for t in FC.case("c2"))                             # 130 and 129 rows
    plain_meter, meter, tuned = M.FidelityMeter(lambda t: t, knn=3), M.FidelityMeter(lambda t: t, knn=3, kid=True), \
        M.FidelityMeter(lambda t: t, knn=3, kid=dict(subsets=4, subset_size=64, degree=2, seed=5))
    for mt in (plain_meter, meter, tuned):
        mt.update(real[:50], real=True)
        mt.update(fake, real=False)
        mt.update(real[50:], real=True)
    plain = plain_meter.compute()
    assert set(plain) == {"precision", "recall", "n_real", "n_fake", "knn", "fd"}
    both = meter.compute()
    assert set(both) == set(plain) | {"kid_mean", "kid_std", "kid_subsets", "kid_subset_size"} and {key: both[key] for key in plain} == plain
    want = M.kid(real, fake, subset_size=129)                                  # the default 1000, cut to the smaller bank
    assert (both["kid_mean"], both["kid_std"], both["kid_subsets"], both["kid_subset_size"]) == (want["kid_mean"], want["kid_std"], 100, 129)
    got = tuned.compute(density_coverage=True)
    want = M.kid(real, fake, subsets=4, subset_size=64, degree=2, seed=5)
    assert (got["kid_mean"], got["kid_std"], got["kid_subsets"], got["kid_subset_size"]) == (want["kid_mean"], want["kid_std"], 4, 64) and "density" in got


def test_evaluate_images_writes_the_kid_keys_only_when_asked(dev, tmp_path, capsys):
    real, fake = FC.case("c2")
    torch.save(real, tmp_path / "real.pt")
    torch.save(fake, tmp_path / "fake.pt")
    ev = _script("evaluate_images")
    args = ["--real", str(tmp_path / "real.pt"), "--fake", str(tmp_path / "fake.pt")]
    plain = ev.main(args + ["--out", str(tmp_path / "plain")])
    assert set(plain) == {"precision", "recall", "n_real", "n_fake", "knn", "fd", "real", "fake", "features", "feature_width", "inception"}
    log = next((tmp_path / "plain").glob("metrics_*.log")).read_text()
    assert "KID" not in log and [line.split(":")[0] for line in log.splitlines()] == ["Samples Real", "Samples Fake", "Inception features", "FD (features", "Precision"]
    assert json.loads(next((tmp_path / "plain").glob("metrics_*.json")).read_text()) == plain
    res = ev.main(args + ["--out", str(tmp_path / "kid"), "--kid", "3", "--kid-subset-size", "8"])
    want = M.kid(real.to(dev), fake.to(dev), subsets=3, subset_size=8)
    assert {key: res[key] for key in plain if key not in ("real", "fake")} == {key: plain[key] for key in plain if key not in ("real", "fake")}
    assert (res["kid_mean"], res["kid_std"], res["kid_subsets"], res["kid_subset_size"]) == (want["kid_mean"], want["kid_std"], 3, 8)
    assert set(res) == set(plain) | {"kid_mean", "kid_std", "kid_subsets", "kid_subset_size"}
    log = sorted((tmp_path / "kid").glob("metrics_*.log"))[-1].read_text(encoding="utf-8")
    assert f"KID: {want['kid_mean']} ± {want['kid_std']} (3 × 8)" in log
    assert json.loads(sorted((tmp_path / "kid").glob("metrics_*.json"))[-1].read_text())["kid_mean"] == want["kid_mean"]
    small = ev.main(args + ["--out", str(tmp_path / "small"), "--kid", "2"])     # 1000 rows a subset asked of 130 and 129: the notice, subsets of 129
    assert small["kid_subset_size"] == 129 and "subsets of 129 rows instead" in sorted((tmp_path / "small").glob("metrics_*.log"))[-1].read_text(encoding="utf-8")
