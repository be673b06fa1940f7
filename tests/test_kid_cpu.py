"""Kernel distances without a device: the fp64 restatement (tests/kid_cases.py) against closed forms, the derived bounds against the fp32 torch form
of the definition, the seeded index draw, plan_kid's numbers, every refusal of kernel_matrix / mmd2 / kid / plan_kid by argument name, the
MfKernelSumDesc boundary (size, offsets, symbols, messages of the MF_EINVAL refusals) and the scripts' arguments."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import medfusion_amd as M
from medfusion_amd import fidelity as F
from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from tests import fidelity_cases as FC
from tests import kid_cases as KC
from tests.test_neighbours_cpu import _script

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("mf_ksum_ok", "mf_ksum_workspace_bytes", "mf_ksum_partial_f32", "mf_ksum_finish_f64", "mf_feat_kernel_f32")


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("name", ["inception", "mixture", "same", "s1", "s3"])
def test_restatement_equals_the_closed_form_of_the_linear_kernel(name):
    real, fake = KC.case(name)
    for gamma in (1.0, KC.gamma_default(real.shape[1])):
        got, terms, _ = KC.mmd2_64(real, fake, kernel="poly", degree=1, gamma=gamma, coef0=0.0)
        want = KC.closed_form_linear_mmd2(real, fake, gamma)
        scale = abs(terms["kxx"]) + abs(terms["kyy"]) + 2 * abs(terms["kxy"])
        assert abs(got - want) <= 1e-12 * scale, (name, got, want)
    x = real.double()
    k, _ = KC.kernel64(real, real, degree=1, gamma=1.0, coef0=0.0)
    assert abs(float(KC.pair_sum(k, True)) - float(x.sum(0) @ x.sum(0) - (x * x).sum())) <= 1e-12 * float(k.abs().sum())
    assert float(KC.pair_sum(k, True, diag=True)) == float(k.sum()) and float(KC.pair_sum(k, False)) == float(k.sum())


def test_cases_are_what_the_device_tests_rely_on():
    for name in ("inception", "mixture", "same") + KC.SHAPE_CASES:
        real, fake = KC.case(name)
        assert real.dtype == fake.dtype == torch.float32 and bool((real >= 0).all()) and bool((fake >= 0).all())
        assert 0.2 < float((real == 0).double().mean()) < 0.8, name             # Inception-like: many exact zeros
    assert [tuple(KC.case(n)[0].shape[:1] + KC.case(n)[1].shape) for n in KC.SHAPE_CASES] == [s for s in KC.SHAPES]
    real, fake = KC.case("inception+64")
    assert float(real.min()) >= 64 and torch.equal(real, KC.case("inception")[0] + 64)
    mixture, _, bound = KC.mmd2_64(*KC.case("mixture"), kernel="poly")
    print(f"[measured] fp64 MMD^2_u of the mixture case {mixture:.6f}, its derived bound {bound:.3e}")
    assert 3e-3 < mixture < 3e-2 and bound < 0.1 * mixture                      # clearly positive, about 1e-2, and informative
    same = KC.mmd2_64(*KC.case("same"), kernel="poly")[0]
    assert abs(same) < 0.1 * mixture
    ia, ib = F.draw_subsets(300, 257, 8, 100, 0)
    values = KC.kid64(*KC.case("same"), ia, ib)[2]
    assert float(values.min()) < 0 < float(values.max())                        # about 0 and of either sign


@pytest.mark.parametrize("name", KC.SHAPE_CASES)
def test_the_fp32_torch_form_is_inside_the_derived_bound(name):
    """a probe of the bound, not of the device: the same definition in fp32 torch (two roundings where the device's fmaf has one)"""
    x, y = KC.case(name)
    g = KC.gamma_default(x.shape[1])
    v = g * (x @ y.t()) + 1.0
    for degree, k32 in ((1, v), (2, v * v), (3, v * v * v), (4, (v * v) * (v * v))):
        k, E = KC.kernel64(x, y, degree=degree)
        ratio = float(((k32.double() - k).abs() / E).max())
        print(f"[measured] {name} degree {degree}: fp32 torch form, max |k - fp64| / E = {ratio:.3f}")
        assert ratio <= 1.0, (name, degree)
    p = FC.pivot_of(x)
    gamma = KC.rbf_gamma(x)
    k, E = KC.kernel64(x, y, kernel="rbf", gamma=gamma, pivot=p)
    xt, yt = x - p, y - p
    d2 = ((xt.double() ** 2).sum(1).float()[:, None] + (yt.double() ** 2).sum(1).float()[None, :] - 2 * (xt @ yt.t())).clamp_min(0)
    assert float(((torch.exp(-(gamma * d2)).double() - k).abs() / E).max()) <= 1.0, name


def test_the_uncentred_formula_leaves_the_rbf_bound_on_the_offset_case():
    real, fake = KC.case("inception+64")
    p, gamma = FC.pivot_of(real), KC.rbf_gamma(real)
    k, E = KC.kernel64(real, fake, kernel="rbf", gamma=gamma, pivot=p)
    plain = torch.exp(-gamma * FC.plain_torch_sqdist(real, fake)).double()
    ratio = float(((plain - k).abs() / E).max())
    print(f"[measured] inception+64 rbf: the un-centred fp32 formula, max |k - fp64| / E = {ratio:.1f}")
    assert ratio > 10.0


# ------------------------------------------------------------------------------------------------ 2. the draw
def test_the_index_draw_is_seeded_and_has_no_repeats():
    torch.manual_seed(123)
    state = torch.get_rng_state()
    ia, ib = F.draw_subsets(300, 257, 7, 130, seed=5)
    assert torch.equal(torch.get_rng_state(), state)                            # the global generator is where it was
    assert ia.dtype == ib.dtype == torch.int32 and ia.shape == ib.shape == (7, 130) and not ia.is_cuda
    for lists, rows in ((ia, 300), (ib, 257)):
        assert int(lists.min()) >= 0 and int(lists.max()) < rows
        assert all(len(set(row.tolist())) == 130 for row in lists)              # no repeats inside a subset
        assert len({tuple(row.tolist()) for row in lists}) == 7                 # the subsets differ
    torch.manual_seed(999)                                                      # another global state: the same lists
    again = F.draw_subsets(300, 257, 7, 130, seed=5)
    assert torch.equal(again[0], ia) and torch.equal(again[1], ib)
    other = F.draw_subsets(300, 257, 7, 130, seed=6)
    assert not torch.equal(other[0], ia) and not torch.equal(other[1], ib)
    # the rule itself: one generator, randperm(n) then randperm(m), subset after subset
    g = torch.Generator().manual_seed(5)
    for s in range(2):
        assert torch.equal(torch.randperm(300, generator=g)[:130].int(), ia[s]) and torch.equal(torch.randperm(257, generator=g)[:130].int(), ib[s])
    full = F.draw_subsets(16, 16, 3, 16, 0)[0]
    assert all(sorted(row.tolist()) == list(range(16)) for row in full)


# ------------------------------------------------------------------------------------------------ 3. the plan
def test_plan_kid_numbers():
    p = M.plan_kid(10000, 10000, 100, 1000)
    assert p["workgroups"] == {"real x real": 100 * 36, "fake x fake": 100 * 36, "real x fake": 100 * 64}       # T = 8: T (T + 1) / 2 = 36
    assert p["workspace_bytes"] == 8 * 100 * 64 and p["index_bytes"] == 2 * 100 * 1000 * 4 and p["matrix_bytes"] == 3 * 100 * 1000 * 1000 * 4
    assert len(p["launches"]) == 6 and sum("ksum_partial_kernel" in x for x in p["launches"]) == 3
    p = M.plan_kid(50000, 10000, None, None)
    T, Tm = 391, 79
    assert p["workgroups"] == {"real x real": T * (T + 1) // 2, "fake x fake": Tm * (Tm + 1) // 2, "real x fake": T * Tm}
    assert p["workspace_bytes"] == 8 * T * (T + 1) // 2 and p["index_bytes"] == 0
    assert p["matrix_bytes"] == (50000 * 50000 + 10000 * 10000 + 50000 * 10000) * 4
    p = M.plan_kid(300, 257, 3, 130)
    assert p["workgroups"] == {"real x real": 9, "fake x fake": 9, "real x fake": 12} and p["workspace_bytes"] == 8 * 12
    assert F.ksum_workspace_bytes(1, 129, 129, True) == 32 and F.ksum_workspace_bytes(1, 128, 128, True) == 16      # 3 tiles -> 24 -> 32; 1 tile -> 16
    # the library's own answer
    for S, sa, sb, same in ((100, 1000, 1000, 1), (100, 1000, 1000, 0), (1, 50000, 50000, 2), (3, 130, 128, 0), (1, 1, 1, 0)):
        d = K.make_ksum_desc(50000, 50000, 64, S, sa, sb, same_bank=same)
        assert K.ksum_ok(d) and K.ksum_workspace_bytes(d) == F.ksum_workspace_bytes(S, sa, sb, bool(same)), (S, sa, sb, same)
    for bad in ((1, 10, 100, 5), (10, 1, 100, 5), (10, 10, 0, 5), (10, 10, 3, 11), (10, 10, 3, 1), (1 << 24, 10, 3, 5)):
        with pytest.raises(ValueError):
            M.plan_kid(*bad)


# ------------------------------------------------------------------------------------------------ 4. refusals, all before the device
def test_every_refusal_names_its_argument():
    x, y = torch.zeros(8, 6), torch.zeros(5, 6)
    for fn in (M.mmd2, M.kid):
        with pytest.raises(ValueError, match="real: fp32"):
            fn(x.double(), y)
        with pytest.raises(ValueError, match="fake: fp32"):
            fn(x, y.half())
        with pytest.raises(ValueError, match="real: a 2-D"):
            fn(x[0], y)
        with pytest.raises(ValueError, match="fake: a 2-D"):
            fn(x, y[None])
        with pytest.raises(ValueError, match="fake: D = 6 like real, got 5"):
            fn(x, y[:, :5])
        with pytest.raises(ValueError, match="real: at least 2 row"):
            fn(x[:1], y)
        for bad in (0, 5, True, 2.0, None):
            with pytest.raises(ValueError, match="degree: an integer in 1 .. 4"):
                fn(x, y, degree=bad)
        for bad in (0.0, -1.0, float("inf"), float("nan"), "1", True, 1e-60):
            with pytest.raises(ValueError, match="gamma"):
                fn(x, y, gamma=bad)
        for bad in (float("inf"), float("nan"), None, 1e60):
            with pytest.raises(ValueError, match="coef0"):
                fn(x, y, coef0=bad)
    with pytest.raises(ValueError, match="kernel: 'poly' or 'rbf'"):
        M.mmd2(x, y, kernel="linear")
    with pytest.raises(ValueError, match="kernel: 'poly' or 'rbf'"):
        M.kernel_matrix(x, y, kernel=None)
    with pytest.raises(ValueError, match="gamma: the rbf kernel needs a bandwidth"):
        M.mmd2(x, y, kernel="rbf")
    with pytest.raises(ValueError, match="gamma: the rbf kernel needs a bandwidth"):
        M.kernel_matrix(x, kernel="rbf")
    with pytest.raises(ValueError, match="real: on a ROCm device"):
        M.mmd2(x, y)
    with pytest.raises(ValueError, match="real: on a ROCm device"):
        M.mmd2(x, y, kernel="rbf", gamma=0.5, unbiased=False, return_terms=True)
    for bad in (1, 6, 0, -1, 2.0, True, None):                                  # min(N, M) = 5
        with pytest.raises(ValueError, match="subset_size: an integer in 2 .. min\\(N, M\\) = 5"):
            M.kid(x, y, subsets=3, subset_size=bad)
    with pytest.raises(ValueError, match="subset_size"):
        M.kid(x, y)                                                             # the default 1000 of two small banks
    for bad in (0, -1, 2.0, True, 65536):
        with pytest.raises(ValueError, match="subsets: None or an integer in 1 .. 65535"):
            M.kid(x, y, subsets=bad, subset_size=4)
    for bad in (-1, 1.0, None):
        with pytest.raises(ValueError, match="seed"):
            M.kid(x, y, subsets=2, subset_size=4, seed=bad)
    with pytest.raises(ValueError, match="real: on a ROCm device"):
        M.kid(x, y, subsets=2, subset_size=5)
    with pytest.raises(ValueError, match="real: on a ROCm device"):
        M.kid(x, y, subsets=None)
    with pytest.raises(ValueError, match="x: fp32"):
        M.kernel_matrix(x.double())
    with pytest.raises(ValueError, match="y: D = 6 like x, got 5"):
        M.kernel_matrix(x, y[:, :5])
    with pytest.raises(ValueError, match="pivot: an fp32 \\[6\\]"):
        M.kernel_matrix(x, y, pivot=torch.zeros(5))
    with pytest.raises(ValueError, match="x: on a ROCm device"):
        M.kernel_matrix(x, y, degree=4, gamma=0.25, coef0=0.0)
    for name in ("kernel_matrix", "mmd2", "kid", "plan_kid"):
        assert getattr(M, name) is getattr(F, name)


def test_meter_takes_the_kid_switch_and_stays_as_it_was_without_it():
    meter = M.FidelityMeter(lambda t: t, knn=2)
    assert meter.kid is False
    assert M.FidelityMeter(lambda t: t, kid=True).kid is True and M.FidelityMeter(lambda t: t, kid={"subsets": 3, "subset_size": 8}).kid["subsets"] == 3
    for bad in (1, "yes", None, {"subset": 3}, {"kernel": "rbf"}):
        with pytest.raises(ValueError, match="kid: False, True or a dict"):
            M.FidelityMeter(lambda t: t, kid=bad)
    meter = M.FidelityMeter(lambda t: t, knn=2, kid=True)
    meter.update(torch.zeros(6, 4), real=True)
    meter.update(torch.zeros(5, 4), real=False)
    with pytest.raises(ValueError, match="real: on a ROCm device"):
        meter.compute()


# ------------------------------------------------------------------------------------------------ 5. the C ABI on the host
def test_descriptor_layout_matches_the_header():
    hdr = (ROOT / "include" / "medfusion_hip.h").read_text()
    body = re.search(r"typedef struct MfKernelSumDesc \{(.*?)\} MfKernelSumDesc;", hdr, re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"^\s*(int32_t|float)\s+([^;]+);", body, re.M):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    assert [n for n, _ in fields] == ["N", "M", "D", "S", "sa", "sb", "kernel", "degree", "gamma", "coef0", "same_bank", "reserved"]
    assert [n for n, _ in L.MfKernelSumDesc._fields_] == [n for n, _ in fields]
    for i, (name, ctype) in enumerate(fields):                                  # every field is four bytes wide: no padding anywhere
        f = getattr(L.MfKernelSumDesc, name)
        assert (f.offset, f.size) == (4 * i, 4), name
        assert dict(L.MfKernelSumDesc._fields_)[name] is (C.c_float if ctype == "float" else C.c_int32), name
    assert C.sizeof(L.MfKernelSumDesc) == 48 and C.sizeof(L.MfFidelityDesc) == 32
    assert int(re.search(r"#define MF_KERNEL_POLY (\d+)", hdr).group(1)) == L.KERNEL_POLY == 0
    assert int(re.search(r"#define MF_KERNEL_RBF (\d+)", hdr).group(1)) == L.KERNEL_RBF == 1


def test_the_entry_points_are_declared_exported_bound_and_documented():
    hdr = (ROOT / "include" / "medfusion_hip.h").read_text()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.exported_symbols() and hasattr(lib, name), name
        assert name in (ROOT / "INTEGRATION.md").read_text(), name
    assert lib.mf_version() == 250


def test_every_refusal_of_the_descriptor_carries_its_message():
    lib = L.load()
    good = dict(N=300, M=257, D=96, S=3, sa=130, sb=128, kernel=L.KERNEL_POLY, degree=3, gamma=0.5, coef0=1.0, same_bank=0)
    assert K.ksum_ok(K.make_ksum_desc(**good)) and K.ksum_workspace_bytes(K.make_ksum_desc(**good)) == 3 * 2 * 1 * 8
    cases = [(dict(N=0), b"N=0"), (dict(N=1 << 24), b"N=16777216"), (dict(M=0), b"M=0"), (dict(D=0), b"D=0"), (dict(D=65537), b"D=65537"),
             (dict(S=0), b"S=0"), (dict(S=65536), b"S=65536"), (dict(sa=0), b"sa=0"), (dict(sa=301), b"sa=301"), (dict(sb=258), b"sb=258"),
             (dict(kernel=2), b"kernel=2"), (dict(degree=0), b"degree=0"), (dict(degree=5), b"degree=5"), (dict(gamma=0.0), b"gamma=0"),
             (dict(gamma=-1.0), b"gamma=-1"), (dict(gamma=float("inf")), b"gamma=inf"), (dict(gamma=float("nan")), b"gamma="),
             (dict(coef0=float("nan")), b"coef0="), (dict(same_bank=3), b"same_bank is 0, 1 or 2"), (dict(same_bank=-1), b"same_bank is 0, 1 or 2"),
             (dict(same_bank=1), b"same_bank with N=300 M=257"), (dict(same_bank=1, M=300, sb=128), b"sa=130 sb=128")]
    p = 1 << 20
    for change, message in cases:
        d = K.make_ksum_desc(**{**good, **change})
        assert not K.ksum_ok(d) and message in lib.mf_last_error(), (change, lib.mf_last_error())
        assert K.ksum_workspace_bytes(d) == 0
        assert lib.mf_ksum_partial_f32(p, None, None, p, None, None, p, p, 1 << 30, C.byref(d), None) == -1 and message in lib.mf_last_error(), change
        assert lib.mf_ksum_finish_f64(p, p, C.byref(d), None) == -1 and message in lib.mf_last_error(), change
        assert lib.mf_feat_kernel_f32(p, None, p, None, p, p, C.byref(d), None) == -1 and message in lib.mf_last_error(), change
    d = K.make_ksum_desc(**good)
    d.reserved = 1
    assert not K.ksum_ok(d) and b"reserved" in lib.mf_last_error()
    assert K.ksum_ok(K.make_ksum_desc(**{**good, "kernel": L.KERNEL_RBF, "degree": 0}))          # the degree belongs to poly
    assert lib.mf_ksum_ok(None) == 0 and lib.mf_ksum_workspace_bytes(None) == 0 and b"no descriptor" in lib.mf_last_error()
    # more tiles per subset pair than a grid holds: 2^24 - 1 rows are 131072 tiles a side
    huge = K.make_ksum_desc((1 << 24) - 1, (1 << 24) - 1, 8)
    assert not K.ksum_ok(huge) and K.ksum_workspace_bytes(huge) == 0 and b"tiles per subset pair" in lib.mf_last_error()
    assert K.ksum_ok(K.make_ksum_desc((1 << 24) - 1, (1 << 24) - 1, 8, 1, 5000000, 5000000, same_bank=1))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """argument checks run on the host (the pointers are never dereferenced, no device is needed)"""
    lib = L.load()
    p = 1 << 20
    d = K.make_ksum_desc(300, 257, 96, 3, 130, 128)
    need = K.ksum_workspace_bytes(d)
    assert need == 48
    assert lib.mf_ksum_partial_f32(p, None, None, p, None, None, p, p, need, None, None) == -1
    assert lib.mf_ksum_partial_f32(None, None, None, p, None, None, p, p, need, C.byref(d), None) == -1 and b"bad args" in lib.mf_last_error()
    assert lib.mf_ksum_partial_f32(p, None, None, p, None, None, None, p, need, C.byref(d), None) == -1
    assert lib.mf_ksum_partial_f32(p, None, None, p, None, None, p, None, need, C.byref(d), None) == -1
    assert lib.mf_ksum_partial_f32(p, None, None, p, None, None, p, p + 8, need, C.byref(d), None) == -1 and b"aligned" in lib.mf_last_error()
    assert lib.mf_ksum_partial_f32(p, None, None, p, None, None, p, p, need - 1, C.byref(d), None) == -4 and b"needed" in lib.mf_last_error()
    rbf = K.make_ksum_desc(300, 257, 96, 3, 130, 128, kernel=L.KERNEL_RBF, gamma=0.5)
    assert lib.mf_ksum_partial_f32(p, p, None, p, None, None, p, p, need, C.byref(rbf), None) == -1 and b"norms" in lib.mf_last_error()
    assert lib.mf_feat_kernel_f32(p, None, p, p, p, p, C.byref(rbf), None) == -1 and b"norms" in lib.mf_last_error()
    same = K.make_ksum_desc(300, 300, 96, 3, 130, 130, same_bank=1)
    assert lib.mf_ksum_partial_f32(p, None, None, p + 64, None, None, p, p, 1 << 20, C.byref(same), None) == -1 and b"two banks" in lib.mf_last_error()
    assert lib.mf_ksum_partial_f32(p, None, p, p, None, p + 64, p, p, 1 << 20, C.byref(same), None) == -1 and b"two index lists" in lib.mf_last_error()
    assert lib.mf_ksum_finish_f64(None, p, C.byref(d), None) == -1 and lib.mf_ksum_finish_f64(p, None, C.byref(d), None) == -1
    assert lib.mf_ksum_finish_f64(p + 8, p, C.byref(d), None) == -1 and b"aligned" in lib.mf_last_error()
    assert lib.mf_feat_kernel_f32(p, None, p, None, p, None, C.byref(d), None) == -1 and lib.mf_feat_kernel_f32(p, None, None, None, p, p, C.byref(d), None) == -1
    with pytest.raises(RuntimeError, match="ROCm"):
        K.kernel_sums(torch.zeros(4, 8), None, None, torch.zeros(4, 8), None, None, torch.zeros(8), K.make_ksum_desc(4, 4, 8))
    with pytest.raises(RuntimeError, match="ROCm"):
        K.feat_kernel(torch.zeros(4, 8), None, torch.zeros(4, 8), None, torch.zeros(8), K.make_ksum_desc(4, 4, 8))


def test_the_new_kernels_are_in_the_linted_assembly_and_do_not_spill():
    from medfusion_amd import build as B
    assert B.lint_isa() == []
    asm = (B.OBJ / "lint" / "fidelity.s").read_text()
    for kernel in ("ksum_partial_kernel", "ksum_finish_kernel", "kernel_matrix_kernel"):
        assert kernel in asm, kernel
    fb = _script("fidelity_bench")
    rows = [r for r in fb.kernel_resources() if r.startswith(("ksum_", "kernel_matrix_"))]
    assert len(rows) == 5 and all(r.rstrip().endswith("scratch 0 B") for r in rows), rows
    recorded = (ROOT / "profiles" / "kid_parity_measured.txt").read_text()
    for r in rows:
        assert " ".join(r.split()) in " ".join(recorded.split()), r                 # the figures the profile file states are the build's


# ------------------------------------------------------------------------------------------------ 6. the scripts, without a device
def test_evaluate_images_kid_flags_are_off_by_default():
    ev = _script("evaluate_images")
    a = ev.parse_args(["--real", "real.pt", "--fake", "fake.npy"])
    assert a.kid is None and a.kid_subset_size == 1000 and a.density_coverage is None and a.memorization is None
    a = ev.parse_args(["--real", "real.pt", "--fake", "fake.npy", "--kid"])
    assert (a.kid, a.kid_subset_size) == (100, 1000)
    a = ev.parse_args(["--real", "real.pt", "--fake", "fake.npy", "--kid", "3", "--kid-subset-size", "8"])
    assert (a.kid, a.kid_subset_size) == (3, 8)
    for bad in (["--kid", "0"], ["--kid", "65536"], ["--kid", "-2"], ["--kid", "x"], ["--kid-subset-size", "1"], ["--kid", "3", "--kid-subset-size", "0"]):
        with pytest.raises(SystemExit):
            ev.parse_args(["--real", "real.pt", "--fake", "fake.npy"] + bad)


def test_scripts_help_and_plan(capsys):
    for name, words in (("kid_bench", ("--plan", "--subsets", "--subset-size", "--big", "--reps")), ("evaluate_images", ("--kid", "--kid-subset-size"))):
        r = subprocess.run([sys.executable, str(ROOT / "scripts" / f"{name}.py"), "--help"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and all(w in r.stdout for w in words), r.stdout + r.stderr
    kb = _script("kid_bench")
    assert kb.main(["--plan", "--n", "300", "--d", "64", "--subsets", "3", "--subset-size", "130"]) == 0
    out = capsys.readouterr().out
    assert "ksum_partial_kernel" in out and "workspace" in out and "30 workgroups" in out and "scratch 0 B" in out
    with pytest.raises(SystemExit):
        kb.main(["--plan", "--n", "100", "--subset-size", "101"])
    x, y = KC.case("s1")
    g = KC.gamma_default(x.shape[1])
    want = KC.mmd2_64(x, y, kernel="poly")[0]                                    # the torch forms of the bench are the definition
    assert abs(float(kb.torch_mmd2(x.double(), y.double(), g)) - want) < 1e-12
    assert abs(float(kb.torch_mmd2_chunked(x.double(), y.double(), g, 2)) - want) < 1e-12
    ia, ib = F.draw_subsets(5, 130, 3, 4, 0)
    mean, std = KC.kid64(x, y, ia, ib)[:2]
    for form in (kb.torch_kid_loop, kb.torch_kid_batched):
        got = form(x.double(), y.double(), ia.long(), ib.long(), g)
        assert abs(got[0] - mean) < 1e-12 and abs(got[1] - std) < 1e-12
