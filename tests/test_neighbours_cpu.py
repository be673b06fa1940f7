"""Neighbours without a device: every refusal of nearest_neighbours / density_coverage / memorization_report, the descriptor rules and the workspace
formula of the mf_nn_* calls against their Python mirror, the fp64 restatement (tests/neighbour_cases.py) against the recorded table of the
mode-dropping cases, the ambiguity caps the GPU tests rely on, and the scripts' plans."""
import ctypes as C
import importlib.util
import inspect
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
from tests import neighbour_cases as NC

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("mf_nn_ok", "mf_nn_workspace_bytes", "mf_nn_partial_f32", "mf_nn_finish_f32", "mf_pair_sqdist_f32", "mf_manifold_count_partial_f32",
               "mf_manifold_count_finish_f32")


# ------------------------------------------------------------------------------------------------ 1. refusals, all before the device
def test_every_refusal_names_its_argument():
    x, y = torch.zeros(8, 6), torch.zeros(5, 6)
    for bad in (0, 17, True, -1, 2.0, None):
        with pytest.raises(ValueError, match="k: an integer in 1 .. 16"):
            M.nearest_neighbours(x, y, bad)
        with pytest.raises(ValueError, match="neighbours: an integer in 1 .. 16"):
            M.memorization_report(x, y, neighbours=bad)
    with pytest.raises(ValueError, match="k: 6 neighbours need at least 6 rows of ref, got 5"):
        M.nearest_neighbours(x, y, 6)
    with pytest.raises(ValueError, match="k: 8 neighbours need more than 8 rows of query, got 8"):
        M.nearest_neighbours(x, None, 8)
    with pytest.raises(ValueError, match="neighbours: 9 neighbours need at least 9 rows of train, got 8"):
        M.memorization_report(x, y, neighbours=9)
    with pytest.raises(ValueError, match="query: fp32"):
        M.nearest_neighbours(x.double(), y)
    with pytest.raises(ValueError, match="ref: fp32"):
        M.nearest_neighbours(x, y.half())
    with pytest.raises(ValueError, match="query: a 2-D"):
        M.nearest_neighbours(x[0], y)
    with pytest.raises(ValueError, match="ref: a 2-D"):
        M.nearest_neighbours(x, y[None])
    with pytest.raises(ValueError, match="ref: D = 6 like query, got 5"):
        M.nearest_neighbours(x, y[:, :5])
    with pytest.raises(ValueError, match="query: a tensor"):
        M.nearest_neighbours(None, y)
    with pytest.raises(ValueError, match="query: at least 2 row"):
        M.nearest_neighbours(x[:1])
    with pytest.raises(ValueError, match="pivot: an fp32 \\[6\\]"):
        M.nearest_neighbours(x, y, pivot=torch.zeros(5))
    for bad in (0, 17, 2.0):
        with pytest.raises(ValueError, match="_splits"):
            M.nearest_neighbours(x, y, _splits=bad)
        with pytest.raises(ValueError, match="_splits"):
            M.density_coverage(x, y, 3, _splits=bad)
        with pytest.raises(ValueError, match="_splits"):
            M.memorization_report(x, y, neighbours=3, _splits=bad)
    with pytest.raises(ValueError, match="query: on a ROCm device"):
        M.nearest_neighbours(x, y, 5)                                           # k equal to the reference rows is allowed; the device is asked last
    with pytest.raises(ValueError, match="query: on a ROCm device"):
        M.nearest_neighbours(x, None, 7)
    for bad in (0, 16, -1, 3.0, True, None):
        with pytest.raises(ValueError, match="knn: an integer in 1 .. 15"):
            M.density_coverage(x, y, bad)
    with pytest.raises(ValueError, match="knn: 8 neighbours need more than the 8 rows of real"):
        M.density_coverage(x, y, 8)
    with pytest.raises(ValueError, match="real: fp32"):
        M.density_coverage(x.double(), y)
    with pytest.raises(ValueError, match="fake: D = 6 like real, got 5"):
        M.density_coverage(x, y[:, :5])
    with pytest.raises(ValueError, match="fake: a 2-D"):
        M.density_coverage(x, y[0])
    with pytest.raises(ValueError, match="real: on a ROCm device"):
        M.density_coverage(x, y, 5)
    with pytest.raises(ValueError, match="train: fp32"):
        M.memorization_report(x.double(), y)
    with pytest.raises(ValueError, match="train: at least 2 row"):
        M.memorization_report(x[:1], y, neighbours=1)
    with pytest.raises(ValueError, match="fake: D = 6 like train, got 5"):
        M.memorization_report(x, y[:, :5], neighbours=2)
    with pytest.raises(ValueError, match="fake: a 2-D"):
        M.memorization_report(x, y[0], neighbours=2)
    with pytest.raises(ValueError, match="train: on a ROCm device"):
        M.memorization_report(x, y, neighbours=8)
    for name in ("nearest_neighbours", "density_coverage", "memorization_report"):
        assert hasattr(M, name) and getattr(M, name) is getattr(F, name)


def test_meter_compute_has_the_new_keywords_and_both_default_to_false():
    sig = inspect.signature(M.FidelityMeter.compute)
    assert list(sig.parameters) == ["self", "density_coverage", "memorization"]
    assert sig.parameters["density_coverage"].default is False and sig.parameters["memorization"].default is False
    meter = M.FidelityMeter(lambda t: t, knn=2)
    meter.update(torch.zeros(6, 4), real=True)
    meter.update(torch.zeros(5, 4), real=False)
    with pytest.raises(ValueError, match="real: on a ROCm device"):             # the defaults still need the device for precision / recall
        meter.compute(density_coverage=True, memorization=True)


# ------------------------------------------------------------------------------------------------ 2. the C ABI on the host
def test_nn_rules_and_workspace_agree_with_the_python_mirror():
    lib = L.load()
    seen = {True: 0, False: 0}
    for n in (1, 2, 16, 17, 300, (1 << 24) - 1, 1 << 24, 0):
        for m in (1, 17, 300, (1 << 24) - 1, 1 << 24, 0):
            for d in (1, 96, 65536, 65537, 0):
                for k in (0, 1, 15, 16, 17):
                    for s in (0, 1, 16, 17):
                        for same in (0, 1):
                            desc = K.make_fidelity_desc(n, m, d, k, s, bool(same))
                            want = F.nn_ok(n, m, d, k, s, bool(same))
                            assert K.nn_ok(desc) == want, (n, m, d, k, s, same)
                            assert K.nn_workspace_bytes(desc) == (F.nn_workspace_bytes(m, s) if want else 0), (n, m, d, k, s, same)
                            seen[want] += 1
    assert seen[True] > 100 and seen[False] > 100
    assert F.nn_workspace_bytes(4096, 16) == 16 * 4096 * 16 * 8 == 8 << 20
    assert K.nn_ok(K.make_fidelity_desc(16, 129, 8, 16, 1)) and not K.nn_ok(K.make_fidelity_desc(16, 16, 8, 16, 1, True))
    assert b"the row itself left out" in lib.mf_last_error()
    assert K.nn_ok(K.make_fidelity_desc(17, 17, 8, 16, 1, True))
    d = K.make_fidelity_desc(300, 257, 96, 3, 2)
    d.same_bank = 2
    assert not K.nn_ok(d) and b"same_bank" in lib.mf_last_error()
    assert lib.mf_nn_ok(None) == 0 and lib.mf_nn_workspace_bytes(None) == 0
    # mf_fidelity_workspace_bytes keeps its meaning (and its rule knn <= 15)
    assert K.fidelity_workspace_bytes(K.make_fidelity_desc(300, 257, 96, 3, 2)) == F.workspace_bytes(300, 257, 2)
    assert K.fidelity_workspace_bytes(K.make_fidelity_desc(300, 257, 96, 16, 2)) == 0


def test_entry_points_refuse_before_any_launch():
    """argument checks run on the host (the pointers are never dereferenced, no device is needed)"""
    lib = L.load()
    p = 1 << 20
    d = K.make_fidelity_desc(300, 257, 96, 5, 2)
    need = K.nn_workspace_bytes(d)
    assert need == 2 * 257 * 16 * 8
    bad = K.make_fidelity_desc(300, 257, 96, 17, 2)
    assert lib.mf_nn_partial_f32(p, p, p, p, p, p, need, C.byref(bad), None) == -1 and b"k=17" in lib.mf_last_error()
    assert lib.mf_nn_partial_f32(p, p, p, p, p, p, need, None, None) == -1
    assert lib.mf_nn_partial_f32(None, p, p, p, p, p, need, C.byref(d), None) == -1 and lib.mf_nn_partial_f32(p, p, p, p, p, None, need, C.byref(d), None) == -1
    assert lib.mf_nn_partial_f32(p, p, p, p, p, p + 8, need, C.byref(d), None) == -1 and b"aligned" in lib.mf_last_error()
    assert lib.mf_nn_partial_f32(p, p, p, p, p, p, need - 1, C.byref(d), None) == -4 and b"needed" in lib.mf_last_error()
    same = K.make_fidelity_desc(300, 300, 96, 5, 2, True)
    assert lib.mf_nn_partial_f32(p, p, p + 64, p, p, p, 1 << 30, C.byref(same), None) == -1 and b"two banks" in lib.mf_last_error()
    assert lib.mf_nn_finish_f32(p, None, p, C.byref(d), None) == -1 and lib.mf_nn_finish_f32(p, p, None, C.byref(d), None) == -1
    assert lib.mf_nn_finish_f32(p, p, p, C.byref(bad), None) == -1
    assert lib.mf_pair_sqdist_f32(p, p, None, p, C.byref(d), None) == -1 and lib.mf_pair_sqdist_f32(p, p, p, p, C.byref(bad), None) == -1
    assert lib.mf_manifold_count_partial_f32(p, p, p, p, p, p, p, 2 * 257 * 4 - 1, C.byref(d), None) == -4
    assert lib.mf_manifold_count_partial_f32(p, p, None, p, p, p, p, need, C.byref(d), None) == -1
    assert lib.mf_manifold_count_finish_f32(p, None, None, C.byref(d), None) == -1 and lib.mf_manifold_count_finish_f32(None, p, p, C.byref(d), None) == -1
    with pytest.raises(RuntimeError, match="ROCm"):
        K.nn_search(torch.zeros(4, 8), torch.zeros(4), torch.zeros(4, 8), torch.zeros(4), torch.zeros(8), 1, 1)
    with pytest.raises(RuntimeError, match="ROCm"):
        K.pair_sqdist(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 1, dtype=torch.int32))


def test_the_entry_points_are_declared_exported_bound_and_documented():
    hdr = (ROOT / "include" / "medfusion_hip.h").read_text()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.exported_symbols() and hasattr(lib, name), name
        assert name in (ROOT / "INTEGRATION.md").read_text(), name
    assert lib.mf_version() == 250


def test_the_new_kernels_pass_the_isa_lint():
    from medfusion_amd import build as B
    assert B.lint_isa() == []
    asm = (B.OBJ / "lint" / "fidelity.s").read_text()
    for kernel in ("nn_partial_kernel", "nn_finish_kernel", "pair_sqdist_kernel", "manifold_count_partial_kernel", "manifold_count_finish_kernel"):
        assert kernel in asm, kernel


# ------------------------------------------------------------------------------------------------ 3. the restatement and the cases
@pytest.mark.parametrize("name", list(NC.DROPPING))
def test_restatement_reproduces_the_recorded_table(name):
    """The table of the mode-dropping cases (fp64, without the two exact copies): coverage, authenticity and the copy ratios to their printed
    digits.  The density is held to ONE count of the printed figure: the noise of the near-copies is not fixed by the table's description, a
    near-copy of a training row that is another row's knn-th neighbour sits exactly on that row's radius and its 1e-3 noise decides the pair.
    These inputs give a sum of counts of 1803 (/ (5 x 257) = 1.40311; the printed 1.404 is 1804) and 1890 (/ (5 x 320) = 1.18125; the printed
    1.182 is 1891)."""
    train, fake = NC.case(name + "-")
    seed, n, m, d = NC.DROPPING[name]
    assert train.shape == (n, d) and fake.shape == (m, d) and train.dtype == torch.float32
    c = FC.pivot_of(train)
    dc = NC.density_coverage64(FC.centred(train, c), FC.centred(fake, c), d, NC.KNN_DC)
    mem = NC.memorization64(train, fake, NC.NEIGHBOURS)
    density, coverage, authenticity = NC.TABLE[name]
    planted = list(NC.PLANTED_NEAR[0])
    others = [j for j in range(m) if j not in planted]
    print(f"[measured] {name} fp64: density {dc['density']:.5f} coverage {dc['coverage']:.5f} authenticity {mem['authenticity']:.5f} "
          f"copy_ratio planted max {float(mem['copy_ratio'][planted].max()):.5f} others min {float(mem['copy_ratio'][others].min()):.5f}")
    assert abs(int(dc["count"].sum()) - round(density * NC.KNN_DC * m)) <= 1
    assert abs(dc["coverage"] - coverage) < 5e-4 and abs(mem["authenticity"] - authenticity) < 5e-4
    assert float(mem["copy_ratio"][planted].max()) <= 0.0012 and abs(float(mem["copy_ratio"][others].min()) - 0.81) < 5e-3
    assert torch.equal(mem["nearest_index"][planted], torch.tensor(NC.PLANTED_NEAR[1]))
    # not saturated, unlike c0 .. c3
    assert 0.3 < dc["coverage"] < 0.7
    full = NC.case(name)[1]
    assert torch.equal(full[list(NC.PLANTED_EXACT[0])], train[list(NC.PLANTED_EXACT[1])]) and torch.equal(full[10:], fake[10:]) and torch.equal(full[:8], fake[:8])


def test_fidelity_cases_are_saturated_in_coverage():
    for name in FC.CASES:
        real, fake = FC.case(name)
        c = FC.pivot_of(real)
        assert NC.density_coverage64(FC.centred(real, c), FC.centred(fake, c), real.shape[1])["coverage"] >= 0.96, name


@pytest.mark.parametrize("name", NC.ALL)
def test_every_case_meets_the_caps_the_device_tests_rely_on(name):
    """conditions on the INPUTS: the ambiguous rows of the index test (k = 1, 5 and leave-one-out at 5) are at most 3 % of a case's rows, the
    ambiguous pairs of the density at most 0.1 % of its pairs, and no row's coverage decision is ambiguous"""
    real, fake = NC.case(name)
    d = real.shape[1]
    c = FC.pivot_of(real)
    rt, ft = FC.centred(real, c), FC.centred(fake, c)
    for k in (1, 5):
        share = NC.ambiguous_rows(ft, rt, d, k).double().mean()
        assert float(share) <= FC.AMBIGUOUS_CAP, (name, k, float(share))
    assert float(NC.ambiguous_rows(rt, rt, d, 5, leave_one_out=True).double().mean()) <= FC.AMBIGUOUS_CAP
    dc = NC.density_coverage64(rt, ft, d)
    assert int(dc["ambiguous_pairs"].sum()) <= 0.001 * real.shape[0] * fake.shape[0], (name, int(dc["ambiguous_pairs"].sum()))
    # (a near-copy of a training row that is another row's knn-th neighbour sits ON that row's radius: the mode-dropping cases have such rows)
    assert int(dc["ambiguous_rows"].sum()) <= (0 if name in FC.ALL else FC.AMBIGUOUS_CAP * real.shape[0]), (name, int(dc["ambiguous_rows"].sum()))


def test_restatement_pieces():
    x, y = FC.case("c2")
    s, i, _ = NC.nearest64(y.double(), x.double(), 4)
    brute = ((y.double()[:, None, :] - x.double()[None, :, :]) ** 2).sum(-1)
    assert torch.equal(i, torch.sort(brute, dim=1, stable=True).indices[:, :4]) and float((s - brute.gather(1, i)).abs().max()) < 1e-9
    assert float((NC.pair_d2_64(y, x, i) - brute.gather(1, i)).abs().max()) < 1e-9
    own = NC.nearest64(x.double(), x.double(), 1, leave_one_out=True)[1][:, 0]
    assert bool((own != torch.arange(x.shape[0])).all())
    assert NC.REFINE_REL == 4 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 4. the scripts, without a device
def _script(name):
    sys.path.insert(0, str(ROOT / "scripts"))
    spec = importlib.util.spec_from_file_location(f"_neighbours_script_{name}", ROOT / "scripts" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name,words", [("nearest_train", ("--train", "--fake", "--features", "--neighbours", "--top", "--out", "--plan")),
                                        ("neighbours_bench", ("--plan", "--reps", "--k")),
                                        ("evaluate_images", ("--density-coverage", "--memorization"))])
def test_scripts_help(name, words):
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / f"{name}.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and all(w in r.stdout for w in words), r.stdout + r.stderr


def test_scripts_plan_without_a_device(capsys):
    nt = _script("nearest_train")
    p = nt.plan(50000, 10000, 2048, 10)
    assert p["splits"] == {"fake_in_train": F.plan_splits(10000, 50000), "train_in_train": 9}
    assert p["workspace_bytes"] == max(F.nn_workspace_bytes(10000, p["splits"]["fake_in_train"]), F.nn_workspace_bytes(50000, 9))
    assert p["matrix_bytes"] == 50000 * 10000 * 4 and len(p["launches"]) == 7
    assert nt.main(["--plan", "--n-train", "300", "--n-fake", "257", "--d", "96"]) == 0
    out = capsys.readouterr().out
    assert "splits" in out and "workspace" in out and "nn_partial" in out
    with pytest.raises(SystemExit):
        nt.plan(5, 10, 8, 10)                                                   # more neighbours than training rows
    with pytest.raises(SystemExit):
        nt.parse_args(["--train", "a.pt"])
    with pytest.raises(SystemExit):
        nt.parse_args(["--train", "a.pt", "--fake", "b.pt", "--neighbours", "17"])
    with pytest.raises(SystemExit):
        nt.parse_args(["--train", "folder", "--fake", "b.pt"])                  # a folder without --features
    assert nt.parse_args(["--train", "folder", "--fake", "b.pt", "--features", "pixels"]).features == "pixels"
    nb = _script("neighbours_bench")
    p = nb.plan(10000, 10000, 2048, [1, 10])
    assert p["splits"]["search"] == 6 and p["workspace_bytes"] == 6 * 10000 * 128 and p["search_flops"] == 2.0 * 2048 * 10000 * 10000
    assert nb.main(["--plan", "--n", "300", "--m", "257", "--d", "96"]) == 0
    out = capsys.readouterr().out
    assert "splits" in out and "workspace" in out and "nn_partial_kernel" in out


def test_evaluate_images_new_flags_are_off_by_default():
    ev = _script("evaluate_images")
    a = ev.parse_args(["--real", "real.pt", "--fake", "fake.npy"])
    assert a.density_coverage is None and a.memorization is None
    a = ev.parse_args(["--real", "real.pt", "--fake", "fake.npy", "--density-coverage", "--memorization"])
    assert (a.density_coverage, a.memorization) == (5, 10)
    a = ev.parse_args(["--real", "real.pt", "--fake", "fake.npy", "--density-coverage", "3", "--memorization", "16"])
    assert (a.density_coverage, a.memorization) == (3, 16)
    for bad in (["--density-coverage", "16"], ["--density-coverage", "0"], ["--memorization", "17"], ["--memorization", "0"]):
        with pytest.raises(SystemExit):
            ev.parse_args(["--real", "real.pt", "--fake", "fake.npy"] + bad)
