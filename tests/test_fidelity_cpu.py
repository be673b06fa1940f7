"""Fidelity without a device: the fp64 restatement (tests/fidelity_cases.py) against the fixtures recorded from the reference's own class, the
3 % ambiguity cap of every case, frechet_distance against closed forms and scipy, every refusal of the public interface, the split planner and
the workspace formula at their edges, the descriptor rules of the C ABI, and the scripts' arguments and plans."""
import ctypes as C
import importlib.util
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import medfusion_amd as M
from medfusion_amd import fidelity as F
from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from tests import fidelity_cases as FC

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("mf_fidelity_ok", "mf_fidelity_workspace_bytes", "mf_feat_colmean_f32", "mf_feat_norms_f32", "mf_feat_sqdist_f32", "mf_knn_partial_f32",
               "mf_knn_finish_f32", "mf_manifold_partial_f32", "mf_manifold_finish_f32")


# ------------------------------------------------------------------------------------------------ 1. the restatement, the fixtures, the cases
@pytest.mark.parametrize("name", ["c0", "c1"])
def test_restatement_reproduces_the_reference_fixtures(name):
    g = FC.golden(name)
    real, fake = FC.case(name)
    assert np.array_equal(g["real"], real.numpy()) and np.array_equal(g["fake"], fake.numpy()) and int(g["knn"]) == FC.KNN
    t = FC.truth(real, fake, None)                                            # the reference's arithmetic (no pivot) in fp64
    assert int(t["precision_hits"].sum()) == round(float(g["precision_f64"]) * fake.shape[0])
    assert int(t["recall_hits"].sum()) == round(float(g["recall_f64"]) * real.shape[0])
    assert abs(t["precision"] - float(g["precision_f64"])) < 1e-6 and abs(t["recall"] - float(g["recall_f64"])) < 1e-6    # (it divides in fp32)
    for key in ("radii_real", "radii_fake"):
        assert float((t[key] / torch.from_numpy(g[f"{key}_f64"]) - 1).abs().max()) <= 1e-12, key
        assert float((torch.from_numpy(g[f"{key}_f32"]).double() / t[key] - 1).abs().max()) < 1e-3                         # fp32, un-centred: three digits
    # the pivot changes no decision on these cases, and the recorded figures are the issue's
    c = FC.case_truth(name)
    assert torch.equal(c["precision_hits"], t["precision_hits"]) and torch.equal(c["recall_hits"], t["recall_hits"])
    assert (round(t["precision"], 5), round(t["recall"], 5)) == {"c0": (0.47471, 0.32333), "c1": (0.54375, 0.34197)}[name]


WANT = {"c0": (0.4747, 0.3233, 1, 0), "c1": (0.5437, 0.3420, 1, 0), "c2": (0.9147, 0.7615, 0, 0), "c3": (0.3568, 0.1816, 4, 6), "c0+64": (0.4747, 0.3233, None, None)}


@pytest.mark.parametrize("name", FC.ALL)
def test_every_case_meets_the_ambiguity_cap(name):
    real, fake = FC.case(name)
    t = FC.case_truth(name)
    p, r, ap, ar = WANT[name]
    assert abs(t["precision"] - p) < 5e-5 and abs(t["recall"] - r) < 5e-5
    n_ap, n_ar = int(t["precision_ambiguous"].sum()), int(t["recall_ambiguous"].sum())
    if ap is not None:
        assert (n_ap, n_ar) == (ap, ar)
    assert n_ap <= FC.AMBIGUOUS_CAP * fake.shape[0] and n_ar <= FC.AMBIGUOUS_CAP * real.shape[0]
    assert n_ap <= 0.012 * fake.shape[0] and n_ar <= 0.012 * real.shape[0]
    assert real.dtype == torch.float32 and (real.shape, fake.shape) == ((FC.CASES[name[:2]][1], FC.CASES[name[:2]][3]), (FC.CASES[name[:2]][2], FC.CASES[name[:2]][3]))
    # a hit is never ambiguous by construction of the rule only when it is far from every radius: both kinds exist in the larger cases
    assert torch.equal(FC.case(name)[0], real)                                # seeded, cached


def test_restatement_pieces():
    x, y = FC.case("c2")
    d = FC.sqdist64(x.double(), y.double())
    brute = ((x.double()[:, None, :] - y.double()[None, :, :]) ** 2).sum(-1)
    assert float((d - brute).abs().max()) < 1e-12 * float(brute.max())
    r2 = FC.radii64(x.double(), 3)
    own = ((x.double()[:, None, :] - x.double()[None, :, :]) ** 2).sum(-1)
    assert float((r2 - own.sort(dim=1).values[:, 3]).abs().max()) < 1e-12 * float(own.max())
    assert float(FC.bound(torch.tensor([1.0]), torch.tensor([3.0]), 8)) == 16 * 2.0 ** -24 * 4
    assert torch.equal(FC.pivot_of(x), x.double().mean(0).float()) and FC.centred(x, None).dtype == torch.float64


# ------------------------------------------------------------------------------------------------ 2. the Frechet distance
def test_frechet_distance_of_diagonal_covariances_is_the_closed_form():
    g = torch.Generator().manual_seed(0)
    n, d = 512, 12
    a = torch.randn(n, d, generator=g, dtype=torch.float64)
    # exactly uncorrelated columns: orthonormalise the centred samples, then scale -- the SAMPLE covariances are diagonal
    def diag_bank(z, scale, shift):
        z = z - z.mean(0)
        q, _ = torch.linalg.qr(z)
        return (q * (n - 1) ** 0.5 * scale + shift)
    va, vb = torch.linspace(0.5, 3.0, d, dtype=torch.float64), torch.linspace(2.0, 0.25, d, dtype=torch.float64)
    x = diag_bank(a, va.sqrt(), torch.arange(d, dtype=torch.float64))
    y = diag_bank(torch.randn(n, d, generator=g, dtype=torch.float64), vb.sqrt(), torch.arange(d, dtype=torch.float64) * 0.5 + 1)
    xf, yf = x.float(), y.float()
    mu1, mu2 = xf.double().mean(0), yf.double().mean(0)
    s1, s2 = torch.cov(xf.double().t()), torch.cov(yf.double().t())
    assert float((s1 - torch.diag(s1.diagonal())).abs().max()) < 1e-6          # (diagonal up to the fp32 rounding of the inputs)
    want = float(((mu1 - mu2) ** 2).sum() + ((s1.diagonal().sqrt() - s2.diagonal().sqrt()) ** 2).sum())
    got = M.frechet_distance(xf, yf)
    assert isinstance(got, float) and abs(got - want) < 1e-5 * want


def test_frechet_distance_against_scipy_sqrtm():
    from scipy import linalg
    g = torch.Generator().manual_seed(1)
    n, d = 4096, 16
    mix_a, mix_b = torch.randn(d, d, generator=g, dtype=torch.float64), torch.randn(d, d, generator=g, dtype=torch.float64)
    x = (torch.randn(n, d, generator=g, dtype=torch.float64) @ mix_a + 0.3).float()
    y = (torch.randn(n, d, generator=g, dtype=torch.float64) @ mix_b - 0.2).float()
    mu1, mu2 = x.double().mean(0).numpy(), y.double().mean(0).numpy()
    s1, s2 = np.cov(x.double().numpy(), rowvar=False), np.cov(y.double().numpy(), rowvar=False)
    root = linalg.sqrtm(s1 @ s2)
    want = float(((mu1 - mu2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2 * np.trace(root).real)
    got = M.frechet_distance(x, y)
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    assert abs(M.frechet_distance(y, x) - got) <= 1e-9 * abs(want)              # symmetric


def test_frechet_distance_of_identical_and_rank_deficient_sets():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(300, 24, generator=g) * 2 + 1
    tr = float(torch.cov(x.double().t()).trace())
    assert abs(M.frechet_distance(x, x.clone())) <= 1e-9 * tr
    few, other = torch.randn(10, 32, generator=g), torch.randn(12, 32, generator=g) + 0.5         # N < D: singular covariances
    fd = M.frechet_distance(few, other)
    assert fd == fd and abs(fd) < float("inf") and fd > 0
    same = M.frechet_distance(few, few)                                       # null eigenvalues of size 1e-16 leave sqrt(1e-16) each: finite, tiny
    assert same == same and abs(same) < 1e-4


# ------------------------------------------------------------------------------------------------ 3. refusals, all before the device
def test_every_refusal_names_its_argument():
    x, y = torch.zeros(8, 6), torch.zeros(5, 6)
    for fn in (M.precision_recall, M.frechet_distance):
        with pytest.raises(ValueError, match="real: fp32"):
            fn(x.double(), y)
        with pytest.raises(ValueError, match="fake: fp32"):
            fn(x, y.half())
        with pytest.raises(ValueError, match="real: a 2-D"):
            fn(x[None], y)
        with pytest.raises(ValueError, match="fake: a 2-D"):
            fn(x, y[0])
        with pytest.raises(ValueError, match="fake: D = 6 like real, got 5"):
            fn(x, y[:, :5])
        with pytest.raises(ValueError, match="real: at least 2 row"):
            fn(x[:1], y)
        with pytest.raises(ValueError, match="fake: at least 2 row"):
            fn(x, y[:1])
        with pytest.raises(ValueError, match="real: a tensor"):
            fn(None, y)
    with pytest.raises(ValueError, match="real: on a ROCm device"):
        M.precision_recall(x, y)
    assert M.frechet_distance(x, y) == 0.0                                    # the one function with a CPU path
    for bad in (0, 16, -1, 3.0, True, None):
        with pytest.raises(ValueError, match="knn: an integer in 1 .. 15"):
            M.precision_recall(x, y, bad)
        with pytest.raises(ValueError, match="knn: an integer in 1 .. 15"):
            M.knn_radii(x, bad)
        with pytest.raises(ValueError, match="knn"):
            M.FidelityMeter(lambda t: t, knn=bad)
    with pytest.raises(ValueError, match="knn: 5 neighbours need more than the 5 rows of fake"):
        M.precision_recall(x, y, 5)
    with pytest.raises(ValueError, match="knn: 8 .* rows of x"):
        M.knn_radii(x, 8)
    with pytest.raises(ValueError, match="x: on a ROCm device"):
        M.knn_radii(x, 3)
    with pytest.raises(ValueError, match="x: fp32"):
        M.pairwise_sqdist(x.double())
    with pytest.raises(ValueError, match="y: D = 6"):
        M.pairwise_sqdist(x, torch.zeros(3, 7))
    with pytest.raises(ValueError, match="y: a 2-D"):
        M.pairwise_sqdist(x, torch.zeros(7))
    with pytest.raises(ValueError, match="pivot: an fp32 \\[6\\]"):
        M.pairwise_sqdist(x, y, pivot=torch.zeros(5))
    with pytest.raises(ValueError, match="pivot: an fp32"):
        M.knn_radii(x, 3, pivot=torch.zeros(6, dtype=torch.float64))
    with pytest.raises(ValueError, match="x: on a ROCm device"):
        M.pairwise_sqdist(x, y)
    with pytest.raises(ValueError, match="radii_sq: an fp32 \\[8\\]"):
        M.manifold_hits(x, torch.zeros(5), y)
    with pytest.raises(ValueError, match="query: D = 6"):
        M.manifold_hits(x, torch.zeros(8), torch.zeros(3, 2))
    with pytest.raises(ValueError, match="ref: on a ROCm device"):
        M.manifold_hits(x, torch.zeros(8), y)
    for bad in (0, 17, 2.0):
        with pytest.raises(ValueError, match="_splits"):
            M.knn_radii(x, 3, _splits=bad)
    feats = M.EmbedderFeatures(object())
    with pytest.raises(ValueError, match="imgs: 2-D images .*3-D features are not built"):
        feats(torch.zeros(1, 3, 8, 8, 8))
    with pytest.raises(ValueError, match="imgs: fp32"):
        feats(torch.zeros(1, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="imgs: on a ROCm device"):
        feats(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="pool"):
        M.EmbedderFeatures(object(), pool=0)
    meter = M.FidelityMeter(lambda t: t.double())
    with pytest.raises(ValueError, match="features: .*fp32"):
        meter.update(x, real=True)
    with pytest.raises(ValueError, match="update"):
        meter.compute()
    for name in ("pairwise_sqdist", "knn_radii", "manifold_hits", "precision_recall", "frechet_distance", "FidelityMeter", "EmbedderFeatures", "fidelity"):
        assert hasattr(M, name)


def test_meter_stores_flattened_features_and_computes_fd_on_the_host():
    meter = M.FidelityMeter(lambda t: t * 2.0, knn=2)
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn(6, 2, 3, generator=g), torch.randn(7, 2, 3, generator=g)
    meter.update(a[:2], real=True)
    meter.update(b, real=False)
    meter.update(a[2:], real=True)
    real, fake = meter.banks()
    assert torch.equal(real, (a * 2).reshape(6, 6)) and torch.equal(fake, (b * 2).reshape(7, 6))
    with pytest.raises(ValueError, match="real: on a ROCm device"):          # compute() needs the device for precision / recall
        meter.compute()
    meter.reset()
    with pytest.raises(ValueError, match="update"):
        meter.banks()


# ------------------------------------------------------------------------------------------------ 4. the planner and the workspace
def test_plan_splits_at_its_edges():
    assert F.plan_splits(1, 1) == 1 and F.plan_splits(128, 128) == 1 and F.plan_splits(129, 129) == 2      # capped by the column tiles
    assert F.plan_splits(300, 257) == 3 and F.plan_splits(257, 300) == 3
    assert F.plan_splits(128, 128 * 16) == 16 and F.plan_splits(128, 128 * 17) == 9                         # capped by 16: two tiles each from 9 splits on
    assert F.plan_splits(128, 128 * 40) == 14                                                               # three tiles each: 14 splits do what 16 do
    assert F.plan_splits(4096, 4096) == 16                                                                  # 32 x 16 = 512 workgroups: one full round
    assert F.plan_splits(10000, 10000) == 6                                                                 # 79 x 6 = 474 <= 512; 7 would open a second round
    assert F.plan_splits(128 * 512, 4096) == 1 and F.plan_splits(128 * 511, 4096) == 1                      # enough row tiles alone
    assert F.plan_splits(128 * 256, 4096) == 2 and F.plan_splits(50000, 50000) == 9      # 391 tiles: 7 full rounds of 44 tiles beat 1 round of 391
    for bad in ((0, 5), (5, 0)):
        with pytest.raises(ValueError):
            F.plan_splits(*bad)


def _desc(**change):
    d = K.make_fidelity_desc(300, 257, 96, 3, 2)
    for key, v in change.items():
        setattr(d, key, v)
    return d


def test_descriptor_rules_and_the_workspace_formula_on_the_host():
    lib = L.load()
    assert C.sizeof(L.MfFidelityDesc) == 8 * 4 and L.FIDELITY_LIST == 16 and L.FIDELITY_MAX_SPLITS == 16
    assert K.fidelity_ok(_desc()) and K.fidelity_workspace_bytes(_desc()) == 2 * 300 * 16 * 4 == F.workspace_bytes(300, 257, 2)
    for n, m, s in ((4096, 4096, 16), (2, 1, 1), (2, 5000, 16), (16, 100, 1), ((1 << 24) - 1, 3, 16), (3, (1 << 24) - 1, 16)):
        assert K.fidelity_workspace_bytes(K.make_fidelity_desc(n, m, 8, 1, s)) == F.workspace_bytes(n, m, s), (n, m, s)
    assert F.workspace_bytes(4096, 4096, 16) == 4 << 20 and F.workspace_bytes(2, 5000, 16) == 80000 and F.workspace_bytes(2, 1, 1) == 128
    assert K.fidelity_ok(_desc(knn=15)) and K.fidelity_ok(_desc(knn=1, N=2)) and K.fidelity_ok(_desc(D=1)) and K.fidelity_ok(_desc(D=65536))
    assert K.fidelity_ok(_desc(splits=16)) and K.fidelity_ok(_desc(M=300, same_bank=1)) and K.fidelity_ok(_desc(M=1))
    for bad, word in ((dict(knn=0), b"knn=0"), (dict(knn=16), b"knn=16"), (dict(knn=3, N=3), b"needs more than 3 rows"), (dict(N=0), b"N=0"),
                      (dict(N=1 << 24), b"N=16777216"), (dict(M=0), b"M=0"), (dict(M=1 << 24), b"M=16777216"), (dict(D=0), b"D=0"), (dict(D=65537), b"D=65537"),
                      (dict(splits=0), b"splits=0"), (dict(splits=17), b"splits=17"), (dict(same_bank=2), b"same_bank"), (dict(same_bank=1), b"same_bank with")):
        d = _desc(**bad)
        assert not K.fidelity_ok(d) and word in lib.mf_last_error(), bad
        assert K.fidelity_workspace_bytes(d) == 0
    assert lib.mf_fidelity_ok(None) == 0


def test_entry_points_refuse_before_any_launch():
    """argument checks run on the host (the pointers are never dereferenced, no device is needed)"""
    lib = L.load()
    p = 1 << 20
    d, need = _desc(), K.fidelity_workspace_bytes(_desc())
    assert lib.mf_knn_partial_f32(p, p, p, p, need, C.byref(_desc(knn=16)), None) == -1 and b"knn=16" in lib.mf_last_error()
    assert lib.mf_knn_partial_f32(p, p, p, p, need, None, None) == -1
    assert lib.mf_knn_partial_f32(None, p, p, p, need, C.byref(d), None) == -1 and lib.mf_knn_partial_f32(p, p, p, None, need, C.byref(d), None) == -1
    assert lib.mf_knn_partial_f32(p, p, p, p + 4, need, C.byref(d), None) == -1 and b"aligned" in lib.mf_last_error()
    assert lib.mf_knn_partial_f32(p, p, p, p, need - 1, C.byref(d), None) == -4 and b"needed" in lib.mf_last_error()      # MF_EWORKSPACE
    assert lib.mf_knn_finish_f32(p, None, C.byref(d), None) == -1 and lib.mf_knn_finish_f32(p, p, C.byref(_desc(splits=0)), None) == -1
    assert lib.mf_manifold_partial_f32(p, p, p, p, p, p, p, 2 * 257 - 1, C.byref(d), None) == -4
    assert lib.mf_manifold_partial_f32(p, p, None, p, p, p, p, need, C.byref(d), None) == -1
    assert lib.mf_manifold_finish_f32(p, None, None, C.byref(d), None) == -1 and lib.mf_manifold_finish_f32(None, p, p, C.byref(d), None) == -1
    assert lib.mf_feat_sqdist_f32(p, p, p + 64, p, p, p, C.byref(_desc(M=300, same_bank=1)), None) == -1 and b"two banks" in lib.mf_last_error()
    assert lib.mf_feat_sqdist_f32(p, p, p, p, None, p, C.byref(d), None) == -1
    assert lib.mf_feat_norms_f32(p, p, p, 0, 8, None) == -1 and lib.mf_feat_norms_f32(p, None, p, 4, 8, None) == -1
    assert lib.mf_feat_colmean_f32(p, p, 4, 65537, None) == -1 and b"feat_colmean" in lib.mf_last_error()
    with pytest.raises(RuntimeError, match="ROCm"):
        K.feat_colmean(torch.zeros(2, 8))                                       # the wrappers have no CPU path
    with pytest.raises(RuntimeError, match="ROCm"):
        K.knn_radii_sq(torch.zeros(4, 8), torch.zeros(4), torch.zeros(8), 1, 1)


def test_the_entry_points_are_declared_exported_bound_and_documented():
    hdr = (ROOT / "include" / "medfusion_hip.h").read_text()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.exported_symbols() and hasattr(lib, name), name
        assert name in (ROOT / "INTEGRATION.md").read_text(), name
    assert lib.mf_version() == 250 and "typedef struct MfFidelityDesc" in hdr
    assert int(re.search(r"#define MF_FIDELITY_LIST (\d+)", hdr).group(1)) == L.FIDELITY_LIST
    assert int(re.search(r"#define MF_FIDELITY_MAX_SPLITS (\d+)", hdr).group(1)) == L.FIDELITY_MAX_SPLITS


def test_fidelity_unit_is_built_without_packed_fp32_and_linted():
    from medfusion_amd import build as B

    assert "fidelity.hip" in B.SOURCES and "-packed-fp32-ops" in B.EXTRA_CFLAGS["fidelity.hip"]
    assert B.lint_isa() == []                                                  # the build's ISA lint walks SOURCES: fidelity.hip with its own flags


# ------------------------------------------------------------------------------------------------ 5. the scripts, without a device
def _script(name):
    spec = importlib.util.spec_from_file_location(f"_fidelity_script_{name}", ROOT / "scripts" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name,words", [("evaluate_images", ("--real", "--fake", "--features", "--knn", "--batch", "--max-samples", "--out")),
                                        ("fidelity_bench", ("--plan", "--reps"))])
def test_scripts_help(name, words):
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / f"{name}.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and all(w in r.stdout for w in words), r.stdout + r.stderr


def test_evaluate_images_argument_rules(tmp_path):
    ev = _script("evaluate_images")
    a = ev.parse_args(["--real", "real.pt", "--fake", "fake.npy"])
    assert (a.knn, a.batch, a.max_samples, a.features) == (3, 100, None, None)
    assert ev.parse_features("embedder:runs/vae.ckpt") == ("VAE", "runs/vae.ckpt", None)
    assert ev.parse_features("embedder:runs/vae.ckpt:4") == ("VAE", "runs/vae.ckpt", 4)
    assert ev.parse_features("VQGAN:runs/q.ckpt:2") == ("VQGAN", "runs/q.ckpt", 2)
    for bad in ("inception", "embedder:", "embedder:x:0", "UNet:x", "embedder:x:two"):
        with pytest.raises(SystemExit):
            ev.parse_features(bad)
    (tmp_path / "scans").mkdir()
    for bad in (["--real", "real.pt"], ["--real", "a.pt", "--fake", "b.pt", "--knn", "0"], ["--real", "a.pt", "--fake", "b.pt", "--knn", "16"],
                ["--real", "a.pt", "--fake", "b.pt", "--batch", "0"], ["--real", "a.pt", "--fake", "b.pt", "--max-samples", "1"],
                ["--real", str(tmp_path / "scans"), "--fake", "b.pt"]):                                   # a folder without --features
        with pytest.raises(SystemExit):
            ev.parse_args(bad)
    assert ev.parse_args(["--real", str(tmp_path / "scans"), "--fake", "b.pt", "--features", "embedder:x.ckpt"]).features == "embedder:x.ckpt"
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(9, 5, generator=g)
    torch.save(feats, tmp_path / "f.pt")
    np.save(tmp_path / "f.npy", feats.double().numpy())
    assert torch.equal(ev.load_features(tmp_path / "f.pt", None), feats) and torch.equal(ev.load_features(tmp_path / "f.npy", 4), feats[:4])
    torch.save(list(feats.chunk(3)), tmp_path / "chunks.pt")                                              # the reference's list of per-batch features
    assert torch.equal(ev.load_features(tmp_path / "chunks.pt", None), feats)
    with pytest.raises(SystemExit, match="\\[N, D\\]"):
        ev.load_features(tmp_path / "f.npy", None, expect_2d=torch.zeros(3))


def test_fidelity_bench_plans_without_a_device(capsys):
    fb = _script("fidelity_bench")
    plan = fb.plan(10000, 10000, 2048, 3)
    assert plan["splits"] == {"knn_real": 6, "knn_fake": 6, "precision": 6, "recall": 6} and plan["workspace_bytes"] == 6 * 10000 * 64
    assert plan["matrix_bytes"] == 10000 * 10000 * 4 and plan["flops"] == 4 * 2.0 * 10000 * 10000 * 2048
    assert fb.main(["--plan", "--n", "300", "--m", "257", "--d", "96"]) == 0
    out = capsys.readouterr().out
    assert "splits" in out and "workspace" in out
