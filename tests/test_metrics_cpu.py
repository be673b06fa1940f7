"""The metrics without a device: the plain-torch restatement the GPU tests check against (closed forms), every refusal of the public interface
and the size rule, the descriptor rules of the C ABI through the library loaded without a GPU, the pair planner, and the scripts' arguments."""
import ctypes as C
import importlib.util
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import medfusion_amd as M
from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from medfusion_amd import metrics as MT
from tests import metrics_cases as MC

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("mf_ssim_ok", "mf_ssim_workspace_bytes", "mf_ssim_pairs_f32", "mf_ssim_finish_f32", "mf_avgpool2_planes_f32", "mf_rows_minmax_f32")


# ------------------------------------------------------------------------------------------------ 1. the restatement against closed forms
def test_restatement_of_identical_images_is_one():
    x, _ = MC.make_inputs("recon", (2, 2, 176, 176))
    t = MC.ref_terms(x, x, torch.float64)
    assert float((t["sim"] - 1).abs().max()) < 1e-12 and float((t["cs"] - 1).abs().max()) < 1e-12 and float(t["mse"].abs().max()) == 0
    assert float((MC.ref_ms_ssim(t) - 1).abs().max()) < 1e-12
    assert t["sim"].shape == (2, 5)


@pytest.mark.parametrize("a,b,data_range", [(0.2, 0.7, 1.0), (0.5, 0.5, 1.0), (30.0, 200.0, 255.0)])
def test_restatement_of_constant_images(a, b, data_range):
    x, y = torch.full((1, 2, 24, 31), a, dtype=torch.float64), torch.full((1, 2, 24, 31), b, dtype=torch.float64)
    t = MC.ref_terms(x, y, torch.float64, data_range=data_range, scales=1)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    # the fp32-rounded taps sum to 1 within ~1e-9: with W = (sum g)^2 every "mean" is W times the constant and every "variance" W (1 - W) times a product
    W = float(MC.taps().double().sum()) ** 2
    assert abs(W - 1) < 1e-7
    cs = (2 * a * b * W * (1 - W) + c2) / ((a * a + b * b) * W * (1 - W) + c2)
    assert abs(float(t["cs"]) - cs) < 1e-12 and abs(float(t["sim"]) - (2 * a * b * W * W + c1) / ((a * a + b * b) * W * W + c1) * cs) < 1e-12
    assert abs(float(t["cs"]) - 1) < 1e-4 and abs(float(t["sim"]) - (2 * a * b + c1) / (a * a + b * b + c1)) < 1e-4       # the closed form of W = 1
    assert abs(float(t["mse"]) - (a - b) ** 2) < 1e-12


def test_restatement_is_symmetric_and_floors_odd_extents():
    x, y = MC.make_inputs("recon", MC.MS_SHAPES["odd183x201"])
    a, b = MC.ref_terms(x, y, torch.float64), MC.ref_terms(y, x, torch.float64)
    assert torch.equal(MC.ref_ms_ssim(a), MC.ref_ms_ssim(b)) and torch.equal(a["cs"], b["cs"])
    none_a, none_b = MC.ref_terms(x, y, torch.float64, data_range=None), MC.ref_terms(y, x, torch.float64, data_range=None)
    assert torch.equal(MC.ref_ms_ssim(none_a), MC.ref_ms_ssim(none_b)) and bool((none_a["L"] < 1).all()) and bool((none_a["L"] > 0.5).all())
    # 183 -> 91 -> 45 -> 22 -> 11: the last scale of the height is one window
    t = MC.ref_terms(x[:, :, :, :176], y[:, :, :, :176], torch.float64)
    assert t["sim"].shape == (2, 5)
    with pytest.raises(RuntimeError):
        MC.ref_terms(x[:, :, :175], y[:, :, :175], torch.float64)       # 175 -> ... -> 10 < 11: conv2d itself refuses


def test_the_cases_are_what_the_gpu_tests_assume():
    shape = MC.MS_SHAPES["min176"]
    recon, _ = MC.references("recon", shape, 1.0)
    assert float(MC.ms_terms(recon).min()) >= 0.8 and 0.97 < float(MC.ref_ms_ssim(recon).min()) < 0.995
    flat, flat32 = MC.references("flat", shape, 1.0)
    assert float(MC.ref_ms_ssim(flat).min()) > 0.999
    assert MC.term_distance(flat32, flat) > 10 * MC.term_distance(*reversed(MC.references("recon", shape, 1.0)))   # where fp32 second moments cancel
    unrelated, _ = MC.references("unrelated", shape, 1.0)
    neg = MC.ms_terms(unrelated).min(dim=1).values < -0.01
    assert bool(neg.any()) and bool((MC.ref_ms_ssim(unrelated)[neg] == 0).all())
    bank = MC.make_bank((4, 1, 176, 176))
    pairs = MC.all_pairs(4)
    t = MC.ref_terms(bank[[p[0] for p in pairs]], bank[[p[1] for p in pairs]], torch.float64)
    assert 0.6 < float(MC.ref_ms_ssim(t).mean()) < 0.9 and MC.MIN_TERM <= float(MC.ms_terms(t).min()) < 0.5
    assert torch.equal(MC.make_inputs("recon", shape)[0], MC.make_inputs("recon", shape)[0])            # seeded, cached


def test_taps_are_normalised_in_fp64_then_rounded():
    for k, sigma in ((11, 1.5), (7, 1.0), (3, 0.5)):
        g = MT.gaussian_taps(k, sigma)
        assert len(g) == k and g == [float(v) for v in MC.taps(k, sigma)] and g == g[::-1] and abs(sum(g) - 1) < 1e-6
        assert all(float(torch.tensor(v, dtype=torch.float32)) == v for v in g)                          # fp32 values
    assert abs(MT.gaussian_taps()[5] / MT.gaussian_taps()[4] - 2.718281828 ** (1 / 4.5)) < 1e-6


# ------------------------------------------------------------------------------------------------ 2. refusals and the size rule
def test_size_rule_at_175_and_176():
    assert MT.min_side() == 176 and MT.min_side(5, 7) == 112 and MT.min_side(1, 11) == 11
    small, ok = torch.zeros(1, 1, 175, 400), torch.zeros(1, 1, 176, 400)
    with pytest.raises(ValueError, match="x: .*at least 176.*175 x 400"):
        M.ms_ssim(small, small)
    with pytest.raises(ValueError, match="x: .*at least 176"):
        M.pairwise_ms_ssim(torch.zeros(3, 1, 200, 175))
    with pytest.raises(ValueError, match="x: on a ROCm device"):       # the size rule passed on the host; the device is asked last
        M.ms_ssim(ok, ok)
    with pytest.raises(ValueError, match="at least 11"):
        M.ssim(torch.zeros(1, 1, 10, 64), torch.zeros(1, 1, 10, 64))
    with pytest.raises(ValueError, match="x: on a ROCm device"):
        M.ssim(torch.zeros(1, 1, 11, 11), torch.zeros(1, 1, 11, 11))
    with pytest.raises(ValueError, match="at least 112"):
        M.ms_ssim(torch.zeros(1, 1, 111, 111), torch.zeros(1, 1, 111, 111), kernel_size=7)
    with pytest.raises(ValueError, match="ROCm"):
        M.ms_ssim(torch.zeros(1, 1, 44, 44), torch.zeros(1, 1, 44, 44), betas=(0.3, 0.3, 0.4))      # three scales: 11 * 4


def test_every_refusal_names_its_argument():
    x = torch.zeros(2, 1, 176, 176)
    for fn in (M.ssim, M.ms_ssim, M.mse):
        with pytest.raises(ValueError, match="x: 2-D images only"):
            fn(x[None], x[None])
        with pytest.raises(ValueError, match="y: 2-D images only"):
            fn(x, x[None])
        with pytest.raises(ValueError, match="x: a non-empty"):
            fn(x[0], x[0])
        with pytest.raises(ValueError, match="y: fp32"):
            fn(x, x.double())
        with pytest.raises(ValueError, match="x: fp32"):
            fn(x.half(), x)
        with pytest.raises(ValueError, match="y: of the shape of x"):
            fn(x, x[:1])
        with pytest.raises(ValueError, match="y: a tensor"):
            fn(x, None)
    with pytest.raises(ValueError, match="x: 2-D images only"):
        M.pairwise_ms_ssim(x[None])
    for bad in (dict(kernel_size=4), dict(kernel_size=13), dict(kernel_size=1), dict(kernel_size=7.0)):
        with pytest.raises(ValueError, match="kernel_size"):
            M.ssim(x, x, **bad)
        with pytest.raises(ValueError, match="kernel_size"):
            M.ms_ssim(x, x, **bad)
    with pytest.raises(ValueError, match="sigma"):
        M.ssim(x, x, sigma=0)
    for bad in (0, -1.0, float("inf"), "1"):
        with pytest.raises(ValueError, match="data_range"):
            M.ms_ssim(x, x, data_range=bad)
    with pytest.raises(ValueError, match="normalize"):
        M.ms_ssim(x, x, normalize="simple")
    with pytest.raises(ValueError, match="betas"):
        M.ms_ssim(x, x, betas=())
    with pytest.raises(ValueError, match="betas"):
        M.ms_ssim(x, x, betas=(0.5, -0.5))
    with pytest.raises(ValueError, match="chunk"):
        M.pairwise_ms_ssim(x, chunk=0)
    with pytest.raises(ValueError, match="chunk"):
        M.pairwise_ms_ssim(x, chunk=65536)
    meter = M.ReconstructionMeter(lambda t: (t,))
    with pytest.raises(ValueError, match="x: .*at least 176"):
        meter.update(torch.zeros(1, 3, 128, 128))
    with pytest.raises(ValueError, match="no update"):
        meter.compute()
    for name in ("ssim", "ms_ssim", "mse", "pairwise_ms_ssim", "ReconstructionMeter", "metrics"):
        assert hasattr(M, name)


# ------------------------------------------------------------------------------------------------ 3. the pair planner
def test_all_pairs_in_lexicographic_order():
    for n in (2, 3, 7):
        idx = MT.plan_pairs(n)
        assert idx.dtype == torch.int64 and idx.tolist() == [list(p) for p in MC.all_pairs(n)] and idx.shape == (n * (n - 1) // 2, 2)


@pytest.mark.parametrize("n,p", [(4, 3), (4, 6), (50, 1000), (3000, 1000)])
def test_drawn_pairs_are_distinct_unordered_and_seeded(n, p):
    a, b, c = MT.plan_pairs(n, p, seed=3), MT.plan_pairs(n, p, seed=3), MT.plan_pairs(n, p, seed=4)
    assert torch.equal(a, b) and a.shape == (p, 2) and a.dtype == torch.int64
    assert not torch.equal(a, c) or p == n * (n - 1) // 2 and sorted(a.tolist()) == sorted(c.tolist())
    rows = {tuple(r) for r in a.tolist()}
    assert len(rows) == p and all(0 <= i < j < n for i, j in rows)      # no duplicates, no (i, i), i < j
    if p == n * (n - 1) // 2:
        assert rows == set(MC.all_pairs(n))


def test_planner_refusals_and_explicit_pairs():
    given = torch.tensor([[2, 0], [0, 1], [2, 0]], dtype=torch.int32)
    assert MT.plan_pairs(3, given).tolist() == given.tolist() and MT.plan_pairs(3, given).dtype == torch.int64
    for bad in (7, 0, -1):
        with pytest.raises(ValueError, match="pairs: 1 .. 6"):
            MT.plan_pairs(4, bad)
    for bad in (torch.tensor([[0, 3]]), torch.tensor([[-1, 0]]), torch.tensor([[1, 1]]), torch.tensor([0, 1]), torch.tensor([[0.0, 1.0]]), torch.zeros(0, 2, dtype=torch.int64),
                "all", 2.0, True):
        with pytest.raises(ValueError, match="pairs"):
            MT.plan_pairs(3, bad)
    with pytest.raises(ValueError, match="at least two"):
        MT.plan_pairs(1)


# ------------------------------------------------------------------------------------------------ 4. the C ABI
def test_the_entry_points_are_declared_exported_and_bound():
    hdr = (ROOT / "include" / "medfusion_hip.h").read_text()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.exported_symbols() and hasattr(lib, name), name
        assert name in (ROOT / "DESIGN.md").read_text() and name in (ROOT / "INTEGRATION.md").read_text(), name
    assert lib.mf_version() == 250 and int(re.search(r"#define MF_VERSION (\d+)", hdr).group(1)) == 250      # additive within ABI 250
    assert "typedef struct MfSsimDesc" in hdr and int(re.search(r"#define MF_SSIM_MAX_K (\d+)", hdr).group(1)) == L.SSIM_MAX_K == 11


def test_metrics_unit_is_built_without_packed_fp32_and_linted():
    from medfusion_amd import build as B

    assert "metrics.hip" in B.SOURCES and "-packed-fp32-ops" in B.EXTRA_CFLAGS["metrics.hip"]
    assert B.lint_isa() == [] and (B.OBJ / "lint" / "metrics.s").exists()                  # the ISA lint walks SOURCES: metrics.hip with its own flags
    asm = (B.OBJ / "lint" / "metrics.s").read_text()
    assert "ssim_pairs_kernel" in asm and not re.search(r"^\s*v_pk_(mul|add|fma)_f32", asm, re.M)
    assert set(re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)) == {"0"}        # no scratch in any kernel of the unit


def test_descriptor_layout_matches_what_a_c_compiler_sees(tmp_path):
    assert C.sizeof(L.MfSsimDesc) == 4 * (10 + 11 + 3)
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "medfusion_hip.h"', 'int main(void) {', '  printf("MfSsimDesc %zu\\n", sizeof(MfSsimDesc));']
    for fname, _ in L.MfSsimDesc._fields_:
        lines.append(f'  printf("MfSsimDesc.{fname} %zu\\n", offsetof(MfSsimDesc, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["MfSsimDesc"]) == C.sizeof(L.MfSsimDesc)
    for fname, _ in L.MfSsimDesc._fields_:
        assert int(got[f"MfSsimDesc.{fname}"]) == getattr(L.MfSsimDesc, fname).offset, fname


def _desc(**change):
    d = K.make_ssim_desc(3, 2, 43, 75, 4, 5, MT.gaussian_taps(), 0.01, 0.03, 1.0, indexed=0, want_mse=True)
    for key, v in change.items():
        setattr(d, key, v)
    return d


def test_descriptor_rules_on_the_host():
    lib = L.load()
    good = _desc()
    assert K.ssim_ok(good) and list(good.taps) == MT.gaussian_taps() and (good.k, good.range_on_device) == (11, 0)
    # 43 x 75 under an 11-tap window: 33 x 65 origins = 2 x 3 tiles of 32 x 32, three fp64 sums per (pair, channel, tile)
    assert lib.mf_ssim_workspace_bytes(C.byref(good)) == 3 * 2 * 6 * 3 * 8
    assert lib.mf_ssim_workspace_bytes(C.byref(_desc(H=11, W=11, k=11))) == 3 * 2 * 1 * 3 * 8
    assert K.ssim_ok(_desc(k=3)) and K.ssim_ok(_desc(H=11, W=11)) and K.ssim_ok(_desc(P=9, indexed=3)) and K.ssim_ok(_desc(P=5, indexed=1))
    none = K.make_ssim_desc(1, 1, 11, 11, 1, 1, MT.gaussian_taps(), 0.01, 0.03, None)
    assert K.ssim_ok(none) and none.range_on_device == 1
    for bad, word in ((dict(k=4), b"k=4"), (dict(k=13), b"k=13"), (dict(k=1), b"k=1"), (dict(H=10), b"extents"), (dict(W=10), b"extents"), (dict(P=0), b"P=0"),
                      (dict(C=0), b"C=0"), (dict(P=65536, indexed=3), b"P=65536"), (dict(Nx=0), b"banks"), (dict(P=5), b"without ix"),
                      (dict(P=5, indexed=1), None), (dict(P=6, indexed=1), b"without iy"), (dict(indexed=4), b"indexed"), (dict(want_mse=2), b"want_mse")):
        d = _desc(**bad)
        if word is None:
            assert K.ssim_ok(d)
            continue
        assert not K.ssim_ok(d) and word in lib.mf_last_error(), bad
        assert lib.mf_ssim_workspace_bytes(C.byref(d)) == 0
    assert lib.mf_ssim_ok(None) == 0


def test_entry_points_refuse_before_any_launch():
    """argument checks run on the host (the pointers are never dereferenced, no device is needed)"""
    lib = L.load()
    p = 1 << 20
    need = lib.mf_ssim_workspace_bytes(C.byref(_desc()))
    pairs = lambda d, ix=None, iy=None, mx=None, my=None, ws=p, nbytes=need: lib.mf_ssim_pairs_f32(p, p, ix, iy, mx, my, ws, nbytes, C.byref(d), None)
    assert pairs(_desc(k=4)) == -1 and b"k=4" in lib.mf_last_error()
    assert lib.mf_ssim_pairs_f32(p, p, None, None, None, None, p, need, None, None) == -1
    assert lib.mf_ssim_pairs_f32(None, p, None, None, None, None, p, need, C.byref(_desc()), None) == -1
    assert pairs(_desc(), ws=None) == -1
    assert pairs(_desc(), ix=p) == -1 and b"indexed" in lib.mf_last_error()                    # an index array the descriptor does not announce
    assert pairs(_desc(indexed=3), ix=p) == -1 and pairs(_desc(indexed=2)) == -1
    assert pairs(_desc(), mx=p, my=p) == -1 and b"range_on_device" in lib.mf_last_error()
    assert pairs(_desc(range_on_device=1), mx=p) == -1
    assert pairs(_desc(), ws=p + 4) == -1 and b"aligned" in lib.mf_last_error()
    assert pairs(_desc(), nbytes=need - 1) == -4 and b"needed" in lib.mf_last_error()          # MF_EWORKSPACE
    finish = lambda d, sim=p, cs=p, mse=p, stride=1: lib.mf_ssim_finish_f32(p, sim, cs, mse, stride, C.byref(d), None)
    assert finish(_desc(H=5)) == -1 and b"extents" in lib.mf_last_error()
    assert finish(_desc(), None, None, None) == -1 and finish(_desc(), stride=0) == -1
    assert finish(_desc(want_mse=0)) == -1 and b"want_mse" in lib.mf_last_error()
    assert lib.mf_ssim_finish_f32(None, p, p, None, 1, C.byref(_desc()), None) == -1
    assert lib.mf_avgpool2_planes_f32(p, p, 0, 8, 8, None) == -1 and lib.mf_avgpool2_planes_f32(p, p, 4, 1, 8, None) == -1
    assert lib.mf_avgpool2_planes_f32(None, p, 4, 8, 8, None) == -1 and b"avgpool2_planes" in lib.mf_last_error()
    assert lib.mf_rows_minmax_f32(p, p, 0, 16, None) == -1 and lib.mf_rows_minmax_f32(p, p, 2, 0, None) == -1 and lib.mf_rows_minmax_f32(p, None, 2, 16, None) == -1
    with pytest.raises(RuntimeError, match="ROCm"):
        K.rows_minmax(torch.zeros(2, 8))                                # the wrappers have no CPU path
    with pytest.raises(RuntimeError, match="ROCm"):
        K.avgpool2_planes(torch.zeros(1, 1, 8, 8))


# ------------------------------------------------------------------------------------------------ 5. the scripts, without a device
def _script(name):
    spec = importlib.util.spec_from_file_location(f"_metrics_script_{name}", ROOT / "scripts" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name,words", [("evaluate_latent_embedder", ("--checkpoint", "--images", "--batch", "--max-samples", "--out")),
                                        ("diversity", ("--images", "--pairs", "--seed")), ("sample_dataset", ("--diversity",)),
                                        ("metrics_bench", ("--plan", "--reps"))])
def test_scripts_help(name, words):
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / f"{name}.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and all(w in r.stdout for w in words), r.stdout + r.stderr


def test_diversity_of_one_image_is_refused_before_sampling():
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "sample_dataset.py"), "--synthetic", "--diversity", "5", "--n-samples", "1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--diversity: at least two images" in r.stderr


def test_scripts_argument_rules(tmp_path, capsys):
    ev, dv = _script("evaluate_latent_embedder"), _script("diversity")
    a = ev.parse_args(["--checkpoint", "x.ckpt", "--images", "scans"])
    assert (a.batch, a.max_samples, a.embedder, a.synthetic) == (100, None, "VAE", False)
    for bad in (["--images", "scans"], ["--images", "scans", "--checkpoint", "x", "--synthetic"], ["--checkpoint", "x"], ["--checkpoint", "x", "--images", "s", "--batch", "0"],
                ["--checkpoint", "x", "--images", "s", "--max-samples", "0"], ["--checkpoint", "x", "--images", "s", "--embedder", "UNet"]):
        with pytest.raises(SystemExit):
            ev.parse_args(bad)
    d = dv.parse_args(["--images", "generated"])
    assert (d.pairs, d.seed, d.max_samples) == (1000, 0, None)
    for bad in ([], ["--images", "g", "--pairs", "0"], ["--images", "g", "--max-samples", "1"], ["--images", "g", "--batch", "0"]):
        with pytest.raises(SystemExit):
            dv.parse_args(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit, match="no PNG files"):
        ev.list_images(tmp_path)
    for i in range(3):
        (tmp_path / f"im_{i}.png").write_bytes(b"")
    assert [f.name for f in ev.list_images(tmp_path, 2)] == ["im_0.png", "im_1.png"]
    rep = dv.report(torch.tensor([0.25, 0.75]), 2, 3)
    assert rep["ms_ssim_pairwise_mean"] == 0.5 and abs(rep["ms_ssim_pairwise_std"] - float(torch.std(torch.tensor([0.25, 0.75])))) < 1e-7 and rep["pairs"] == 2
    bench = _script("metrics_bench")
    b = bench.compulsory_bytes(1, 2, 3, 256, 256)
    assert b["kernel"] == sum(2 * 4 * 3 * (256 >> s) ** 2 for s in range(5)) and b["torch_form"] > 10 * b["kernel"]
    rows = bench.kernel_resources()
    assert any("ssim_pairs_kernel<K=11, V=4>" in r for r in rows) and all("scratch 0 B" in r for r in rows)
