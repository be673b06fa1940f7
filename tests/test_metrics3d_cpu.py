"""The volume metrics without a device: every refusal of the public interface and the size rule, betas_for / min_side3d, the descriptor rules of
the C ABI through the library loaded without a GPU, the plain-torch restatement the GPU tests check against (self-checks), and the scripts' arguments."""
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
from medfusion_amd import metrics3d as M3
from tests import metrics3d_cases as MC
from tests import metrics_cases as MC2

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("mf_ssim3d_ok", "mf_ssim3d_workspace_bytes", "mf_ssim3d_pairs_f32", "mf_ssim3d_finish_f32", "mf_avgpool2_volumes_f32")


# ------------------------------------------------------------------------------------------------ 1. host-side argument rules
def test_betas_for_and_min_side3d():
    for s in range(1, 6):
        b = M.betas_for(s)
        assert len(b) == s and abs(sum(b) - 1) < 1e-12 and b == MC.betas_for(s)
        for i in range(s):
            assert abs(b[i] / b[0] - MT.BETAS[i] / MT.BETAS[0]) < 1e-12          # the published ratios
    assert M.betas_for(5) == tuple(v / sum(MT.BETAS) for v in MT.BETAS) and M.betas_for(1) == (1.0,)
    for bad in (0, 6, -1, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="scales"):
            M.betas_for(bad)
    assert M.min_side3d() == 176 and M.min_side3d(3, 11) == 44 and M.min_side3d(4, 7) == 56 and M.min_side3d(1, 11) == 11 and M.min_side3d(2, 5) == 10
    # the published 64 x 128 x 128 volume: three scales at k = 11, four at k = 7
    assert M3.max_scales3d(64, 11) == 3 and M3.max_scales3d(64, 7) == 4 and M3.max_scales3d(10, 11) == 0 and M3.max_scales3d(176, 11) == 5


def test_size_rule_names_the_minimum_side_and_the_admissible_scales():
    pub = torch.zeros(1, 1, 64, 128, 128)
    with pytest.raises(ValueError, match=r"x: 5 scale\(s\) of a 11-tap window need sides of at least 176, got 64 x 128 x 128, which admits at most 3 scale\(s\) "
                                         r"\(betas=betas_for\(3\)\) at kernel_size=11"):
        M.ms_ssim3d(pub, pub)                                                    # the 2-D defaults
    with pytest.raises(ValueError, match="x: on a ROCm device"):               # the size rule passed on the host; the device is asked last
        M.ms_ssim3d(pub, pub, betas=M.betas_for(3))
    with pytest.raises(ValueError, match="x: on a ROCm device"):
        M.ms_ssim3d(pub, pub, betas=M.betas_for(4), kernel_size=7)
    with pytest.raises(ValueError, match=r"at least 88.*at most 3 scale"):
        M.ms_ssim3d(pub, pub, betas=M.betas_for(4))
    with pytest.raises(ValueError, match=r"at least 112.*at most 4 scale.*kernel_size=7"):
        M.ms_ssim3d(pub, pub, betas=M.betas_for(5), kernel_size=7)
    small, ok = torch.zeros(1, 1, 44, 43, 60), torch.zeros(1, 1, 44, 44, 60)
    with pytest.raises(ValueError, match=r"x: .*at least 44, got 44 x 43 x 60.*at most 2"):
        M.ms_ssim3d(small, small, betas=M.betas_for(3))
    with pytest.raises(ValueError, match=r"x: .*at least 44"):
        M.pairwise_ms_ssim3d(small.expand(3, -1, -1, -1, -1), betas=M.betas_for(3))
    with pytest.raises(ValueError, match="x: on a ROCm device"):
        M.ms_ssim3d(ok, ok, betas=M.betas_for(3))
    with pytest.raises(ValueError, match=r"at least 11, got 10 x 64 x 64.*not even one scale"):
        M.ssim3d(torch.zeros(1, 1, 10, 64, 64), torch.zeros(1, 1, 10, 64, 64))
    with pytest.raises(ValueError, match="x: on a ROCm device"):
        M.ssim3d(torch.zeros(1, 1, 11, 11, 11), torch.zeros(1, 1, 11, 11, 11))
    with pytest.raises(ValueError, match="at least 3"):
        M.mse3d(torch.zeros(1, 1, 2, 8, 8), torch.zeros(1, 1, 2, 8, 8))


def test_every_refusal_names_its_argument():
    x = torch.zeros(2, 1, 44, 44, 44)
    b3 = M.betas_for(3)
    fns = (M.ssim3d, lambda p, q: M.ms_ssim3d(p, q, betas=b3), M.mse3d, lambda p, q: M3.ms_ssim3d_and_mse(p, q, betas=b3), M.pair_range3d)
    for fn in fns:
        with pytest.raises(ValueError, match="x: volumes only.*2-D function"):
            fn(x[0], x[0])
        with pytest.raises(ValueError, match="y: volumes only.*2-D function"):
            fn(x, x[0])
        with pytest.raises(ValueError, match="x: a non-empty"):
            fn(x[0, 0], x[0, 0])
        with pytest.raises(ValueError, match="x: a non-empty"):
            fn(x[None], x[None])
        with pytest.raises(ValueError, match="x: a non-empty"):
            fn(x[:0], x[:0])
        with pytest.raises(ValueError, match="y: fp32"):
            fn(x, x.double())
        with pytest.raises(ValueError, match="x: fp32"):
            fn(x.half(), x)
        with pytest.raises(ValueError, match="y: of the shape of x"):
            fn(x, x[:1])
        with pytest.raises(ValueError, match="y: a tensor"):
            fn(x, None)
    with pytest.raises(ValueError, match="x: volumes only"):
        M.pairwise_ms_ssim3d(x[0], betas=b3)
    for bad in (dict(kernel_size=4), dict(kernel_size=13), dict(kernel_size=1), dict(kernel_size=7.0)):
        with pytest.raises(ValueError, match="kernel_size"):
            M.ssim3d(x, x, **bad)
        with pytest.raises(ValueError, match="kernel_size"):
            M.ms_ssim3d(x, x, betas=b3, **bad)
    with pytest.raises(ValueError, match="sigma"):
        M.ssim3d(x, x, sigma=0)
    for bad in (0, -1.0, float("inf"), "1"):
        with pytest.raises(ValueError, match="data_range"):
            M.ms_ssim3d(x, x, betas=b3, data_range=bad)
    with pytest.raises(ValueError, match="normalize"):
        M.ms_ssim3d(x, x, betas=b3, normalize="simple")
    with pytest.raises(ValueError, match="betas"):
        M.ms_ssim3d(x, x, betas=())
    with pytest.raises(ValueError, match="betas"):
        M.ms_ssim3d(x, x, betas=(0.5, -0.5))
    for bad in (0, 65536, 2.0, True):
        with pytest.raises(ValueError, match="chunk"):
            M.pairwise_ms_ssim3d(x, betas=b3, chunk=bad)
    with pytest.raises(ValueError, match="x: on a ROCm device"):               # (the pairs are planned after the device is asked, as in 2-D)
        M.pairwise_ms_ssim3d(x, betas=b3)
    meter = M.VolumeReconstructionMeter(lambda t: (t,))
    assert meter.betas == M.betas_for(3) and (meter.kernel_size, meter.sigma) == (11, 1.5)
    with pytest.raises(ValueError, match=r"x: .*at least 44.*at most 2"):
        meter.update(torch.zeros(1, 1, 32, 64, 64))
    with pytest.raises(ValueError, match="x: volumes only"):
        meter.update(torch.zeros(1, 3, 176, 176))
    with pytest.raises(ValueError, match="no update"):
        meter.compute()
    with pytest.raises(ValueError, match="kernel_size"):
        M.VolumeReconstructionMeter(lambda t: (t,), kernel_size=6)
    for name in ("ssim3d", "ms_ssim3d", "mse3d", "ms_ssim3d_and_mse", "pairwise_ms_ssim3d", "pyramid3d", "pair_range3d", "min_side3d", "betas_for",
                 "VolumeReconstructionMeter"):
        assert hasattr(M, name), name


def test_the_2d_functions_keep_refusing_volumes():
    x = torch.zeros(1, 1, 16, 176, 176)
    for fn in (M.ssim, M.ms_ssim, M.mse):
        with pytest.raises(ValueError, match="x: 2-D images only.*5-D volume"):
            fn(x, x)
    with pytest.raises(ValueError, match="x: 2-D images only"):
        M.ReconstructionMeter(lambda t: (t,)).update(x)


def test_pair_chunk_is_bounded_by_the_workspace():
    # 64 x 128 x 128 at k = 11: 54 x 118 x 118 origins = 4 x 8 x 8 tiles of 16^3, 24 bytes each
    assert M3._pair_chunk(1, 64, 128, 128, 11) == (64 << 20) // (256 * 24) == 10922
    assert M3._pair_chunk(1, 256, 256, 256, 11) == (64 << 20) // (4096 * 24) == 682
    assert M3._pair_chunk(1, 11, 11, 11, 11) == 65535 and M3._pair_chunk(16, 1024, 1024, 1024, 3) == 1


# ------------------------------------------------------------------------------------------------ 2. the C ABI
def test_the_entry_points_are_declared_exported_and_bound():
    hdr = (ROOT / "include" / "medfusion_hip.h").read_text()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.exported_symbols() and hasattr(lib, name), name
        assert name in (ROOT / "INTEGRATION.md").read_text(), name
    assert lib.mf_version() == 250 and int(re.search(r"#define MF_VERSION (\d+)", hdr).group(1)) == 250      # additive within ABI 250
    assert "typedef struct MfSsim3dDesc" in hdr


def test_metrics3d_unit_is_built_without_packed_fp32_and_linted():
    from medfusion_amd import build as B

    assert "metrics3d.hip" in B.SOURCES and "-packed-fp32-ops" in B.EXTRA_CFLAGS["metrics3d.hip"]
    assert B.lint_isa() == [] and (B.OBJ / "lint" / "metrics3d.s").exists()
    asm = (B.OBJ / "lint" / "metrics3d.s").read_text()
    assert "ssim3d_pairs_kernel" in asm and not re.search(r"^\s*v_pk_(mul|add|fma)_f32", asm, re.M)
    assert set(re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)) == {"0"}        # no scratch in any kernel of the unit: the ring is registers
    vgprs = [int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", asm)]
    assert max(vgprs) <= 128                                                               # four waves per SIMD at the least (the header's budget)


def test_descriptor_layout_matches_what_a_c_compiler_sees(tmp_path):
    assert C.sizeof(L.MfSsim3dDesc) == 4 * (11 + 11 + 3)
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "medfusion_hip.h"', 'int main(void) {', '  printf("MfSsim3dDesc %zu\\n", sizeof(MfSsim3dDesc));']
    for fname, _ in L.MfSsim3dDesc._fields_:
        lines.append(f'  printf("MfSsim3dDesc.{fname} %zu\\n", offsetof(MfSsim3dDesc, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["MfSsim3dDesc"]) == C.sizeof(L.MfSsim3dDesc)
    for fname, _ in L.MfSsim3dDesc._fields_:
        assert int(got[f"MfSsim3dDesc.{fname}"]) == getattr(L.MfSsim3dDesc, fname).offset, fname


def _desc(**change):
    d = K.make_ssim3d_desc(3, 2, 24, 43, 75, 4, 5, MT.gaussian_taps(), 0.01, 0.03, 1.0, indexed=0, want_mse=True)
    for key, v in change.items():
        setattr(d, key, v)
    return d


def test_descriptor_rules_on_the_host():
    lib = L.load()
    good = _desc()
    assert K.ssim3d_ok(good) and list(good.taps) == MT.gaussian_taps() and (good.k, good.range_on_device, good.D) == (11, 0, 24)
    # 24 x 43 x 75 under an 11-tap window: 14 x 33 x 65 origins = 1 x 3 x 5 tiles of 16 x 16 x 16, three fp64 sums per (pair, channel, tile)
    assert lib.mf_ssim3d_workspace_bytes(C.byref(good)) == 3 * 2 * 15 * 3 * 8
    assert lib.mf_ssim3d_workspace_bytes(C.byref(_desc(D=11, H=11, W=11))) == 3 * 2 * 1 * 3 * 8
    assert lib.mf_ssim3d_workspace_bytes(C.byref(_desc(D=40, H=23, W=40, k=7))) == 3 * 2 * (3 * 2 * 3) * 3 * 8       # 34 x 17 x 34 origins
    assert lib.mf_ssim3d_workspace_bytes(C.byref(_desc(P=1, C=1, D=64, H=128, W=128))) == 256 * 3 * 8                 # the published volume
    assert K.ssim3d_ok(_desc(k=3)) and K.ssim3d_ok(_desc(D=11, H=11, W=11)) and K.ssim3d_ok(_desc(P=9, indexed=3)) and K.ssim3d_ok(_desc(P=5, indexed=1))
    none = K.make_ssim3d_desc(1, 1, 11, 11, 11, 1, 1, MT.gaussian_taps(), 0.01, 0.03, None)
    assert K.ssim3d_ok(none) and none.range_on_device == 1
    for bad, word in ((dict(k=4), b"k=4"), (dict(k=13), b"k=13"), (dict(k=1), b"k=1"), (dict(D=10), b"extents"), (dict(H=10), b"extents"), (dict(W=10), b"extents"),
                      (dict(P=0), b"P=0"), (dict(C=0), b"C=0"), (dict(P=65536, indexed=3), b"P=65536"), (dict(C=65536), b"C=65536"), (dict(Nx=0), b"banks"),
                      (dict(Ny=0), b"banks"), (dict(P=5), b"without ix"), (dict(P=5, indexed=1), None), (dict(P=6, indexed=1), b"without iy"),
                      (dict(indexed=4), b"indexed"), (dict(want_mse=2), b"want_mse"), (dict(range_on_device=2), b"range_on_device"),
                      (dict(D=2048, H=2048, W=2048), b"a volume of")):
        d = _desc(**bad)
        if word is None:
            assert K.ssim3d_ok(d)
            continue
        assert not K.ssim3d_ok(d) and word in lib.mf_last_error(), bad
        assert lib.mf_ssim3d_workspace_bytes(C.byref(d)) == 0
    assert lib.mf_ssim3d_ok(None) == 0


def test_entry_points_refuse_before_any_launch():
    """argument checks run on the host (the pointers are never dereferenced, no device is needed)"""
    lib = L.load()
    p = 1 << 20
    need = lib.mf_ssim3d_workspace_bytes(C.byref(_desc()))
    pairs = lambda d, ix=None, iy=None, mx=None, my=None, ws=p, nbytes=need: lib.mf_ssim3d_pairs_f32(p, p, ix, iy, mx, my, ws, nbytes, C.byref(d), None)
    assert pairs(_desc(k=4)) == -1 and b"k=4" in lib.mf_last_error()
    assert pairs(_desc(D=5)) == -1 and b"extents" in lib.mf_last_error()
    assert lib.mf_ssim3d_pairs_f32(p, p, None, None, None, None, p, need, None, None) == -1
    assert lib.mf_ssim3d_pairs_f32(None, p, None, None, None, None, p, need, C.byref(_desc()), None) == -1
    assert pairs(_desc(), ws=None) == -1
    assert pairs(_desc(), ix=p) == -1 and b"indexed" in lib.mf_last_error()                    # an index array the descriptor does not announce
    assert pairs(_desc(indexed=3), ix=p) == -1 and pairs(_desc(indexed=2)) == -1
    assert pairs(_desc(), mx=p, my=p) == -1 and b"range_on_device" in lib.mf_last_error()
    assert pairs(_desc(range_on_device=1), mx=p) == -1
    assert pairs(_desc(), ws=p + 4) == -1 and b"aligned" in lib.mf_last_error()
    assert pairs(_desc(), nbytes=need - 1) == -4 and b"needed" in lib.mf_last_error()          # MF_EWORKSPACE
    finish = lambda d, sim=p, cs=p, mse=p, stride=1: lib.mf_ssim3d_finish_f32(p, sim, cs, mse, stride, C.byref(d), None)
    assert finish(_desc(H=5)) == -1 and b"extents" in lib.mf_last_error()
    assert finish(_desc(), None, None, None) == -1 and finish(_desc(), stride=0) == -1
    assert finish(_desc(want_mse=0)) == -1 and b"want_mse" in lib.mf_last_error()
    assert lib.mf_ssim3d_finish_f32(None, p, p, None, 1, C.byref(_desc()), None) == -1
    assert lib.mf_avgpool2_volumes_f32(p, p, 0, 8, 8, 8, None) == -1 and lib.mf_avgpool2_volumes_f32(p, p, 4, 1, 8, 8, None) == -1
    assert lib.mf_avgpool2_volumes_f32(p, p, 4, 8, 1, 8, None) == -1 and lib.mf_avgpool2_volumes_f32(p, p, 4, 8, 8, 1, None) == -1
    assert lib.mf_avgpool2_volumes_f32(None, p, 4, 8, 8, 8, None) == -1 and b"avgpool2_volumes" in lib.mf_last_error()
    with pytest.raises(RuntimeError, match="ROCm"):
        K.avgpool2_volumes(torch.zeros(1, 1, 8, 8, 8))                  # the wrappers have no CPU path
    with pytest.raises(RuntimeError, match="ROCm"):
        K.ssim3d_pairs(torch.zeros(4, 2, 24, 43, 75), torch.zeros(5, 2, 24, 43, 75), _desc(), torch.zeros(3), None)


# ------------------------------------------------------------------------------------------------ 3. the restatement's self-checks
def test_restatement_on_a_volume_constant_along_depth_is_the_2d_restatement_of_the_slice():
    x2, y2 = MC2.make_inputs("recon", (2, 2, 24, 31))
    x3, y3 = (t[:, :, None].expand(-1, -1, 14, -1, -1).contiguous() for t in (x2, y2))
    for data_range in (1.0, None):
        t2 = MC2.ref_terms(x2, y2, torch.float64, data_range=data_range, scales=1)
        t3 = MC.ref_terms3d(x3, y3, torch.float64, data_range=data_range, scales=1)
        # the taps' sum misses 1 by a few 1e-9: one more filtered axis moves every moment by that much
        assert MC.term_distance(t3, t2) < 1e-6 and torch.equal(t3["L"], t2["L"])
        assert float((t3["mse"] - t2["mse"]).abs().max()) < 1e-15


def test_restatement_is_invariant_under_a_permutation_of_the_axes():
    shape, k, sigma, scales = MC.MS_CASES["k7s3"]
    x, y = MC.make_inputs("recon", shape)
    want = MC.ref_terms3d(x, y, torch.float64, k=k, sigma=sigma, scales=scales)
    for perm in ((0, 1, 4, 2, 3), (0, 1, 3, 4, 2), (0, 1, 2, 4, 3)):
        got = MC.ref_terms3d(x.permute(perm).contiguous(), y.permute(perm).contiguous(), torch.float64, k=k, sigma=sigma, scales=scales)
        assert MC.term_distance(got, want) < 1e-12, perm
    assert torch.equal(MC.ref_ms_ssim3d(MC.ref_terms3d(y, x, torch.float64, k=k, sigma=sigma, scales=scales)), MC.ref_ms_ssim3d(want))


def test_the_cases_are_what_the_gpu_tests_assume():
    for name, (shape, k, sigma, scales) in MC.MS_CASES.items():
        assert min(shape[2:]) >= M.min_side3d(scales, k), name
        for data_range in (1.0, None):
            for kind in ("recon", "flat"):
                assert float(MC.ms_terms(MC.references(kind, shape, data_range, k, sigma, scales)[0]).min()) >= 0.6, (name, kind)
            inv = MC.ms_terms(MC.references("inverted", shape, data_range, k, sigma, scales)[0])
            assert bool((inv.min(dim=1).values <= -0.5).all()), name                      # a clearly negative term in every row
    shape, k, sigma, scales = MC.MS_CASES["odd"]
    flat, flat32 = MC.references("flat", shape, None, k, sigma, scales)
    assert MC.term_distance(flat32, flat) > 0.1                                            # where fp32 second moments cancel: d32 is useless, hence FLAT_CAP_3D
    assert abs(MC.FLAT_CAP_3D - 4 * (36 * 2.0 ** -24 * 26 * 2e-6) / 3e-6) < 1e-5
    assert len(MC.KERNEL_CASES) == 15 and ("deep", "k7") in MC.KERNEL_CASES and ("deep", "k3") in MC.KERNEL_CASES
    # every axis of the edge cases has at least two tiles and a partial last one
    _, _, D, H, W = MC.KERNEL_SHAPES["edges_scalar"]
    assert (H - 10) > MC.TILE and (H - 10) % MC.TILE and (W - 10) > MC.TILE and (W - 10) % MC.TILE and W % 4
    assert (MC.KERNEL_SHAPES["deep"][2] - 6) > 2 * MC.DCHUNK and (MC.KERNEL_SHAPES["deep"][2] - 6) % MC.DCHUNK
    assert MC.KERNEL_SHAPES["vec4"][4] % 4 == 0
    assert torch.equal(MC.make_inputs("recon", shape)[0], MC.make_inputs("recon", shape)[0])            # seeded, cached


# ------------------------------------------------------------------------------------------------ 4. the scripts, without a device
def _script(name):
    spec = importlib.util.spec_from_file_location(f"_metrics3d_script_{name}", ROOT / "scripts" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_plan_runs_without_a_device():
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "metrics3d_bench.py"), "--plan"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "4 pairs of 1 x 64 x 128 x 128" in r.stdout and "1024 workgroups" in r.stdout and "ssim3d_pairs_kernel<K=11, V=4>" in r.stdout
    assert all("scratch 0 B" in ln for ln in r.stdout.splitlines() if "vgpr" in ln)
    bench = _script("metrics3d_bench")
    b = bench.compulsory_bytes(1, 2, 1, 64, 128, 128)
    assert b["kernel"] == sum(2 * 4 * (64 >> s) * (128 >> s) ** 2 for s in range(3)) and b["torch_form"] > 10 * b["kernel"]


def test_evaluate_volumes_arguments(tmp_path, capsys):
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "evaluate_volumes.py"), "--help"], capture_output=True, text=True, timeout=120)
    words = ("--checkpoint", "--volumes", "--scales", "--kernel-size", "--batch", "--max-samples", "--pairs", "--seed", "--out", "--unit-range")
    assert r.returncode == 0 and all(w in r.stdout for w in words), r.stdout + r.stderr
    ev = _script("evaluate_volumes")
    a = ev.parse_args(["--checkpoint", "x.ckpt", "--volumes", "scans"])
    assert (a.scales, a.kernel_size, a.batch, a.max_samples, a.pairs, a.seed, a.unit_range) == (3, 11, 2, None, None, 0, False)
    assert ev.parse_args(["--volumes", "scans", "--pairs", "10"]).checkpoint is None
    for bad in (["--checkpoint", "x"], ["--volumes", "s"], ["--volumes", "s", "--pairs", "0"], ["--volumes", "s", "--checkpoint", "x", "--batch", "0"],
                ["--volumes", "s", "--checkpoint", "x", "--scales", "6"], ["--volumes", "s", "--checkpoint", "x", "--kernel-size", "4"],
                ["--volumes", "s", "--checkpoint", "x", "--max-samples", "0"]):
        with pytest.raises(SystemExit):
            ev.parse_args(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit, match="no .npy or .pt files"):
        ev.list_volumes(tmp_path)
    import numpy as np
    np.save(tmp_path / "a.npy", np.linspace(-1, 1, 4 * 5 * 6, dtype=np.float64).reshape(4, 5, 6))
    torch.save(torch.linspace(0, 1, 2 * 4 * 5 * 6).reshape(2, 4, 5, 6), tmp_path / "b.pt")
    files = ev.list_volumes(tmp_path)
    assert [f.name for f in files] == ["a.npy", "b.pt"] and [f.name for f in ev.list_volumes(tmp_path, 1)] == ["a.npy"]
    v = ev.load_volume(files[0], unit_range=False)
    assert v.shape == (1, 4, 5, 6) and v.dtype == torch.float32 and float(v.min()) == -1 and float(v.max()) == 1
    w = ev.load_volume(files[1], unit_range=True)                       # [0, 1] on disk -> [-1, 1]
    assert w.shape == (2, 4, 5, 6) and float(w.min()) == -1 and float(w.max()) == 1
    torch.save(torch.zeros(5, 6), tmp_path / "c.pt")
    with pytest.raises(SystemExit, match=r"c.pt: a \[C, D, H, W\] or \[D, H, W\]"):
        ev.load_volume(tmp_path / "c.pt", unit_range=False)
    rep = ev.report_pairs(torch.tensor([0.25, 0.75]), 2, 3)
    assert rep["ms_ssim_pairwise_mean"] == 0.5 and rep["pairs"] == 2 and rep["volumes"] == 3
