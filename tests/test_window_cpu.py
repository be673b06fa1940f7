"""Windowed denoising on the host: the window plan (origins, order, cover counts, refusals), the plain-torch merge the GPU tests check against
(its own fp32 error under the derived bound, exact where one window covers), the pipeline's refusals, and the C ABI of the two entry points."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

import medfusion_amd as M
from medfusion_amd import lib as L
from medfusion_amd.window import MF_WINDOW_MAX_PER_AXIS, WindowPlan
from oracle import restate as R
from oracle import synth as S
from tests import window_cases as WC
from tests.util import to_product_kwargs

ROOT = Path(__file__).resolve().parents[1]


def _flat(t):
    return [x for u in t for x in _flat(u)] if isinstance(t, list) else [t]


# ------------------------------------------------------------------------------------------------ 1. the plan
@pytest.mark.parametrize("name", list(WC.GEOMETRIES))
def test_plan_geometry(name):
    g = WC.GEOMETRIES[name]
    plan = WindowPlan(g["canvas"], g["window"], g["stride"])
    ref = WC.RefPlan(g["canvas"], g["window"], g["stride"])
    assert plan.origins == g["origins"] == ref.origins
    assert plan.M == g["M"] == ref.M and plan.windows == ref.windows           # row-major, the last axis fastest
    assert plan.windows[1][-1] != plan.windows[0][-1] or len(plan.origins[-1]) == 1
    assert set(_flat(plan.cover)) == g["cover"]
    assert torch.equal(torch.tensor(plan.cover), ref.cover())
    assert not plan.none
    for a, (L_, h) in enumerate(zip(g["canvas"], g["window"])):                 # total coverage, nothing outside the canvas
        assert plan.origins[a][0] == 0 and plan.origins[a][-1] == L_ - h


def test_default_stride_weights_and_the_single_window():
    plan = WindowPlan((6, 12, 12), (4, 8, 8))
    assert plan.stride == (2, 4, 4) and plan.weight == "tent" and plan.M == 8
    assert WindowPlan((5, 5), (1, 3)).stride == (1, 1)                          # h // 2, at least 1
    assert plan.profile(1) == [1, 2, 3, 4, 4, 3, 2, 1] and WindowPlan((9,) * 2, (7, 7)).profile(0) == [1, 2, 3, 4, 3, 2, 1]
    assert WindowPlan((9, 9), (7, 7), weight="uniform").profile(0) == [1] * 7
    assert torch.equal(WC.RefPlan((9, 9), (7, 7)).weights()[3], torch.tensor([4.0, 8, 12, 16, 12, 8, 4]))
    one = WindowPlan((8, 8), (8, 8))
    assert one.none and one.M == 1 and one.origins == ((0,), (0,))
    assert one.M == 1 and WindowPlan((8, 8), (8, 8), 3).none
    assert "M = 4" in WindowPlan((12, 12), (8, 8), 4).describe()


def test_plan_refusals():
    with pytest.raises(ValueError, match="spatial axis"):
        WindowPlan((12, 12), (8, 8), dims=3)                                    # the model is 3-D
    with pytest.raises(ValueError, match="spatial axis"):
        WindowPlan((12, 12), (4, 8, 8))
    with pytest.raises(ValueError, match="spatial axis"):
        WindowPlan((12,), (8,))
    with pytest.raises(ValueError, match="fit"):
        WindowPlan((12, 7), (8, 8))                                             # L < h
    for s in (0, 9, (4, 9), -1):
        with pytest.raises(ValueError, match="stride"):
            WindowPlan((12, 12), (8, 8), s)                                     # outside 1 .. h: gaps
    with pytest.raises(ValueError, match="stride"):
        WindowPlan((12, 12), (8, 8), (4, 4, 4))
    with pytest.raises(ValueError, match="MF_WINDOW_MAX_PER_AXIS"):
        WindowPlan((8, 8 + MF_WINDOW_MAX_PER_AXIS), (8, 8), 1)                  # 33 origins
    assert len(WindowPlan((8, 7 + MF_WINDOW_MAX_PER_AXIS), (8, 8), 1).origins[1]) == MF_WINDOW_MAX_PER_AXIS
    with pytest.raises(ValueError, match="window_weight"):
        WindowPlan((12, 12), (8, 8), weight="gauss")


def test_descriptor_carries_the_plan():
    d = WindowPlan((8, 13), (8, 8), 4, "uniform").desc(4, 8)
    assert (d.dims, list(d.canvas), list(d.window), list(d.count)) == (2, [1, 8, 13], [1, 8, 8], [1, 1, 3])
    assert list(d.origin[2])[:3] == [0, 4, 5] and d.origin[0][0] == 0 and (d.weight, d.B, d.C) == (L.WINDOW_UNIFORM, 4, 8)
    d = WindowPlan((6, 12, 12), (4, 8, 8)).desc(1, 4)
    assert (d.dims, list(d.count), list(d.origin[0])[:2], d.weight) == (3, [2, 2, 2], [0, 2], L.WINDOW_TENT)


# ------------------------------------------------------------------------------------------------ 2. the merge the GPU tests check against
@pytest.mark.parametrize("weight", ["uniform", "tent"])
@pytest.mark.parametrize("name", list(WC.GEOMETRIES))
def test_ref_merge_fp32_against_fp64(name, weight):
    """|fp32 - fp64| <= (K + 2) * 2^-24 * max|p| per cell (tests/window_cases.merge_bound); cover-1 cells are the window's bits"""
    g = WC.GEOMETRIES[name]
    plan = WC.RefPlan(g["canvas"], g["window"], g["stride"], weight)
    wins = S.synth_input(f"window.cpu.{name}", (2 * plan.M, 3, *plan.window), 1.7)
    got, want = WC.ref_merge(wins, plan, torch.float32), WC.ref_merge(wins, plan, torch.float64)
    assert got.dtype == torch.float32 and want.dtype == torch.float64 and got.shape == (2, 3, *plan.canvas)
    err, bound = (got.double() - want).abs(), WC.merge_bound(wins, plan)
    worst = float((err / bound).max())
    print(f"[measured] ref_merge fp32 vs fp64, {name} / {weight}: worst {worst:.2f} of the bound")
    assert worst <= 1.0
    single = (plan.cover() == 1).expand_as(got)
    for b in range(2):
        for m in range(plan.M):
            idx = (b, slice(None), *plan.slices(m))
            assert torch.equal(got[idx][single[idx]], wins[b * plan.M + m][single[idx]])
    if name == "tiling2d":
        assert bool(single.all())


def test_ref_gather_and_merge_round_trip_and_partition_of_unity():
    plan = WC.RefPlan((9, 13), (7, 6), (3, 5))
    canvas = S.synth_input("window.cpu.rt", (2, 3, 9, 13))
    wins = WC.ref_gather(canvas, plan)
    assert wins.shape == (2 * plan.M, 3, 7, 6) and torch.equal(wins[plan.M + 1], canvas[1][:, 0:7, 5:11])
    back = WC.ref_merge(wins, plan, torch.float64)          # every covering window holds the same value: the average is that value
    assert float((back - canvas.double()).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ 3. the pipeline's rules (no device)
def _pipe(**flags):
    ukw = R.tiny_unet_kwargs(3, "none")
    return M.DiffusionPipeline(M.GaussianNoiseScheduler, M.UNet, None, R.published_scheduler_kwargs(), to_product_kwargs(ukw), **flags).eval()


def test_the_rules_are_checked_before_anything_touches_the_device():
    pipe = _pipe()
    for bad, match in ((dict(window=(4, 8, 8)), "spatial axis"), (dict(window=(8, 16)), "fit"), (dict(window=(8, 8), window_stride=9), "stride"),
                       (dict(window=(8, 8), window_weight="gauss"), "window_weight"), (dict(window_stride=4), "needs window"),
                       (dict(window=(8, 8), cold_diffusion=True, use_ddim=False), "cold_diffusion")):
        with pytest.raises(ValueError, match=match):
            pipe.sample(2, (8, 12, 12), steps=5, **bad)                   # (a CPU pipeline: reaching the device check would be a RuntimeError)
        with pytest.raises(ValueError, match=match):
            pipe.denoise(torch.zeros(2, 8, 12, 12), steps=5, **bad)
        if "cold_diffusion" not in bad:                                    # (sample_from refuses cold diffusion by itself)
            with pytest.raises(ValueError, match=match):
                pipe.sample_from(torch.zeros(2, 8, 12, 12), 0.5, is_latent=True, steps=5, **bad)
    for flag in ("use_self_conditioning", "estimate_variance"):
        with pytest.raises(ValueError, match=flag):
            _pipe(**{flag: True}).sample(2, (8, 12, 12), steps=5, window=(8, 8))
    z = torch.zeros(2, 8, 12, 12)
    with pytest.raises(ValueError, match="window= is not built for invert"):
        pipe.invert(z, steps=8, is_latent=True, window=(8, 8))
    with pytest.raises(ValueError, match="window= is not built for edit"):
        pipe.edit(z, None, steps=8, is_latent=True, window=(8, 8))
    with pytest.raises(RuntimeError, match="ROCm"):                       # a valid window passes the rules and reaches the device check
        pipe.sample(2, (8, 12, 12), steps=5, window=(8, 8))


# ------------------------------------------------------------------------------------------------ 4. the C ABI
def test_the_entry_points_are_declared_exported_and_bound():
    hdr = (ROOT / "include" / "medfusion_hip.h").read_text()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    for name in ("mf_window_gather_f32", "mf_window_merge_f32"):
        assert name in declared and name in L.exported_symbols() and hasattr(lib, name)
        assert name in (ROOT / "DESIGN.md").read_text() and name in (ROOT / "INTEGRATION.md").read_text()
    assert lib.mf_version() == 250 and int(re.search(r"#define MF_VERSION (\d+)", hdr).group(1)) == 250      # additive within ABI 250
    assert "typedef struct MfWindowDesc" in hdr
    assert int(re.search(r"#define MF_WINDOW_MAX_PER_AXIS (\d+)", hdr).group(1)) == MF_WINDOW_MAX_PER_AXIS == L.WINDOW_MAX_PER_AXIS == WC.MAX_PER_AXIS
    from medfusion_amd import build as B

    assert "window_ops.hip" in B.SOURCES and "-packed-fp32-ops" in B.EXTRA_CFLAGS["window_ops.hip"]


def test_descriptor_layout_matches_what_a_c_compiler_sees(tmp_path):
    assert C.sizeof(L.MfWindowDesc) == 4 * (1 + 3 * 3 + 3 * 32 + 4)
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "medfusion_hip.h"', 'int main(void) {', '  printf("MfWindowDesc %zu\\n", sizeof(MfWindowDesc));']
    for fname, _ in L.MfWindowDesc._fields_:
        lines.append(f'  printf("MfWindowDesc.{fname} %zu\\n", offsetof(MfWindowDesc, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["MfWindowDesc"]) == C.sizeof(L.MfWindowDesc)
    for fname, _ in L.MfWindowDesc._fields_:
        assert int(got[f"MfWindowDesc.{fname}"]) == getattr(L.MfWindowDesc, fname).offset, fname


def test_host_validation_of_the_descriptor():
    """argument checks run on the host before any launch (the pointers are never dereferenced)"""
    lib = L.load()
    p = 1 << 20
    good = lambda: WindowPlan((8, 13), (8, 8), 4).desc(2, 8)
    for fn in (lib.mf_window_gather_f32, lib.mf_window_merge_f32):
        assert fn(p, p + (1 << 16), None, None) != 0
        assert fn(None, p, C.byref(good()), None) != 0 and fn(p, None, C.byref(good()), None) != 0

        def refused(change, word):
            d = good()
            change(d)
            return fn(p, p + (1 << 16), C.byref(d), None) != 0 and word in lib.mf_last_error()

        assert refused(lambda d: setattr(d, "dims", 4), b"dims")
        assert refused(lambda d: setattr(d, "B", 0), b"B=0")
        assert refused(lambda d: setattr(d, "weight", 2), b"weight")
        assert refused(lambda d: d.count.__setitem__(2, 33), b"origins")
        assert refused(lambda d: d.count.__setitem__(2, 0), b"origins")
        assert refused(lambda d: d.window.__setitem__(2, 14), b"window")                  # larger than the canvas
        assert refused(lambda d: d.origin[2].__setitem__(2, 6), b"canvas - window")       # the last window would leave the canvas
        assert refused(lambda d: d.origin[2].__setitem__(0, 1), b"from 0")
        assert refused(lambda d: d.origin[2].__setitem__(1, 0), b"ascend")
        assert refused(lambda d: d.canvas.__setitem__(0, 2), b"2-D")                      # dims = 2 with a leading extent

        def gap(d):   # origins 0, 5 with window 4 on a canvas of 9: cell 4 is uncovered
            d.canvas[2], d.window[2], d.count[2] = 9, 4, 2
            d.origin[2][0], d.origin[2][1] = 0, 5

        assert refused(gap, b"gap")
