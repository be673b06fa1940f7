"""Guidance rescale, dynamic thresholding and guidance schedules without a GPU: the argument rules (ValueError naming the argument before anything
touches the device), the host table of the three schedule forms on the executed grid, the properties of the fp64 restatement the GPU tests compare
against (tests/guide_cases.py), and the C ABI of the new entry points."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import medfusion_amd as M
from medfusion_amd import lib as L
from oracle import restate as R
from tests import guide_cases as GC
from tests.util import to_product_kwargs

ROOT = Path(__file__).resolve().parents[1]


def _pipe(**flags):
    ukw = R.tiny_unet_kwargs(3, "none")
    return M.DiffusionPipeline(M.GaussianNoiseScheduler, M.UNet, None, R.published_scheduler_kwargs(), to_product_kwargs(ukw), **flags).eval()


COND = torch.tensor([1, 0])
PAIR = dict(condition=COND, guidance_scale=4.0)


# ------------------------------------------------------------------------------------------------ 1. the rules
BAD = [
    (dict(guidance_rescale=-0.1, **PAIR), "guidance_rescale"),
    (dict(guidance_rescale=1.5, **PAIR), "guidance_rescale"),
    (dict(guidance_rescale=float("nan"), **PAIR), "guidance_rescale"),
    (dict(guidance_rescale=float("inf"), **PAIR), "guidance_rescale"),
    (dict(guidance_rescale=0.7), "guidance_rescale"),                                           # no condition: no pair
    (dict(guidance_rescale=0.7, condition=COND, guidance_scale=1.0), "guidance_rescale"),       # scalar scale 1 and no schedule: no pair
    (dict(guidance_schedule=[2.0] * 6), "guidance_schedule"),                                   # a schedule without a condition
    (dict(dynamic_threshold=0.0), "dynamic_threshold"),
    (dict(dynamic_threshold=1.01), "dynamic_threshold"),
    (dict(dynamic_threshold=float("nan")), "dynamic_threshold"),
    (dict(dynamic_threshold=0.9, threshold_max=1.0), "threshold_max"),
    (dict(dynamic_threshold=0.9, threshold_max=0.5), "threshold_max"),
    (dict(threshold_max=2.0), "threshold_max"),                                                 # a cap without a threshold
    (dict(guidance_schedule=[2.0] * 5, **PAIR), "guidance_schedule"),                           # 6 iterations execute
    (dict(guidance_schedule=[2.0] * 5 + [float("inf")], **PAIR), "guidance_schedule"),
    (dict(guidance_schedule=lambda t: float("nan"), **PAIR), "guidance_schedule"),
    (dict(guidance_schedule=("interval", 600, 200), **PAIR), "guidance_schedule"),
    (dict(guidance_schedule=3.0, **PAIR), "guidance_schedule"),
    (dict(guidance_rescale=0.5, cold_diffusion=True, **PAIR), "cold_diffusion"),
    (dict(dynamic_threshold=0.9, cold_diffusion=True), "cold_diffusion"),
    (dict(guidance_schedule=[2.0] * 6, cold_diffusion=True, **PAIR), "cold_diffusion"),
]


@pytest.mark.parametrize("bad,match", BAD, ids=[f"{i}-{m}" for i, (_, m) in enumerate(BAD)])
def test_the_rules_are_checked_before_anything_touches_the_device(bad, match):
    pipe = _pipe()      # (a CPU pipeline: reaching the device check would be a RuntimeError, a draw would advance torch's generator)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match=match):
        pipe.sample(2, (8, 8, 8), steps=6, **bad)
    with pytest.raises(ValueError, match=match):
        pipe.denoise(torch.zeros(2, 8, 8, 8), steps=6, **bad)
    if "cold_diffusion" not in bad:      # (sample_from, invert and edit refuse cold diffusion by themselves)
        with pytest.raises(ValueError, match=match):
            pipe.sample_from(torch.zeros(2, 8, 8, 8), 1.0, is_latent=True, steps=6, **bad)
        up = dict(bad)
        if isinstance(up.get("guidance_schedule"), list):
            up["guidance_schedule"] = up["guidance_schedule"][1:]       # an inversion over 6 grid points runs 5 upward iterations
        with pytest.raises(ValueError, match=match):
            pipe.invert(torch.zeros(2, 8, 8, 8), is_latent=True, steps=6, **up)
        down = dict(bad)
        cond = down.pop("condition", None)
        with pytest.raises(ValueError, match=match):
            pipe.edit(torch.zeros(2, 8, 8, 8), cond, is_latent=True, steps=6, **down)
    assert torch.equal(state, torch.get_rng_state())


def test_the_twins_of_edit_name_themselves_and_the_other_rules():
    pipe = _pipe()
    z = torch.zeros(2, 8, 8, 8)
    with pytest.raises(ValueError, match="source_guidance_rescale"):
        pipe.edit(z, COND, is_latent=True, steps=6, source_guidance_rescale=0.5)                          # no source pair
    with pytest.raises(ValueError, match="source_guidance_schedule"):
        pipe.edit(z, COND, is_latent=True, steps=6, source_condition=COND, source_guidance_schedule=[2.0] * 6)   # 5 upward iterations
    with pytest.raises(RuntimeError, match="ROCm"):                                                        # valid: reaches the device check
        pipe.edit(z, COND, is_latent=True, steps=6, source_condition=COND, source_guidance_schedule=[2.0] * 5, guidance_schedule=[3.0] * 6,
                  guidance_scale=3.0, guidance_rescale=0.5, dynamic_threshold=0.99)
    for kw in (dict(guidance_rescale=0.5, **PAIR), dict(dynamic_threshold=0.9), dict(guidance_schedule=[2.0] * 6, **PAIR)):
        with pytest.raises(ValueError, match="estimate_variance"):
            _pipe(estimate_variance=True).sample(2, (8, 8, 8), steps=6, **kw)
    with pytest.raises(TypeError, match="eta"):
        pipe.sample_from(z, 1.0, is_latent=True, steps=6, eta=0.0, dynamic_threshold=0.9)
    with pytest.raises(TypeError):                                                                         # forward() is unchanged
        pipe.forward(z, torch.zeros(2, dtype=torch.long), dynamic_threshold=0.9)
    with pytest.raises(RuntimeError, match="ROCm"):                                                        # valid arguments pass the rules
        pipe.sample(2, (8, 8, 8), steps=6, guidance_rescale=0.7, dynamic_threshold=0.995, threshold_max=4.0, guidance_schedule=[8.0] * 6, condition=COND)
    with pytest.raises(RuntimeError, match="ROCm"):                                                        # the defaults, spelled out, are the plain call
        pipe.sample(2, (8, 8, 8), steps=6, guidance_rescale=0.0, dynamic_threshold=None, threshold_max=None, guidance_schedule=None)


# ------------------------------------------------------------------------------------------------ 2. the host table
def test_the_three_schedule_forms_on_the_executed_grids():
    pipe = _pipe()
    sch = pipe.noise_scheduler
    scales = M.DiffusionPipeline._guide_scales
    for spacing, steps in ((None, 7), ("logsnr", 40)):
        ts, executed = sch.loop_timesteps(steps, True, spacing)
        rev = list(reversed(ts))
        assert len(rev) == executed and (spacing is None or executed < steps)     # the log-SNR grid dropped duplicates
        seq = [1.0 + 0.5 * i for i in range(executed)]
        assert scales(seq, rev, 8.0) == seq
        with pytest.raises(ValueError, match=f"{steps} entries for {executed}" if executed != steps else "entries"):
            scales([1.0] * (steps if executed != steps else steps + 1), rev, 8.0)
        assert scales(lambda t: 1.0 + t / 1000.0, rev, 8.0) == [1.0 + t / 1000.0 for t in rev]
        lo, hi = rev[-2], rev[1]
        got = scales(("interval", lo, hi), rev, 8.0)
        assert got == [8.0 if lo <= t <= hi else 1.0 for t in rev] and got[0] == 1.0 and got[-1] == 1.0 and got[1] == 8.0 and got[-2] == 8.0
        assert scales(None, rev, 8.0) == [8.0] * executed
    # strength < 1: the schedule covers the iterations that run
    ts, _ = sch.loop_timesteps(8, True)
    s, k = M.DiffusionPipeline._strength_span(8, 0.5)
    assert (s, k) == (4, 4)
    spec, g = pipe._guide_spec(dict(guidance_schedule=[5.0, 4.0, 3.0, 2.0], guidance_scale=8.0), COND, list(reversed(ts))[s:])
    assert g == [5.0, 4.0, 3.0, 2.0] and spec[0] == 0.0 and spec[1] is None
    with pytest.raises(ValueError, match="8 entries for 4"):
        pipe.sample_from(torch.zeros(2, 8, 8, 8), 0.5, is_latent=True, steps=8, condition=COND, guidance_schedule=[2.0] * 8)
    assert pipe._guide_spec(dict(guidance_scale=8.0), COND, [5, 3]) == (None, None)
    spec, g = pipe._guide_spec(dict(dynamic_threshold=0.995, threshold_max=float("inf"), guidance_scale=8.0), COND, [5, 3])
    assert spec == (0.0, 0.995, None, None) and g == [8.0, 8.0]


# ------------------------------------------------------------------------------------------------ 3. the restatement's own properties
@pytest.mark.parametrize("n", [4, 36, 1000])
def test_the_restatement_has_the_papers_properties(n):
    pc, pu, xt = GC.contents("normal", n, 5)
    a, b = GC.SCHED["a"], GC.SCHED["b"]
    r = GC.restate(pc, pu, xt, 8.0, 1.0, None, None, a, b, 0)
    assert abs(float(torch.std(r["k"] * r["p32"].double())) / float(torch.std(pc.double())) - 1.0) < 1e-13   # phi = 1: the conditional prediction's spread
    assert abs(float(torch.std(r["out"])) / float(torch.std(pc.double())) - 1.0) < 1e-6          # (and of the unrounded combine, to fp32 rounding)
    r0 = GC.restate(pc, pu, xt, 8.0, 0.0, None, None, a, b, 0)
    assert r0["k"] == 1.0 and torch.equal(r0["out"], r0["p"])                                  # phi = 0
    mid = GC.restate(pc, pu, xt, 8.0, 0.7, None, None, a, b, 0)["k"]
    assert min(1.0, r["k"]) < mid < max(1.0, r["k"])
    for objective in (0, 1):
        top = GC.restate(pc, pu, xt, 8.0, 0.0, 1.0, None, a, b, objective)
        assert top["s"] == max(1.0, float(top["x0"].abs().max()))                              # q = 1: the row's maximum
        assert float(top["x0n"].abs().max()) <= 1.0
        small = GC.restate(pc * 1e-3, pu * 1e-3, xt * 1e-3, 1.5, 0.0, 0.5, None, a, b, objective)
        assert small["s"] == 1.0 and torch.equal(small["x0n"], small["x0"])                    # s >= 1: a row inside [-1, 1] is left alone
        cap = GC.restate(pc, pu, xt, 8.0, 0.0, 1.0, 1.5, a, b, objective)
        assert cap["s"] == 1.5
        # the prediction handed on gives the thresholded estimate back
        back = a * xt.double() - b * top["out"] if objective == 0 else top["out"]
        assert float((back - top["x0n"]).abs().max()) < 1e-12
    flat = torch.full((n,), 0.75)
    assert GC.restate(flat, flat.clone(), xt, 4.0, 0.7, None, None, a, b, 0)["k"] == 1.0       # sigma_cfg = 0


def test_the_fp32_chain_and_the_bounds_agree_with_the_restatement():
    """chain32 (fp32 operators, exact order statistics) lands inside element_bound of the fp64 restatement on every case family: the bound is
    derived from the formats, this checks the derivation on the CPU before a kernel is held to it"""
    worst = 0.0
    for case in GC.all_cases():
        if case["n"] > 64:
            continue
        for pc, pu, xt in GC.case_rows(case):
            phi, q = case["phi"], case["q"]
            if pu is None:
                phi = 0.0
            r = GC.restate(pc, pu, xt, case["g"], phi, q, case["s_max"], case["a"], case["b"], case["objective"])
            k32 = GC.f32(r["k"]) if phi else None
            out, s, _ = GC.chain32(pc, pu, xt, case["g"], k32, q, case["s_max"], case["a"], case["b"], case["objective"])
            bound = GC.element_bound(r, pc, pu, xt, case["g"], case["a"], case["b"], case["objective"], bool(phi), q is not None)
            ratio = float(((out.double() - r["out"]).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (case["name"], ratio)
            if q is not None:
                assert float(s) >= 1.0
    assert worst > 0.0


def test_every_mandated_shape_and_content_is_among_the_cases():
    cases = GC.all_cases()
    ns = {(c["n"], c["B"]) for c in cases}
    assert {(4, 1), (4, 3), (36, 2), (GC.ONE_WG, 2), (GC.ONE_WG + 4, 2), (2 * GC.ONE_WG + 12, 2)} <= ns
    assert {c["kind"] for c in cases} == {"normal", "ties3", "all_equal", "low_byte", "zeros_denormals", "offset"}
    assert {0.5, GC.f32(0.995), 1.0} <= {c["q"] for c in cases}
    assert any(c["q"] is not None and c["q"] < 1.0 and (c["q"] * (c["n"] - 1)).is_integer() for c in cases)
    assert all(c["offset"] == 1 for c in cases if c["n"] == 36)
    pc, _, _ = GC.contents("ties3", 36, 1, 0.5)
    v = torch.sort(pc.abs()).values
    assert len(set(v.tolist())) == 3 and float(v[17]) != float(v[18])           # the quantile position lies between two of the three values
    pc, _, _ = GC.contents("low_byte", 64, 1)
    assert len({b >> 8 for b in pc.abs().view(torch.int32).tolist()}) == 1


# ------------------------------------------------------------------------------------------------ 4. the C ABI
def test_header_exports_and_layout():
    hdr = (ROOT / "include" / "medfusion_hip.h").read_text()
    lib = L.load()
    assert lib.mf_version() == 250 and "#define MF_VERSION 250" in hdr
    for name in ("mf_guide_f32", "mf_guide_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", hdr) and hasattr(lib, name) and name in L.exported_symbols()
    one = int(re.search(r"#define MF_GUIDE_ROW_ONE_WG (\d+)", hdr).group(1))
    assert one == L.GUIDE_ROW_ONE_WG == GC.ONE_WG
    assert (L.GUIDE_RESCALE, L.GUIDE_THRESHOLD) == tuple(int(re.search(rf"#define MF_GUIDE_{k} (\d+)", hdr).group(1)) for k in ("RESCALE", "THRESHOLD"))
    assert C.sizeof(L.MfGuideStep) == 32 and C.sizeof(L.MfGuideArgs) == 9 * 8 + 8 + 8 + 6 * 4
    for cls, name in ((L.MfGuideStep, "MfGuideStep"), (L.MfGuideArgs, "MfGuideArgs")):
        body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in cls._fields_], name        # (one field per declaration in these two structs)
    import shutil
    import subprocess
    import tempfile
    gcc = shutil.which("gcc")
    if gcc is not None:      # the offsets a C compiler sees (tests/test_boundary_cpu.py's method)
        lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "medfusion_hip.h"', 'int main(void) {']
        for cls, name in ((L.MfGuideStep, "MfGuideStep"), (L.MfGuideArgs, "MfGuideArgs")):
            lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
            lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
        lines += ['  return 0;', '}']
        with tempfile.TemporaryDirectory() as tmp:
            (Path(tmp) / "layout.c").write_text("\n".join(lines))
            subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(Path(tmp) / "layout.c"), "-o", str(Path(tmp) / "layout")], check=True)
            got = dict(ln.split() for ln in subprocess.run([str(Path(tmp) / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
        for cls, name in ((L.MfGuideStep, "MfGuideStep"), (L.MfGuideArgs, "MfGuideArgs")):
            assert int(got[name]) == C.sizeof(cls), name
            for f, _ in cls._fields_:
                assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, f"{name}.{f}"
    # workspace sizing and argument validation are host code
    assert lib.mf_guide_workspace_bytes(16, one) == 0 and lib.mf_guide_workspace_bytes(0, 10 * one) == 0
    w1, w2 = lib.mf_guide_workspace_bytes(1, one + 4), lib.mf_guide_workspace_bytes(3, one + 4)
    assert w1 > 0 and w2 == 3 * w1 and w1 % 8 == 0
    assert lib.mf_guide_workspace_bytes(1, 1 << 30) < (1 << 20)                      # at most 64 workgroups per row
    assert lib.mf_guide_f32(None, None) == -1 and b"guide" in lib.mf_last_error()
    a = L.MfGuideArgs(None, 16, None, 16, None, None, 16, None, None, 0, 8, 0, 0, 1, L.GUIDE_RESCALE, 0, 0)
    assert lib.mf_guide_f32(C.byref(a), None) == -1 and b"pred_uncond" in lib.mf_last_error()   # a rescale without a pair
    a = L.MfGuideArgs(None, 16, None, 16, None, None, 16, None, None, 0, 8, 0, 0, 1, L.GUIDE_THRESHOLD, 0, 0)
    assert lib.mf_guide_f32(C.byref(a), None) == -1 and b"x_t" in lib.mf_last_error()           # objective 'x_T' reads x_t
    a = L.MfGuideArgs(None, 16, 32, 16, None, None, 16, None, None, 0, one + 4, 0, 1, 1, L.GUIDE_RESCALE, 0, 0)
    assert lib.mf_guide_f32(C.byref(a), None) != 0 and b"workspace" in lib.mf_last_error()      # a long row needs its workspace


def test_build_flags_of_the_new_unit():
    from medfusion_amd import build as B
    assert "guide.hip" in B.SOURCES and "-ffp-contract=off" in B.CFLAGS
    assert B.EXTRA_CFLAGS["guide.hip"] == B.EXTRA_CFLAGS["loss.hip"] and "-packed-fp32-ops" in B.EXTRA_CFLAGS["guide.hip"]
