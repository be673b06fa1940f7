"""The deterministic few-step samplers (sampler="ddim0" / "dpmpp2m", spacing="logsnr") without a GPU: the coefficient rows against an independent
fp64 evaluation, the log-SNR grid, solver accuracy on a problem with a closed-form solution, the argument rules, and the C-ABI additions."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import medfusion_amd as M
from medfusion_amd import lib as L
from oracle import restate as R
from tests import solver_cases as SC
from tests.util import to_product_kwargs

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("mf_solver_step_f32", "mf_solver_step_blend_f32")


def published():
    return M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())


def table64(sch):
    return sch.host_tables()["alphas_cumprod"].numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. the rows
@pytest.mark.parametrize("steps,spacing,start", [(8, None, 0), (25, "uniform", 0), (20, "logsnr", 0), (20, "logsnr", 7), (12, None, 9), (1, None, 0), (2, "logsnr", 0)])
def test_dpmpp2m_rows_against_fp64(steps, spacing, start):
    """every coefficient within one fp32 rounding (relative 2^-23 allows for the last bits of two fp64 evaluations) of
    A = sigma_n / sigma_t, B = -alpha_n expm1(-h) (1 + 1/(2r)), C = alpha_n expm1(-h) / (2r), r = h_prev / h; first executed row first-order"""
    sch = published()
    ts, n = sch.loop_timesteps(steps, True, spacing)
    rows = sch.solver_records(ts, "dpmpp2m", start=start)
    ac = table64(sch)
    rev = list(reversed(ts))
    assert len(rows) == n - start
    h_prev = None
    for j, r in enumerate(rows):
        i = start + j
        t = rev[i]
        assert r.t == t and r.reserved == 0
        assert r.sqrt_recip_ac == float(sch.host_tables()["sqrt_recip_alphas_cumprod"][t])
        assert r.sqrt_recipm1_ac == float(sch.host_tables()["sqrt_recipm1_alphas_cumprod"][t])
        if i == n - 1:
            assert (r.mode, r.A, r.B, r.C) == (L.SOLVER_FINAL, 0.0, 0.0, 0.0)
            continue
        tn = rev[i + 1]
        lam = lambda u: np.log(np.sqrt(ac[u]) / np.sqrt(1.0 - ac[u]))
        h = lam(tn) - lam(t)
        e = -np.sqrt(ac[tn]) * np.expm1(-h)
        want_a = np.sqrt(1.0 - ac[tn]) / np.sqrt(1.0 - ac[t])
        if h_prev is None:
            want_b, want_c, mode = e, 0.0, L.SOLVER_ORDER1
        else:
            rr = h_prev / h
            want_b, want_c, mode = e * (1.0 + 1.0 / (2.0 * rr)), -e / (2.0 * rr), L.SOLVER_ORDER2
        h_prev = h
        assert r.mode == mode
        for got, want in ((r.A, want_a), (r.B, want_b), (r.C, want_c)):
            assert abs(got - want) <= 2.0 ** -23 * abs(want), (i, got, want)
    assert rows[0].mode in (L.SOLVER_ORDER1, L.SOLVER_FINAL) and rows[0].C == 0.0


@pytest.mark.parametrize("steps,start", [(150, 0), (6, 0), (10, 4), (1, 0)])
def test_ddim0_rows_are_the_references_scalars_at_sigma_zero(steps, start):
    sch = published()
    ts, n = sch.loop_timesteps(steps, True)
    rows = sch.solver_records(ts, "ddim0", start=start)
    recs = sch.step_records(ts, True, eta=0)[start:]
    assert len(rows) == len(recs) == n - start
    for r, s in zip(rows, recs):
        assert (r.t, r.sqrt_recip_ac, r.sqrt_recipm1_ac) == (s.t, s.sqrt_recip_ac, s.sqrt_recipm1_ac)
        if s.mode == 1:
            assert r.mode == L.SOLVER_DDIM0 and s.ddim_sigma == 0.0
            assert np.float32(r.B).tobytes() == np.float32(s.ddim_sqrt_an).tobytes() and np.float32(r.A).tobytes() == np.float32(s.ddim_c).tobytes()
            assert r.C == 0.0
        else:
            assert r.mode == L.SOLVER_FINAL
    assert rows[-1].mode == L.SOLVER_FINAL and rows[-1].t == 0


def test_rows_refusals():
    sch = published()
    ts, _ = sch.loop_timesteps(8, True)
    with pytest.raises(ValueError):
        sch.solver_records(ts, "euler")
    with pytest.raises(ValueError):
        sch.solver_records(ts, "dpmpp2m", start=8)
    with pytest.raises(ValueError):      # a repeated timestep (steps > T on the uniform grid) has h = 0
        sch.solver_records(sch.loop_timesteps(1500, True)[0], "dpmpp2m")
    with pytest.raises(ValueError):
        sch.loop_timesteps(8, True, "karras")
    with pytest.raises(ValueError):
        sch.loop_timesteps(8, False, "logsnr")


# ------------------------------------------------------------------------------------------------ 2. the grid
def _h(ac, ts):
    lam = 0.5 * np.log(ac / (1.0 - ac))
    return np.abs(np.diff(lam[np.asarray(ts)]))


@pytest.mark.parametrize("steps", [2, 5, 15, 20, 30, 150, 1000, 1200])
def test_logsnr_grid_shape(steps):
    sch = published()
    ts, n = sch.loop_timesteps(steps, True, "logsnr")
    assert n == len(ts) <= steps and ts[0] == 0 and ts[-1] == sch.T - 1
    assert all(b > a for a, b in zip(ts, ts[1:])) and all(isinstance(t, int) for t in ts)


def test_logsnr_grid_evens_out_the_steps_the_uniform_grid_does_not():
    sch = published()
    ac = table64(sch)
    ts, n = sch.loop_timesteps(20, True, "logsnr")
    h = _h(ac, ts)
    assert h.max() <= 1.5 * h.mean(), (h.max(), h.mean())
    tu, nu = sch.loop_timesteps(20, True, "uniform")
    assert (tu, nu) == sch.loop_timesteps(20, True) == sch.loop_timesteps(20, True, None)       # "uniform" IS the reference's grid
    hu = _h(ac, tu)
    assert hu.max() >= 3.0 * hu.mean(), (hu.max(), hu.mean())
    assert sch.loop_timesteps(1, True, "logsnr") == ([0], 1) == sch.loop_timesteps(1, True)


# ------------------------------------------------------------------------------------------------ 3. solver accuracy on the closed form
X_T = torch.tensor([1.0, -0.7, 2.0], dtype=torch.float64)


def _error(sch, steps, sampler, spacing, s2):
    ac = table64(sch)
    ts, _ = sch.loop_timesteps(steps, True, spacing)
    got = SC.drive_rows(sch.solver_records(ts, sampler), ac, s2, X_T)
    want = SC.gaussian_exact(ac, s2, X_T)
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("s2", [0.25, 0.04])
def test_2m_on_the_logsnr_grid_at_20_beats_ddim0_at_150_on_the_published_schedule(s2):
    sch = published()
    few, many = _error(sch, 20, "dpmpp2m", "logsnr", s2), _error(sch, 150, "ddim0", None, s2)
    print(f"[measured] closed form, published schedule, s2={s2}: dpmpp2m+logsnr@20 {few:.2e}  ddim0+uniform@150 {many:.2e}")
    assert few < many


@pytest.mark.parametrize("s2", [0.25, 0.04])
def test_convergence_orders_on_the_cosine_schedule(s2):
    """uniform grid, 40 -> 80 -> 160 iterations: the second-order solver's error falls by >= 3x per doubling (theory 4x), DDIM's by 1.8 .. 2.2x"""
    sch = M.GaussianNoiseScheduler(timesteps=1000)
    assert sch.schedule_strategy == "cosine"
    e2 = [_error(sch, n, "dpmpp2m", None, s2) for n in (40, 80, 160)]
    e1 = [_error(sch, n, "ddim0", None, s2) for n in (40, 80, 160)]
    print(f"[measured] closed form, cosine schedule, s2={s2}: dpmpp2m {' '.join(f'{e:.2e}' for e in e2)}  ddim0 {' '.join(f'{e:.2e}' for e in e1)}")
    assert e2[0] / e2[1] >= 3.0 and e2[1] / e2[2] >= 3.0
    assert 1.8 <= e1[0] / e1[1] <= 2.2 and 1.8 <= e1[1] / e1[2] <= 2.2


# ------------------------------------------------------------------------------------------------ 4. argument rules
def _cpu_pipe(**kw):
    return M.DiffusionPipeline(M.GaussianNoiseScheduler, M.UNet, None, R.published_scheduler_kwargs(), to_product_kwargs(R.tiny_unet_kwargs(None, "none")), **kw)


def test_argument_rules():
    pipe = _cpu_pipe()
    z = torch.zeros((2, 8, 8, 8))
    calls = {
        "sample": lambda **kw: pipe.sample(2, (8, 8, 8), steps=8, **kw),
        "denoise": lambda **kw: pipe.denoise(z, steps=8, **kw),
        "sample_from": lambda **kw: pipe.sample_from(z, 0.5, is_latent=True, steps=8, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="sampler"):       # unknown names
            call(sampler="euler")
        with pytest.raises(ValueError, match="spacing"):
            call(sampler="ddim0", spacing="karras")
        with pytest.raises(ValueError, match="needs a sampler"):      # a grid other than the reference's belongs to a sampler
            call(spacing="logsnr")
        with pytest.raises(ValueError, match="use_ddim"):
            call(sampler="dpmpp2m", use_ddim=False)
        with pytest.raises(ValueError):
            call(sampler="ddim0", cold_diffusion=True)
        for ok in (dict(sampler="ddim0"), dict(sampler="dpmpp2m", spacing="logsnr"), dict(sampler="dpmpp2m", spacing="uniform"), dict(spacing="uniform"), {}):
            with pytest.raises(RuntimeError, match="no CPU"):      # past the rules: the device check
                call(**ok)
    with pytest.raises(TypeError):       # `eta` stays what it was, with or without a sampler
        pipe.sample_from(z, 0.5, is_latent=True, steps=8, sampler="ddim0", eta=0.0)
    with pytest.raises(TypeError):
        pipe.sample_from(z, 0.5, is_latent=True, steps=8, sampler="ddim0", no_such_keyword=1)


def test_strength_applies_to_the_executed_grid():
    """sample_from's "last k iterations" on a log-SNR grid that dropped duplicates: k of len(grid), not of `steps`"""
    sch = published()
    ts, n = sch.loop_timesteps(1200, True, "logsnr")
    assert n < 1200
    s, k = M.DiffusionPipeline._strength_span(n, 0.5)
    assert (s, k) == (n - int(0.5 * n + 0.5), int(0.5 * n + 0.5))
    rows = sch.solver_records(ts, "dpmpp2m", start=s)
    assert len(rows) == k and rows[0].mode == L.SOLVER_ORDER1 and rows[1].mode == L.SOLVER_ORDER2 and rows[-1].mode == L.SOLVER_FINAL
    assert sch.blend_records(ts, s).shape == (k, 2)


# ------------------------------------------------------------------------------------------------ 5. the C ABI
def test_new_entry_points_are_declared_exported_and_bound():
    hdr = (ROOT / "include" / "medfusion_hip.h").read_text()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.exported_symbols() and hasattr(lib, name), name
    assert lib.mf_version() == 250      # additive within ABI 250
    assert C.sizeof(L.MfSchedStep) == 12 * 4 and C.sizeof(L.MfSchedArgs) == 8 * 6 + 8 + 8 * 5 + 4 * 4 + 8      # (unchanged)
    md = (ROOT / "INTEGRATION.md").read_text()
    for name in NEW_SYMBOLS:
        assert name in md, f"INTEGRATION.md does not list {name}"
    m = re.search(r"enum \{ MF_SOLVER_FINAL = (\d), MF_SOLVER_DDIM0 = (\d), MF_SOLVER_ORDER1 = (\d), MF_SOLVER_ORDER2 = (\d) \}", hdr)
    assert tuple(int(v) for v in m.groups()) == (L.SOLVER_FINAL, L.SOLVER_DDIM0, L.SOLVER_ORDER1, L.SOLVER_ORDER2)


def test_solver_struct_layouts_match_what_a_c_compiler_sees(tmp_path):
    assert C.sizeof(L.MfSolverStep) == 8 * 4                       # 5 f32, 3 i32
    assert C.sizeof(L.MfSolverArgs) == 8 * 11 + 4 * 4 + 8          # 11 ptr, 3 i32 + f32, i64
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    structs = {"MfSolverStep": L.MfSolverStep, "MfSolverArgs": L.MfSolverArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "medfusion_hip.h"', 'int main(void) {']
    for name, cls in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for name, cls in structs.items():
        assert int(got[name]) == C.sizeof(cls), name
        for fname, _ in cls._fields_:
            assert int(got[f"{name}.{fname}"]) == getattr(cls, fname).offset, f"{name}.{fname}"


def test_host_validation_of_the_solver_step():
    """argument checks run on the host before any launch"""
    lib = L.load()
    p, n = 1 << 20, 2 * 8 * 64
    ok = dict(x_t=p, pred=p + 4 * n, x_t_out=p, table=p + 64 * n, n=n)

    def args(**kw):
        return L.MfSolverArgs(**{**ok, **kw})
    assert lib.mf_solver_step_f32(None, None) != 0
    assert lib.mf_solver_step_f32(C.byref(args(n=0)), None) != 0
    assert lib.mf_solver_step_f32(C.byref(args(table=None)), None) != 0
    assert lib.mf_solver_step_f32(C.byref(args(objective=2)), None) != 0 and b"objective" in lib.mf_last_error()
    assert lib.mf_solver_step_f32(C.byref(args(step_counter=p + 128 * n)), None) != 0 and b"ticket" in lib.mf_last_error()     # a counter without its ticket
    assert lib.mf_solver_step_f32(C.byref(args(step=-1)), None) != 0
    assert lib.mf_solver_step_f32(C.byref(args(x0_hist=p + 4 * n - 16)), None) != 0 and b"overlaps" in lib.mf_last_error()     # the history inside pred
    assert lib.mf_solver_step_blend_f32(C.byref(args()), None, None) != 0 and b"blend" in lib.mf_last_error()
    bl = L.MfSchedBlend(p, p, p, p, 60, 8, 0)          # 2 * 8 * 64 values are not whole samples of 8 x 60
    assert lib.mf_solver_step_blend_f32(C.byref(args()), C.byref(bl), None) != 0
