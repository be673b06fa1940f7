"""DDIM inversion and counterfactual editing without a GPU: the upward rows (GaussianNoiseScheduler.inversion_records), their accuracy on the
problem with a closed-form solution, the argument rules of invert() / edit(), and the C-ABI additions."""
import ctypes as C
import math
import re
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
NEW_SYMBOLS = ("mf_solver_step_traj_f32", "mf_absdiff_mean_c_f32")
X_0 = torch.tensor([0.7, -1.3, 0.05, 2.1], dtype=torch.float64)


def published():
    return M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())


def table64(sch):
    return sch.host_tables()["alphas_cumprod"].numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. the rows
@pytest.mark.parametrize("steps,spacing,stop", [(8, None, None), (8, None, 4), (25, "logsnr", None), (25, "logsnr", 2), (12, "uniform", 12)])
@pytest.mark.parametrize("sampler", ["ddim0", "dpmpp2m"])
def test_inversion_rows(sampler, steps, spacing, stop):
    sch = published()
    tb = sch.host_tables()
    ts, n = sch.loop_timesteps(steps, True, spacing)
    k = stop or n
    rows = sch.inversion_records(ts, sampler, stop=stop)
    assert len(rows) == k - 1
    assert [r.t for r in rows] == ts[:k - 1] and all(b.t > a.t for a, b in zip(rows, rows[1:]))      # ascending: evaluated at ts[j]
    assert all(r.mode != L.SOLVER_FINAL and r.reserved == 0 for r in rows)
    ac = table64(sch)
    lam = lambda u: np.log(np.sqrt(ac[u]) / np.sqrt(1.0 - ac[u]))
    h_prev = None
    for j, r in enumerate(rows):
        t, tn = ts[j], ts[j + 1]
        assert r.sqrt_recip_ac == float(tb["sqrt_recip_alphas_cumprod"][t]) and r.sqrt_recipm1_ac == float(tb["sqrt_recipm1_alphas_cumprod"][t])
        if sampler == "ddim0":
            assert r.mode == L.SOLVER_DDIM0 and r.C == 0.0
            # byte-equal to the fp32 table entries at tn: the row is the reference's estimate_x_t(x_0_est, tn, x_T=x_T_est)
            assert np.float32(r.B).tobytes() == tb["sqrt_alphas_cumprod"][tn].numpy().tobytes()
            assert np.float32(r.A).tobytes() == tb["sqrt_one_minus_alphas_cumprod"][tn].numpy().tobytes()
            continue
        h = lam(tn) - lam(t)
        assert h < 0
        e = -np.sqrt(ac[tn]) * np.expm1(-h)
        if h_prev is None:
            want, mode = (np.sqrt(1.0 - ac[tn]) / np.sqrt(1.0 - ac[t]), e, 0.0), L.SOLVER_ORDER1
        else:
            c = 1.0 / (2.0 * (h_prev / h))
            want, mode = (np.sqrt(1.0 - ac[tn]) / np.sqrt(1.0 - ac[t]), e * (1.0 + c), -e * c), L.SOLVER_ORDER2
        assert r.mode == mode
        for got, w in zip((r.A, r.B, r.C), want):     # one fp32 rounding of an fp64 evaluation
            assert abs(got - w) <= 2.0 ** -23 * abs(w), (j, got, w)
        h_prev = h


def test_inversion_rows_refusals():
    sch = published()
    ts, _ = sch.loop_timesteps(8, True)
    with pytest.raises(ValueError, match="sampler"):
        sch.inversion_records(ts, "euler")
    with pytest.raises(ValueError):
        sch.inversion_records(ts, "ddim0", stop=1)          # k < 2
    with pytest.raises(ValueError):
        sch.inversion_records(ts[:1], "dpmpp2m")
    with pytest.raises(ValueError):
        sch.inversion_records(ts, "ddim0", stop=9)          # more than the grid has
    for sampler in ("ddim0", "dpmpp2m"):
        with pytest.raises(ValueError, match="increasing"):
            sch.inversion_records(list(reversed(ts)), sampler)
        with pytest.raises(ValueError, match="increasing"):
            sch.inversion_records([0, 5, 5, 9], sampler)


# ------------------------------------------------------------------------------------------------ 2. the closed form
def exact_up(ac, ts, s2):
    """x_0 ~ N(0, s2) data: the probability-flow ODE's solution carried from ts[0] to ts[-1]"""
    a0, aT = float(ac[ts[0]]), float(ac[ts[-1]])
    return X_0 * math.sqrt((aT * s2 + 1.0 - aT) / (a0 * s2 + 1.0 - a0))


def _up_error(sch, steps, sampler, spacing, s2):
    ac = table64(sch)
    ts, _ = sch.loop_timesteps(steps, True, spacing)
    got = SC.drive_rows(sch.inversion_records(ts, sampler), ac, s2, X_0)
    want = exact_up(ac, ts, s2)
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("s2", [0.25, 0.04])
def test_inversion_orders_on_the_cosine_schedule(s2):
    """uniform grid, 40 -> 80 -> 160 asked steps: DDIM inversion's error falls by 1.8 .. 2.2x per doubling (first order); the 2M rows' by >= 2.5x
    (between first and second order: their first row is first-order)"""
    sch = M.GaussianNoiseScheduler(timesteps=1000)
    assert sch.schedule_strategy == "cosine"
    e1 = [_up_error(sch, n, "ddim0", None, s2) for n in (40, 80, 160)]
    e2 = [_up_error(sch, n, "dpmpp2m", None, s2) for n in (40, 80, 160)]
    print(f"[measured] closed form upward, cosine schedule, s2={s2}: ddim0 {' '.join(f'{e:.2e}' for e in e1)} (ratios {e1[0] / e1[1]:.2f} {e1[1] / e1[2]:.2f})  "
          f"dpmpp2m {' '.join(f'{e:.2e}' for e in e2)} (ratios {e2[0] / e2[1]:.2f} {e2[1] / e2[2]:.2f})")
    assert 1.8 <= e1[0] / e1[1] <= 2.2 and 1.8 <= e1[1] / e1[2] <= 2.2
    assert e2[0] / e2[1] >= 2.5 and e2[1] / e2[2] >= 2.5


def _round_trip_error(sch, steps, sampler, spacing, s2):
    """invert, then solver_records back down: the distance to the input's denoised value (what the exact flow's round trip returns)"""
    ac = table64(sch)
    ts, _ = sch.loop_timesteps(steps, True, spacing)
    top = SC.drive_rows(sch.inversion_records(ts, sampler), ac, s2, X_0)
    back = SC.drive_rows(sch.solver_records(ts, sampler), ac, s2, top)
    want = SC.gaussian_denoiser(float(ac[ts[0]]), s2) * X_0
    return float((back - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("s2", [0.25, 0.04])
def test_round_trip_2m_on_the_logsnr_grid_at_40_beats_ddim0_at_160(s2):
    sch = published()
    few, many = _round_trip_error(sch, 40, "dpmpp2m", "logsnr", s2), _round_trip_error(sch, 160, "ddim0", None, s2)
    print(f"[measured] closed form round trip, published schedule, s2={s2}: dpmpp2m+logsnr@40 {few:.2e}  ddim0+uniform@160 {many:.2e}")
    assert few < many


# ------------------------------------------------------------------------------------------------ 3. argument rules
def _cpu_pipe(**kw):
    return M.DiffusionPipeline(M.GaussianNoiseScheduler, M.UNet, None, R.published_scheduler_kwargs(), to_product_kwargs(R.tiny_unet_kwargs(None, "none")), **kw)


def test_argument_rules():
    pipe = _cpu_pipe()
    z = torch.zeros((2, 8, 8, 8))
    lab = torch.tensor([0, 1])
    calls = {"invert": lambda **kw: pipe.invert(z, is_latent=True, steps=8, **kw), "edit": lambda **kw: pipe.edit(z, lab, is_latent=True, steps=8, **kw)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="sampler"):
            call(sampler="euler")
        with pytest.raises(ValueError, match="sampler"):        # the stochastic loop has no upward form
            call(sampler=None)
        with pytest.raises(ValueError, match="spacing"):
            call(spacing="karras")
        with pytest.raises(ValueError, match="cold_diffusion"):
            call(cold_diffusion=True)
        with pytest.raises(ValueError, match="strength"):
            call(strength=0.0)
        with pytest.raises(ValueError, match="strength"):        # one grid point: no upward iteration
            call(strength=0.1)
        with pytest.raises(TypeError):
            call(eta=0.0)
        with pytest.raises(TypeError):
            call(no_such_keyword=1)
        for ok in ({}, dict(sampler="dpmpp2m", spacing="logsnr"), dict(strength=0.5), dict(guidance_scale=4.0)):
            with pytest.raises(RuntimeError, match="no CPU"):      # past the rules: the device check
                call(**ok)
    with pytest.raises(ValueError, match="composite"):
        pipe.edit(z, lab, is_latent=True, steps=8, composite=True, mask=torch.ones((2, 1, 8, 8)))
    with pytest.raises(ValueError, match="return_map"):
        pipe.edit(z, lab, is_latent=True, steps=8, return_map=True)
    with pytest.raises(ValueError, match="return_map"):
        pipe.edit(z, lab, steps=8, return_map=True, decode=False)


# ------------------------------------------------------------------------------------------------ 4. the C ABI
def test_new_entry_points_are_declared_exported_and_bound():
    hdr = (ROOT / "include" / "medfusion_hip.h").read_text()
    assert "MfSolverTraj" in hdr
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    md = (ROOT / "INTEGRATION.md").read_text()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.exported_symbols() and hasattr(lib, name), name
        assert name in md, f"INTEGRATION.md does not list {name}"
    assert lib.mf_version() == 250      # additive within ABI 250
    m = re.search(r"enum \{ MF_TRAJ_RECORD = (\d), MF_TRAJ_KEEP = (\d) \}", hdr)
    assert tuple(int(v) for v in m.groups()) == (L.TRAJ_RECORD, L.TRAJ_KEEP)
    assert C.sizeof(L.MfSolverTraj) == 8 * 2 + 8 + 4 * 6                                           # 2 ptr, i64, 6 i32
    assert C.sizeof(L.MfSolverStep) == 8 * 4 and C.sizeof(L.MfSolverArgs) == 8 * 11 + 4 * 4 + 8    # (unchanged)
    body = re.search(r"typedef struct MfSolverTraj \{(.*?)\} MfSolverTraj;", hdr, re.S).group(1)
    assert [f[0] for f in L.MfSolverTraj._fields_] == re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", body, re.M)                   # the binding's fields in the header's order
