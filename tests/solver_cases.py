"""The deterministic-sampler cases (sampler="ddim0" / "dpmpp2m") shared by scripts/gen_solver_golden.py (which runs the DDIM ones through the
reference at eta = 0) and the tests: pipeline arguments, noise seeds and loop arguments of the tests/golden/solver_ddim0_* fixtures; the
closed-form Gaussian problem the solver-accuracy test runs on; and `composed_solver_loop`, the oracle of DPM-Solver++(2M) -- the restatement's
CPU UNet driven by a plain torch loop over the scheduler's (A, B, C) rows (the reference has no such solver)."""
from __future__ import annotations

import math

import torch

from oracle import restate as R

# fixture name -> spatial dims, pipeline (tag of the synthetic weights, label classes, constructor flags), loop arguments, batch, noise seed.
# 2-D: latent (8, 8, 8) through the tiny VAE's decoder; 3-D: the tests/d3_cases.unet_kwargs architecture on a (4, 4, 8, 8) latent, no embedder.
DDIM0_CASES = {
    "solver_ddim0_uncond": dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3), steps=6, n=2, seed=61),
    "solver_ddim0_cfg8": dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3), steps=6, n=3, seed=62, condition=[2, 0, 1], guidance_scale=8.0),
    "solver_ddim0_x0obj_clip": dict(dims=2, pipe=dict(tag="pipe_tiny_x0", ncls=None, clip_x0=True, objective="x_0"), steps=5, n=2, seed=63),
    "solver_ddim0_3d": dict(dims=3, pipe=dict(tag="solver_ddim0_3d", ncls=2), steps=5, n=2, seed=64, condition=[1, 0], guidance_scale=1.0),
}
SIZE = {2: (8, 8, 8), 3: (4, 4, 8, 8)}

# DPM-Solver++(2M) end to end: 8 executed iterations (uniform grid)
DPMPP2M_CASES = {
    "tiny2d": dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3), steps=8, n=2, seed=71),
    "tiny2d_cfg4": dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3), steps=8, n=2, seed=72, condition=[2, 0], guidance_scale=4.0),
    "tiny3d": dict(dims=3, pipe=dict(tag="solver_ddim0_3d", ncls=2), steps=8, n=2, seed=73, condition=[0, 1], guidance_scale=1.0),
}


def pipe_args(case: dict):
    """-> (unet kwargs in the oracle's form, vae kwargs or None, tag, constructor flags)"""
    from tests.d3_cases import unet_kwargs

    p = dict(case["pipe"])
    tag, ncls = p.pop("tag"), p.pop("ncls")
    if case["dims"] == 3:
        return unet_kwargs([1, 2, 2, 2], in_ch=4), None, tag, p
    return R.tiny_unet_kwargs(ncls, "none"), R.tiny_vae_kwargs(), tag, p


def loop_kwargs(case: dict, device=None) -> dict:
    if "condition" not in case:
        return {}
    return dict(condition=torch.tensor(case["condition"], device=device), guidance_scale=case["guidance_scale"], un_cond=None)


def rows_array(rows):
    """MfSolverStep rows as one float64 array [len, 5] = (t, mode, A, B, C): fp32 coefficients are exact in fp64"""
    return torch.tensor([[r.t, r.mode, r.A, r.B, r.C] for r in rows], dtype=torch.float64).numpy()


# ------------------------------------------------------------------------------------------------ the closed form (fp64)
def gaussian_denoiser(ac_t: float, s2: float) -> float:
    """E[x_0 | x_t] = k x_t for data x_0 ~ N(0, s2): k = alpha s2 / (alpha^2 s2 + sigma^2)"""
    return math.sqrt(ac_t) * s2 / (ac_t * s2 + (1.0 - ac_t))


def gaussian_exact(ac, s2: float, x_T: torch.Tensor) -> torch.Tensor:
    """the probability-flow ODE's solution carried from t = T - 1 to t = 0, then denoised there (what the loop's last iteration returns)"""
    a0, aT = float(ac[0]), float(ac[-1])
    x_0 = x_T * math.sqrt((a0 * s2 + (1.0 - a0)) / (aT * s2 + (1.0 - aT)))
    return gaussian_denoiser(a0, s2) * x_0


def drive_rows(rows, ac, s2: float, x_T: torch.Tensor) -> torch.Tensor:
    """a plain fp64 loop over MfSolverStep rows with the Gaussian denoiser in the estimator's place: the modes as include/medfusion_hip.h states them"""
    x, prev = x_T.double().clone(), None
    for r in rows:
        a = float(ac[r.t])
        x0 = gaussian_denoiser(a, s2) * x
        xT = (x - math.sqrt(a) * x0) / math.sqrt(1.0 - a)
        if r.mode == 0:
            x = x0
        elif r.mode == 1:
            x = r.B * x0 + r.A * xT
        elif r.mode == 2:
            x = r.A * x + r.B * x0
        else:
            x = r.A * x + r.B * x0 + r.C * prev
        prev = x0
    return x


# ------------------------------------------------------------------------------------------------ the oracle of dpmpp2m
@torch.no_grad()
def composed_solver_loop(ora, x_T: torch.Tensor, rows, condition=None, guidance_scale=1.0, un_cond=None, decode=True):
    """`ora`: the restatement pipeline, or the reference's (they share the interface), in fp32 or .double() with x_T.double(); rows:
    GaussianNoiseScheduler.solver_records(...) of the product, whose fp32 coefficients are data here.  Every iteration: the pipeline's own forward() for the x_0 estimate (its posterior sample is not used),
    then x = A x + B x_0 + C x_0_prev (x_0 on the last row)."""
    x, prev, n = x_T, None, x_T.shape[0]
    for r in rows:
        _, x0, xT, _ = ora(x, torch.tensor(r.t).expand(n), condition, self_cond=None, guidance_scale=guidance_scale, un_cond=un_cond)
        if r.mode == 0:
            x = x0
        elif r.mode == 1:
            x = x0 * r.B + r.A * xT
        elif r.mode == 2:
            x = r.A * x + r.B * x0
        else:
            x = r.A * x + r.B * x0 + r.C * prev
        prev = x0
    if decode and ora.latent_embedder is not None:
        x = ora.latent_embedder.decode(x)
    return x
