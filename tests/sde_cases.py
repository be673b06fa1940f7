"""The stochastic-sampler cases (sampler="ddim1" / "dpmpp2m_sde") shared by scripts/gen_sde_golden.py and the tests: pipeline arguments, noise
seeds and loop arguments of the tests/golden/sde_* fixtures (the tiny pipelines of tests/solver_cases.py); `composed_sde_loop`, the oracle of
SDE-DPM-Solver++(2M) -- a pipeline's own forward() under a plain torch loop over the scheduler's rows, scales and injected draws (the reference
has no such solver); and the closed-form Gaussian problem's exact output variance under a sampler's linear recurrence."""
from __future__ import annotations

import math

import numpy as np
import torch

from tests.solver_cases import SIZE, gaussian_denoiser, loop_kwargs, pipe_args  # noqa: F401  (re-exported: one import for the users of the cases)

# the reference's own denoise(use_ddim=True) -- DDIM at eta = 1 -- with its DDIM draw of iteration i = oracle-Philox draw #(i + 1) of `seed`
DDIM1_CASES = {
    "sde_ddim1_uncond": dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3), steps=6, n=2, seed=81),
    "sde_ddim1_cfg8": dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3), steps=6, n=3, seed=82, condition=[2, 0, 1], guidance_scale=8.0),
    "sde_ddim1_3d": dict(dims=3, pipe=dict(tag="solver_ddim0_3d", ncls=2), steps=5, n=2, seed=83, condition=[1, 0], guidance_scale=1.0),
}

# SDE-DPM-Solver++(2M) end to end: 8 executed iterations, on the log-SNR grid it is meant for and once on the reference's grid
SDE2M_CASES = {
    "sde_dpmpp2m_sde_2d": dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3), steps=8, spacing="logsnr", n=2, seed=91),
    "sde_dpmpp2m_sde_cfg4": dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3), steps=8, spacing=None, n=2, seed=92, condition=[2, 0], guidance_scale=4.0),
    "sde_dpmpp2m_sde_3d": dict(dims=3, pipe=dict(tag="solver_ddim0_3d", ncls=2), steps=8, spacing="logsnr", n=2, seed=93, condition=[0, 1], guidance_scale=1.0),
}


def rows_array(rows, scales):
    """MfSolverStep rows and their noise scales as one float64 array [len, 6] = (t, mode, A, B, C, S): fp32 coefficients are exact in fp64"""
    return np.asarray([[r.t, r.mode, r.A, r.B, r.C, s] for r, s in zip(rows, scales)], dtype=np.float64)


@torch.no_grad()
def composed_sde_loop(ora, x_T: torch.Tensor, rows, scales, draw, condition=None, guidance_scale=1.0, un_cond=None, decode=True, record=None):
    """tests/solver_cases.composed_solver_loop with the draw: every iteration the pipeline's own forward() for the x_0 / x_T estimates (its
    posterior sample is not used), the row's deterministic update, then + S * draw(x) on every row but the last.  `draw(like)`: the injected draws
    in order (draw #1, #2, ...), already in x's dtype.  record: a list that receives (x_0, latent) per iteration."""
    x, prev, n = x_T, None, x_T.shape[0]
    for r, s in zip(rows, scales):
        _, x0, xT, _ = ora(x, torch.tensor(r.t).expand(n), condition, self_cond=None, guidance_scale=guidance_scale, un_cond=un_cond)
        if r.mode == 0:
            x = x0
        else:
            if r.mode == 1:
                x = x0 * r.B + r.A * xT
            elif r.mode == 2:
                x = r.A * x + r.B * x0
            else:
                x = r.A * x + r.B * x0 + r.C * prev
            x = x + s * draw(x)
        prev = x0
        if record is not None:
            record.append((x0.clone(), x.clone()))
    if decode and ora.latent_embedder is not None:
        x = ora.latent_embedder.decode(x)
    return x


# ------------------------------------------------------------------------------------------------ the closed form (fp64)
def output_variance(rows, scales, ac, s2: float) -> float:
    """Data x_0 ~ N(0, s2), the exact denoiser E[x_0 | x_t] = k_t x_t, x_T ~ N(0, 1): every sampler here is a linear recurrence in
    (x, x_0_prev) driven by independent standard normal draws, so the exact 2 x 2 covariance of that pair is carried through the rows in fp64
    (the modes as include/medfusion_hip.h states them) -> the variance of what the last row returns."""
    cov = np.array([[1.0, 0.0], [0.0, 0.0]])
    for r, s in zip(rows, scales):
        a = float(ac[r.t])
        k = gaussian_denoiser(a, s2)
        if r.mode == 0:
            return k * k * cov[0, 0]
        if r.mode == 1:      # B x_0 + A x_T with x_T = (x - sqrt(a) x_0) / sqrt(1 - a)
            m = np.array([[r.B * k + r.A * (1.0 - math.sqrt(a) * k) / math.sqrt(1.0 - a), 0.0], [k, 0.0]])
        else:
            m = np.array([[r.A + r.B * k, r.C], [k, 0.0]])
        cov = m @ cov @ m.T
        cov[0, 0] += float(s) ** 2
    raise ValueError("no MF_SOLVER_FINAL row")


def exact_variance(ac, s2: float) -> float:
    """the variance of the exact posterior mean at the grid's lowest timestep, E[x_0 | x_t0] with x_t0 ~ N(0, a s2 + 1 - a): what a perfect
    sampler's last row returns"""
    a = float(ac[0])
    return gaussian_denoiser(a, s2) ** 2 * (a * s2 + 1.0 - a)


def variance_error(sch, steps, sampler, spacing, s2: float) -> float:
    ac = sch.host_tables()["alphas_cumprod"].numpy().astype(np.float64)
    ts, _ = sch.loop_timesteps(steps, True, spacing)
    rows, scales = sch.stochastic_records(ts, sampler)
    want = exact_variance(ac, s2)
    return abs(output_variance(rows, scales, ac, s2) - want) / want
