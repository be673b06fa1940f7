"""The inversion / counterfactual-editing cases shared by scripts/gen_edit_golden.py (which runs them through the reference) and the tests:
pipeline arguments, inputs, masks and loop arguments of the tests/golden/edit_* fixtures, and the loops they drive -- `composed_invert` and
`composed_descent`, compositions of the pipeline's own `forward` (x_0 / x_T estimates) with, for "ddim0", the scheduler's own `estimate_x_t`
upward and the reference's DDIM update at eta = 0 downward; for "dpmpp2m" the product scheduler's (A, B, C) rows are data, as in
tests/solver_cases.composed_solver_loop.  They run on the reference pipeline and on its restatement alike (shared interface)."""
from __future__ import annotations

import torch

from oracle import synth as S
from tests.solver_cases import SIZE

# fixture name -> dims, sampler, asked steps (8, uniform grid), strength, batch, source / target labels and guidance, mask.
# 2-D: the tiny pipeline of tests/solver_cases (latent 8 x 8 x 8, tiny VAE decoder); 3-D: its (4, 4, 8, 8) case, no embedder.
_P2, _P3 = dict(tag="pipe_tiny", ncls=3), dict(tag="solver_ddim0_3d", ncls=2)
CASES = {
    "edit_invert_ddim0_2d": dict(dims=2, pipe=_P2, sampler="ddim0", n=2, kind="invert", source=[1, 2]),
    "edit_invert_dpmpp2m_2d": dict(dims=2, pipe=_P2, sampler="dpmpp2m", n=3, kind="invert", source=[0, 2, 1]),
    "edit_invert_ddim0_3d": dict(dims=3, pipe=_P3, sampler="ddim0", n=2, kind="invert", source=[1, 0]),
    "edit_invert_dpmpp2m_3d": dict(dims=3, pipe=_P3, sampler="dpmpp2m", n=2, kind="invert", source=[0, 1]),
    "edit_swap_ddim0_2d": dict(dims=2, pipe=_P2, sampler="ddim0", n=3, kind="edit", source=[0, 1, 2], target=[2, 0, 1], guidance_scale=4.0),
    "edit_swap_dpmpp2m_3d": dict(dims=3, pipe=_P3, sampler="dpmpp2m", n=2, kind="edit", source=[0, 1], target=[1, 0], guidance_scale=4.0),
    "edit_mask_dpmpp2m_2d": dict(dims=2, pipe=_P2, sampler="dpmpp2m", n=2, kind="edit", source=[1, 0], target=[2, 2], guidance_scale=1.0, mask=True,
                                 strength=0.5),
    "edit_mask_ddim0_3d": dict(dims=3, pipe=_P3, sampler="ddim0", n=2, kind="edit", source=[1, 1], target=[0, 1], guidance_scale=1.0, mask=True,
                               strength=0.5),
}
STEPS = 8


def span(case: dict):
    """-> k: the grid points an inversion covers, the strength rule of sample_from on the 8-step grid"""
    return min(STEPS, int(case.get("strength", 1.0) * STEPS + 0.5))


def case_inputs(name: str):
    """-> (z0 latent, boolean cell mask [n, 1, ...] (True = regenerate) or None)"""
    c = CASES[name]
    size = SIZE[c["dims"]]
    z0 = S.synth_input(f"{name}.z0", (c["n"], *size))
    m = (S.synth_input(f"{name}.mask", (c["n"], 1, *size[1:])) > 0.2) if c.get("mask") else None
    return z0, m


def source_kwargs(case: dict, device=None) -> dict:
    return dict(condition=torch.tensor(case["source"], device=device), guidance_scale=1.0, un_cond=None)


def target_kwargs(case: dict, device=None) -> dict:
    return dict(condition=torch.tensor(case["target"], device=device), guidance_scale=case["guidance_scale"], un_cond=None)


def _estimates(pipe, x, t: int, kw: dict):
    _, x0, xT, _ = pipe(x, torch.tensor(t).expand(x.shape[0]), kw.get("condition"), self_cond=None, guidance_scale=kw.get("guidance_scale", 1.0),
                        un_cond=kw.get("un_cond"))
    return x0, xT


def _row(r, x, x0, prev):
    if r.mode == 2:
        return r.A * x + r.B * x0
    return r.A * x + r.B * x0 + r.C * prev


@torch.no_grad()
def composed_invert(pipe, z0, ts, sampler, rows, **kw):
    """the upward pass: rows = GaussianNoiseScheduler.inversion_records(ts, sampler, stop=k) of the product (their t and, for "dpmpp2m", their
    coefficients are data) -> the trajectory, a list of the k latents at ts[0] .. ts[k-1] (slot 0 is z0)"""
    sch, x, prev, traj = pipe.noise_scheduler, z0, None, [z0]
    for j, r in enumerate(rows):
        assert r.t == ts[j]
        x0, xT = _estimates(pipe, x, r.t, kw)
        if sampler == "ddim0":
            x = sch.estimate_x_t(x0, torch.tensor(ts[j + 1]).expand(x.shape[0]), xT)
        else:
            x = _row(r, x, x0, prev)
        prev = x0
        traj.append(x)
    return traj


@torch.no_grad()
def composed_descent(pipe, x, ts, k, sampler, rows, traj=None, cells=None, decode=True, **kw):
    """the last k iterations of the deterministic loop over reversed(ts) from x (the latent at ts[k-1]); rows =
    solver_records(ts, sampler, start=len(ts) - k).  "ddim0": the reference's DDIM update (diffusion_pipeline.py:297-304) with eta = 0.
    cells (True = regenerate) with traj: after the iteration that produced the latent at ts[j] the kept cells take traj[j]; traj[0] after the last."""
    sch, prev = pipe.noise_scheduler, None
    for i, r in enumerate(rows):
        j = k - 1 - i                       # this iteration evaluates at ts[j]
        assert r.t == ts[j]
        x0, xT = _estimates(pipe, x, r.t, kw)
        if r.mode == 0:
            x = x0
        elif sampler == "ddim0":
            alpha, alpha_next = sch.alphas_cumprod[ts[j]], sch.alphas_cumprod[ts[j - 1]]
            sigma = 0 * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
            c = (1 - alpha_next - sigma ** 2).sqrt()
            x = x0 * alpha_next.sqrt() + c * xT
        else:
            x = _row(r, x, x0, prev)
        if cells is not None:
            x = torch.where(cells, x, traj[max(j - 1, 0)])
        prev = x0
    if decode and pipe.latent_embedder is not None:
        x = pipe.latent_embedder.decode(x)
    return x


def run_case(pipe, name: str, sch_product, dtype=torch.float32):
    """the whole case on `pipe` (reference or restatement, already in `dtype`) -> the result: the inverted latent ("invert") or the edited
    latent ("edit": decode=False keeps the fixtures at a few KB; the decoder has its own parity tests).  sch_product: the product's scheduler, the source of the grid and the rows."""
    c = CASES[name]
    z0, m = case_inputs(name)
    z0 = z0.to(dtype)
    ts, _ = sch_product.loop_timesteps(STEPS, True)
    k = span(c)
    traj = composed_invert(pipe, z0, ts, c["sampler"], sch_product.inversion_records(ts, c["sampler"], stop=k), **source_kwargs(c))
    if c["kind"] == "invert":
        return traj[-1]
    rows = sch_product.solver_records(ts, c["sampler"], start=len(ts) - k)
    return composed_descent(pipe, traj[-1], ts, k, c["sampler"], rows, traj=traj, cells=m, decode=False, **target_kwargs(c))
