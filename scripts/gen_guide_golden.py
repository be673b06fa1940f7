#!/usr/bin/env python3
"""Writes tests/golden/guide_*.npz: sampling with guidance rescale, dynamic thresholding and a guidance schedule, composed from the REAL
reference's own pieces, reached through oracle/shims like scripts/gen_solver_golden.py.

The reference has no such options, so its loop cannot be called as it is.  Every iteration here is its forward() taken apart at the line where
the guided prediction exists (diffusion_pipeline.py:242-244): the reference estimator's two passes, then the stage restated in plain torch
(tests/guide_cases.stage_torch: torch.std, torch.quantile, clamp, with the reference scheduler's estimate_x_0 / estimate_x_T), then the rest of
forward() and denoise() by the reference scheduler's own functions -- estimate_x_t_prior_from_x_T / _from_x_0 and the DDIM update of :297-304 for
the default loop; estimate_x_0 / estimate_x_T and the product scheduler's solver rows (data, as in gen_solver_golden.py) for "ddim0" / "dpmpp2m".
Weights are oracle.synth hash tensors keyed by the state-dict names; the fixtures hold the outputs and the noise seed only.  Runs on the CPU;
needs the reference checkout.

Run from the repository root:  python scripts/gen_guide_golden.py [reference root]
"""
from __future__ import annotations

import sys
import unittest.mock as um
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
REF = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT.parent / "reference"
sys.path.insert(0, str(ROOT / "oracle" / "shims"))
sys.path.insert(0, str(REF))
sys.path.insert(0, str(ROOT))

import numpy as np
import torch

torch.set_num_threads(1)   # fixed summation order for the stored vectors

from medical_diffusion.models.pipelines import DiffusionPipeline as RefPipeline

import medfusion_amd as M
from oracle import gen_golden as G
from oracle import restate as R
from oracle import synth as S
from tests.guide_cases import PIPE_CASES, stage_torch
from tests.solver_cases import SIZE, pipe_args

GOLD = ROOT / "tests" / "golden"
LIMIT = 400 * 1024


def ref_pipe(case):
    unet_kw, vae_kw, tag, flags = pipe_args(case)
    ref = RefPipeline(noise_scheduler=G.RefScheduler, noise_estimator=G.RefUNet, latent_embedder=None, noise_scheduler_kwargs=R.published_scheduler_kwargs(),
                      noise_estimator_kwargs=G.ref_unet_kwargs(unet_kw), estimator_objective=flags.get("objective", "x_T"),
                      clip_x0=flags.get("clip_x0", False), do_input_centering=False)
    if vae_kw:
        ref.latent_embedder = G.ref_vae(vae_kw)
    ref.eval()
    S.synth_state_dict(ref.noise_estimator, f"{tag}.unet.")
    if vae_kw:
        S.synth_state_dict(ref.latent_embedder, f"{tag}.vae.")
    return ref


def schedule_scales(schedule, rev, g):
    """the guidance scale of every executed iteration, restated here from the issue's text -- not taken from the product: no schedule = g
    everywhere; ("interval", t_lo, t_hi) = g where t_lo <= t <= t_hi and 1 elsewhere; a sequence = itself"""
    if schedule is None:
        return [float(g)] * len(rev)
    if schedule[0] == "interval":
        return [float(g) if schedule[1] <= t <= schedule[2] else 1.0 for t in rev]
    assert len(schedule) == len(rev)
    return [float(v) for v in schedule]


@torch.no_grad()
def guided_loop(ref, case, dtype=torch.float32):
    """-> the decoded result.  Draws through torch.randn_like (patched by the caller): x_T, then what the reference's loop draws."""
    n, size = case["n"], SIZE[case["dims"]]
    sch, est, opts = ref.noise_scheduler, ref.noise_estimator, case["opts"]
    cond = torch.tensor(case["condition"])
    psch = M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())
    sampler = case["sampler"]
    ts, _ = psch.loop_timesteps(case["steps"], True, case["spacing"] if sampler else None)
    rev = list(reversed(ts))
    scales = schedule_scales(opts.get("guidance_schedule"), rev, case["guidance_scale"])
    rows = psch.solver_records(ts, sampler) if sampler else None
    phi, q, s_max = opts.get("guidance_rescale", 0.0), opts.get("dynamic_threshold"), opts.get("threshold_max")
    x = sch.x_final(torch.zeros((n, *size), dtype=dtype))                                                       # draw #0
    prev = None
    for i, t in enumerate(rev):
        tt = torch.tensor(t).expand(n)
        pu, _ = est(x, tt, condition=None, self_cond=None)              # diffusion_pipeline.py:242-243, un-guided pass first
        pc, _ = est(x, tt, condition=cond, self_cond=None)
        pred = stage_torch(x, pc, pu, tt, sch, scales[i], phi, q, s_max, ref.estimator_objective)
        if sampler is None:                                              # the rest of forward() (:264-271) and of denoise() (:297-304)
            if ref.estimator_objective == "x_0":
                x_prior, x0 = sch.estimate_x_t_prior_from_x_0(x, tt, pred, clip_x0=ref.clip_x0, var_scale=0)
                xT = sch.estimate_x_T(x, x_0=pred, t=tt, clip_x0=ref.clip_x0)
            else:
                x_prior, x0 = sch.estimate_x_t_prior_from_x_T(x, tt, pred, clip_x0=ref.clip_x0, var_scale=0)
                xT = pred
            x = x_prior
            if len(rev) - i - 1 > 0:
                alpha, alpha_next = sch.alphas_cumprod[t], sch.alphas_cumprod[rev[i + 1]]
                sigma = ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
                c = (1 - alpha_next - sigma ** 2).sqrt()
                x = x0 * alpha_next.sqrt() + c * xT + sigma * torch.randn_like(x)
            continue
        if ref.estimator_objective == "x_0":
            x0 = pred.clamp(-1, 1) if ref.clip_x0 else pred
            xT = sch.estimate_x_T(x, x_0=pred, t=tt, clip_x0=ref.clip_x0)
        else:
            x0 = sch.estimate_x_0(x, pred, tt, clip_x0=ref.clip_x0)
            xT = pred
        r = rows[i]
        if r.mode == 0:
            x = x0
        elif r.mode == 1:
            x = x0 * r.B + r.A * xT
        elif r.mode == 2:
            x = r.A * x + r.B * x0
        else:
            x = r.A * x + r.B * x0 + r.C * prev
        prev = x0
    if ref.latent_embedder is not None:
        x = ref.latent_embedder.decode(x)
    return x


def main():
    for name, case in PIPE_CASES.items():
        ref = ref_pipe(case)
        with um.patch.object(torch, "randn_like", side_effect=S.PhiloxNoise(case["seed"])) as mk:
            img = guided_loop(ref, case)
            draws = mk.call_count
        ref64 = ref.double()
        nz = S.PhiloxNoise(case["seed"])
        torch.set_default_dtype(torch.float64)
        try:
            with um.patch.object(torch, "randn_like", side_effect=lambda like: nz(like).double()):
                img64 = guided_loop(ref64, case, torch.float64)
        finally:
            torch.set_default_dtype(torch.float32)
        drift = float((img.double() - img64).abs().max() / img64.abs().max())
        G.save(name, image=img, n=case["n"], size=np.asarray(SIZE[case["dims"]]), seed=case["seed"], steps=case["steps"], draws=draws, fp64_drift=drift)
        assert (GOLD / f"{name}.npz").stat().st_size < LIMIT, name
        print(f"  {name}: {tuple(img.shape)}, {draws} draws, the fp32 composition vs its fp64 self {drift:.2e}")


if __name__ == "__main__":
    main()
