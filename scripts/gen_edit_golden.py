#!/usr/bin/env python3
"""Writes tests/golden/edit_*.npz: DDIM inversion and counterfactual editing composed from the REAL reference's own pieces, reached through
oracle/shims like oracle/gen_golden.py (tests/edit_cases.py: composed_invert / composed_descent).

  "ddim0"    upward: DiffusionPipeline.forward's x_0 / x_T estimates, then GaussianNoiseScheduler.estimate_x_t(x_0_est, t_next, x_T=x_T_est);
             downward: the reference's DDIM update (diffusion_pipeline.py:297-304) at eta = 0, as scripts/gen_solver_golden.py runs it;
  "dpmpp2m"  the reference pipeline's forward under a plain loop over the product scheduler's rows, which are data (the reference has no such
             solver), as tests/solver_cases.composed_solver_loop does.

Every case runs twice: in fp32 (`result`) and, for the conditioning of the case, in fp64 (`result64`).  Weights, inputs and masks are hash tensors
keyed by name (tests/edit_cases.py rebuilds them), so the fixtures hold results only.  forward() draws a posterior sample the composition does
not use: it comes from a patched randn_like.  Runs on the CPU; needs the reference checkout.

Run from the repository root:  python scripts/gen_edit_golden.py [reference root]
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
from tests import edit_cases as E
from tests.solver_cases import pipe_args

GOLD = ROOT / "tests" / "golden"
LIMIT = 64 * 1024


def ref_pipe(case):
    unet_kw, vae_kw, tag, flags = pipe_args(case)
    ref = RefPipeline(noise_scheduler=G.RefScheduler, noise_estimator=G.RefUNet, latent_embedder=None, noise_scheduler_kwargs=R.published_scheduler_kwargs(),
                      noise_estimator_kwargs=G.ref_unet_kwargs(unet_kw), estimator_objective="x_T", clip_x0=False, do_input_centering=False)
    if vae_kw:
        ref.latent_embedder = G.ref_vae(vae_kw)
    ref.eval()
    S.synth_state_dict(ref.noise_estimator, f"{tag}.unet.")
    if vae_kw:
        S.synth_state_dict(ref.latent_embedder, f"{tag}.vae.")
    return ref


@torch.no_grad()
def run(name):
    case = E.CASES[name]
    sch = M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())
    ref = ref_pipe(case)
    nz = S.PhiloxNoise(1000)
    with um.patch.object(torch, "randn_like", side_effect=nz):
        w32 = E.run_case(ref, name, sch)
    ref64 = ref.double()
    torch.set_default_dtype(torch.float64)
    try:
        with um.patch.object(torch, "randn_like", side_effect=lambda like: nz(like).double()):
            w64 = E.run_case(ref64, name, sch, dtype=torch.float64)
    finally:
        torch.set_default_dtype(torch.float32)
    assert w32.dtype == torch.float32 and w64.dtype == torch.float64 and bool(w64.isfinite().all())
    drift = float((w32.double() - w64).abs().max() / w64.abs().max())
    G.save(name, result=w32, result64=w64.numpy(), steps=E.STEPS, k=E.span(case))
    assert (GOLD / f"{name}.npz").stat().st_size < LIMIT, name
    print(f"  {name}: result {tuple(w32.shape)}, the fp32 composition vs its fp64 self {drift:.2e}")


if __name__ == "__main__":
    for name in E.CASES:
        run(name)
