#!/usr/bin/env python3
"""Writes tests/golden/solver_ddim0_*.npz from the REAL reference's sample() at eta = 0, reached through oracle/shims like oracle/gen_golden.py
(and solver_dpmpp2m_tiny3d.npz: see case_dpmpp2m_3d).

The reference reads `eta = kwargs.get('eta', 1)` in denoise (diffusion_pipeline.py:301) but forwards **kwargs to forward(), which rejects the
keyword.  Here forward() is wrapped -- by unittest.mock, nothing is edited -- to drop that one keyword, so the loop runs the
reference's own DDIM arithmetic at sigma = 0.  (It still draws its posterior and DDIM noise, which sigma = 0 and the t = 0 posterior multiply by
zero; a deterministic sampler consumes draw #0 only.)  Weights are oracle.synth hash tensors keyed by the state-dict names, so the fixtures hold
the reference's outputs and the noise seed only; the tests rebuild the weights from the same names (tests/solver_cases.py).  Runs on the CPU;
needs the reference checkout.

Run from the repository root:  python scripts/gen_solver_golden.py [reference root]
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

from oracle import gen_golden as G
from oracle import restate as R
from oracle import synth as S
from tests.solver_cases import DDIM0_CASES, DPMPP2M_CASES, SIZE, composed_solver_loop, loop_kwargs, pipe_args, rows_array

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


@torch.no_grad()
def case_dpmpp2m_3d(name="tiny3d"):
    """The restatement has no spatial_dims=3 UNet, so the CPU composition of the 3-D DPM-Solver++(2M) case runs HERE, on the reference's own 3-D
    pipeline (tests/solver_cases.composed_solver_loop: its forward() under a plain torch loop over the product scheduler's (A, B, C) rows, which
    are data), in fp32 and -- for the conditioning of the case -- in fp64.  The rows travel in the fixture: the test refuses a stale one."""
    import medfusion_amd as M

    case = DPMPP2M_CASES[name]
    sch = M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())
    rows = sch.solver_records(sch.loop_timesteps(case["steps"], True)[0], "dpmpp2m")
    n, size, seed = case["n"], SIZE[case["dims"]], case["seed"]
    x_T = S.PhiloxNoise(seed)(torch.empty((n, *size)))       # draw #0
    ref = ref_pipe(case)
    nz = S.PhiloxNoise(seed + 1000)                              # (forward() draws a posterior sample the composition does not use)
    with um.patch.object(torch, "randn_like", side_effect=nz):
        w32 = composed_solver_loop(ref, x_T, rows, **loop_kwargs(case))
    ref64 = ref.double()
    torch.set_default_dtype(torch.float64)
    try:
        with um.patch.object(torch, "randn_like", side_effect=lambda like: nz(like).double()):
            w64 = composed_solver_loop(ref64, x_T.double(), rows, **loop_kwargs(case))
    finally:
        torch.set_default_dtype(torch.float32)
    drift = float((w32.double() - w64).abs().max() / w64.abs().max())
    G.save(f"solver_dpmpp2m_{name}", image=w32, n=n, size=np.asarray(size), seed=seed, steps=case["steps"], rows=rows_array(rows), fp64_drift=drift)
    assert (GOLD / f"solver_dpmpp2m_{name}.npz").stat().st_size < LIMIT
    print(f"  {name}: the fp32 composition vs its fp64 self {drift:.2e}")


@torch.no_grad()
def main():
    forward = RefPipeline.forward

    def forward_without_eta(self, *args, eta=None, **kw):
        return forward(self, *args, **kw)

    for name, case in DDIM0_CASES.items():
        ref = ref_pipe(case)
        n, size = case["n"], SIZE[case["dims"]]
        with um.patch.object(RefPipeline, "forward", forward_without_eta), um.patch.object(torch, "randn_like", side_effect=S.PhiloxNoise(case["seed"])) as mk:
            img = ref.sample(n, size, steps=case["steps"], use_ddim=True, eta=0, **loop_kwargs(case))
            draws = mk.call_count
        G.save(name, image=img, n=n, size=np.asarray(size), seed=case["seed"], steps=case["steps"], reference_draws=draws)
        assert (GOLD / f"{name}.npz").stat().st_size < LIMIT, name


if __name__ == "__main__":
    main()
    case_dpmpp2m_3d()
