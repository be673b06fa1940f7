#!/usr/bin/env python3
"""Writes tests/golden/val_*.npz: the held-out denoising loss of the REAL reference -- its own DiffusionPipeline._step at state 'val'
(diffusion_pipeline.py:78-201), reached through oracle/shims like oracle/gen_golden.py -- for the cases of tests/val_cases.py.

`noise_scheduler.sample` is patched to inject the case's timesteps and the Philox x_T (draw #0 of the case's seed) through the reference's own
estimate_x_t; the VAE encoder's torch.randn is the Philox draw #0 of the case's encoder seed; classifier_free_guidance_dropout is 0, so the
condition is kept; `log` records what the reference logs, `global_step` is 0 (no image logging).  Every case runs twice: in fp32 (`<scalar>`)
and in fp64 (`<scalar>64`).  Weights and inputs are hash tensors keyed by name (tests/val_cases.py rebuilds them), so the fixtures hold results only.
Runs on the CPU; needs the reference checkout.

Run from the repository root:  python scripts/gen_val_golden.py [reference root]
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

torch.set_num_threads(1)   # fixed summation order for the stored scalars

from medical_diffusion.models.pipelines import DiffusionPipeline as RefPipeline

from oracle import gen_golden as G
from oracle import restate as R
from oracle import synth as S
from tests import val_cases as V

GOLD = ROOT / "tests" / "golden"
LIMIT = 64 * 1024


def ref_pipe(case):
    unet_kw, vae_kw, tag, flags = V.pipe_args(case)
    ref = RefPipeline(noise_scheduler=G.RefScheduler, noise_estimator=G.RefUNet, latent_embedder=None, noise_scheduler_kwargs=R.published_scheduler_kwargs(),
                      noise_estimator_kwargs=G.ref_unet_kwargs(unet_kw), estimator_objective=flags.get("objective", "x_T"),
                      estimate_variance=flags.get("estimate_variance", False), clip_x0=flags.get("clip_x0", False),
                      do_input_centering=bool(case.get("image")), classifier_free_guidance_dropout=0.0,
                      loss=torch.nn.L1Loss if case["loss"] == "l1" else torch.nn.MSELoss)
    if vae_kw:
        ref.latent_embedder = G.ref_vae(vae_kw)
    ref.eval()
    S.synth_state_dict(ref.noise_estimator, f"{tag}.unet.")
    if vae_kw:
        S.synth_state_dict(ref.latent_embedder, f"{tag}.vae.")
    return ref


@torch.no_grad()
def step(ref, name, dtype):
    case = V.CASES[name]
    t = torch.tensor(case["t"])
    x_T_src, enc = S.PhiloxNoise(case["seed"]), S.PhiloxNoise(case.get("enc_seed", 0))
    sch = ref.noise_scheduler

    def sample(x_0):
        x_T = x_T_src(x_0).to(dtype)
        return sch.estimate_x_t(x_0, t, x_T), x_T, t

    logged = {}
    ref.log = lambda key, value, **kw: logged.__setitem__(key, value)
    ref.global_step = 0
    batch = {"source": V.case_input(name).to(dtype)}
    if case.get("condition") is not None:
        batch["target"] = V.case_condition(name)
    with um.patch.object(sch, "sample", side_effect=sample), \
            um.patch.object(torch, "randn", side_effect=lambda shape, generator=None, device=None: enc(torch.empty(tuple(shape))).to(dtype)):
        ref._step(batch, 0, "val", 0, 0)
    assert x_T_src.draw == 1
    return {k.split("/", 1)[1]: v for k, v in logged.items()}


def run(name):
    ref = ref_pipe(V.CASES[name])
    r32 = step(ref, name, torch.float32)
    ref64 = ref.double()
    torch.set_default_dtype(torch.float64)
    try:
        r64 = step(ref64, name, torch.float64)
    finally:
        torch.set_default_dtype(torch.float32)
    out = {}
    for k in V.SCALARS:
        if k in r32:
            assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64 and bool(r64[k].isfinite()), (name, k)
            out[k], out[k + "64"] = r32[k].reshape(1), r64[k].reshape(1).numpy()
    G.save(name, t=np.asarray(V.CASES[name]["t"]), seed=V.CASES[name]["seed"], **out)
    assert (GOLD / f"{name}.npz").stat().st_size < LIMIT, name
    print("  " + name + ": " + ", ".join(f"{k} {float(r32[k]):.6g} (fp32 vs fp64 {abs(float(r32[k]) - float(r64[k])) / abs(float(r64[k])):.1e})" for k in V.SCALARS if k in r32))


if __name__ == "__main__":
    for name in V.CASES:
        run(name)
