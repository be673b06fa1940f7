#!/usr/bin/env python3
"""Writes tests/golden/sde_ddim1_*.npz and sde_dpmpp2m_sde_*.npz, reaching the REAL reference through oracle/shims like scripts/gen_solver_golden.py.

sde_ddim1_*: the reference's own denoise(use_ddim=True) -- DDIM at its eta = 1 -- on the tiny pipelines of tests/solver_cases.py.  torch.randn_like
is patched (unittest.mock, nothing is edited) so that its draw at position 0 (x_T) is oracle-Philox draw #0 of the case's seed and its DDIM draw of
iteration i is draw #(i + 1): the order sampler="ddim1" consumes.  The posterior draws in between, which the DDIM branch never uses, come from another
key.  forward() is wrapped to record every iteration's x_0 estimate and the latent it was given.

sde_dpmpp2m_sde_*: the reference has no such solver, so the reference's forward() (for the x_0 estimate) is composed with the product scheduler's
fp32 rows and scales -- data here -- and the same injected draws in a plain torch loop (tests/sde_cases.composed_sde_loop), the precedent of
solver_dpmpp2m_tiny3d.  The rows travel in the fixture: the test refuses a stale one.

Every fixture also holds `fp64_drift`, the distance of the stored fp32 result from the same computation in fp64 (the conditioning of the case).
Weights are oracle.synth hash tensors keyed by the state-dict names, so the fixtures hold outputs and seeds only.  Runs on the CPU; needs the
reference checkout.

Run from the repository root:  python scripts/gen_sde_golden.py [reference root]
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
from tests import sde_cases as SD

GOLD = ROOT / "tests" / "golden"
LIMIT = 400 * 1024


def ref_pipe(case):
    unet_kw, vae_kw, tag, flags = SD.pipe_args(case)
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


class ReferenceDraws:
    """randn_like in the reference's call order: call 0 = x_T, then per iteration the posterior draw (odd calls) and the DDIM draw (even calls).
    Even calls walk the case's Philox key -- draw #0, #1, ... -- the odd ones another key."""

    def __init__(self, seed, dtype=torch.float32):
        self.main, self.unused, self.calls, self.dtype = S.PhiloxNoise(seed), S.PhiloxNoise(seed + 1000), 0, dtype

    def __call__(self, like):
        src = self.main if self.calls % 2 == 0 else self.unused
        self.calls += 1
        return src(like).to(self.dtype)


def in_fp64(fn):
    torch.set_default_dtype(torch.float64)
    try:
        return fn()
    finally:
        torch.set_default_dtype(torch.float32)


def drift(w32, w64):
    return float((w32.double() - w64).abs().max() / w64.abs().max())


@torch.no_grad()
def case_ddim1(name, case):
    n, size, seed, steps = case["n"], SD.SIZE[case["dims"]], case["seed"], case["steps"]
    forward = RefPipeline.forward

    def run(ref, dtype):
        seen = []

        def recording_forward(self, x_t, *args, **kw):
            out = forward(self, x_t, *args, **kw)
            seen.append((x_t.clone(), out[1].clone()))
            return out

        draws = ReferenceDraws(seed, dtype)
        with um.patch.object(RefPipeline, "forward", recording_forward), um.patch.object(torch, "randn_like", side_effect=draws):
            img = ref.sample(n, size, steps=steps, use_ddim=True, **SD.loop_kwargs(case))
        assert draws.calls == 2 * steps, (draws.calls, steps)      # x_T, `steps` posterior draws, steps - 1 DDIM draws
        return img, torch.stack([s[0] for s in seen]), torch.stack([s[1] for s in seen])

    ref = ref_pipe(case)
    img, lat_in, x0 = run(ref, torch.float32)
    ref64 = ref.double()
    img64, _, _ = in_fp64(lambda: run(ref64, torch.float64))
    d = drift(img, img64)
    # lat_in[i]: the latent iteration i was given (lat_in[0] = x_T), so the latent iteration i PRODUCED is lat_in[i + 1]; the last one is x_0[-1]
    latents = torch.cat([lat_in[1:], x0[-1:]])
    G.save(name, image=img, x0=x0, latents=latents, n=n, size=np.asarray(size), seed=seed, steps=steps, fp64_drift=d)
    assert (GOLD / f"{name}.npz").stat().st_size < LIMIT, name
    print(f"  {name}: the reference in fp32 vs its fp64 self {d:.2e}")


@torch.no_grad()
def case_sde2m(name, case):
    import medfusion_amd as M

    sch = M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())
    ts, executed = sch.loop_timesteps(case["steps"], True, case["spacing"])
    assert executed == 8, (name, executed)
    rows, scales = sch.stochastic_records(ts, "dpmpp2m_sde")
    n, size, seed = case["n"], SD.SIZE[case["dims"]], case["seed"]

    def run(ref, dtype):
        nz = S.PhiloxNoise(seed)
        x_T = nz(torch.empty((n, *size))).to(dtype)                      # draw #0
        unused = S.PhiloxNoise(seed + 1000)                               # (forward() draws a posterior sample the composition does not use)
        rec = []
        with um.patch.object(torch, "randn_like", side_effect=lambda like: unused(like).to(dtype)):
            img = SD.composed_sde_loop(ref, x_T, rows, scales, lambda like: nz(like).to(dtype), record=rec, **SD.loop_kwargs(case))
        assert nz.draw == len(rows)                                        # x_T and one draw per non-final iteration
        return img, torch.stack([r[0] for r in rec]), torch.stack([r[1] for r in rec])

    ref = ref_pipe(case)
    img, x0, latents = run(ref, torch.float32)
    ref64 = ref.double()
    img64, _, _ = in_fp64(lambda: run(ref64, torch.float64))
    d = drift(img, img64)
    G.save(name, image=img, x0=x0, latents=latents, n=n, size=np.asarray(size), seed=seed, steps=case["steps"], rows=SD.rows_array(rows, scales), fp64_drift=d)
    assert (GOLD / f"{name}.npz").stat().st_size < LIMIT, name
    print(f"  {name}: the fp32 composition vs its fp64 self {d:.2e}")


if __name__ == "__main__":
    for name, case in SD.DDIM1_CASES.items():
        case_ddim1(name, case)
    for name, case in SD.SDE2M_CASES.items():
        case_sde2m(name, case)
