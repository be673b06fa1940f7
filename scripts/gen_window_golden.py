#!/usr/bin/env python3
"""Writes tests/golden/md_*.npz (windowed denoising, tests/window_cases.PARITY_CASES), reaching the REAL reference through oracle/shims like
scripts/gen_solver_golden.py and scripts/gen_sde_golden.py.

The reference knows no windows.  Its own loop runs on the CANVAS; only its estimator's forward() is wrapped -- by unittest.mock, nothing is edited
-- to crop the canvas into the plan's windows, call the original forward on the B * M rows and merge the prediction with the plain-torch
ref_merge (tests/window_cases.windowed).  The plan is the restatement of tests/window_cases.RefPlan, not the product's; its origins travel in the
fixture and the test refuses a fixture whose origins are not the product's plan.

  md_ddim_cfg_2d     the reference's denoise(use_ddim=True) with guidance; torch.randn_like walks the case's oracle-Philox key, which is the order
                     the product's default loop consumes (x_T, then the posterior and the DDIM draw of every iteration); decoded by the tiny VAE,
                     the latent recorded where decode() receives it
  md_uniform_odd_2d  the reference has no DPM-Solver++(2M): tests/solver_cases.composed_solver_loop over the product scheduler's rows (data here)
                     with the restatement pipeline, whose estimator is wrapped the same way; draw #0 is x_T, the solver draws nothing
  md_3d              the reference's 3-D pipeline at eta = 0 (forward() wrapped to drop that one keyword, as in scripts/gen_solver_golden.py)

Every fixture also holds `fp64_drift`, the distance of the stored fp32 result from the same computation in fp64 (merge included).  Weights are
oracle.synth hash tensors keyed by the state-dict names, so the fixtures hold outputs, seeds and the plan only.  Runs on the CPU; needs the
reference checkout.

Run from the repository root:  python scripts/gen_window_golden.py [reference root]
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
from tests import window_cases as WC
from tests.solver_cases import composed_solver_loop

GOLD = ROOT / "tests" / "golden"
LIMIT = 400 * 1024


def ref_pipe(case):
    unet_kw, vae_kw, tag, flags = WC.pipe_args(case)
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


def restated_pipe(case):
    unet_kw, vae_kw, tag, flags = WC.pipe_args(case)
    ora = R.DiffusionPipeline(R.GaussianNoiseScheduler(**R.published_scheduler_kwargs()), R.UNet(**unet_kw), None, clip_x0=flags.get("clip_x0", False)).eval()
    S.synth_state_dict(ora.noise_estimator, f"{tag}.unet.")
    return ora


def plan_of(case):
    return WC.RefPlan(case["size"][1:], case["window"], case["window_stride"], case["window_weight"])


def in_fp64(fn):
    torch.set_default_dtype(torch.float64)
    try:
        return fn()
    finally:
        torch.set_default_dtype(torch.float32)


def drift(w32, w64):
    return float((w32.double() - w64).abs().max() / w64.abs().max())


def origins_array(plan):
    """[axes][longest] int64, rows padded with -1"""
    out = np.full((len(plan.origins), max(len(o) for o in plan.origins)), -1, dtype=np.int64)
    for a, o in enumerate(plan.origins):
        out[a, :len(o)] = o
    return out


def save(name, case, plan, w32, w64, draws, **more):
    d = drift(w32, w64)
    G.save(name, image=w32, n=case["n"], size=np.asarray(case["size"]), seed=case["seed"], steps=case["steps"], origins=origins_array(plan), M=plan.M,
           draws=draws, fp64_drift=d, **more)
    assert (GOLD / f"{name}.npz").stat().st_size < LIMIT, name
    print(f"  {name}: M = {plan.M}, origins {[list(o) for o in plan.origins]}, {draws} draws, fp32 vs its fp64 self {d:.2e}")


@torch.no_grad()
def case_reference_loop(name):
    """the reference's own sample() on the canvas: md_ddim_cfg_2d (its DDIM loop at eta = 1) and md_3d (eta = 0)"""
    case = WC.PARITY_CASES[name]
    plan = plan_of(case)
    forward = RefPipeline.forward
    eta0 = case["sampler"] == "ddim0"

    def forward_without_eta(self, *args, eta=None, **kw):
        return forward(self, *args, **kw)

    def run(ref, dtype):
        est = type(ref.noise_estimator)
        seen = {}
        nz = S.PhiloxNoise(case["seed"])
        calls = [0]

        def randn_like(like):
            calls[0] += 1
            return nz(like).to(dtype)

        patches = [um.patch.object(est, "forward", WC.windowed(est.forward, plan, dtype)), um.patch.object(torch, "randn_like", side_effect=randn_like)]
        if eta0:
            patches.append(um.patch.object(RefPipeline, "forward", forward_without_eta))
        if ref.latent_embedder is not None:
            decode = ref.latent_embedder.decode
            patches.append(um.patch.object(ref.latent_embedder, "decode", lambda z: (seen.__setitem__("latent", z.clone()), decode(z))[1]))
        for p in patches:
            p.start()
        try:
            img = ref.sample(case["n"], case["size"], steps=case["steps"], use_ddim=True, **({"eta": 0} if eta0 else {}), **WC.loop_kwargs(case))
        finally:
            for p in reversed(patches):
                p.stop()
        return img, seen.get("latent"), calls[0]

    ref = ref_pipe(case)
    img, latent, calls = run(ref, torch.float32)
    ref64 = ref.double()
    img64, _, _ = in_fp64(lambda: run(ref64, torch.float64))
    # the draws the PRODUCT consumes: all of the reference's in the default loop (x_T, a posterior draw per iteration, a DDIM draw per non-final
    # iteration); draw #0 alone for the deterministic sampler (the reference's other draws are multiplied by zero at eta = 0)
    draws = 1 if eta0 else calls
    assert calls == 2 * case["steps"], (calls, case["steps"])
    assert tuple(img.shape[2:]) == (tuple(8 * v for v in case["size"][1:]) if case["decode"] else tuple(case["size"][1:]))
    save(name, case, plan, img, img64, draws, **({} if latent is None else {"latent": latent}))


@torch.no_grad()
def case_dpmpp2m(name="md_uniform_odd_2d"):
    import medfusion_amd as M

    case = WC.PARITY_CASES[name]
    plan = plan_of(case)
    sch = M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())
    rows = sch.solver_records(sch.loop_timesteps(case["steps"], True)[0], "dpmpp2m")
    assert len(rows) == case["steps"] == 8

    def run(ora, dtype):
        x_T = S.PhiloxNoise(case["seed"])(torch.empty((case["n"], *case["size"]))).to(dtype)        # draw #0
        unused = S.PhiloxNoise(case["seed"] + 1000)                       # (forward() draws a posterior sample the composition does not use)
        ora.set_noise_fn(lambda like: unused(like).to(dtype))
        with um.patch.object(R.UNet, "forward", WC.windowed(R.UNet.forward, plan, dtype)):
            return composed_solver_loop(ora, x_T, rows, decode=False, **WC.loop_kwargs(case))

    ora = restated_pipe(case)
    w32 = run(ora, torch.float32)
    ora64 = ora.double()
    w64 = in_fp64(lambda: run(ora64, torch.float64))
    save(name, case, plan, w32, w64, 1, rows=np.asarray([[r.t, r.mode, r.A, r.B, r.C] for r in rows], dtype=np.float64))


if __name__ == "__main__":
    case_reference_loop("md_ddim_cfg_2d")
    case_dpmpp2m()
    case_reference_loop("md_3d")
