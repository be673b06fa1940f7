#!/usr/bin/env python3
"""Writes tests/golden/i2i_*.npz: image-conditioned sampling (img2img, masked inpainting) composed from the REAL reference's own
DiffusionPipeline.forward and GaussianNoiseScheduler.estimate_x_t (tests/i2i_cases.py: composed_loop), reached through oracle/shims like
oracle/gen_golden.py.  The oracle restatement driven the same way must be bit-equal before anything is written.  Weights, inputs and masks are
hash tensors keyed by name (tests/i2i_cases.py rebuilds them), so the fixtures hold the reference's outputs and the seeds only.  Runs on the CPU;
needs the reference checkout.

Run from the repository root:  python scripts/gen_i2i_golden.py [reference root]
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

from oracle import gen_golden as G
from oracle import restate as R
from oracle import synth as S
from tests import i2i_cases as I

GOLD = ROOT / "tests" / "golden"
LIMIT = 400 * 1024


@torch.no_grad()
def run(name):
    c = I.CASES[name]
    unet_kw, vae_kw, tag, flags = I.pipe_args(name)
    ref, ora = G.build_pipes(unet_kw, vae_kw, R.published_scheduler_kwargs(), tag, clip_x0=flags.get("clip_x0", False),
                             objective=flags.get("objective", "x_T"), estimate_variance=flags.get("estimate_variance", False))
    x, mask, is_latent = I.case_inputs(name)
    kw = dict(strength=c["strength"], steps=c["steps"], use_ddim=c["use_ddim"], mask=mask, is_latent=is_latent, centering=c.get("centering", False),
              composite=c["mask"] == "pixels", **I.loop_kwargs(name))
    enc = S.PhiloxNoise(c.get("enc_seed", 0))
    tr_ref, tr_ora = [], []
    with um.patch.object(torch, "randn_like", side_effect=S.PhiloxNoise(c["seed"])) as mk, \
            um.patch.object(torch, "randn", side_effect=lambda shape, generator=None, device=None: enc(torch.empty(shape))):
        out_ref, z0_ref = I.composed_loop(ref, lambda like: torch.randn_like(like), x, trace=tr_ref, **kw)
        draws = mk.call_count
    ora.set_noise_fn(S.PhiloxNoise(c["seed"]))
    enc2 = S.PhiloxNoise(c.get("enc_seed", 0))
    ora.latent_embedder.quantizer.noise_fn = lambda shape, device: enc2(torch.empty(shape))
    out_ora, z0_ora = I.composed_loop(ora, ora._randn_like, x, trace=tr_ora, **kw)
    assert ora.noise_fn.draw == draws, (ora.noise_fn.draw, draws)
    k = I.EXECUTED[name]
    assert len(tr_ref) == k and draws == (2 * k if c["use_ddim"] else 1 + k), (name, len(tr_ref), draws)
    G.check_equal(name, out_ref, out_ora)
    G.check_equal(name + ".z0", z0_ref, z0_ora)
    for i, ((a0, at), (b0, bt)) in enumerate(zip(tr_ref, tr_ora)):
        G.check_equal(f"{name}.x0[{i}]", a0, b0)
        G.check_equal(f"{name}.xt[{i}]", at, bt)
    if mask is not None:   # the kept cells of the final latent ARE z0
        keep = ~I.cell_mask(mask, z0_ref.shape).expand_as(z0_ref)
        assert torch.equal(tr_ref[-1][1][keep], z0_ref[keep]), name
    G.save(name, result=out_ref, latent=tr_ref[-1][1], x0_trace=torch.stack([a for a, _ in tr_ref]), seed=c["seed"], draws=draws, executed=k)
    assert (GOLD / f"{name}.npz").stat().st_size < LIMIT, name


if __name__ == "__main__":
    for name in I.CASES:
        run(name)
    print("all i2i cases: oracle == reference")
