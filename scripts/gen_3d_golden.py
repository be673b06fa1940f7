#!/usr/bin/env python3
"""Writes tests/golden/d3_*.npz from the REAL reference at spatial_dims=3 (conv_blocks.py, unet2.py, latent_embedders.py, diffusion_pipeline.py),
reached through oracle/shims (Conv[..., 3], per-axis get_padding) like oracle/gen_golden.py.  Weights are oracle.synth hash tensors keyed by the
state-dict names (synth_state_dict re-randomises the zero-initialised convolutions as well) and inputs are synth_input hash tensors keyed
by name, so the fixtures hold the reference's outputs (and the noise seeds) only; the tests rebuild weights and inputs from the same names
(tests/d3_cases.py).  Runs on the CPU; needs the reference checkout.

Run from the repository root:  python scripts/gen_3d_golden.py [reference root]
"""
from __future__ import annotations

import json
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
from medical_diffusion.models.utils import conv_blocks as RC

from oracle import gen_golden as G
from oracle import restate as R
from oracle import synth as S
from tests.d3_cases import BLOCK_CASES, SAMPLE_CASES, UNET_CASES, VAE_CASE, block_kwargs, unet_kwargs

GOLD = ROOT / "tests" / "golden"
LIMIT = 400 * 1024


def save(name, **arrs):
    G.save(name, **arrs)
    assert (GOLD / f"{name}.npz").stat().st_size < LIMIT, name


def keys_of(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


@torch.no_grad()
def case_blocks():
    out, keys = {}, {}
    for name, (cls, kw, shapes, emb) in BLOCK_CASES.items():
        m = getattr(RC, cls)(**block_kwargs(cls, kw)).eval()
        S.synth_state_dict(m, f"d3.{name}.")
        keys[name] = keys_of(m)
        xs = [S.synth_input(f"d3.{name}.x{i}", s) for i, s in enumerate(shapes)]
        x = torch.cat(xs, 1) if len(xs) > 1 else xs[0]
        e = S.synth_input(f"d3.{name}.emb", (shapes[0][0], emb)) if emb else None
        y = m(x, e) if cls in ("UnetResBlock", "UnetBasicBlock") else m(x)
        out[f"{name}.y"] = y      # (inputs: synth_input of the names above, rebuilt by the tests)
    save("d3_blocks", **out)
    return keys


@torch.no_grad()
def case_unets():
    keys = {}
    out = {}
    for name, (strides, shape) in UNET_CASES.items():
        kw = unet_kwargs(strides)
        m = G.RefUNet(**G.ref_unet_kwargs(kw)).eval()
        S.synth_state_dict(m, f"d3.{name}.")
        keys[name] = keys_of(m)
        x = S.synth_input(f"d3.{name}.x", shape)
        t = torch.tensor([17, 503])
        c = torch.tensor([1, 0])
        y, _ = m(x, t, c)
        out.update({f"{name}.t": t, f"{name}.c": c, f"{name}.y": y})
    save("d3_unet", **out)
    return keys


@torch.no_grad()
def case_vae():
    kw = VAE_CASE
    m = G.ref_vae(kw).eval()
    S.synth_state_dict(m, "d3.vae.")
    img = S.synth_input("d3.vae.img", (2, 1, 16, 32, 32), 0.5)
    nz = S.PhiloxNoise(31)
    with um.patch.object(torch, "randn", side_effect=lambda shape, generator=None, device=None: nz(torch.empty(shape))):
        z = m.encode(img)
    zd = S.synth_input("d3.vae.z", (2, kw["emb_channels"], 2, 4, 4))
    x = m.decode(zd)
    save("d3_vae", z=z, seed=31, x_dec=x)     # (img, z_dec: synth_input of the names above)
    return {"vae": keys_of(m)}


@torch.no_grad()
def case_samples():
    sk = R.published_scheduler_kwargs()
    for name, (seed, steps, use_ddim, gs, cond, objective) in SAMPLE_CASES.items():
        kw = unet_kwargs([1, 2, 2, 2], in_ch=4)
        ref = RefPipeline(noise_scheduler=G.RefScheduler, noise_estimator=G.RefUNet, latent_embedder=None, noise_scheduler_kwargs=dict(sk),
                          noise_estimator_kwargs=G.ref_unet_kwargs(kw), estimator_objective=objective, clip_x0=False, do_input_centering=False)
        ref.eval()
        S.synth_state_dict(ref.noise_estimator, f"d3.{name}.unet.")
        n, size = 2, (4, 4, 8, 8)
        extra = {} if cond is None else dict(condition=torch.tensor(cond), guidance_scale=gs, un_cond=None)
        with um.patch.object(torch, "randn_like", side_effect=S.PhiloxNoise(seed)) as mk:
            img = ref.sample(n, size, steps=steps, use_ddim=use_ddim, **extra)
            draws = mk.call_count
        save(name, image=img, n=n, size=np.asarray(size), seed=seed, draws=draws)


if __name__ == "__main__":
    keys = {}
    keys.update(case_blocks())
    keys.update(case_unets())
    keys.update(case_vae())
    case_samples()
    (GOLD / "d3_keys.json").write_text(json.dumps(keys, indent=0))
    print("wrote tests/golden/d3_keys.json")
