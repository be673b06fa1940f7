#!/usr/bin/env python3
"""Writes tests/golden/vq_*.npz and tests/golden/vq_keys.json from the REAL reference's VQVAE / VQGAN / VAEGAN (latent_embedders.py), reached
through oracle/shims like oracle/gen_golden.py, after asserting that the test-side restatement (tests/vq_restate.py) equals the reference bit for
bit on every case.  Needs the reference checkout (REF below); the fixtures are data only.

Run from the repository root:  python scripts/gen_vq_golden.py [reference root]
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

from medical_diffusion.models.embedders.latent_embedders import VAEGAN as RefVAEGAN, VQGAN as RefVQGAN, VQVAE as RefVQVAE
from medical_diffusion.models.pipelines import DiffusionPipeline as RefPipeline

from oracle import gen_golden as G
from oracle import restate as R
from oracle import synth as S
from tests import vq_restate as V

GOLD = ROOT / "tests" / "golden"
MARGIN = 1e-3
TRAIN_ONLY = dict(perceiver=None)


def ref_model(cls, kw):
    return cls(**kw, **TRAIN_ONLY).eval()


def synth_pair(ref, ora, prefix):
    """same weights on both (the restatement has no discriminator: its keys are the reference's minus `discriminator.`)"""
    S.synth_state_dict(ref, prefix)
    S.synth_state_dict(ora, prefix)
    rs = {k: v for k, v in ref.state_dict().items() if not k.startswith("discriminator.")}
    os_ = ora.state_dict()
    assert list(rs) == list(os_), set(rs) ^ set(os_)
    for k in rs:
        assert torch.equal(rs[k], os_[k]), k


def margined_latent(name, codebook, shape):
    """z [N,C,H,W] near codebook rows, every pixel's best and second-best fp64 distances apart by >= MARGIN relative"""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    n, c, h, w = shape
    out = torch.empty((n * h * w, c))
    for p in range(n * h * w):
        for _ in range(1000):
            k = int(torch.randint(codebook.shape[0], (1,), generator=g))
            cand = codebook[k] + 0.05 * torch.randn(c, generator=g)
            if float(V.exact_margins(cand.view(1, c, 1, 1), codebook)[0]) >= MARGIN:
                out[p] = cand
                break
        else:
            raise RuntimeError("no margined latent")
    return torch.moveaxis(out.view(n, h, w, c), -1, 1).contiguous()


def check_equal(name, a, b):
    G.check_equal(name, a, b)


def save(name, **arrs):
    G.save(name, **arrs)


@torch.no_grad()
def case_keys():
    out = {}
    for tag, cls, kw in (("VQVAE_tiny", RefVQVAE, V.tiny_vq_kwargs()), ("VQGAN_tiny", RefVQGAN, V.tiny_vq_kwargs(num_embeddings=1000, emb_channels=8)),
                         ("VAEGAN_tiny", RefVAEGAN, V.tiny_vaegan_kwargs()), ("VQVAE_default", RefVQVAE, {}), ("VQGAN_default", RefVQGAN, {}),
                         ("VAEGAN_default", RefVAEGAN, {})):
        m = ref_model(cls, kw)
        out[tag] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        print(f"  {tag}: {len(out[tag])} tensors")
    (GOLD / "vq_keys.json").write_text(json.dumps({"kwargs": {"VQVAE_tiny": V.tiny_vq_kwargs(), "VQGAN_tiny": V.tiny_vq_kwargs(num_embeddings=1000, emb_channels=8),
                                                               "VAEGAN_tiny": V.tiny_vaegan_kwargs()}, "keys": out}, indent=0))


def quantizer_of(m):
    return (m.vqvae if hasattr(m, "vqvae") else m).quantizer


@torch.no_grad()
def vq_case(name, ref_cls, ora_cls, kw, prefix, img_names):
    ref, ora = ref_model(ref_cls, kw), ora_cls(**kw).eval()
    synth_pair(ref, ora, prefix)
    q = quantizer_of(ref)
    cb = q.embedder.weight.detach().clone()
    # decode of a margined latent
    z = margined_latent(name, cb, (2, kw["emb_channels"], 4, 4))
    xa, xb = ref.decode(z), ora.decode(z)
    check_equal(f"{name} decode", xa, xb)
    idx_dec = V.VectorQuantizer.indices(quantizer_of(ora), z)
    check_equal(f"{name} decode idx", torch.argmin(_ref_dist(q, z), dim=1), idx_dec)
    # forward of an image whose encoder output is margined (first image name that gives one)
    for img_name in img_names:
        img = S.synth_input(img_name, (2, 3, 32, 32), 0.5)
        ze = ref.encode(img)
        check_equal(f"{name} encode", ze, ora.encode(img))
        m = float(V.exact_margins(ze, cb).min())
        if m >= MARGIN:
            break
        print(f"  {name}: {img_name} has a fp64 margin {m:.1e}: next image")
    else:
        raise RuntimeError(f"{name}: no margined image")
    oa, ha, la = ref(img)
    ob, hb, lb = ora(img)
    check_equal(f"{name} forward out", oa, ob)
    assert len(ha) == len(hb) == 2
    for i in range(2):
        check_equal(f"{name} forward hor{i}", ha[i], hb[i])
    check_equal(f"{name} emb_loss", la.reshape(1), lb.reshape(1))
    idx_fwd = V.VectorQuantizer.indices(quantizer_of(ora), ze)
    save(name, z=z, x_dec=xa, idx_dec=idx_dec.int(), img=img, z_enc=ze, out=oa, hor0=ha[0], hor1=ha[1], emb_loss=la.reshape(1),
         idx_fwd=idx_fwd.int(), margin_dec=float(V.exact_margins(z, cb).min()), margin_fwd=m)


def _ref_dist(q, z):
    """the reference's own distance matrix, recomputed by calling its forward with argmin captured"""
    got = {}
    real = torch.argmin

    def spy(d, dim=None):
        got["d"] = d
        return real(d, dim=dim)

    with um.patch.object(torch, "argmin", side_effect=spy):
        q(z)
    return got["d"]


@torch.no_grad()
def case_vaegan():
    kw = V.tiny_vaegan_kwargs()
    ref, ora = ref_model(RefVAEGAN, kw), V.VAEGAN(**kw).eval()
    synth_pair(ref, ora, "vaegan_tiny.")
    z = S.synth_input("vaegan_z", (2, 4, 4, 4))
    xa, xb = ref.decode(z), ora.decode(z)
    check_equal("vaegan decode", xa, xb)
    img = S.synth_input("vaegan_img", (2, 3, 32, 32), 0.5)
    nz = S.PhiloxNoise(17)
    with um.patch.object(torch, "randn", side_effect=lambda shape, generator=None, device=None: nz(torch.empty(shape))):
        oa, ha, ka = ref(img)
    nz2 = S.PhiloxNoise(17)
    ora.vqvae.quantizer.noise_fn = lambda shape, device: nz2(torch.empty(shape))
    ob, hb, kb = ora(img)
    check_equal("vaegan forward out", oa, ob)
    for i in range(2):
        check_equal(f"vaegan forward hor{i}", ha[i], hb[i])
    check_equal("vaegan kl", ka.reshape(1), kb.reshape(1))
    save("vq_vaegan_tiny", z=z, x_dec=xa, img=img, out=oa, hor0=ha[0], hor1=ha[1], emb_loss=ka.reshape(1), seed=17)


@torch.no_grad()
def case_pipeline():
    """a tiny DiffusionPipeline whose latent embedder is a VQGAN: the reference's sample() (images) and the latents it decodes"""
    ukw = R.tiny_unet_kwargs(None, "none", in_ch=4, out_ch=4)
    vkw = V.tiny_vq_kwargs(num_embeddings=1000, deep_supervision=0)
    sk = R.published_scheduler_kwargs()
    ref = RefPipeline(noise_scheduler=G.RefScheduler, noise_estimator=G.RefUNet, latent_embedder=None, noise_scheduler_kwargs=dict(sk),
                      noise_estimator_kwargs=G.ref_unet_kwargs(ukw), estimator_objective="x_T", clip_x0=False, do_input_centering=False)
    ref.latent_embedder = ref_model(RefVQGAN, vkw)
    ora = R.DiffusionPipeline(R.GaussianNoiseScheduler(**sk), R.UNet(**ukw), V.VQGAN(**vkw), estimator_objective="x_T", clip_x0=False)
    ref.eval(), ora.eval()
    G.synth_pair(ref.noise_estimator, ora.noise_estimator, "vq_pipe.unet.")
    synth_pair(ref.latent_embedder, ora.latent_embedder, "vq_pipe.vqgan.")
    seed, n, size, steps = 21, 2, (4, 8, 8), 4
    with um.patch.object(torch, "randn_like", side_effect=S.PhiloxNoise(seed)) as mk:
        ia = ref.sample(n, size, steps=steps, use_ddim=True)
        draws = mk.call_count
    emb = ora.latent_embedder
    ora.latent_embedder = None
    ora.set_noise_fn(S.PhiloxNoise(seed))
    lat = ora.sample(n, size, steps=steps, use_ddim=True)
    ora.latent_embedder = emb
    check_equal("vq pipeline image", ia, emb.decode(lat))
    cb = emb.vqvae.quantizer.embedder.weight.detach()
    save("vq_pipeline_tiny", image=ia, latents=lat, idx=V.VectorQuantizer.indices(emb.vqvae.quantizer, lat).int(), n=n, size=np.asarray(size),
         steps=steps, seed=seed, draws=draws, margin=float(V.exact_margins(lat, cb).min()))


if __name__ == "__main__":
    case_keys()
    vq_case("vq_vqvae_tiny", RefVQVAE, V.VQVAE, V.tiny_vq_kwargs(), "vqvae_tiny.", [f"vqvae_img{i}" for i in range(20)])
    vq_case("vq_vqgan_tiny", RefVQGAN, V.VQGAN, V.tiny_vq_kwargs(num_embeddings=1000, emb_channels=8), "vqgan_tiny.", [f"vqgan_img{i}" for i in range(20)])
    case_vaegan()
    case_pipeline()
    big = [p for p in GOLD.glob("vq_*") if p.stat().st_size > (1 << 20)]
    assert not big, big
    print("all vq cases: restatement == reference")
