#!/usr/bin/env python3
"""ORACLE -- TEST INFRASTRUCTURE ONLY (build container only; needs /root/reference).

Writes a checkpoint pair with the LAYOUT of a real Medfusion run, produced by the reference's own classes:
  tests/golden/ckpt/runs/tiny_vae/last_vae.ckpt     VAE.save (hyper_parameters captured by save_hyperparameters(), model_base.py:15,98)
  tests/golden/ckpt/runs/tiny_diffusion/last.ckpt   DiffusionPipeline with `latent_embedder=VAE, latent_embedder_checkpoint='runs/tiny_vae/last_vae.ckpt'`
                                                    (a path RELATIVE to the training cwd, like scripts/train_diffusion.py:114), use_ema=True with
                                                    EMA weights that differ from the live ones (diffusion_pipeline.py:57-60, 70-74)
and tests/golden/ckpt_sample.npz: what the reference samples from that checkpoint (EMA weights and live weights) with injected noise.
The pipeline checkpoint is committed as last.ckpt.npz, its compact byte-exact form (oracle/ckpt_fixture.py).
The hyper-parameters hold reference CLASS objects pickled by reference (medical_diffusion.models...), torch.optim.AdamW, torch.nn.L1Loss:
exactly what the product's Lightning-free reader (medfusion_amd/checkpoint.py) has to cope with.

Run:  python oracle/gen_ckpt_fixture.py      (from the repo root)
"""
from __future__ import annotations

import os
import sys
import unittest.mock as um
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle" / "shims"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, str(ROOT))

import numpy as np
import torch

torch.set_num_threads(1)

from oracle import restate as R
from oracle import synth as S
from medical_diffusion.models.pipelines import DiffusionPipeline as RefPipeline
from medical_diffusion.models.estimators import UNet as RefUNet
from medical_diffusion.models.noise_schedulers import GaussianNoiseScheduler as RefScheduler
from medical_diffusion.models.embedders.latent_embedders import VAE as RefVAE
from medical_diffusion.models.embedders import LabelEmbedder as RefLabel, TimeEmbbeding as RefTime

OUT = ROOT / "tests" / "golden" / "ckpt"


@torch.no_grad()
def main():
    (OUT / "runs" / "tiny_vae").mkdir(parents=True, exist_ok=True)
    (OUT / "runs" / "tiny_diffusion").mkdir(parents=True, exist_ok=True)
    os.chdir(OUT)  # the baked VAE path is relative to the "training" cwd
    vae_kw = dict(in_channels=3, out_channels=3, emb_channels=8, spatial_dims=2, hid_chs=[32, 32, 32, 32], kernel_sizes=[3, 3, 3, 3],
                  strides=[1, 2, 2, 2], deep_supervision=1, use_attention="none", perceiver=None, loss=torch.nn.MSELoss, loss_kwargs={},
                  embedding_loss_weight=1e-6)
    vae = RefVAE(**vae_kw)
    S.synth_state_dict(vae, "ckpt.vae.")
    torch.save(vae.checkpoint_dict(epoch=7, global_step=1234), "runs/tiny_vae/last_vae.ckpt")

    unet_kw = dict(in_ch=8, out_ch=8, spatial_dims=2, hid_chs=[32, 32, 32, 32], kernel_sizes=[3, 3, 3, 3], strides=[1, 2, 2, 2], num_res_blocks=1,
                   time_embedder=RefTime, time_embedder_kwargs={"emb_dim": 64, "pos_embedder_kwargs": {}}, cond_embedder=RefLabel,
                   cond_embedder_kwargs={"emb_dim": 64, "num_classes": 3}, deep_supervision=False, use_res_block=True, use_attention="none")
    pipe = RefPipeline(noise_scheduler=RefScheduler, noise_estimator=RefUNet, latent_embedder=RefVAE,
                       noise_scheduler_kwargs=dict(R.published_scheduler_kwargs()), noise_estimator_kwargs=unet_kw,
                       latent_embedder_checkpoint="runs/tiny_vae/last_vae.ckpt", estimator_objective="x_T", clip_x0=False, use_ema=True,
                       do_input_centering=False)
    pipe.eval()
    S.synth_state_dict(pipe.noise_estimator, "ckpt.unet.")
    S.synth_state_dict(pipe.ema_model.averaged_model, "ckpt.ema.")          # EMA weights that differ from the live ones
    assert torch.equal(pipe.latent_embedder.state_dict()["outc.conv.weight"], vae.state_dict()["outc.conv.weight"])  # nested load worked
    hp = pipe.hparams
    assert hp["latent_embedder"] is RefVAE and hp["noise_estimator"] is RefUNet and hp["use_ema"] is True
    torch.save(pipe.checkpoint_dict(epoch=3, global_step=4321), "runs/tiny_diffusion/last.ckpt")

    # what the reference itself produces from the checkpoint (fresh load through its own classmethod)
    ref = RefPipeline.load_from_checkpoint("runs/tiny_diffusion/last.ckpt").eval()
    cond = torch.tensor([2, 0, 1])
    out = {}
    for tag, use_ema in (("ema", True), ("live", False)):
        ref.use_ema = use_ema
        with um.patch.object(torch, "randn_like", side_effect=S.PhiloxNoise(21)) as m:
            out[tag] = ref.sample(3, (8, 8, 8), steps=5, use_ddim=True, condition=cond, guidance_scale=1.0, un_cond=None)
            draws = m.call_count
    assert not torch.equal(out["ema"], out["live"])
    np.savez_compressed(ROOT / "tests" / "golden" / "ckpt_sample.npz", image_ema=out["ema"].numpy(), image_live=out["live"].numpy(),
                        condition=cond.numpy(), seed=21, steps=5, draws=draws)
    # the pipeline checkpoint is committed in its compact form (oracle/ckpt_fixture.py; tests/util.py:ckpt_runs rebuilds it byte for byte)
    from oracle import ckpt_fixture
    ckpt_fixture.pack(Path("runs/tiny_diffusion/last.ckpt"), Path("runs/tiny_diffusion/last.ckpt.npz"))
    os.remove("runs/tiny_diffusion/last.ckpt")
    for f in ("runs/tiny_vae/last_vae.ckpt", "runs/tiny_diffusion/last.ckpt.npz"):
        print(f, os.path.getsize(f) // 1024, "KiB")
    print("checkpoint fixture written; reference sampled it with EMA and live weights")


if __name__ == "__main__":
    main()
