#!/usr/bin/env python3
"""Image-conditioned sampling from a checkpoint: variations of given images at a chosen strength (img2img) and, with --mask, inpainting.

A folder of PNG files goes to the device as bytes, becomes fp32 NCHW in [-1, 1] there (mf_image_ingress_u8: (x / 255 - 0.5) / 0.5, the
normalisation of the reference's scripts/evaluate_latent_embedder.py), runs through `DiffusionPipeline.sample_from` (encode -> estimate_x_t -> the
last strength * steps iterations of the loop -> decode; with a mask the kept region is re-imposed inside every iteration's scheduler launch and
composited back in pixel space) and leaves through the existing egress (clip -> uint8 -> channel-last on the device, asynchronous copy, writer
thread): one PNG per input, same file name, under --out.

  python scripts/img2img.py --checkpoint runs/.../last.ckpt --images scans/ --out variations/ --strength 0.5
  python scripts/img2img.py --checkpoint runs/.../last.ckpt --images scans/ --mask lesion.png --out inpainted/ --strength 1.0 --condition 0

The mask PNG has the images' size; non-zero pixels are REGENERATED, zero pixels kept (a latent cell is regenerated if any of its pixels is).
Draws: #0 diffuses the encoded image, then the loop's draws as in sample() (Philox key --seed; the encoder's draw uses key --seed + 1).
--sampler ddim0 | dpmpp2m (with --spacing logsnr: fewer iterations for the same solver accuracy) runs the loop deterministically: draw #0 only.
--sampler ddim1 | dpmpp2m_sde (the latter meant for --spacing logsnr) keeps the loop stochastic at few steps: one more draw per non-final iteration.
--window H W (latent cells) [--window-stride ...] [--window-weight tent|uniform]: images larger than the trained size -- the estimator runs on
overlapping windows of the trained size, everything else on the whole latent (DiffusionPipeline.sample_from(window=...)).
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from medfusion_amd import DiffusionPipeline, PhiloxDeviceNoise
from medfusion_amd import ingest
from medfusion_amd.egress import AsyncImageWriter
from medfusion_amd.utils import add_guidance_arguments, guidance_kwargs


class _ChunkNoise(PhiloxDeviceNoise):
    """the rows of one chunk of the folder at their offset in the whole folder's batch (Philox draws depend on the global sample index only)"""

    def __init__(self, seed, offset, total):
        super().__init__(seed)
        self.offset, self.total = offset, total

    def begin(self, local_batch, device, sample_offset=0, global_batch=None):
        super().begin(local_batch, device, sample_offset + self.offset, self.total)


def load_png(path, channels):
    from PIL import Image
    img = Image.open(path).convert("L" if channels == 1 else "RGB")
    arr = np.asarray(img, dtype=np.uint8)
    return arr[..., None] if arr.ndim == 2 else arr


def load_images(files, channels, device, args=None):
    """files -> [n, C, h, w] fp32 in [-1, 1] on the device: the bytes of equal-sized PNG files through mf_image_ingress_u8, or, with --resize /
    --crop, files of any sizes through the data set's transform (medfusion_amd.ingest: PIL-exact resize, centre crop, the same value map)"""
    return ingest.load_batch(files, channels, device, args, loader=load_png)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--latent-embedder-ckpt", default=None, help="VAE checkpoint when the path baked into --checkpoint does not exist here")
    ap.add_argument("--images", required=True, help="folder of PNG files, all of one size")
    ap.add_argument("--mask", default=None, help="mask PNG of the images' size: non-zero = regenerate")
    ap.add_argument("--out", required=True)
    ap.add_argument("--strength", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--guidance", type=float, default=1.0)
    ap.add_argument("--condition", type=int, default=None, help="class label for every image")
    ap.add_argument("--ddpm", action="store_true", help="the posterior loop instead of DDIM")
    ap.add_argument("--sampler", default=None, choices=["ddim0", "dpmpp2m", "ddim1", "dpmpp2m_sde"],
                    help="a few-step sampler in place of the reference's update: deterministic (ddim0, dpmpp2m) or stochastic (ddim1, dpmpp2m_sde)")
    ap.add_argument("--spacing", default=None, choices=["uniform", "logsnr"], help="timestep grid of --sampler (logsnr: uniform in log-SNR)")
    ap.add_argument("--window", type=int, nargs="+", default=None, help="windowed denoising: the trained extents, in latent cells (smaller than the images' latent)")
    ap.add_argument("--window-stride", type=int, nargs="+", default=None, help="stride of the windows per axis (default: half a window)")
    ap.add_argument("--window-weight", default="tent", choices=["tent", "uniform"], help="weights of the per-cell average over the windows")
    add_guidance_arguments(ap)
    ingest.add_ingest_arguments(ap)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save-tensor", action="store_true", help="also write result.pt: the fp32 images behind the PNG files")
    args = ap.parse_args()

    device = torch.device("cuda")
    ckpt_kw = {"latent_embedder_checkpoint": args.latent_embedder_ckpt} if args.latent_embedder_ckpt else {}
    pipeline = DiffusionPipeline.load_from_checkpoint(args.checkpoint, **ckpt_kw).to(device).eval()
    emb = pipeline.latent_embedder
    channels = 3 if emb is None else getattr(emb, "out_channels", 3)      # (the autoencoders of the reference reconstruct their input: same channels)
    files = ingest.list_images(args.images, args.ext)
    if not files:
        raise SystemExit(f"no {'PNG' if args.ext is None else '/'.join(args.ext)} files in {args.images}")
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    mask = None
    if args.mask:
        mask = ingest.load_mask(args.mask, device, args, loader=load_png)                         # uint8 [1, 1, H, W]

    writer = AsyncImageWriter(device, normalize_each=False)
    kept = []
    for lo in range(0, len(files), args.batch):
        chunk = files[lo:lo + args.batch]
        x = load_images(chunk, channels, device, args)
        n = x.shape[0]
        cond = None if args.condition is None else torch.full((n,), args.condition, device=device)
        # (one Philox key for the whole folder, the chunk's rows at their global offset: the result does not depend on --batch)
        res = pipeline.sample_from(x, args.strength, condition=cond, mask=None if mask is None else mask.expand(n, -1, -1, -1).contiguous(),
                                   steps=args.steps, use_ddim=not args.ddpm, guidance_scale=args.guidance, un_cond=None, composite=mask is not None,
                                   sampler=args.sampler, spacing=args.spacing, window=None if args.window is None else tuple(args.window),
                                   window_stride=None if args.window_stride is None else tuple(args.window_stride), window_weight=args.window_weight,
                                   noise=_ChunkNoise(args.seed, lo, len(files)), encode_noise=_ChunkNoise(args.seed + 1, lo, len(files)), **guidance_kwargs(args))
        writer.submit(res, [out / f.name for f in chunk])
        if args.save_tensor:
            kept.append(res.cpu())
    count = writer.close()
    if args.save_tensor:
        torch.save(torch.cat(kept), out / "result.pt")
    print(f"wrote {count} images to {out}")
