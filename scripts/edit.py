#!/usr/bin/env python3
"""Counterfactual editing from a checkpoint: "these scans, as the model would draw them for class B".

A folder of PNG files goes to the device as bytes and becomes fp32 NCHW in [-1, 1] there (the ingress of scripts/img2img.py), runs through
`DiffusionPipeline.edit` -- encode -> DDIM inversion under the source label, recording the trajectory -> the deterministic sampler back down under
the target label -> decode; with --mask the kept region follows the recorded trajectory inside every iteration's solver launch and is composited
back in pixel space -- and leaves through the existing egress: one PNG per input, same file name, under --out; with --map-out also one
change-map PNG per input (mean over channels of |edited - input|, each map scaled to its own maximum).

  python scripts/edit.py --checkpoint runs/.../last.ckpt --images scans/ --out edited/ --target 1 --source 0 --guidance 4
  python scripts/edit.py --checkpoint runs/.../last.ckpt --images scans/ --labels labels.txt --target 1 --mask lesion.png --out edited/ --map-out maps/

--labels: a text file with one source label per PNG (in sorted file order) instead of one --source for all.  The mask PNG has the images' size;
non-zero pixels are REGENERATED, zero pixels kept.  Nothing is drawn but the encoder's sample (Philox key --seed).
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from img2img import _ChunkNoise, load_images, load_png
from medfusion_amd import DiffusionPipeline, ingest
from medfusion_amd.egress import AsyncImageWriter
from medfusion_amd.utils import add_guidance_arguments, guidance_kwargs

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--latent-embedder-ckpt", default=None, help="VAE checkpoint when the path baked into --checkpoint does not exist here")
    ap.add_argument("--images", required=True, help="folder of PNG files, all of one size")
    ap.add_argument("--mask", default=None, help="mask PNG of the images' size: non-zero = regenerate")
    ap.add_argument("--out", required=True)
    ap.add_argument("--map-out", default=None, help="folder for the change maps")
    ap.add_argument("--target", type=int, required=True, help="class label every image is redrawn under")
    ap.add_argument("--source", type=int, default=None, help="class label of every input (default: unconditional inversion)")
    ap.add_argument("--labels", default=None, help="text file: one source label per PNG, in sorted file order")
    ap.add_argument("--strength", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--guidance", type=float, default=1.0, help="guidance scale of the target pass")
    ap.add_argument("--source-guidance", type=float, default=1.0, help="guidance scale of the inversion")
    ap.add_argument("--sampler", default="ddim0", choices=["ddim0", "dpmpp2m"])
    ap.add_argument("--spacing", default=None, choices=["uniform", "logsnr"])
    add_guidance_arguments(ap)      # (of the target pass; the threshold holds for the inversion too)
    ingest.add_ingest_arguments(ap)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    device = torch.device("cuda")
    ckpt_kw = {"latent_embedder_checkpoint": args.latent_embedder_ckpt} if args.latent_embedder_ckpt else {}
    pipeline = DiffusionPipeline.load_from_checkpoint(args.checkpoint, **ckpt_kw).to(device).eval()
    emb = pipeline.latent_embedder
    channels = 3 if emb is None else getattr(emb, "out_channels", 3)
    files = ingest.list_images(args.images, args.ext)
    if not files:
        raise SystemExit(f"no {'PNG' if args.ext is None else '/'.join(args.ext)} files in {args.images}")
    labels = None
    if args.labels:
        labels = [int(v) for v in Path(args.labels).read_text().split()]
        if len(labels) != len(files):
            raise SystemExit(f"{args.labels}: {len(labels)} labels for {len(files)} PNG files")
    elif args.source is not None:
        labels = [args.source] * len(files)
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    mask = None
    if args.mask:
        mask = ingest.load_mask(args.mask, device, args, loader=load_png)                         # uint8 [1, 1, H, W]
    writer = AsyncImageWriter(device, normalize_each=False)
    map_writer = None
    if args.map_out:
        Path(args.map_out).mkdir(parents=True, exist_ok=True)
        map_writer = AsyncImageWriter(device, normalize_each=True)
    for lo in range(0, len(files), args.batch):
        chunk = files[lo:lo + args.batch]
        x = load_images(chunk, channels, device, args)
        n = x.shape[0]
        res = pipeline.edit(x, torch.full((n,), args.target, device=device),
                            source_condition=None if labels is None else torch.tensor(labels[lo:lo + n], device=device), strength=args.strength,
                            steps=args.steps, sampler=args.sampler, spacing=args.spacing, guidance_scale=args.guidance,
                            source_guidance_scale=args.source_guidance, un_cond=None, mask=None if mask is None else mask.expand(n, -1, -1, -1).contiguous(),
                            composite=mask is not None, return_map=map_writer is not None, encode_noise=_ChunkNoise(args.seed, lo, len(files)),
                            **guidance_kwargs(args))
        if map_writer is not None:
            res, cmap = res
            map_writer.submit(cmap, [Path(args.map_out) / f.name for f in chunk])
        writer.submit(res, [out / f.name for f in chunk])
    count = writer.close()
    if map_writer is not None:
        map_writer.close()
    print(f"wrote {count} images to {out}")
