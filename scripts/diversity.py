#!/usr/bin/env python3
"""Diversity of a generated set: the mean ± std of the MS-SSIM between randomly paired images of a folder (the paper's diversity figure: LOWER is
more diverse), computed on the device (medfusion_amd.metrics.pairwise_ms_ssim).

The folder's PNG files (one size, sides of at least 176) become ONE bank of fp32 images in [0, 1] on the device; one pyramid per image is built,
--pairs distinct unordered pairs are drawn without replacement by a seeded host generator, and every scale of all pairs is one launch.  The
summary is the only host sync.

  python scripts/diversity.py --images generated_diffusion3_150/Cardiomegaly --pairs 1000 --seed 0"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", required=True, help="folder of PNG files, all of one size")
    ap.add_argument("--pairs", type=int, default=1000, help="distinct unordered pairs to draw (at most N (N - 1) / 2; fewer files: all pairs)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-samples", type=int, default=None, help="only the first N files (default: all)")
    ap.add_argument("--batch", type=int, default=256, help="files per host-to-device copy")
    from medfusion_amd.ingest import add_ingest_arguments
    add_ingest_arguments(ap)
    args = ap.parse_args(argv)
    if args.pairs < 1:
        ap.error("--pairs: at least 1")
    if args.batch < 1:
        ap.error("--batch: at least 1")
    if args.max_samples is not None and args.max_samples < 2:
        ap.error("--max-samples: at least 2 images make a pair")
    return args


def report(values, pairs: int, images: int) -> dict:
    """mean ± std of the per-pair values (one copy to the host)"""
    import torch
    stats = torch.stack([values.mean(), torch.std(values) if values.numel() > 1 else values.new_zeros(())]).tolist()
    return {"ms_ssim_pairwise_mean": stats[0], "ms_ssim_pairwise_std": stats[1], "pairs": pairs, "images": images}


def diversity(bank01, pairs: int, seed: int) -> dict:
    """bank01: fp32 [N, C, H, W] in [0, 1] on the device"""
    from medfusion_amd import pairwise_ms_ssim
    n = bank01.shape[0]
    total = n * (n - 1) // 2
    values, index = pairwise_ms_ssim(bank01, None if pairs >= total else pairs, seed=seed)
    return report(values, int(index.shape[0]), n)


def main(argv=None):
    args = parse_args(argv)
    import torch

    from evaluate_latent_embedder import list_images, load_batch
    device = torch.device("cuda")
    files = list_images(args.images, args.max_samples, args.ext)
    if len(files) < 2:
        raise SystemExit(f"{args.images}: at least two images make a pair")
    bank = torch.cat([(load_batch(files[lo:lo + args.batch], 3, device, args) + 1) / 2 for lo in range(0, len(files), args.batch)])
    res = diversity(bank, args.pairs, args.seed)
    print(f"MS-SSIM (pairwise, {res['pairs']} pairs of {res['images']} images): {res['ms_ssim_pairwise_mean']} ± {res['ms_ssim_pairwise_std']}")
    print(json.dumps(dict(res, images_folder=str(args.images), seed=args.seed)))
    return res


if __name__ == "__main__":
    main()
