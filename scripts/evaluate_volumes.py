#!/usr/bin/env python3
"""Reconstruction quality of a 3-D latent embedder over a folder of volumes, and / or the diversity of the folder: MS-SSIM and MSE of
embedder(x)[0].clamp(-1, 1) against x (medfusion_amd.VolumeReconstructionMeter) and the mean pairwise MS-SSIM of the set
(medfusion_amd.pairwise_ms_ssim3d), computed on the device with the volume metric of README "Metrics, volumes".

--volumes is a folder of .npy / .pt files, each one volume [C, D, H, W] or [D, H, W], all of one shape, with values in [-1, 1] (the default) or,
with --unit-range, in [0, 1].  With --checkpoint every batch runs through the embedder (a 3-D VAE), both volumes are mapped to [0, 1], and the
per-volume MS-SSIM (the range of each pair as data range, relu-normalised) and MSE stay on the device until the end.  With --pairs N the folder
becomes one bank in [0, 1] and N distinct unordered pairs are drawn by a seeded host generator (fewer possible pairs: all of them).  The pyramid is
--scales levels of --kernel-size taps: min(D, H, W) // 2^(scales - 1) >= kernel size, so the published 64 x 128 x 128 volume takes 3 scales of
11 taps (the default) or 4 of 7.

  python scripts/evaluate_volumes.py --checkpoint runs/.../last_vae3d.ckpt --volumes scans_test/ --out results/metrics3d
  python scripts/evaluate_volumes.py --volumes generated_volumes/ --pairs 1000 --seed 0

Writes metrics3d_<time>.log (MS-SSIM: mean ± std, MSE: mean ± std) and metrics3d_<time>.json next to it.  NIfTI / DICOM files are not read."""
import argparse
import json
import logging
import sys
from datetime import datetime
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--checkpoint", default=None, help="checkpoint of a 3-D VAE: reconstruction MS-SSIM / MSE")
    ap.add_argument("--volumes", required=True, help="folder of .npy / .pt files, one [C, D, H, W] or [D, H, W] volume each, all of one shape")
    ap.add_argument("--unit-range", action="store_true", help="the files hold values in [0, 1] (default: in [-1, 1])")
    ap.add_argument("--scales", type=int, default=3, help="levels of the pyramid, 1 .. 5 (weights betas_for(scales))")
    ap.add_argument("--kernel-size", type=int, default=11, help="taps of the window per axis: odd, 3 .. 11")
    ap.add_argument("--batch", type=int, default=2, help="volumes per pass through the embedder")
    ap.add_argument("--max-samples", type=int, default=None, help="only the first N files (default: all)")
    ap.add_argument("--pairs", type=int, default=None, help="also / only the pairwise MS-SSIM of the set over this many distinct random pairs")
    ap.add_argument("--seed", type=int, default=0, help="Philox key of the draws a VAE makes; seed of the pair draw")
    ap.add_argument("--out", default="results/metrics3d", help="folder of the log and the JSON")
    from medfusion_amd.lpips import add_lpips_arguments, net_from_args
    add_lpips_arguments(ap)
    args = ap.parse_args(argv)
    args.lpips = net_from_args(args, ap.error)
    if args.lpips is not None and args.checkpoint is None:
        ap.error("--lpips-net: LPIPS is a figure of the reconstructions (--checkpoint)")
    if args.checkpoint is None and args.pairs is None:
        ap.error("at least one of --checkpoint (reconstruction) and --pairs (diversity)")
    if not 1 <= args.scales <= 5:
        ap.error("--scales: 1 .. 5")
    if args.kernel_size < 3 or args.kernel_size > 11 or args.kernel_size % 2 == 0:
        ap.error("--kernel-size: odd, 3 .. 11")
    if args.batch < 1:
        ap.error("--batch: at least 1")
    if args.max_samples is not None and args.max_samples < 1:
        ap.error("--max-samples: at least 1")
    if args.pairs is not None and args.pairs < 1:
        ap.error("--pairs: at least 1")
    return args


def list_volumes(folder, max_samples=None):
    files = sorted(f for f in Path(folder).iterdir() if f.suffix in (".npy", ".pt"))[slice(max_samples)] if Path(folder).is_dir() else []
    if not files:
        raise SystemExit(f"no .npy or .pt files in {folder}")
    return files


def load_volume(path, unit_range: bool):
    """one file -> fp32 [C, D, H, W] in [-1, 1] on the host"""
    import numpy as np
    import torch
    v = torch.from_numpy(np.load(path)) if Path(path).suffix == ".npy" else torch.load(path, map_location="cpu")
    if not isinstance(v, torch.Tensor) or v.dim() not in (3, 4):
        raise SystemExit(f"{Path(path).name}: a [C, D, H, W] or [D, H, W] array, got {tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__}")
    v = v.to(torch.float32)
    v = v[None] if v.dim() == 3 else v
    return v * 2 - 1 if unit_range else v


def load_batch(files, unit_range: bool, device):
    import torch
    vols = [load_volume(f, unit_range) for f in files]
    if len({tuple(v.shape) for v in vols}) != 1:
        raise SystemExit(f"the volumes are not of one shape: {sorted({tuple(v.shape) for v in vols})}")
    return torch.stack(vols).to(device)


def report_pairs(values, pairs: int, volumes: int) -> dict:
    """mean ± std of the per-pair values (one copy to the host)"""
    import torch
    stats = torch.stack([values.mean(), torch.std(values) if values.numel() > 1 else values.new_zeros(())]).tolist()
    return {"ms_ssim_pairwise_mean": stats[0], "ms_ssim_pairwise_std": stats[1], "pairs": pairs, "volumes": volumes}


def main(argv=None):
    args = parse_args(argv)
    import torch

    import medfusion_amd as M

    class FolderNoise(M.PhiloxDeviceNoise):
        """the rows of one batch at their offset in the whole folder (Philox draws depend on the global sample index: the result does not depend on --batch)"""
        offset = 0

        def begin(self, local_batch, device, sample_offset=0, global_batch=None):
            super().begin(local_batch, device, sample_offset + self.offset, global_batch)

    device = torch.device("cuda")
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    stamp = datetime.now().strftime("%Y_%m_%d_%H%M%S")
    logger = logging.getLogger("evaluate_volumes")
    logger.setLevel(logging.INFO)
    logger.addHandler(logging.StreamHandler(sys.stdout))
    logger.addHandler(logging.FileHandler(out / f"metrics3d_{stamp}.log", "w"))

    files = list_volumes(args.volumes, args.max_samples)
    logger.info(f"Samples Real: {len(files)}")
    betas = M.betas_for(args.scales)
    res = dict(volumes_folder=str(args.volumes), checkpoint=args.checkpoint, scales=args.scales, kernel_size=args.kernel_size, seed=args.seed)
    if args.checkpoint is not None:
        from medfusion_amd.checkpoint import load_module_from_checkpoint
        model = load_module_from_checkpoint(M.VAE, args.checkpoint).to(device).eval()
        noise = FolderNoise(args.seed)
        meter = M.VolumeReconstructionMeter(model, noise=noise, betas=betas, kernel_size=args.kernel_size, lpips=args.lpips)
        for lo in range(0, len(files), args.batch):
            noise.offset = lo
            meter.update(load_batch(files[lo:lo + args.batch], args.unit_range, device))
        res.update(meter.compute())
        logger.info(f"MS-SSIM: {res['ms_ssim_mean']} ± {res['ms_ssim_std']}")
        logger.info(f"MSE: {res['mse_mean']} ± {res['mse_std']}")
        if args.lpips is not None:
            logger.info(f"LPIPS Score: {res['lpips_score']}")
    if args.pairs is not None:
        if len(files) < 2:
            raise SystemExit(f"{args.volumes}: at least two volumes make a pair")
        bank = torch.cat([(load_batch(files[lo:lo + args.batch], args.unit_range, device) + 1) / 2 for lo in range(0, len(files), args.batch)])
        n = bank.shape[0]
        values, index = M.pairwise_ms_ssim3d(bank, None if args.pairs >= n * (n - 1) // 2 else args.pairs, seed=args.seed, betas=betas,
                                            kernel_size=args.kernel_size)
        res.update(report_pairs(values, int(index.shape[0]), n))
        logger.info(f"MS-SSIM (pairwise, {res['pairs']} pairs of {res['volumes']} volumes): {res['ms_ssim_pairwise_mean']} ± {res['ms_ssim_pairwise_std']}")
    (out / f"metrics3d_{stamp}.json").write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main()
