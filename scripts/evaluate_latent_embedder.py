#!/usr/bin/env python3
"""Reconstruction quality of a latent embedder over a folder of images: MS-SSIM and MSE of embedder(x)[0].clamp(-1, 1) against x, the two
figures of the reference's evaluation driver that need no downloaded weights, computed on the device (medfusion_amd.metrics.ReconstructionMeter),
and -- given the trunk and linear-layer files -- its third figure, LPIPS (medfusion_amd.lpips).

A folder of PNG files of one size goes to the device as bytes and becomes fp32 NCHW in [-1, 1] there (mf_image_ingress_u8); every batch runs
through the embedder, both images are mapped to [0, 1], and the per-image MS-SSIM (the range of each pair as data range, relu-normalised -- what
the reference's per-image call computes) and MSE stay on the device until the end: the summary is the only host sync.

  python scripts/evaluate_latent_embedder.py --checkpoint runs/.../last_vae.ckpt --images reference_test/ --out results/metrics

Writes metrics_<time>.log (MS-SSIM: mean ± std, MSE: mean ± std, in the reference's wording) and metrics_<time>.json next to it.  LPIPS needs a
pretrained trunk: --lpips-net vgg|alex --lpips-trunk FILE --lpips-lin FILE take the torchvision state dict and the lpips package's linear-layer file from
disk (nothing is downloaded) and add `LPIPS Score: 1 - mean`; without them the log says so.  --synthetic builds the tiny test architecture with
seeded weights in place of a checkpoint (a smoke run)."""
import argparse
import json
import logging
import sys
from datetime import datetime
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

EMBEDDERS = ("VAE", "VQVAE", "VQGAN", "VAEGAN")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--checkpoint", default=None, help="checkpoint of the embedder")
    ap.add_argument("--embedder", default="VAE", choices=EMBEDDERS, help="class of the checkpoint")
    ap.add_argument("--synthetic", action="store_true", help="seeded weights on the tiny architecture instead of --checkpoint")
    ap.add_argument("--images", required=True, help="folder of PNG files, all of one size (sides of at least 176)")
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--max-samples", type=int, default=None, help="only the first N files (default: all)")
    ap.add_argument("--out", default="results/metrics", help="folder of the log and the JSON")
    ap.add_argument("--seed", type=int, default=0, help="Philox key of the draws a VAE / VAEGAN makes")
    from medfusion_amd.ingest import add_ingest_arguments
    add_ingest_arguments(ap)
    from medfusion_amd.lpips import add_lpips_arguments, net_from_args
    add_lpips_arguments(ap)
    args = ap.parse_args(argv)
    args.lpips = net_from_args(args, ap.error)
    if (args.checkpoint is None) == (not args.synthetic):
        ap.error("exactly one of --checkpoint and --synthetic")
    if args.batch < 1:
        ap.error("--batch: at least 1")
    if args.max_samples is not None and args.max_samples < 1:
        ap.error("--max-samples: at least 1")
    return args


def list_images(folder, max_samples=None, exts=None):
    """the files of a folder by name: *.png, or the extensions of --ext"""
    from medfusion_amd.ingest import list_images as ls
    files = ls(folder, exts)[slice(max_samples)]
    if not files:
        raise SystemExit(f"no {'PNG' if exts is None else '/'.join(exts)} files in {folder}")
    return files


def load_png(path, channels):
    import numpy as np
    from PIL import Image
    arr = np.asarray(Image.open(path).convert("L" if channels == 1 else "RGB"), dtype=np.uint8)
    return arr[..., None] if arr.ndim == 2 else arr


def load_batch(files, channels, device, args=None):
    """PNG files -> fp32 [n, C, H, W] in [-1, 1] on the device; with --resize / --crop (args): files of any sizes through the data set's transform
    (medfusion_amd.ingest)"""
    from medfusion_amd import ingest
    if args is not None and ingest.ingest_requested(args):
        return ingest.load_batch(files, channels, device, args)
    import numpy as np
    import torch

    from medfusion_amd import kernels as K
    arrs = [load_png(f, channels) for f in files]
    if len({a.shape for a in arrs}) != 1:
        raise SystemExit(f"the images are not of one size: {sorted({a.shape for a in arrs})}")
    return K.image_ingress(torch.from_numpy(np.stack(arrs)).to(device))


def build_embedder(args):
    import medfusion_amd as M
    cls = getattr(M, args.embedder)
    if not args.synthetic:
        from medfusion_amd.checkpoint import load_module_from_checkpoint
        return load_module_from_checkpoint(cls, args.checkpoint)
    from oracle import synth as S
    kw = dict(in_channels=3, out_channels=3, emb_channels=4, spatial_dims=2, hid_chs=[32, 32, 64, 64], kernel_sizes=[3, 3, 3, 3], strides=[1, 2, 2, 2],
              deep_supervision=0, use_attention="none")
    if args.embedder in ("VQVAE", "VQGAN"):
        kw["num_embeddings"] = 256
    model = cls(**kw)
    S.synth_state_dict(model, f"evaluate.{args.embedder}.")
    return model.eval()


def main(argv=None):
    args = parse_args(argv)
    import torch

    from medfusion_amd import PhiloxDeviceNoise, ReconstructionMeter

    class FolderNoise(PhiloxDeviceNoise):
        """the rows of one batch at their offset in the whole folder (Philox draws depend on the global sample index: the result does not depend on --batch)"""
        offset = 0

        def begin(self, local_batch, device, sample_offset=0, global_batch=None):
            super().begin(local_batch, device, sample_offset + self.offset, global_batch)

    device = torch.device("cuda")
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    stamp = datetime.now().strftime("%Y_%m_%d_%H%M%S")
    logger = logging.getLogger("evaluate_latent_embedder")
    logger.setLevel(logging.INFO)
    logger.addHandler(logging.StreamHandler(sys.stdout))
    logger.addHandler(logging.FileHandler(out / f"metrics_{stamp}.log", "w"))

    files = list_images(args.images, args.max_samples, args.ext)
    logger.info(f"Samples Real: {len(files)}")
    model = build_embedder(args).to(device).eval()
    channels = getattr(model, "in_channels", None) or 3
    noise = FolderNoise(args.seed)
    meter = ReconstructionMeter(model, noise=noise, lpips=args.lpips)
    for lo in range(0, len(files), args.batch):
        noise.offset = lo
        meter.update(load_batch(files[lo:lo + args.batch], channels, device, args))
    res = meter.compute()
    if args.lpips is None:
        logger.info("LPIPS: not built (needs VGG weights)")
    else:
        logger.info(f"LPIPS Score: {res['lpips_score']}")
    logger.info(f"MS-SSIM: {res['ms_ssim_mean']} ± {res['ms_ssim_std']}")
    logger.info(f"MSE: {res['mse_mean']} ± {res['mse_std']}")
    res.update(images=str(args.images), checkpoint=args.checkpoint, embedder=args.embedder, synthetic=args.synthetic, lpips=None)
    if args.lpips is not None:
        res.update(lpips=res["lpips_score"], lpips_net=args.lpips_net)
    (out / f"metrics_{stamp}.json").write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main()
