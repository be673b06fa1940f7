#!/usr/bin/env python3
"""The held-out denoising loss of a checkpoint: what the reference's Lightning loop logs as val/loss, val/L1, val/L2 and val/variance_loss, on a
folder of scans the model was not trained on -- to pick a checkpoint, compare EMA against raw weights, see at which noise levels the model is weak
and rank scans by how well the model explains them.

  python scripts/validate.py --checkpoint runs/.../last.ckpt --images heldout/ [--labels labels.txt] [--passes 4] [--ema | --no-ema] [--uncond]
  python scripts/validate.py --checkpoint runs/.../last.ckpt --images volumes/ --profile 20 --out val.json      (.npy / .pt volumes: the model's input as stored)
  python scripts/validate.py --plan [--batch 16 --passes 4 --profile 20]                                        (no device, no checkpoint: what would run)

A folder of PNG files goes to the device as bytes and becomes fp32 NCHW in [-1, 1] there (the ingress of scripts/img2img.py); a folder of .npy /
.pt files holds one fp32 [C, spatial...] input each.  Every pass draws a timestep per scan (torch's CPU generator, --seed) and a noise sample
(Philox, keyed by --seed and the pass) and runs DiffusionPipeline.validation_step through a ValidationMeter; the log gives mean +- std over the
passes and the per-timestep-bin table of all passes together.  --labels: a text file with one class label per file, in sorted file order
(otherwise, or with --uncond, the unconditional pass).  --profile [K]: additionally every scan at K log-SNR-spaced timesteps
(DiffusionPipeline.denoising_profile) and the per-scan scores sorted worst first.  A JSON with everything printed is written next to the log
(--out, default validate.json in the images' folder).
"""
import argparse
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(Path(__file__).resolve().parent))

KEYS = ("loss", "L1", "L2", "variance_loss")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--latent-embedder-ckpt", default=None, help="VAE checkpoint when the path baked into --checkpoint does not exist here")
    ap.add_argument("--images", default=None, help="folder of PNG files of one size, or of .npy / .pt volumes")
    ap.add_argument("--labels", default=None, help="text file: one class label per file, in sorted file order")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--passes", type=int, default=1, help="passes over the folder, each with its own timesteps and noise")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ema", dest="ema", action="store_true", default=None, help="evaluate the EMA weights (default: what the checkpoint says)")
    ap.add_argument("--no-ema", dest="ema", action="store_false", help="evaluate the raw weights")
    ap.add_argument("--uncond", action="store_true", help="ignore --labels: the unconditional pass")
    ap.add_argument("--loss", default="l1", choices=["l1", "l2"])
    ap.add_argument("--bins", type=int, default=10)
    ap.add_argument("--profile", type=int, nargs="?", const=20, default=None, metavar="K", help="per-scan loss at K log-SNR-spaced timesteps (default 20)")
    ap.add_argument("--out", default=None, help="the JSON (default: validate.json in --images)")
    from medfusion_amd.ingest import add_ingest_arguments
    add_ingest_arguments(ap)
    ap.add_argument("--plan", action="store_true", help="print what would run; touches no device and needs no checkpoint")
    a = ap.parse_args(argv)
    if a.batch < 1 or a.passes < 1 or a.bins < 1 or (a.profile is not None and a.profile < 1):
        ap.error("--batch, --passes, --bins and --profile are positive")
    if not a.plan and not (a.checkpoint and a.images):
        ap.error("--checkpoint and --images are required (or --plan)")
    return a


def plan_lines(a, files=None):
    n = "N" if files is None else str(files)
    lines = [f"{a.passes} passes over {n} scans in batches of {a.batch}: one estimator pass, one forward-process launch and the loss launches per batch; "
             f"{a.bins} timestep bins; one host sync per pass"]
    if a.profile is not None:
        lines.append(f"profile: every scan at {a.profile} timesteps (log-SNR spaced), one estimator pass per (timestep, batch); one host sync")
    return lines


def load_inputs(folder, channels, device, args=None):
    """-> (list of files, loader(chunk) -> fp32 device tensor [n, C, spatial...])"""
    import numpy as np
    import torch

    from medfusion_amd import kernels as K
    folder = Path(folder)
    from medfusion_amd import ingest
    files = ingest.list_images(folder, getattr(args, "ext", None))
    if files and args is not None and ingest.ingest_requested(args):      # files of any sizes through the data set's transform
        return files, lambda chunk: ingest.load_batch(chunk, channels, device, args)
    if files:
        from img2img import load_png
        return files, lambda chunk: K.image_ingress(torch.from_numpy(np.stack([load_png(f, channels) for f in chunk])).to(device))
    files = sorted(f for f in folder.iterdir() if f.suffix in (".npy", ".pt"))
    if not files:
        raise SystemExit(f"no PNG, .npy or .pt files in {folder}")
    one = lambda f: torch.from_numpy(np.load(f)) if f.suffix == ".npy" else torch.load(f, map_location="cpu")
    return files, lambda chunk: torch.stack([one(f).to(torch.float32) for f in chunk]).to(device).contiguous()


def mean_std(values):
    m = sum(values) / len(values)
    return m, math.sqrt(sum((v - m) ** 2 for v in values) / len(values))


def main(argv=None):
    a = parse_args(argv)
    if a.plan:
        print("\n".join(plan_lines(a)))
        return 0
    import torch

    from img2img import _ChunkNoise
    from medfusion_amd import DiffusionPipeline, ValidationMeter

    device = torch.device("cuda")
    ckpt_kw = {"latent_embedder_checkpoint": a.latent_embedder_ckpt} if a.latent_embedder_ckpt else {}
    pipe = DiffusionPipeline.load_from_checkpoint(a.checkpoint, **ckpt_kw).to(device).eval()
    if a.ema is not None:
        if a.ema and not hasattr(pipe, "ema_model"):
            raise SystemExit("--ema: the checkpoint holds no EMA weights")
        pipe.use_ema = a.ema
    emb = pipe.latent_embedder
    files, load = load_inputs(a.images, 3 if emb is None else getattr(emb, "in_channels", 3), device, a)
    labels = None
    if a.labels and not a.uncond:
        labels = [int(v) for v in Path(a.labels).read_text().split()]
        if len(labels) != len(files):
            raise SystemExit(f"{a.labels}: {len(labels)} labels for {len(files)} files")
    cond = lambda lo, n: None if labels is None else torch.tensor(labels[lo:lo + n], device=device)
    log = plan_lines(a, len(files)) + [f"checkpoint {a.checkpoint}: {'EMA' if pipe.use_ema else 'raw'} weights, objective {pipe.estimator_objective}, "
                                       f"{'labels' if labels is not None else 'unconditional'}"]
    torch.manual_seed(a.seed)
    total, per_pass = ValidationMeter(pipe, bins=a.bins, loss=a.loss), []
    for p in range(a.passes):
        meter = ValidationMeter(pipe, bins=a.bins, loss=a.loss)
        for lo in range(0, len(files), a.batch):
            x = load(files[lo:lo + a.batch])
            kw = dict(noise=_ChunkNoise(a.seed + 7919 * (p + 1), lo, len(files)), encode_noise=_ChunkNoise(a.seed, lo, len(files)))
            meter.update(x, cond(lo, x.shape[0]), **kw)
            total._rows += meter._rows[-1:]
            total._t += meter._t[-1:]
        per_pass.append(meter.compute())
    result = {"checkpoint": str(a.checkpoint), "images": str(a.images), "files": len(files), "passes": a.passes, "ema": bool(pipe.use_ema), "seed": a.seed}
    for k in KEYS:
        if k in per_pass[0]:
            m, s = mean_std([r[k] for r in per_pass])
            result[f"val/{k}"] = {"mean": m, "std": s, "passes": [r[k] for r in per_pass]}
            log.append(f"val/{k:14s} {m:.6g} +- {s:.3g} over {a.passes} passes")
    table = total.compute()["bins"]
    result["bins"] = table
    log.append("timestep bin        count " + " ".join(f"{k:>12s}" for k in KEYS if k in table))
    for i, c in enumerate(table["count"]):
        log.append(f"[{table['edges'][i]:5d}, {table['edges'][i + 1]:5d}) {c:8d} " + " ".join(f"{table[k][i]:12.6g}" for k in KEYS if k in table))
    if a.profile is not None:
        ts = pipe.noise_scheduler.loop_timesteps(a.profile, True, "logsnr")[0]
        scores, curve = [], None
        for lo in range(0, len(files), a.batch):
            x = load(files[lo:lo + a.batch])
            prof = pipe.denoising_profile(x, cond(lo, x.shape[0]), timesteps=ts, noise=_ChunkNoise(a.seed + 1, lo, len(files)), loss=a.loss)
            scores += prof["score"].tolist()
            curve = prof["loss"].sum(1) if curve is None else curve + prof["loss"].sum(1)
        order = sorted(range(len(files)), key=lambda i: -scores[i])
        result["profile"] = {"t": ts, "loss": (curve / len(files)).tolist(), "scores": [{"file": files[i].name, "score": scores[i]} for i in order]}
        log.append(f"profile over {len(ts)} timesteps: mean loss per timestep " + " ".join(f"{t}:{v:.4g}" for t, v in zip(ts, result["profile"]["loss"])))
        log.append("scans by score, worst first:")
        log += [f"  {scores[i]:.6g}  {files[i].name}" for i in order]
    print("\n".join(log))
    out = Path(a.out) if a.out else Path(a.images) / "validate.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1))
    print(f"wrote {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
