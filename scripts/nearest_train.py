#!/usr/bin/env python3
"""Copy audit of a generated set: for every generated sample its nearest training samples in a feature space, whether it is closer to the training
set than that training sample's own nearest neighbour (authenticity, Alaa et al. 2022) and how much closer than to its other neighbours (the copy
ratio, Carlini et al. 2023) -- medfusion_amd.memorization_report on the device, no N x M matrix.

Each of --train and --fake is a folder of PNG files of one size, or a .pt / .npy file of precomputed [N, D] features (as scripts/evaluate_images.py
reads them).  Folders need --features: embedder:CKPT[:pool] (or VQVAE:CKPT, VQGAN:CKPT, VAEGAN:CKPT) for the encoder of a latent embedder, or
`pixels` for the flattened pixels themselves (D = channels x H x W <= 65536: one channel of 256 x 256; --channels 1 or 3).

  python scripts/nearest_train.py --train data/train/ --fake generated/ --features pixels --out results/audit
  python scripts/nearest_train.py --train train_feats.pt --fake fake_feats.pt --neighbours 10 --top 32
  python scripts/nearest_train.py --plan --n-train 50000 --n-fake 10000 --d 2048          (no device: launches, splits, workspace)

Writes nearest_train.json -- the authenticity, the quantiles of the copy ratio, the --top most suspicious generated samples (smallest copy ratio
first; exact copies, whose ratio is 0 or 0 / 0, before all others) with their nearest training samples and distances -- and, for folders,
nearest_train.png: one row per listed sample, the generated image and its three nearest training images."""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(1, str(Path(__file__).resolve().parent))      # evaluate_images' and evaluate_latent_embedder's readers

SHEET_NEIGHBOURS = 3


def parse_args(argv=None):
    import evaluate_images as ev
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--train", help="the training set: folder of PNG files, or a .pt / .npy file of [N, D] features")
    ap.add_argument("--fake", help="the generated set, likewise")
    ap.add_argument("--features", default=None, help="embedder:CKPT[:pool] | pixels -- needed when a folder is given")
    ap.add_argument("--channels", type=int, default=1, choices=(1, 3), help="channels the PNG files are read with under --features pixels")
    ap.add_argument("--neighbours", type=int, default=10, help="training neighbours of the copy ratio (1 .. 16)")
    ap.add_argument("--top", type=int, default=32, help="how many of the most suspicious generated samples are listed")
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--max-samples", type=int, default=None)
    ap.add_argument("--out", default="results/audit", help="folder of the JSON and the contact sheet")
    from medfusion_amd.ingest import add_ingest_arguments
    add_ingest_arguments(ap)
    ap.add_argument("--plan", action="store_true", help="print launches, splits and workspace, touch no device")
    ap.add_argument("--n-train", type=int, default=50000, help="--plan: training rows")
    ap.add_argument("--n-fake", type=int, default=10000, help="--plan: generated rows")
    ap.add_argument("--d", type=int, default=2048, help="--plan: feature width")
    args = ap.parse_args(argv)
    if not 1 <= args.neighbours <= 16:
        ap.error("--neighbours: 1 .. 16")
    if args.top < 1 or args.batch < 1:
        ap.error("--top, --batch: at least 1")
    if args.plan:
        return args
    if not args.train or not args.fake:
        ap.error("--train and --fake are needed (or --plan)")
    if args.features is not None and args.features != "pixels":
        ev.parse_features(args.features)
    elif args.features is None and not (ev.is_feature_file(args.train) and ev.is_feature_file(args.fake)):
        ap.error("--features embedder:CKPT[:pool] | pixels is needed when --train or --fake is a folder of images")
    return args


def plan(n_train: int, n_fake: int, d: int, neighbours: int) -> dict:
    """the launches of memorization_report, their splits and the workspace, from the host-side planner alone"""
    from medfusion_amd import fidelity as F
    if not (F.nn_ok(n_train, n_fake, d, neighbours, 1) and F.nn_ok(n_train, n_train, d, 1, 1, True)):
        raise SystemExit(f"train {n_train} x fake {n_fake} x D {d}, neighbours {neighbours}: outside the rules of the neighbour search "
                         f"(rows under 2^24, D <= 65536, 1 <= neighbours <= 16 and <= training rows)")
    splits = {"fake_in_train": F.plan_splits(n_fake, n_train), "train_in_train": F.plan_splits(n_train, n_train)}
    ws = max(F.nn_workspace_bytes(n_fake, splits["fake_in_train"]), F.nn_workspace_bytes(n_train, splits["train_in_train"]))
    launches = ["feat_colmean(train)", "feat_norms(train)", "feat_norms(fake)",
                f"nn_partial + nn_finish: fake -> train, k = {neighbours}, {splits['fake_in_train']} split(s)",
                f"pair_sqdist: {n_fake} x {neighbours} pairs", f"nn_partial + nn_finish: train -> train leave-one-out, k = 1, {splits['train_in_train']} split(s)",
                f"pair_sqdist: {n_train} x 1 pairs"]
    return {"splits": splits, "workspace_bytes": ws, "matrix_bytes": n_train * n_fake * 4, "flops": 2.0 * d * (n_train * n_fake + n_train * n_train),
            "launches": launches}


def plan_lines(n_train, n_fake, d, neighbours):
    p = plan(n_train, n_fake, d, neighbours)
    return ([f"memorization_report of train [{n_train}, {d}] and fake [{n_fake}, {d}], neighbours = {neighbours}: splits {p['splits']}, workspace "
             f"{p['workspace_bytes'] / 2 ** 20:.2f} MiB (one materialised matrix: {p['matrix_bytes'] / 2 ** 20:.1f} MiB), {p['flops'] / 1e12:.3f} TFLOP",
             "launches:"] + ["  " + ln for ln in p["launches"]])


def load_set(src, args, extractor, channels, device):
    """-> (features [N, D] on the device, the files or None)"""
    import evaluate_images as ev
    from evaluate_latent_embedder import list_images, load_batch
    import torch
    if ev.is_feature_file(src):
        return ev.load_features(src, args.max_samples).to(device), None
    files = list_images(src, args.max_samples, getattr(args, "ext", None))
    feats = torch.cat([extractor(load_batch(files[lo:lo + args.batch], channels, device, args)) for lo in range(0, len(files), args.batch)])
    return feats, files


def suspicion_order(copy_ratio, nearest_dist):
    """most suspicious first: an exact copy (distance 0: ratio 0 or 0 / 0) before everything, then ascending copy ratio; ties by the sample's index"""
    import torch
    key = torch.where(nearest_dist == 0, torch.full_like(copy_ratio, -1.0), torch.nan_to_num(copy_ratio, nan=float("inf")))
    return torch.sort(key, stable=True).indices


def contact_sheet(rows, channels, path):
    """rows: lists of PNG paths (generated, its nearest training files) -> one image, a row per entry"""
    import numpy as np
    from evaluate_latent_embedder import load_png
    from medfusion_amd.egress import save_png
    sheet = np.concatenate([np.concatenate([load_png(f, channels) for f in row], axis=1) for row in rows], axis=0)
    save_png(sheet, path)


def main(argv=None):
    args = parse_args(argv)
    if args.plan:
        print("\n".join(plan_lines(args.n_train, args.n_fake, args.d, args.neighbours)))
        return 0
    import torch

    import evaluate_images as ev
    import medfusion_amd as M

    device = torch.device("cuda")
    extractor, channels = None, args.channels
    if args.features == "pixels":
        extractor = lambda imgs: imgs.reshape(imgs.shape[0], -1).contiguous()
    elif args.features is not None and not (ev.is_feature_file(args.train) and ev.is_feature_file(args.fake)):
        from medfusion_amd.checkpoint import load_module_from_checkpoint
        kind, ckpt, pool = ev.parse_features(args.features)
        model = load_module_from_checkpoint(getattr(M, kind), ckpt).to(device).eval()
        channels = getattr(model, "in_channels", None) or 3
        extractor = M.EmbedderFeatures(model, pool=pool)
    train, train_files = load_set(args.train, args, extractor, channels, device)
    fake, fake_files = load_set(args.fake, args, extractor, channels, device)
    if train.shape[1] > 65536:
        raise SystemExit(f"D = {train.shape[1]} features per sample: at most 65536 (one channel of 256 x 256); pool them (embedder:CKPT:pool)")
    k = min(args.neighbours, train.shape[0])
    rep = M.memorization_report(train, fake, neighbours=k)
    shown = min(SHEET_NEIGHBOURS, train.shape[0])
    near_d, near_i = M.nearest_neighbours(fake, train, shown)                  # the files of the list and the sheet
    order = suspicion_order(rep["copy_ratio"], rep["nearest_dist"])[:args.top]
    ratio = rep["copy_ratio"]
    finite = ratio[~torch.isnan(ratio)].double()
    qs = torch.quantile(finite, torch.tensor([0.0, 0.01, 0.05, 0.25, 0.5], dtype=torch.float64, device=device)).tolist() if finite.numel() else []
    name = lambda files, i: str(files[i]) if files is not None else int(i)
    top = []
    for j in order.tolist():
        top.append({"fake": name(fake_files, j), "copy_ratio": float(ratio[j]), "authentic": bool(rep["authentic"][j]), "train_gap": float(rep["train_gap"][j]),
                    "nearest": [{"train": name(train_files, int(i)), "dist": float(d)} for i, d in zip(near_i[j].tolist(), near_d[j].tolist())]})
    res = {"authenticity": rep["authenticity"], "copy_ratio_quantiles": dict(zip(("min", "q01", "q05", "q25", "median"), qs)),
           "exact_copies": int((rep["nearest_dist"] == 0).sum()), "n_train": int(train.shape[0]), "n_fake": int(fake.shape[0]),
           "neighbours": k, "features": args.features, "feature_width": int(train.shape[1]), "train": str(args.train), "fake": str(args.fake), "top": top}
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "nearest_train.json").write_text(json.dumps(res, indent=1) + "\n")
    if train_files is not None and fake_files is not None:
        contact_sheet([[e["fake"]] + [n["train"] for n in e["nearest"]] for e in top], channels, out / "nearest_train.png")
        res["contact_sheet"] = str(out / "nearest_train.png")
    print(f"authenticity {res['authenticity']:.4f}, exact copies {res['exact_copies']}, smallest copy ratios: "
          + " ".join(f"{e['copy_ratio']:.4f}" for e in top[:8]))
    return res


if __name__ == "__main__":
    r = main()
    sys.exit(r if isinstance(r, int) else 0)
