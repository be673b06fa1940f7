#!/usr/bin/env python3
"""Fidelity of a generated set against a real one in a feature space: the Frechet distance and improved precision / recall, the figures of the
reference's evaluate_images.py, computed on the device (medfusion_amd.fidelity).

Each of --real and --fake is a folder of PNG files of one size, or a .pt / .npy file of precomputed [N, D] features (what the reference script's
commented "Load features" block reads; a .pt holding a list of per-batch tensors is concatenated).  Folders need an extractor:
--features embedder:CKPT[:pool] takes the encoder of a latent embedder the user already has (VAE; or VQVAE:CKPT, VQGAN:CKPT, VAEGAN:CKPT for the other
classes), optionally average-pooled to pool x pool cells (medfusion_amd.EmbedderFeatures).  --features inception:FILE[:layer] is the reference's own
extractor, the FID variant of Inception-v3 (medfusion_amd.InceptionNet), from the weight file a reference run has on disk
(pt_inception-2015-12-05-6726825d.pth; nothing is downloaded): the log then reads "FID Score"; layer: 64, 192, 768, 2048 (default), logits_unbiased or
logits.  --inception-score [SPLITS] adds the Inception Score of the generated set (needs inception features and a folder as --fake).

  python scripts/evaluate_images.py --real real_ipr.pt --fake fake_ipr.pt --out results/metrics
  python scripts/evaluate_images.py --real reference/ --fake generated/ --features embedder:runs/.../last_vae.ckpt:4
  python scripts/evaluate_images.py --real reference/ --fake generated/ --features inception:pt_inception-2015-12-05-6726825d.pth --inception-score

--density-coverage [KNN] adds density / coverage, --memorization [NEIGHBOURS] the authenticity and the quantiles of the copy ratio of the generated set
against --real as the training set (medfusion_amd.density_coverage, memorization_report; scripts/nearest_train.py lists the suspicious files); both
are off by default and leave the log and the JSON of a call without them as they were.  --kid [SUBSETS] adds the Kernel Inception Distance
(medfusion_amd.kid: the mean and the spread of the unbiased MMD^2 over SUBSETS pairs of subsets of --kid-subset-size rows; smaller sets fall back
to subsets of min(N, M) rows, with a notice in the log); off by default likewise.

Writes metrics_<time>.log (Samples Real / Samples Fake / FD / Precision, Recall in the reference's wording) and metrics_<time>.json next to it."""
import argparse
import json
import logging
import sys
from datetime import datetime
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(1, str(Path(__file__).resolve().parent))      # evaluate_latent_embedder's folder reader

EMBEDDERS = ("VAE", "VQVAE", "VQGAN", "VAEGAN")
FEATURE_FILES = (".pt", ".npy")


def is_feature_file(path) -> bool:
    return Path(path).suffix in FEATURE_FILES


def parse_features(spec: str):
    """'embedder:CKPT[:pool]' (a VAE) or 'VQVAE:CKPT[:pool]' etc. -> (class name, checkpoint, pool or None)"""
    parts = spec.split(":")
    kind = "VAE" if parts[0] == "embedder" else parts[0]
    if kind not in EMBEDDERS or len(parts) not in (2, 3) or not parts[1]:
        raise SystemExit(f"--features: embedder:CKPT[:pool] (or one of {', '.join(EMBEDDERS)} in place of 'embedder'), got {spec!r}")
    pool = None
    if len(parts) == 3:
        if not parts[2].isdigit() or int(parts[2]) < 1:
            raise SystemExit(f"--features: pool is a positive integer, got {parts[2]!r}")
        pool = int(parts[2])
    return kind, parts[1], pool


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--real", required=True, help="folder of PNG files, or a .pt / .npy file of [N, D] features")
    ap.add_argument("--fake", required=True, help="the generated set, likewise")
    ap.add_argument("--features", default=None, help="embedder:CKPT[:pool] -- needed when a folder is given")
    ap.add_argument("--knn", type=int, default=3, help="neighbours of the manifold radii (the reference's 3)")
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--max-samples", type=int, default=None, help="only the first N files / rows of each set (default: all)")
    ap.add_argument("--out", default="results/metrics", help="folder of the log and the JSON")
    ap.add_argument("--density-coverage", type=int, nargs="?", const=5, default=None, metavar="KNN",
                    help="also density / coverage (Naeem et al. 2020) with KNN neighbours (5 when given without a value)")
    ap.add_argument("--memorization", type=int, nargs="?", const=10, default=None, metavar="NEIGHBOURS",
                    help="also the authenticity and the copy ratios of the generated set against --real as the training set (10 neighbours when given without a value)")
    ap.add_argument("--kid", type=int, nargs="?", const=100, default=None, metavar="SUBSETS",
                    help="also the Kernel Inception Distance over SUBSETS pairs of subsets (100 when given without a value)")
    from medfusion_amd.ingest import add_ingest_arguments
    add_ingest_arguments(ap)
    ap.add_argument("--kid-subset-size", type=int, default=1000, metavar="ROWS", help="rows of a subset of --kid (at most the rows of the smaller set)")
    ap.add_argument("--inception-score", type=int, nargs="?", const=1, default=None, metavar="SPLITS",
                    help="also the Inception Score of the generated set over SPLITS splits (1 when given without a value); needs --features inception:FILE")
    args = ap.parse_args(argv)
    if args.kid is not None and not 1 <= args.kid <= 65535:
        ap.error("--kid: 1 .. 65535 subsets")
    if args.kid_subset_size < 2:
        ap.error("--kid-subset-size: at least 2")
    if not 1 <= args.knn <= 15:
        ap.error("--knn: 1 .. 15")
    if args.density_coverage is not None and not 1 <= args.density_coverage <= 15:
        ap.error("--density-coverage: 1 .. 15")
    if args.memorization is not None and not 1 <= args.memorization <= 16:
        ap.error("--memorization: 1 .. 16")
    if args.batch < 1:
        ap.error("--batch: at least 1")
    if args.max_samples is not None and args.max_samples < 2:
        ap.error("--max-samples: at least 2")
    inception = args.features is not None and args.features.startswith("inception:")
    if inception:
        from medfusion_amd.ingest import ingest_requested
        try:
            parse_inception(args.features)
        except ValueError as e:
            ap.error(str(e))
        if ingest_requested(args):
            ap.error("--features inception: the network resizes the files itself; not with --resize / --crop")
    if args.inception_score is not None:
        if args.inception_score < 1:
            ap.error("--inception-score: at least 1 split")
        if not inception or is_feature_file(args.fake):
            ap.error("--inception-score: needs --features inception:FILE and a folder of images as --fake")
    if inception:
        pass                                   # (checked above)
    elif args.features is not None:
        parse_features(args.features)
    elif not (is_feature_file(args.real) and is_feature_file(args.fake)):
        ap.error("--features embedder:CKPT[:pool] is needed when --real or --fake is a folder of images")
    return args


def parse_inception(spec: str):
    """'inception:FILE[:layer]' -> (FILE, layer); a ValueError otherwise"""
    from medfusion_amd.inception import parse_features_spec
    return parse_features_spec(spec)


def inception_folder_features(folder, net, layers, batch, max_samples, device, args=None):
    """the files' own bytes through the network: a tuple of [N, D] tensors, one per layer"""
    import numpy as np
    import torch

    from evaluate_latent_embedder import list_images, load_png
    files = list_images(folder, max_samples, getattr(args, "ext", None))
    parts = []
    for lo in range(0, len(files), batch):
        arrs = [load_png(f, 3) for f in files[lo:lo + batch]]
        if len({a.shape for a in arrs}) != 1:
            raise SystemExit(f"the images of a batch are not of one size: {sorted({a.shape for a in arrs})}")
        x = torch.from_numpy(np.stack(arrs)).to(device).permute(0, 3, 1, 2).contiguous()
        parts.append(net.features(x, tuple(layers)))
    return tuple(torch.cat([p[i] for p in parts]) for i in range(len(layers)))


def load_features(path, max_samples, expect_2d=None):
    """a .pt / .npy file -> fp32 [N, D] host tensor (`expect_2d`: a tensor to check in place of the file's, for the refusal's test)"""
    import numpy as np
    import torch
    path = Path(path)
    if expect_2d is not None:
        t = expect_2d
    elif path.suffix == ".npy":
        t = torch.from_numpy(np.load(path))
    else:
        t = torch.load(path, map_location="cpu")
        if isinstance(t, (list, tuple)):
            t = torch.cat([torch.as_tensor(c) for c in t])
        t = torch.as_tensor(t)
    if t.dim() != 2 or t.shape[0] < 2:
        raise SystemExit(f"{path}: features [N, D] with at least two rows, got shape {tuple(t.shape)}")
    return t[slice(max_samples)].to(torch.float32).contiguous()


def folder_features(folder, extractor, channels, batch, max_samples, device, args=None):
    import torch

    from evaluate_latent_embedder import list_images, load_batch
    files = list_images(folder, max_samples, getattr(args, "ext", None))
    return torch.cat([extractor(load_batch(files[lo:lo + batch], channels, device, args)) for lo in range(0, len(files), batch)])


def main(argv=None):
    args = parse_args(argv)
    import torch

    import medfusion_amd as M

    device = torch.device("cuda")
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    stamp = datetime.now().strftime("%Y_%m_%d_%H%M%S")
    logger = logging.getLogger("evaluate_images")
    logger.setLevel(logging.INFO)
    logger.addHandler(logging.StreamHandler(sys.stdout))
    logger.addHandler(logging.FileHandler(out / f"metrics_{stamp}.log", "w", encoding="utf-8"))      # (the KID line is not ASCII; the others are)

    extractor, channels, what = None, 3, "precomputed feature files"
    inception = args.features is not None and args.features.startswith("inception:")
    net = layer = logits = None
    if inception:
        path, layer = parse_inception(args.features)
        what = f"Inception-v3 (FID variant) of {path}, layer {layer}"
        if not (is_feature_file(args.real) and is_feature_file(args.fake)):
            net = M.InceptionNet.from_file(path).to(device)
    elif args.features is not None and not (is_feature_file(args.real) and is_feature_file(args.fake)):
        from medfusion_amd.checkpoint import load_module_from_checkpoint
        kind, ckpt, pool = parse_features(args.features)
        model = load_module_from_checkpoint(getattr(M, kind), ckpt).to(device).eval()
        channels = getattr(model, "in_channels", None) or 3
        extractor = M.EmbedderFeatures(model, pool=pool)
        what = f"{kind} encoder of {ckpt}" + (f", pooled to {pool} x {pool}" if pool else "")
    sets = {}
    for name, src in (("real", args.real), ("fake", args.fake)):
        if is_feature_file(src):
            sets[name] = load_features(src, args.max_samples).to(device)
        elif inception:
            layers = (layer, "logits") if name == "fake" and args.inception_score is not None else (layer,)
            got = inception_folder_features(src, net, layers, args.batch, args.max_samples, device, args)
            sets[name], logits = got[0], got[1] if len(got) == 2 else logits
        else:
            sets[name] = folder_features(src, extractor, channels, args.batch, args.max_samples, device, args)
    real, fake = sets["real"], sets["fake"]
    logger.info(f"Samples Real: {real.shape[0]}")
    logger.info(f"Samples Fake: {fake.shape[0]}")
    res = M.precision_recall(real, fake, args.knn)
    res["fd"] = M.frechet_distance(real, fake)
    if inception:
        logger.info(f"FID Score: {res['fd']}")
        logger.info(f"Features: {what}, D = {real.shape[1]}")
    else:
        logger.info("Inception features: not built (needs downloaded weights); pass precomputed feature files")
        logger.info(f"FD (features: {what}, D = {real.shape[1]}): {res['fd']}")
    logger.info(f"Precision: {res['precision']}, Recall {res['recall']} ")
    if args.density_coverage is not None:
        dc = M.density_coverage(real, fake, args.density_coverage)
        res.update(density=dc["density"], coverage=dc["coverage"], density_coverage_knn=args.density_coverage)
        logger.info(f"Density: {dc['density']}, Coverage {dc['coverage']} (knn = {args.density_coverage})")
    if args.memorization is not None:
        rep = M.memorization_report(real, fake, neighbours=args.memorization)
        q = torch.quantile(rep["copy_ratio"][~torch.isnan(rep["copy_ratio"])].double(), torch.tensor([0.0, 0.01, 0.05, 0.5], dtype=torch.float64, device=device))
        res.update(authenticity=rep["authenticity"], copy_ratio_quantiles=dict(zip(("min", "q01", "q05", "median"), q.tolist())),
                   memorization_neighbours=args.memorization)
        logger.info(f"Authenticity: {rep['authenticity']}, smallest copy ratio {res['copy_ratio_quantiles']['min']} (neighbours = {args.memorization})")
    if args.kid is not None:
        size = args.kid_subset_size
        if size > min(real.shape[0], fake.shape[0]):
            size = min(real.shape[0], fake.shape[0])
            logger.info(f"KID: the sets hold fewer than {args.kid_subset_size} rows, subsets of {size} rows instead")
        kid = M.kid(real, fake, subsets=args.kid, subset_size=size)
        res.update(kid_mean=kid["kid_mean"], kid_std=kid["kid_std"], kid_subsets=args.kid, kid_subset_size=size)
        logger.info(f"KID: {kid['kid_mean']} ± {kid['kid_std']} ({args.kid} × {size})")
    if logits is not None:
        score = M.inception_score(logits, args.inception_score)
        res.update(score, inception_score_splits=args.inception_score)
        logger.info(f"Inception Score: {score['inception_score_mean']} ± {score['inception_score_std']} ({args.inception_score} splits)")
    res.update(real=str(args.real), fake=str(args.fake), features=args.features, feature_width=int(real.shape[1]), inception=layer)
    (out / f"metrics_{stamp}.json").write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main()
