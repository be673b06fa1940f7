#!/usr/bin/env python3
"""What inversion and counterfactual editing cost, measured on one box in one process (profiles/edit_bench.txt).

  python scripts/edit_bench.py [--batch 16] [--rounds 3]      (on a ROCm device)

cfg2 of bench.py: published architecture (two classes) with seeded weights, B = 16, latent (8, 32, 32), images (3, 256, 256), VAE encode and decode
included.  Every time is the wall time of ONE call, synchronised before and after, after one warm-up call per configuration; the
configurations are interleaved over `rounds` rounds.
  * images/s of `edit` (label swap, guidance 1, strength 1) at 20 / 30 / 50 asked steps for both samplers, next to `sample_from` (strength 1) with
    the same sampler and steps: an edit runs 2 k - 1 estimator calls where sample_from runs k;
  * ms per upward iteration next to a downward solver iteration: (wall(100) - wall(50)) / 50 of `invert` and of `denoise` on latents, per round --
    the fixed cost of a call cancels.  The same launches plus one extra store of the latent: expected equal within the run-to-run spread;
  * the fixed cost of an edit call: encode + decode, timed on their own.
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

STEPS = (20, 30, 50)
SAMPLERS = ("ddim0", "dpmpp2m")
SLOPE_STEPS = (50, 100)


def stats(v):
    return sum(v) / len(v), max(v) - min(v)


def main(a):
    import torch

    import medfusion_amd as M
    from medfusion_amd import published as P

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe = P.build_published_pipeline(dev, 2)
    B = a.batch
    x = torch.from_numpy(P.hashed_uniform("edit_bench.x", B * 3 * 256 * 256)).reshape(B, 3, 256, 256).to(dev, torch.float32)
    src, tgt = torch.arange(B, device=dev) % 2, (torch.arange(B, device=dev) + 1) % 2
    z = pipe.invert(x, src, steps=4, strength=0.5, encode_noise=M.PhiloxDeviceNoise(3), return_trajectory=True)[1][0].clone()      # the encoded input

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    configs = {}
    for s in SAMPLERS:
        for n in STEPS:
            configs[f"edit {s} @{n}"] = lambda s=s, n=n: pipe.edit(x, tgt, source_condition=src, steps=n, sampler=s, encode_noise=M.PhiloxDeviceNoise(3))
            configs[f"sample_from {s} @{n}"] = lambda s=s, n=n: pipe.sample_from(x, 1.0, condition=tgt, steps=n, sampler=s, noise=M.PhiloxDeviceNoise(4),
                                                                               encode_noise=M.PhiloxDeviceNoise(3))
        for n in SLOPE_STEPS:
            configs[f"invert {s} /{n}"] = lambda s=s, n=n: pipe.invert(z, src, steps=n, sampler=s, is_latent=True)
            configs[f"denoise {s} /{n}"] = lambda s=s, n=n: pipe.denoise(z, steps=n, condition=src, sampler=s, decode=False, noise=M.PhiloxDeviceNoise(4))
    for label, fn in configs.items():          # warm-up: weights packed, workspaces sized, kernels loaded
        pipe.last_cmdlist_launches = 0
        _, out = timed(fn)
        assert bool(out.isfinite().all()), label
        assert pipe.last_cmdlist_launches > 0, f"{label}: the loop fell back to Python"
    wall = {label: [] for label in configs}
    for _ in range(a.rounds):
        for label, fn in configs.items():
            wall[label].append(timed(fn)[0])
    fmt = lambda ts: " ".join(f"{t * 1e3:.1f}" for t in ts)
    print(f"B = {B}, images (3, 256, 256), latent (8, 32, 32), published architecture (2 classes), seeded weights, guidance 1, encode and decode included; "
          f"one call, ms; {a.rounds} interleaved rounds after a warm-up")
    print("-- images/s")
    for s in SAMPLERS:
        for n in STEPS:
            (me, se), (mf, sf) = stats(wall[f"edit {s} @{n}"]), stats(wall[f"sample_from {s} @{n}"])
            print(f"{s:8s} @{n:3d} | edit {fmt(wall[f'edit {s} @{n}'])} mean {me * 1e3:.1f} spread {se * 1e3:.1f} -> {B / me:6.1f} images/s | sample_from "
                  f"{fmt(wall[f'sample_from {s} @{n}'])} mean {mf * 1e3:.1f} spread {sf * 1e3:.1f} -> {B / mf:6.1f} images/s | edit / sample_from {me / mf:.2f}")
    print(f"-- ms per iteration: (wall({SLOPE_STEPS[1]}) - wall({SLOPE_STEPS[0]})) / {SLOPE_STEPS[1] - SLOPE_STEPS[0]} per round, latents in and out")
    for s in SAMPLERS:
        for kind in ("invert", "denoise"):
            per = [(hi - lo) / (SLOPE_STEPS[1] - SLOPE_STEPS[0]) for lo, hi in zip(wall[f"{kind} {s} /{SLOPE_STEPS[0]}"], wall[f"{kind} {s} /{SLOPE_STEPS[1]}"])]
            m, sp = stats(per)
            print(f"{s:8s} {'upward (invert)' if kind == 'invert' else 'downward (denoise)':20s} {' '.join(f'{p * 1e3:.4f}' for p in per)} | mean {m * 1e3:.4f} spread {sp * 1e3:.4f}")
    print("-- fixed cost of an edit call")
    enc, dec = [], []
    for _ in range(a.rounds + 1):
        enc.append(timed(lambda: pipe.latent_embedder.encode(x, noise=M.PhiloxDeviceNoise(3)))[0])
        dec.append(timed(lambda: pipe.latent_embedder.decode(z))[0])
    print(f"encode {stats(enc[1:])[0] * 1e3:.1f} ms + decode {stats(dec[1:])[0] * 1e3:.1f} ms")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    main(ap.parse_args())
