#!/usr/bin/env python3
"""VQGAN.decode at the reference's default sizes (hid 64..512, 4 latent channels, K = 8192 codes, 32 x 32 latents -> 256 x 256 images):
`--batch` decodes after one warm-up each, for a `rocprofv3 --kernel-trace --stats` run that puts the quantizer's launches (vq_* kernels) next
to the whole decode.  Seeded weights and latents; prints host wall time per decode as a cross-check.

    rocprofv3 --kernel-trace --stats -d OUT -o vq -- python scripts/vq_decode_prof.py --batch 16 200
"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch

import medfusion_amd as M
from oracle import synth as S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[16, 200])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    m = M.VQGAN()
    S.synth_state_dict(m, "vqgan_default.")
    m.to(dev).eval()
    for b in args.batch:
        z = S.synth_input(f"vq_prof_z{b}", (b, 4, 32, 32)).to(dev)
        m.decode(z)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            x = m.decode(z)
        torch.cuda.synchronize()
        print(f"B={b}: VQGAN.decode {1e3 * (time.perf_counter() - t0) / args.reps:.2f} ms per call (host wall), image {tuple(x.shape)}", flush=True)


if __name__ == "__main__":
    main()
