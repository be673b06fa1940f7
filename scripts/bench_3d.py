#!/usr/bin/env python3
"""spatial_dims=3 sampling on one GPU: the published UNet and VAE architectures (hid 256/256/512/1024 and 64/128/256/512, emb 1024,
8 latent channels) at spatial_dims=3 with seeded weights, 1-channel volumes 64 x 128 x 128 (latent 8 x 8 x 16 x 16), B = 4, 25 DDIM steps,
a condition given, guidance 1 and 8.  Reports volumes/s of the whole sample() (denoise + decode), the UNet forward and the VAE decode, and
per 3x3x3 convolution shape of those two passes the TFLOP/s of mf_conv3d_f16x2 next to torch's own fp32 F.conv3d on the same device and to
the 2-D fp16-pair kernel on the GEMM-equivalent shape (same M, K = 27 Cin as a 3x3 convolution with 3 Cin input channels).

    timeout -k 10 900 python scripts/bench_3d.py [--batch 4] [--steps 25] [--reps 3]
"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch
import torch.nn.functional as F

import medfusion_amd as M
from medfusion_amd import blocks3d as B3
from medfusion_amd import kernels as K
from medfusion_amd.published import published_scheduler_kwargs, published_unet_kwargs, published_vae_kwargs, seeded_fill
from medfusion_amd.utils import no_init


def build(dev):
    ukw = dict(published_unet_kwargs(2, 8), spatial_dims=3)
    vkw = dict(published_vae_kwargs(8), spatial_dims=3, in_channels=1, out_channels=1)
    with no_init():
        pipe = M.DiffusionPipeline(M.GaussianNoiseScheduler, M.UNet, None, published_scheduler_kwargs(), ukw, estimator_objective="x_T",
                                   clip_x0=False)
        pipe.latent_embedder = M.VAE(**vkw)
    seeded_fill(pipe.noise_estimator, "d3bench.unet.")
    seeded_fill(pipe.latent_embedder, "d3bench.vae.")
    return pipe.to(dev).eval()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def event_ms(fn, reps):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def conv_shapes(pipe, B, dev):
    """every distinct 3x3x3 convolution of one UNet forward (B rows) and one VAE decode (B rows)"""
    seen = {}
    real = B3.Conv3d.forward

    def spy(self, x):
        x1, x2 = B3._split(x)
        if self.k == 3:
            key = (x1.shape[0], B3.dims(x1), x1.shape[-1], 0 if x2 is None else x2.shape[-1], self.out_ch, self.stride, self.upsample)
            seen[key] = seen.get(key, 0) + 1
        return real(self, x)

    B3.Conv3d.forward = spy
    try:
        x = torch.randn((B, 8, 8, 16, 16), device=dev)
        pipe.noise_estimator(x, torch.full((B,), 500, device=dev), torch.zeros((B,), dtype=torch.long, device=dev))
        pipe.latent_embedder.decode(x)
    finally:
        B3.Conv3d.forward = real
    return seen


def bench_conv(key, count, dev, reps):
    n, (d, h, w), c1, c2, co, stride, up = key
    cin = c1 + c2
    pad = (1, 1, 1)
    g = torch.Generator().manual_seed(1)
    x = torch.randn((n, d * h, w, cin), generator=g).to(dev)
    wt = (torch.randn((co, cin, 3, 3, 3), generator=g) / (27 * cin) ** 0.5).to(dev)
    b = torch.zeros(co, device=dev)
    desc = K.make_conv3d_desc(n, d, h, w, cin, 0, co, 3, stride, pad, up)
    do, ho, wo = K.conv3d_out_dims(desc)
    tile, sk = K.conv3d_plan(desc)
    wh = K.split_weight_f16x2(K.pack_conv3d_weight(wt))
    M_ = n * do * ho * wo
    flop = 2.0 * M_ * co * 27 * cin
    t3 = event_ms(lambda: K.conv3d_f16x2(x, wh, b, desc), reps)
    # torch fp32 F.conv3d (NCDHW; the upsample as F.interpolate in front, as the reference does it, timed with it)
    xt = x.view(n, d, h, w, cin).permute(0, 4, 1, 2, 3).contiguous()
    if any(up):
        ttorch = event_ms(lambda: F.conv3d(F.interpolate(xt, scale_factor=tuple(2.0 if u else 1.0 for u in up), mode="nearest"), wt, b, stride, pad),
                          reps)
    else:
        ttorch = event_ms(lambda: F.conv3d(xt, wt, b, stride, pad), reps)
    # the 2-D fp16-pair kernel on the GEMM-equivalent shape: M = n do ho wo voxels as a (n do) x ho x wo image, 3 cin input channels
    t2 = float("nan")
    d2 = K.make_conv_desc(n * do, ho, wo, 3 * cin, 0, co, 3, 1, 1, 0, precision=5)
    if K.conv_f16x2_ok(d2):
        x2 = torch.randn((n * do, ho, wo, 3 * cin), generator=g).to(dev)
        w2 = K.split_weight_f16x2(K.pack_conv_weight((torch.randn((co, 3 * cin, 3, 3), generator=g) / (27 * cin) ** 0.5).to(dev)))
        pinned = K.pin_conv_plan(d2)
        t2 = event_ms(lambda: K.conv2d_f16x2(x2, w2, b, d2, pinned=pinned), reps)
    tf = lambda ms: flop / (ms * 1e-3) / 1e12
    print(f"  N={n} DHW={d}x{h}x{w} Cin={c1}+{c2} Cout={co} s={stride} up={up} (x{count}, tile {tile} split-K {sk}): M={M_} K={27 * cin}  "
          f"conv3d {t3:8.3f} ms {tf(t3):7.1f} TFLOP/s | torch fp32 F.conv3d {ttorch:8.3f} ms {tf(ttorch):7.1f} | 2-D pairs kernel (same GEMM) "
          f"{t2:8.3f} ms {tf(t2):7.1f}", flush=True)
    return t3 * count, flop * count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--conv-reps", type=int, default=5)
    ap.add_argument("--skip-convs", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    pipe = build(dev)
    B = args.batch
    print(f"3-D workload: published UNet + VAE at spatial_dims=3, volumes 1 x 64 x 128 x 128, latent 8 x 8 x 16 x 16, B = {B}, "
          f"{args.steps} DDIM steps, condition given", flush=True)
    cond = torch.tensor([i % 2 for i in range(B)], device=dev)
    z = torch.randn((B, 8, 8, 16, 16), device=dev)
    t = torch.full((B,), 500, device=dev)
    with torch.no_grad():
        ms_unet = 1e3 * timed(lambda: pipe.noise_estimator(z, t, cond), args.reps)[0]
        ms_dec = 1e3 * timed(lambda: pipe.latent_embedder.decode(z), args.reps)[0]
    print(f"UNet forward (B={B}): {ms_unet:.2f} ms   VAE decode (B={B}): {ms_dec:.2f} ms", flush=True)
    for gs in (1.0, 8.0):
        sec, vol = timed(lambda: pipe.sample(B, (8, 8, 16, 16), condition=cond, guidance_scale=gs, steps=args.steps, use_ddim=True,
                                             noise=M.PhiloxDeviceNoise(5)), 1)
        assert vol.shape == (B, 1, 64, 128, 128) and bool(vol.isfinite().all())
        print(f"sample guidance {gs:g}: {sec:.3f} s per batch, {B / sec:.3f} volumes/s", flush=True)
    if not args.skip_convs:
        print("per 3x3x3 shape of one UNet forward + one VAE decode:", flush=True)
        tot_ms = tot_flop = 0.0
        for key, count in sorted(conv_shapes(pipe, B, dev).items(), key=lambda kv: -kv[0][0] * kv[0][2]):
            ms, fl = bench_conv(key, count, dev, args.conv_reps)
            tot_ms += ms
            tot_flop += fl
        print(f"  all 3x3x3 convolutions: {tot_ms:.2f} ms, {tot_flop / (tot_ms * 1e-3) / 1e12:.1f} TFLOP/s", flush=True)


if __name__ == "__main__":
    main()
