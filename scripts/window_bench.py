#!/usr/bin/env python3
"""What windowed denoising costs, measured on one box in one process (profiles/window_bench.txt).

  python scripts/window_bench.py [--batch 4] [--rounds 3]      (on a ROCm device)
  python scripts/window_bench.py --plan                        (no device: the geometry)

Published architecture with seeded weights, guidance 1, device Philox noise.  Canvas latent (8, 32, 96) -- a 256 x 768 image -- window (32, 32),
stride 16, tent weights: M = 5 windows.  B = 4 canvases, 25 iterations of "dpmpp2m" + "logsnr", VAE decode of the whole canvas included.  Every
time is the wall time of ONE call, synchronised before and after, after one warm-up call per configuration; the configurations are interleaved
over `rounds` rounds.
  * canvases/s of the windowed call;
  * ms per windowed iteration next to an un-windowed iteration of B * M = 20 rows at (8, 32, 32): (wall(50) - wall(25)) / 25 on the uniform grid
    with decode=False, per round -- the fixed cost of a call cancels.  The un-windowed figure is taken TWICE per round (two configurations of
    the same call): their difference is the run-to-run spread a windowed overhead is read against;
  * the device time of the crop and of the merge alone (scripts/_devtime.py: recorded once, re-issued from C);
  * for orientation only: the un-windowed UNet run directly on the canvas at B = 4 (the repeated-structure failure the windows avoid, and a
    different token count for attention models) -- its iteration and its call.
EXPECTATION: a windowed iteration costs the 20-row iteration plus the two launch-bound kernels.  An overhead outside the spread plus the two
kernels' device time is a finding to explain, not a threshold.
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

CANVAS, WINDOW, STRIDE, WEIGHT = (8, 32, 96), (32, 32), 16, "tent"
STEPS, SLOPE_STEPS = 25, (25, 50)


def plan():
    from medfusion_amd.window import WindowPlan

    return WindowPlan(CANVAS[1:], WINDOW, STRIDE, WEIGHT)


def stats(v):
    return sum(v) / len(v), max(v) - min(v)


def main(a):
    import torch
    from _devtime import device_us

    import medfusion_amd as M
    from medfusion_amd import kernels as K
    from medfusion_amd import published as P

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe = P.build_published_pipeline(dev, None)
    wp = plan()
    B, rows = a.batch, a.batch * wp.M
    win = dict(window=WINDOW, window_stride=STRIDE, window_weight=WEIGHT)

    def call(n, size, steps, spacing, decode, seed, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe.sample(n, size, steps=steps, sampler="dpmpp2m", spacing=spacing, noise=M.PhiloxDeviceNoise(seed), decode=decode, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    # label -> (rows, latent, steps, spacing, decode, window kwargs)
    configs = {"windowed call": (B, CANVAS, STEPS, "logsnr", True, win), "direct call": (B, CANVAS, STEPS, "logsnr", True, {})}
    for n in SLOPE_STEPS:
        configs[f"windowed/{n}"] = (B, CANVAS, n, None, False, win)
        configs[f"rows a/{n}"] = (rows, (8, *WINDOW), n, None, False, {})
        configs[f"rows b/{n}"] = (rows, (8, *WINDOW), n, None, False, {})
        configs[f"direct/{n}"] = (B, CANVAS, n, None, False, {})
    launches = {}
    for label, (n, size, steps, sp, dec, kw) in configs.items():      # warm-up: weights packed, workspaces sized, kernels loaded
        _, out = call(n, size, steps, sp, dec, 1, **kw)
        assert bool(out.isfinite().all()), label
        assert pipe.last_cmdlist_launches > 0 and pipe.last_cmdlist_foreign_ops == [], f"{label}: the loop fell back to Python"
        launches[label] = pipe.last_cmdlist_launches
    assert launches[f"windowed/{SLOPE_STEPS[0]}"] == launches[f"rows a/{SLOPE_STEPS[0]}"] + 2, launches
    wall = {label: [] for label in configs}
    for r in range(a.rounds):
        for label, (n, size, steps, sp, dec, kw) in configs.items():
            wall[label].append(call(n, size, steps, sp, dec, 100 + r, **kw)[0])
    fmt = lambda ts: " ".join(f"{t * 1e3:.1f}" for t in ts)
    executed = pipe.noise_scheduler.loop_timesteps(STEPS, True, "logsnr")[1]
    print(f"{wp.describe()}")
    print(f"B = {B} canvases ({rows} estimator rows), published architecture, seeded weights, guidance 1; one call, ms; {a.rounds} interleaved rounds after a warm-up")
    print(f"-- the call: dpmpp2m + logsnr at {STEPS} ({executed} executed), decode of the whole canvas included")
    for label in ("windowed call", "direct call"):
        m, s = stats(wall[label])
        print(f"{label:16s} {fmt(wall[label])} | mean {m * 1e3:.1f} spread {s * 1e3:.1f} | {B / m:6.2f} canvases/s" + ("   (orientation only)" if label.startswith("direct") else ""))
    d = SLOPE_STEPS[1] - SLOPE_STEPS[0]
    print(f"-- ms per iteration: (wall({SLOPE_STEPS[1]}) - wall({SLOPE_STEPS[0]})) / {d} per round, decode=False; recorded launches per iteration in brackets")
    it = {}
    for label in ("windowed", "rows a", "rows b", "direct"):
        per = [(hi - lo) / d for lo, hi in zip(wall[f"{label}/{SLOPE_STEPS[0]}"], wall[f"{label}/{SLOPE_STEPS[1]}"])]
        it[label] = (per, *stats(per))
        what = {"windowed": f"windowed, {B} canvases", "rows a": f"un-windowed, {rows} rows at {WINDOW}", "rows b": "the same again", "direct": f"un-windowed on the canvas, {B} rows (orientation)"}[label]
        print(f"{what:48s} [{launches[f'{label}/{SLOPE_STEPS[0]}']:3d}] {' '.join(f'{p * 1e3:.4f}' for p in per)} | mean {it[label][1] * 1e3:.4f} spread {it[label][2] * 1e3:.4f}")
    base = (it["rows a"][1] + it["rows b"][1]) / 2
    spread = max(it["rows a"][2], it["rows b"][2], abs(it["rows a"][1] - it["rows b"][1]))
    print("-- device time of the two kernels alone (re-issued from C, 100 repetitions)")
    canvas = torch.randn((B, *CANVAS), device=dev)
    wins = K.window_gather(canvas, wp)
    g_us, _ = device_us(lambda: K.window_gather(canvas, wp, out=wins))
    out = torch.empty_like(canvas)
    m_us, _ = device_us(lambda: K.window_merge(wins, wp, out=out))
    print(f"crop  {tuple(canvas.shape)} -> {tuple(wins.shape)}: {g_us:.1f} us      merge back: {m_us:.1f} us")
    over = it["windowed"][1] - base
    print(f"-- overhead of a windowed iteration over the {rows}-row iteration: {over * 1e3:.4f} ms = {100 * over / base:.2f} % "
          f"(run-to-run spread of the un-windowed figure {spread * 1e3:.4f} ms; the two kernels {(g_us + m_us) * 1e-3:.4f} ms)")
    print("inside the spread plus the two kernels" if over <= spread + (g_us + m_us) * 1e-6 else "OUTSIDE the spread plus the two kernels: a finding to explain")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--plan", action="store_true", help="print the geometry, touch no device")
    a = ap.parse_args()
    if a.plan:
        p = plan()
        print(p.describe())
        flat = lambda t: [x for u in t for x in flat(u)] if isinstance(t, list) else [t]
        print(f"cover counts {sorted(set(flat(p.cover)))}; {a.batch} canvases -> {a.batch * p.M} estimator rows at (8, {WINDOW[0]}, {WINDOW[1]}); image {8 * CANVAS[1]} x {8 * CANVAS[2]}")
        sys.exit(0)
    main(a)
