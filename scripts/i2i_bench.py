#!/usr/bin/env python3
"""What image-conditioned sampling costs next to sample(), measured on one box in one session (profiles/i2i_bench.txt).

  python scripts/i2i_bench.py --parent <checkout of the parent commit, library built>  [--reps 5] [--batch 16] [--steps 150]

Every figure is the wall time of ONE call at cfg2 of bench.py (published architecture, B = 16, latent (8, 32, 32), 150 DDIM iterations, device Philox
noise, VAE decode included), synchronised before and after, after one warm-up call, in a process of its own:
  * the parent commit's sample(), `reps` times: the reference time (mean) and its run-to-run spread (max - min);
  * this tree's sample(): it runs the kernels the parent runs, so it must sit inside  reference + 2 x spread  (two runs are compared) -- the GATE;
  * sample_from(is_latent=True, strength=1.0) without and with a mask (a rectangle: half of the cells kept), per loop form ("cmdlist", "graph",
    "eager"), reported beside it and held to the same gate on the default form: the select adds two fp32 reads per latent element and a mask
    byte per cell to the scheduler step's launch; a miss means the blend left the fused launch or a loop form fell back to the Python loop.
Without --parent the reference is this tree's own sample() (no gate on it).  Exit status 1 when a gate is missed.
"""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def worker(args):
    sys.path.insert(0, str(Path(args.tree).resolve()))
    import torch

    import medfusion_amd as M
    from medfusion_amd import published as P

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe = P.build_published_pipeline(dev, None)
    B, latent = args.batch, (8, 32, 32)
    kw = dict(steps=args.steps, use_ddim=True)
    if args.loop != "default":
        kw["loop"] = args.loop
    if args.what == "sample":
        call = lambda seed: pipe.sample(B, latent, noise=M.PhiloxDeviceNoise(seed), **kw)
    else:
        z0 = torch.empty((B, *latent), device=dev)
        M.kernels.philox_normal(z0, 99, 0)
        mask = None
        if args.what == "from_mask":
            mask = torch.zeros((B, 1, 32, 32), dtype=torch.uint8, device=dev)
            mask[:, :, 8:24, :] = 1
        call = lambda seed: pipe.sample_from(z0, 1.0, mask=mask, is_latent=True, noise=M.PhiloxDeviceNoise(seed), **kw)
    call(1)   # warm-up: weights packed, workspaces sized
    times = []
    for k in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = call(100 + k)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    assert img.shape == (B, 3, 256, 256) and bool(img.isfinite().all())
    print("I2I_BENCH " + json.dumps(dict(times=times, cmdlist_launches=int(getattr(pipe, "last_cmdlist_launches", 0)))))


def run(tree, what, loop, a):
    tree = Path(tree).resolve()
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", "--tree", str(tree), "--what", what, "--loop", loop, "--reps", str(a.reps),
           "--batch", str(a.batch), "--steps", str(a.steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tree), env=dict(os.environ))
    if r.returncode != 0:
        raise SystemExit(f"{what} / {loop} on {tree} failed:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("I2I_BENCH ")][-1][len("I2I_BENCH "):])


def stats(times):
    return sum(times) / len(times), max(times) - min(times)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=str(ROOT))
    ap.add_argument("--what", default="sample", choices=["sample", "from_nomask", "from_mask"])
    ap.add_argument("--loop", default="default", choices=["default", "cmdlist", "graph", "eager"])
    a = ap.parse_args()
    if a.worker:
        worker(a)
        sys.exit(0)

    fmt = lambda ts: " ".join(f"{t * 1e3:.1f}" for t in ts)
    ref = run(a.parent or ROOT, "sample", "default", a)
    ref_mean, spread = stats(ref["times"])
    gate = ref_mean + 2 * spread
    print(f"B = {a.batch}, latent (8, 32, 32), {a.steps} DDIM iterations, decode included; one call, ms; {a.reps} calls after a warm-up")
    print(f"reference: {'parent commit' if a.parent else 'this tree'} sample(): {fmt(ref['times'])} | mean {ref_mean * 1e3:.1f} spread (max - min) {spread * 1e3:.1f}"
          f" | gate = mean + 2 x spread = {gate * 1e3:.1f}")
    failed = []
    if a.parent:
        cur = run(ROOT, "sample", "default", a)
        m, s = stats(cur["times"])
        ok = m <= gate
        print(f"this tree  sample():                       {fmt(cur['times'])} | mean {m * 1e3:.1f} spread {s * 1e3:.1f} | {'inside the gate' if ok else 'GATE MISSED'}")
        if not ok:
            failed.append("sample()")
    for loop in ("cmdlist", "graph", "eager"):
        for what, label in (("from_nomask", "no mask"), ("from_mask", "mask   ")):
            res = run(ROOT, what, loop, a)
            m, s = stats(res["times"])
            note = ""
            if loop == "cmdlist":      # the default form: held to the gate, and the list must really have been replayed
                ok = m <= gate and res["cmdlist_launches"] > 0
                note = f" | {res['cmdlist_launches']} launches per replayed iteration | {'inside the gate' if ok else 'GATE MISSED'}"
                if not ok:
                    failed.append(f"sample_from {label.strip()} ({loop})")
            print(f"sample_from(strength=1.0) {label} {loop:8s}: {fmt(res['times'])} | mean {m * 1e3:.1f} spread {s * 1e3:.1f} | {m / ref_mean:.3f} x reference{note}")
    if failed:
        print("GATE MISSED: " + ", ".join(failed))
        sys.exit(1)
    print("all gated figures inside reference + 2 x spread")
