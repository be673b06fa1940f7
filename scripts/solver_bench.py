#!/usr/bin/env python3
"""What the few-step samplers -- deterministic and stochastic -- cost and how far the deterministic ones land from the ODE limit, measured on one
box in one process (profiles/solver_bench.txt; the stochastic samplers' rows: profiles/sde_bench.txt).

  python scripts/solver_bench.py [--batch 16] [--rounds 3] [--limit-steps 1000]      (on a ROCm device)
  python scripts/solver_bench.py --plan                                               (no device: the configurations and their executed counts)

cfg2 of bench.py: published architecture with seeded weights, B = 16, latent (8, 32, 32), device Philox noise, VAE decode included.  Every time is
the wall time of ONE call, synchronised before and after, after one warm-up call per configuration; the configurations are interleaved
over `rounds` rounds.
  * images/s: sampler=None at 150 iterations (the loop every earlier commit runs: the baseline), "ddim0" at 150, "dpmpp2m" + "logsnr" and
    "dpmpp2m_sde" + "logsnr" at 20 / 25 / 30;
  * ms per executed iteration of each loop kind (None / "ddim0" / "dpmpp2m" / "ddim1" / "dpmpp2m_sde"): (wall(150) - wall(75)) / 75 on the uniform
    grid, per round -- the decode and the fixed cost of a call cancel.  GATE (the deterministic samplers): a solver iteration is not slower than a
    sampler=None iteration beyond the larger of the two run-to-run spreads (max - min over the rounds); it launches strictly less (no Philox
    draws).  Exit status 1 when the gate is missed.  The stochastic samplers draw inside the same one launch: reported next to the others, not gated;
  * the fixed cost of a call at 20 executed iterations: wall(20) - 18 x the replayed iteration's time (iterations 0 and 1 go through Python --
    eager, then recorded -- and the list is rebuilt on every call), next to the decoder's own time;
  * solver error ON SYNTHETIC WEIGHTS: max-norm relative error of the final latent of each few-step run against "ddim0" on the uniform grid at
    `limit-steps` iterations from the same x_T (the ODE limit of the reference's own sampler).  The weights are hash-filled, not trained: this is
    a solver-accuracy figure, not an image-quality one.
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

# label -> (sampler, spacing, steps)
HEADLINE = {"sampler=None @150": (None, None, 150), "ddim0 @150": ("ddim0", None, 150), "dpmpp2m+logsnr @20": ("dpmpp2m", "logsnr", 20),
            "dpmpp2m+logsnr @25": ("dpmpp2m", "logsnr", 25), "dpmpp2m+logsnr @30": ("dpmpp2m", "logsnr", 30),
            "dpmpp2m_sde+logsnr @20": ("dpmpp2m_sde", "logsnr", 20), "dpmpp2m_sde+logsnr @25": ("dpmpp2m_sde", "logsnr", 25),
            "dpmpp2m_sde+logsnr @30": ("dpmpp2m_sde", "logsnr", 30)}
SLOPE = {"sampler=None": (None, None), "ddim0": ("ddim0", None), "dpmpp2m": ("dpmpp2m", None), "ddim1": ("ddim1", None), "dpmpp2m_sde": ("dpmpp2m_sde", None)}
STOCHASTIC = ("ddim1", "dpmpp2m_sde")     # (one Philox draw per non-final iteration: they have no ODE limit to be compared with)
SLOPE_STEPS = (75, 150)


def plan():
    """every configuration of a run with the iterations it executes (host arithmetic only)"""
    from medfusion_amd import GaussianNoiseScheduler
    from medfusion_amd.published import published_scheduler_kwargs

    sch = GaussianNoiseScheduler(**published_scheduler_kwargs())
    rows = [(label, sampler, spacing, steps, sch.loop_timesteps(steps, True, spacing)[1]) for label, (sampler, spacing, steps) in HEADLINE.items()]
    rows += [(f"{label} @{steps} (per-iteration slope)", sampler, spacing, steps, sch.loop_timesteps(steps, True, spacing)[1])
             for label, (sampler, spacing) in SLOPE.items() for steps in SLOPE_STEPS]
    return rows


def stats(v):
    return sum(v) / len(v), max(v) - min(v)


def main(a):
    import torch

    import medfusion_amd as M
    from medfusion_amd import published as P

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe = P.build_published_pipeline(dev, None)
    B, latent = a.batch, (8, 32, 32)

    def call(sampler, spacing, steps, seed, decode=True):
        kw = {} if sampler is None else dict(sampler=sampler, spacing=spacing)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe.sample(B, latent, steps=steps, use_ddim=True, noise=M.PhiloxDeviceNoise(seed), decode=decode, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    configs = {label: (s, sp, n) for label, (s, sp, n) in HEADLINE.items()}
    configs.update({f"{label}/{n}": (s, sp, n) for label, (s, sp) in SLOPE.items() for n in SLOPE_STEPS})
    executed = {}
    for label, (s, sp, n) in configs.items():          # warm-up: weights packed, workspaces sized, kernels loaded
        _, img = call(s, sp, n, 1)
        assert img.shape == (B, 3, 256, 256) and bool(img.isfinite().all()), label
        executed[label] = pipe.noise_scheduler.loop_timesteps(n, True, sp)[1]
        assert s is None or pipe.last_cmdlist_launches > 0, f"{label}: the loop fell back to Python"
    wall = {label: [] for label in configs}
    for r in range(a.rounds):
        for label, (s, sp, n) in configs.items():
            wall[label].append(call(s, sp, n, 100 + r)[0])
    fmt = lambda ts: " ".join(f"{t * 1e3:.1f}" for t in ts)
    print(f"B = {B}, latent (8, 32, 32), published architecture, seeded weights, decode included; one call, ms; {a.rounds} interleaved rounds after a warm-up")
    print("-- images/s")
    base = stats(wall["sampler=None @150"])[0]
    for label in HEADLINE:
        m, sp_ = stats(wall[label])
        print(f"{label:24s} executed {executed[label]:4d} | {fmt(wall[label])} | mean {m * 1e3:.1f} spread {sp_ * 1e3:.1f} | {B / m:7.1f} images/s | {base / m:.2f} x baseline")
    print(f"-- ms per executed iteration: (wall({SLOPE_STEPS[1]}) - wall({SLOPE_STEPS[0]})) / {SLOPE_STEPS[1] - SLOPE_STEPS[0]} per round")
    it = {}
    for label in SLOPE:
        per = [(hi - lo) / (SLOPE_STEPS[1] - SLOPE_STEPS[0]) for lo, hi in zip(wall[f"{label}/{SLOPE_STEPS[0]}"], wall[f"{label}/{SLOPE_STEPS[1]}"])]
        it[label] = stats(per)
        print(f"{label:22s} {' '.join(f'{p * 1e3:.4f}' for p in per)} | mean {it[label][0] * 1e3:.4f} spread {it[label][1] * 1e3:.4f}")
    failed = []
    for label in ("ddim0", "dpmpp2m"):
        allow = max(it[label][1], it["sampler=None"][1])
        ok = it[label][0] <= it["sampler=None"][0] + allow
        print(f"gate {label}: {it[label][0] * 1e3:.4f} <= {it['sampler=None'][0] * 1e3:.4f} + {allow * 1e3:.4f} : {'inside' if ok else 'GATE MISSED'}")
        if not ok:
            failed.append(label)
    print("-- fixed cost of a call at 20 executed iterations")
    dec = []
    z = pipe.sample(B, latent, steps=20, sampler="dpmpp2m", spacing="logsnr", noise=M.PhiloxDeviceNoise(5), decode=False)
    for _ in range(a.rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.latent_embedder.decode(z)
        torch.cuda.synchronize()
        dec.append(time.perf_counter() - t0)
    w20 = stats(wall["dpmpp2m+logsnr @20"])[0]
    fixed = w20 - (executed["dpmpp2m+logsnr @20"] - 2) * it["dpmpp2m"][0]
    print(f"wall {w20 * 1e3:.1f} - {executed['dpmpp2m+logsnr @20'] - 2} x {it['dpmpp2m'][0] * 1e3:.4f} = {fixed * 1e3:.1f} ms, of which the decoder {stats(dec[1:])[0] * 1e3:.1f} ms"
          f" -> {100 * fixed / w20:.0f} % of the call ({100 * (fixed - stats(dec[1:])[0]) / w20:.0f} % without the decoder)")
    print(f"-- solver error on SYNTHETIC weights (a solver-accuracy figure, not an image-quality one): final latent vs ddim0 + uniform at {a.limit_steps} from the same x_T")
    rel = lambda x, y: float((x.double() - y.double()).abs().max() / y.double().abs().max())
    limit = call("ddim0", None, a.limit_steps, 77, decode=False)[1]
    for label, (s, sp, n) in HEADLINE.items():
        if s is None or s in STOCHASTIC:
            continue
        print(f"{label:22s} relerr {rel(call(s, sp, n, 77, decode=False)[1], limit):.3e}")
    for s, sp, n in (("dpmpp2m", None, 20), ("ddim0", "logsnr", 20), ("ddim0", None, 20)):
        print(f"{s + ('+' + sp if sp else '') + ' @' + str(n):22s} relerr {rel(call(s, sp, n, 77, decode=False)[1], limit):.3e}")
    if failed:
        print("GATE MISSED: " + ", ".join(failed))
        sys.exit(1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit-steps", type=int, default=1000)
    ap.add_argument("--plan", action="store_true", help="print the configurations and their executed iteration counts, touch no device")
    a = ap.parse_args()
    if a.plan:
        for label, sampler, spacing, steps, executed in plan():
            print(f"{label:44s} sampler={sampler!s:11s} spacing={spacing!s:7s} steps={steps:4d} executed={executed}")
        sys.exit(0)
    main(a)
