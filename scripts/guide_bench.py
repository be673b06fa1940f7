#!/usr/bin/env python3
"""What guidance rescale, dynamic thresholding and a guidance schedule cost, measured on one box in one process (profiles/guide_bench.txt).

  python scripts/guide_bench.py [--batch 16] [--rounds 3]      (on a ROCm device)
  python scripts/guide_bench.py --plan                         (no device: the configurations, their executed counts and launch sequences)

cfg2-like: the published architecture with seeded weights, B = 16, latent (8, 32, 32) -- a row of 8192 floats, the one-workgroup path --,
classifier-free guidance 8, "dpmpp2m" + "logsnr" at 25 iterations, device Philox noise, no decode.
  * ms per executed iteration of the whole call with each option on, against the same call with the options off: device time between two
    events around the call, after one warm-up call per configuration, the configurations interleaved over `rounds` rounds;
  * the launches of the recorded iteration (last_cmdlist_launches) of each configuration: the added launches per iteration;
  * the stage alone: mf_guide_f32 on B x 8192 random rows, `reps` back-to-back calls between two events, per stage combination;
  * the same for ONE row of 8 x 64 x 64 = 32768 floats (a 64 x 64 canvas): the multi-workgroup sequence (1, 2 or 6 launches).
"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

STEPS, G, LATENT = 25, 8.0, (8, 32, 32)
# label -> the options of the call
CONFIGS = {"options off": {}, "guidance_schedule (constant)": dict(guidance_schedule="constant"), "guidance_rescale=0.7": dict(guidance_rescale=0.7),
           "dynamic_threshold=0.995": dict(dynamic_threshold=0.995),
           "all three": dict(guidance_schedule="constant", guidance_rescale=0.7, dynamic_threshold=0.995)}
STAGES = {"combine only": 0, "rescale": 1, "threshold": 2, "rescale + threshold": 3}
LONG_ROW = 8 * 64 * 64


def executed_count():
    from medfusion_amd import GaussianNoiseScheduler
    from medfusion_amd.published import published_scheduler_kwargs

    return GaussianNoiseScheduler(**published_scheduler_kwargs()).loop_timesteps(STEPS, True, "logsnr")[1]


def stage_launches(n, stages):
    """the launch sequence of mf_guide_f32 for a row of n elements (include/medfusion_hip.h)"""
    from medfusion_amd import lib as L

    if n <= L.GUIDE_ROW_ONE_WG:
        return 1
    return 1 + (4 if stages & L.GUIDE_THRESHOLD else 0) + (1 if stages else 0)


def plan():
    ex = executed_count()
    print(f"dpmpp2m + logsnr, steps={STEPS}: {ex} executed iterations; B rows of {LATENT[0] * LATENT[1] * LATENT[2]} floats (one workgroup per row)")
    for label, opts in CONFIGS.items():
        print(f"  {label:30s} {'the plain path: no launch added' if not opts else '+1 launch per iteration (mf_guide_f32, one workgroup per row)'}")
    for label, st in STAGES.items():
        print(f"  stage alone, {label:20s} row of 8192: {stage_launches(8192, st)} launch; row of {LONG_ROW}: {stage_launches(LONG_ROW, st)} launches")


def main(a):
    import torch

    import medfusion_amd as M
    from medfusion_amd import kernels as K
    from medfusion_amd import lib as L
    from medfusion_amd import published as P

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe = P.build_published_pipeline(dev, None)
    B, ex = a.batch, executed_count()
    cond = torch.tensor([i % 2 for i in range(B)], device=dev)

    def call(opts, seed):
        kw = dict(opts)
        if kw.get("guidance_schedule") == "constant":
            kw["guidance_schedule"] = [G] * ex
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = pipe.sample(B, LATENT, steps=STEPS, sampler="dpmpp2m", spacing="logsnr", condition=cond, guidance_scale=G, un_cond=None,
                          noise=M.PhiloxDeviceNoise(seed), decode=False, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    launches = {}
    for label, opts in CONFIGS.items():          # warm-up: weights packed, workspaces sized, kernels loaded
        _, lat = call(opts, 1)
        assert bool(lat.isfinite().all()), label
        assert pipe.last_cmdlist_launches > 0 and pipe.last_cmdlist_foreign_ops == [], f"{label}: the loop fell back to Python"
        launches[label] = pipe.last_cmdlist_launches
    ms = {label: [] for label in CONFIGS}
    for r in range(a.rounds):
        for label, opts in CONFIGS.items():
            ms[label].append(call(opts, 100 + r)[0])
    print(f"B = {B}, latent {LATENT}, published architecture, seeded weights, guidance {G}, dpmpp2m + logsnr, {ex} executed iterations, no decode; device ms "
          f"between two events around one call; {a.rounds} interleaved rounds after a warm-up")
    base = sum(ms["options off"]) / a.rounds / ex
    for label in CONFIGS:
        per = [v / ex for v in ms[label]]
        mean = sum(per) / len(per)
        print(f"{label:30s} ms / iteration {' '.join(f'{p:.4f}' for p in per)} | mean {mean:.4f} spread {max(per) - min(per):.4f} | {mean - base:+.4f} ms "
              f"({100 * (mean - base) / base:+.2f} %) | launches / iteration {launches[label]} ({launches[label] - launches['options off']:+d})")

    def stage_alone(Bs, n, reps):
        x, pc, pu = (torch.randn(Bs, n, device=dev) for _ in range(3))
        rows = [L.MfGuideStep(G, 0.7, 0.995, 0.0, 1.0206207, 0.2041241, 500, 0)]
        table = K.guide_table(rows, dev)
        ws = K.guide_workspace(Bs, n, dev)
        out = torch.empty_like(pc)
        for label, st in STAGES.items():
            run = lambda: K.guide(pc, table, pred_uncond=pu, x_t=x, objective=0, stages=st, out=out, workspace=ws)
            for _ in range(10):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            print(f"  {label:20s} {1e3 * e0.elapsed_time(e1) / reps:8.2f} us per call ({stage_launches(n, st)} launch{'es' if stage_launches(n, st) > 1 else ''}; "
                  f"{reps} back-to-back calls, host-enqueued)")

    print(f"-- the stage alone, {B} rows of 8192 floats (one workgroup per row)")
    stage_alone(B, 8192, a.reps)
    print(f"-- the stage alone, 1 row of {LONG_ROW} floats (the multi-workgroup sequence)")
    stage_alone(1, LONG_ROW, a.reps)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--plan", action="store_true", help="print the configurations and their launch sequences, touch no device")
    a = ap.parse_args()
    if a.plan:
        plan()
        sys.exit(0)
    main(a)
