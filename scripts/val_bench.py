#!/usr/bin/env python3
"""Device time and peak extra memory of DiffusionPipeline.validation_step next to the plain-torch composition of the same definition (host-gathered
coefficients through rows_axpby, the draw and x_t materialised, F.l1_loss / F.mse_loss / F.interpolate(mode='area') and the variance fields in
fp32) on the same GPU, in the same process, at the published 2-D architecture (profiles/val_bench.txt).

  python scripts/val_bench.py [--batch 16] [--reps 5] [--rounds 3] [--out profiles/val_bench.txt]   (on a ROCm device)
  python scripts/val_bench.py --plan [--batch 16]          (no device: launches, workgroups, workspace, kernel resources)

Two comparisons: a WHOLE call (encode nothing: the input is the latent; one estimator pass; the losses) in both forms, and the loss launches ALONE
-- the forward process, the error sums of the horizontal prediction and of two pooled heads, the learned-variance terms -- against their compulsory
bytes and against the torch composition on the same tensors.  Every time is the time between two device events around back-to-back whole calls,
after a warm-up of each form; the forms alternate over `rounds` rounds and every round is printed.  Peak extra memory:
torch.cuda.max_memory_allocated over one call above what was allocated before it.  No ratio is set in advance: the file records what is measured,
whichever way it falls."""
import argparse
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

LATENT = (8, 32, 32)      # the published 2-D latent


def kernel_resources():
    """VGPRs, LDS and scratch of the kernels of loss.hip, from the device assembly the build's ISA lint keeps"""
    from medfusion_amd import build as B
    asm = B.OBJ / "lint" / "loss.s"
    if not asm.exists() or asm.stat().st_mtime < (B.CSRC / "loss.hip").stat().st_mtime:
        B.lint_isa()
    out, cur = [], {}
    for line in asm.read_text().splitlines():
        mt = re.match(r"\s*\.(name|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count):\s*(\S+)", line)
        if not mt:
            continue
        cur[mt.group(1)] = mt.group(2)
        if mt.group(1) == "vgpr_spill_count":
            name = re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", cur.get("name", "?"))
            flags = ", ".join(("false", "true")[int(b)] for b in re.findall(r"Lb(\d)E", name.split("Ev")[0]))
            short = re.match(r"[a-z0-9_]+kernel", name).group(0) + (f"<{flags}>" if flags else "")
            out.append(f"{short:36s} vgpr {cur.get('vgpr_count'):>3s}  sgpr {cur.get('sgpr_count'):>3s}  lds {cur.get('group_segment_fixed_size'):>5s} B  "
                       f"scratch {cur.get('private_segment_fixed_size')} B  spilled vgprs {cur.get('vgpr_spill_count')}")
            cur = {}
    return out


def plan_lines(batch):
    from medfusion_amd import lib as L
    lib = L.load()
    per = LATENT[0] * LATENT[1] * LATENT[2]
    lines = [f"validation_step at the published 2-D architecture, latent {LATENT}, B = {batch}: {per} elements per row"]
    for what, p, values in (("horizontal prediction", per, 2), ("head at 1/2", per // 4, 2), ("head at 1/4", per // 16, 2), ("learned-variance terms", per, 3)):
        parts = lib.mf_loss_parts(p)
        lines.append(f"  {what:24s} {parts} partial(s) per row, {batch * parts} workgroups of 256 + 1 finish launch, workspace {lib.mf_loss_workspace_bytes(batch, p, values)} B")
    lines.append(f"  forward process          1 launch over {batch * per // 4} quads; with a device source the draw is never stored: {4 * batch * per * 2} B moved instead of "
                 f"{4 * batch * per * 4} B (draw written, then read twice)")
    lines.append("kernels of loss.hip (gfx950):")
    return lines + ["  " + r for r in kernel_resources()]


def torch_step(pipe, z0, condition, t, noise, loss="l1"):
    """the plain-torch composition of validation_step: the same estimator pass, everything around it as a user would write it from the library's
    existing pieces -- the coefficients gathered on the host from t (a sync), the draw and x_t materialised, fp32 torch reductions"""
    import torch
    import torch.nn.functional as F
    sch, est = pipe.noise_scheduler, pipe._estimator()
    noise.begin(z0.shape[0], z0.device)
    x_T = noise.draw(tuple(z0.shape))
    x_t = sch.estimate_x_t(z0, t, x_T=x_T)
    pred, heads = est(x_t, t.to(z0.device), condition=condition)
    target = x_T if pipe.estimator_objective == "x_T" else z0
    fct = F.l1_loss if loss == "l1" else F.mse_loss
    w = pipe.deep_supervision_weights(len(heads))
    total = fct(pred, target) * w[0]
    for i, p in enumerate(heads):
        total = total + fct(p, F.interpolate(target, size=p.shape[2:], mode="area")) * w[i + 1]
    return {"loss": total, "L1": F.l1_loss(pred, target), "L2": F.mse_loss(pred, target)}


def torch_losses(tb, x0, x_T, t, pred, heads, pred_var):
    """the loss arithmetic alone in plain torch: forward process, L1 / L2 of the prediction and of two area-pooled heads, the variance fields"""
    import torch
    import torch.nn.functional as F
    g = lambda n: tb[n].gather(0, t).reshape(-1, 1, 1, 1)
    x_t = g("sqrt_alphas_cumprod") * x0 + g("sqrt_one_minus_alphas_cumprod") * x_T
    out = [F.l1_loss(pred, x_T), F.mse_loss(pred, x_T)]
    for h in heads:
        tg = F.interpolate(x_T, size=h.shape[2:], mode="area")
        out += [F.l1_loss(h, tg), F.mse_loss(h, tg)]
    vs = (pred_var + 1) / 2
    lmin, lmax = torch.log(g("posterior_variance").clamp(min=1e-20)), torch.log(g("betas").clamp(min=1e-20))
    plv = vs * lmax + (1 - vs) * lmin
    px0 = (g("sqrt_recip_alphas_cumprod") * x_t - g("sqrt_recipm1_alphas_cumprod") * x_T).clamp(-1, 1)
    pm, tm = g("posterior_mean_coef1") * px0 + g("posterior_mean_coef2") * x_t, g("posterior_mean_coef1") * x0 + g("posterior_mean_coef2") * x_t
    kl = 0.5 * (plv - lmin + torch.exp(lmin - plv) + torch.pow(tm - pm, 2) * torch.exp(-plv) - 1.0)
    nll = F.gaussian_nll_loss(px0, x0, torch.exp(plv), reduction="none")
    out.append(torch.mean(torch.where(t == 0, nll.mean((1, 2, 3)), kl.mean((1, 2, 3)))))
    return torch.stack(out)


def run(a):
    import torch

    import medfusion_amd as M
    from medfusion_amd import kernels as K
    from oracle import restate as R
    from oracle import synth as S
    from tests.util import to_product_kwargs

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = a.batch
    lines = plan_lines(B)
    lines.append(f"device: {torch.cuda.get_device_name(dev)}; {a.rounds} alternating rounds, device events around {a.reps} whole calls; ms per call")

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated(dev) - before

    def compare(title, forms, reps, nbytes=None):
        outs, mem, times = {}, {}, {label: [] for label in forms}
        for label, fn in forms.items():
            fn()                                                              # warm-up (workspace, plans)
            outs[label], mem[label] = peak(fn)
        for _ in range(a.rounds):
            for label, fn in forms.items():
                times[label].append(timed(fn, reps))
        med = {label: sorted(ts)[len(ts) // 2] for label, ts in times.items()}
        for label, ts in times.items():
            lines.append(f"{title} {label:8s} {' '.join(f'{t:9.4f}' for t in ts)} | median {med[label]:9.4f} ms; peak extra memory {mem[label] / 2 ** 20:8.2f} MiB; "
                         f"result {outs[label]}")
        extra = f"; {nbytes / 1e6:.2f} MB compulsory: {nbytes / med['library'] / 1e6:.1f} GB/s" if nbytes else ""
        lines.append(f"{title}: library {med['library']:.4f} ms, torch {med['torch']:.4f} ms: measured ratio torch / library {med['torch'] / med['library']:.2f}"
                     + (" (the library form is SLOWER)" if med["library"] > med["torch"] else "") + extra)

    pipe = M.DiffusionPipeline(M.GaussianNoiseScheduler, M.UNet, None, R.published_scheduler_kwargs(), to_product_kwargs(R.published_unet_kwargs(2)),
                               do_input_centering=False)
    S.synth_state_dict(pipe.noise_estimator, "published.unet.")
    pipe = pipe.to(dev).eval()
    z0 = S.synth_input("val_bench.z0", (B, *LATENT), 0.6).to(dev)
    cond = (torch.arange(B, device=dev) % 2).long()
    t_host = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(0))
    show = lambda r: [round(float(r[k]), 6) for k in ("loss", "L1", "L2")]
    compare(f"validation_step B={B}", {"library": lambda: show(pipe.validation_step(z0, cond, t=t_host, noise=M.PhiloxDeviceNoise(1), is_latent=True)),
                                       "torch": lambda: show(torch_step(pipe, z0, cond, t_host, M.PhiloxDeviceNoise(1)))}, a.reps)

    # the loss launches alone, on fixed tensors
    sch = pipe.noise_scheduler
    tb = sch.device_tables(dev)
    t32, tl = t_host.to(dev, torch.int32), t_host.to(dev)
    x_T = K.philox_normal(torch.empty_like(z0), 1, 0, 0)
    pred, pv = (S.synth_input(f"val_bench.{n}", z0.shape).to(dev) for n in ("pred", "pv"))
    heads = [S.synth_input(f"val_bench.h{f}", (B, LATENT[0], LATENT[1] // f, LATENT[2] // f)).to(dev) for f in (2, 4)]
    n = z0.numel()

    def library_losses():
        x_t = K.diffuse_rows(z0, t32, tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"], philox=(1, 0, 0))
        sums = [K.denoise_loss(p, philox=(1, 0, 0), target_shape=z0.shape) for p in (pred, *heads)]
        return sums, K.variance_loss(z0, x_t, x_T, pred, pv, t32, tb, 0, True)

    # compulsory bytes: x_0 in, x_t out; pred and the heads in (the target is regenerated); five fields in for the variance terms
    nbytes = 4 * (2 * n + n + n // 4 + n // 16 + 5 * n)
    compare(f"loss launches alone B={B}", {"library": lambda: float(library_losses()[0][0][0, 0]), "torch": lambda: float(torch_losses(tb, z0, x_T, tl, pred, heads, pv)[0])},
            a.reps * 4, nbytes)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "val_bench.txt"))
    ap.add_argument("--plan", action="store_true", help="print launches, workgroups, workspace and kernel resources, touch no device")
    a = ap.parse_args(argv)
    if a.batch < 1 or a.reps < 1 or a.rounds < 1:
        ap.error("--batch, --reps and --rounds are positive")
    if a.plan:
        print("\n".join(plan_lines(a.batch)))
        return 0
    run(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
