#!/usr/bin/env python3
"""Device time of ms_ssim and pairwise_ms_ssim next to the plain-torch restatement of the same definition (tests/metrics_cases.py: grouped F.conv2d
on the full 2-D window, F.avg_pool2d) on the same GPU, in the same process (profiles/metrics_bench.txt).

  python scripts/metrics_bench.py [--reps 20] [--rounds 3] [--out profiles/metrics_bench.txt]      (on a ROCm device)
  python scripts/metrics_bench.py --plan                                                            (no device: shapes, bytes, kernel resources)

Shapes: the reference evaluation script's batch (B = 100 pairs of 3 x 256 x 256), and a bank of 256 such images with 1000 random pairs (the
diversity figure; the torch form has to gather the 2 x 1000 images first, the library reads the bank in place).  Every time is the time
between two device events around back-to-back calls (at least `reps`, and as many as fill --window seconds; the host's launch gaps are inside),
after a warm-up of each form; the forms alternate over `rounds` rounds and every round is printed.  A call is the whole public function: pyramids,
every scale, the combination.  The library's own launches of the batch shape are also timed alone, re-issued from C (scripts/_devtime.py).
Before timing, the two forms are compared at the timed size.  No ratio is promised: the file records what is measured."""
import argparse
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

BATCH = (100, 3, 256, 256)
BANK, PAIRS = (256, 3, 256, 256), 1000
SCALES, K = 5, 11


def compulsory_bytes(pairs: int, bank_images: int, C: int, H: int, W: int) -> dict:
    """HBM bytes the definition needs (two planes read once per pair and scale) against the torch form's (five filtered planes written and read
    again per pair and scale, on top of three product planes written and read)"""
    px = [C * (H >> s) * (W >> s) for s in range(SCALES)]
    kernel = sum(2 * 4 * p for p in px) * pairs
    pyramid = sum(4 * (px[s] + px[s + 1]) for s in range(SCALES - 1)) * bank_images
    torch_form = sum(4 * p * (2 + 3 * 2 + 5 * 2 + 5) for p in px) * pairs     # inputs, 3 products w + r, 5 filtered w + r (valid ~ full), 5 read by the maps
    return {"kernel": kernel, "pyramid": pyramid, "torch_form": torch_form}


def kernel_resources():
    """VGPRs, LDS and scratch of the kernels of metrics.hip, from the device assembly the build's ISA lint keeps"""
    from medfusion_amd import build as B
    asm = B.OBJ / "lint" / "metrics.s"
    if not asm.exists():
        B.lint_isa()
    rows, cur = [], {}
    for line in asm.read_text().splitlines():
        m = re.match(r"\s*\.(name|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size):\s*(\S+)", line)
        if not m:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1) == "vgpr_count":
            rows.append(cur)
            cur = {}
    out = []
    for r in rows:
        name = re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", r.get("name", "?"))
        tmpl = re.search(r"ILi(\d+)ELi(\d+)E", name)
        short = re.match(r"[a-z0-9_]+", name).group(0) + (f"<K={tmpl.group(1)}, V={tmpl.group(2)}>" if tmpl else "")
        out.append(f"{short:36s} vgpr {r.get('vgpr_count'):>3s}  sgpr {r.get('sgpr_count'):>3s}  lds {r.get('group_segment_fixed_size'):>6s} B  scratch {r.get('private_segment_fixed_size')} B")
    return out


def plan_lines():
    lines = []
    for label, pairs, images, shape in (("batch", BATCH[0], 2 * BATCH[0], BATCH), ("bank", PAIRS, BANK[0], BANK)):
        b = compulsory_bytes(pairs, images, *shape[1:])
        lines.append(f"{label}: {pairs} pairs of {shape[1]} x {shape[2]} x {shape[3]}, {images} images in the pyramids: the kernels' compulsory bytes "
                     f"{(b['kernel'] + b['pyramid']) / 1e6:.1f} MB (pairs {b['kernel'] / 1e6:.1f} + pyramids {b['pyramid'] / 1e6:.1f}), the torch form's {b['torch_form'] / 1e6:.1f} MB")
    lines.append("kernels of metrics.hip (gfx950):")
    lines += ["  " + r for r in kernel_resources()]
    return lines


def main(a):
    import torch

    import medfusion_amd as M
    from tests import metrics_cases as MC

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    x, y = (t.to(dev) for t in MC.make_inputs("recon", BATCH))
    bank = MC.make_bank(BANK).to(dev)
    index = M.metrics.plan_pairs(BANK[0], PAIRS, 0).to(dev)

    def torch_ms(p, q):
        return MC.ref_ms_ssim(MC.ref_terms(p, q, torch.float32, device=dev))

    forms = {
        "batch / library": lambda: M.ms_ssim(x, y),
        "batch / torch": lambda: torch_ms(x, y),
        "bank / library": lambda: M.pairwise_ms_ssim(bank, index)[0],
        "bank / torch": lambda: torch_ms(bank[index[:, 0]], bank[index[:, 1]]),
    }
    lines = plan_lines()

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n

    outs = {}
    for label, fn in forms.items():                                  # warm-up: code objects, workspaces, the convolution library's choice
        for _ in range(2):
            outs[label] = fn()
        torch.cuda.synchronize()
    for what in ("batch", "bank"):
        lib, ref = outs[f"{what} / library"].double(), outs[f"{what} / torch"].double()
        lines.append(f"{what}: library vs torch fp32 form at the timed size: max |diff| {float((lib - ref).abs().max()):.3e} (values {float(ref.min()):.4f} .. {float(ref.max()):.4f})")
    reps = {label: max(a.reps, int(a.window * 1e3 / timed(fn, 3)) + 1) for label, fn in forms.items()}
    lines.append(f"device: {torch.cuda.get_device_name(dev)}; {a.rounds} alternating rounds, device events around {reps} calls; ms per call")
    times = {label: [] for label in forms}
    for _ in range(a.rounds):
        for label, fn in forms.items():
            times[label].append(timed(fn, reps[label]))
    for label, ts in times.items():
        lines.append(f"{label:16s} {' '.join(f'{t:8.3f}' for t in ts)} | mean {sum(ts) / len(ts):8.3f} spread {max(ts) - min(ts):.3f}")
    for what, pairs in (("batch", BATCH[0]), ("bank", PAIRS)):
        lib, ref = (sum(times[f"{what} / {f}"]) / a.rounds for f in ("library", "torch"))
        lines.append(f"{what}: {pairs / lib * 1e3:.0f} pairs/s (library) against {pairs / ref * 1e3:.0f} pairs/s (torch form): measured ratio {ref / lib:.2f}")
    from _devtime import device_us
    MT, taps = M.metrics, M.metrics.gaussian_taps()

    def launches_only():                                             # (everything the launches write stays alive while they are re-issued)
        xp, yp = MT.pyramid(x, SCALES), MT.pyramid(y, SCALES)
        return xp, yp, MT._terms(xp, yp, None, None, BATCH[0], None, 1.0, taps, 0.01, 0.03, False)

    us, n = device_us(launches_only)
    b = compulsory_bytes(BATCH[0], 2 * BATCH[0], *BATCH[1:])
    lines.append(f"batch: the library's {n} launches alone (two pyramids, five scales), re-issued from C: {us:.1f} us per call = "
                 f"{(b['kernel'] + b['pyramid']) / us / 1e6:.2f} TB/s of the compulsory bytes")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timing at least")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "metrics_bench.txt"))
    ap.add_argument("--plan", action="store_true", help="print shapes, bytes and kernel resources, touch no device")
    a = ap.parse_args()
    if a.plan:
        print("\n".join(plan_lines()))
        sys.exit(0)
    main(a)
