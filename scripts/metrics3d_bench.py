#!/usr/bin/env python3
"""Device time of ms_ssim3d and pairwise_ms_ssim3d next to the plain-torch restatement of the same definition (tests/metrics3d_cases.py: grouped
F.conv3d on the full k^3 window, F.avg_pool3d) on the same GPU, in the same process (profiles/metrics3d_bench.txt).

  python scripts/metrics3d_bench.py [--reps 5] [--rounds 3] [--out profiles/metrics3d_bench.txt]      (on a ROCm device)
  python scripts/metrics3d_bench.py --plan                                                             (no device: shapes, bytes, kernel resources)

Shapes: 4 pairs of the published 1 x 64 x 128 x 128 volume with betas_for(3) at k = 11, and a bank of 16 such volumes with 64 random pairs (the
diversity figure; the torch form has to gather the 2 x 64 volumes first, the library reads the bank in place).  Every time is the time between
two device events around back-to-back calls (at least `reps`, and as many as fill --window seconds; the host's launch gaps are inside), after a
warm-up of each form; the forms alternate over `rounds` rounds and every round is printed.  A call is the whole public function: pyramids, every
scale, the combination.  The main launch of scale 0 is also timed alone, as GB/s of its compulsory bytes.  Before timing, the two forms are
compared at the timed size.  No ratio is promised: the file records what is measured."""
import argparse
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

BATCH = (4, 1, 64, 128, 128)
BANK, PAIRS = (16, 1, 64, 128, 128), 64
SCALES, K, SIGMA = 3, 11, 1.5


def compulsory_bytes(pairs: int, bank_volumes: int, C: int, D: int, H: int, W: int) -> dict:
    """HBM bytes the definition needs (two volumes read once per pair and scale) against the torch form's (three product volumes written and read,
    five filtered volumes written and read again by the maps)"""
    vox = [C * (D >> s) * (H >> s) * (W >> s) for s in range(SCALES)]
    kernel = sum(2 * 4 * v for v in vox) * pairs
    pyramid = sum(4 * (vox[s] + vox[s + 1]) for s in range(SCALES - 1)) * bank_volumes
    torch_form = sum(4 * v * (2 + 3 * 2 + 5 * 2 + 5) for v in vox) * pairs
    return {"kernel": kernel, "pyramid": pyramid, "torch_form": torch_form, "scale0": 2 * 4 * vox[0] * pairs}


def kernel_resources():
    """VGPRs, LDS and scratch of the kernels of metrics3d.hip, from the device assembly the build's ISA lint keeps"""
    from medfusion_amd import build as B
    asm = B.OBJ / "lint" / "metrics3d.s"
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
    for label, pairs, volumes, shape in (("batch", BATCH[0], 2 * BATCH[0], BATCH), ("bank", PAIRS, BANK[0], BANK)):
        b = compulsory_bytes(pairs, volumes, *shape[1:])
        tiles = -(-(shape[2] - K + 1) // 16) * -(-(shape[3] - K + 1) // 16) * -(-(shape[4] - K + 1) // 16)
        lines.append(f"{label}: {pairs} pairs of {' x '.join(str(v) for v in shape[1:])}, {volumes} volumes in the pyramids, {SCALES} scales of {K} taps; "
                     f"{pairs * shape[1] * tiles} workgroups at scale 0; the kernels' compulsory bytes {(b['kernel'] + b['pyramid']) / 1e6:.1f} MB "
                     f"(pairs {b['kernel'] / 1e6:.1f} + pyramids {b['pyramid'] / 1e6:.1f}), the torch form's {b['torch_form'] / 1e6:.1f} MB")
    lines.append("kernels of metrics3d.hip (gfx950):")
    lines += ["  " + r for r in kernel_resources()]
    return lines


def main(a):
    import torch

    import medfusion_amd as M
    from medfusion_amd import kernels as KK
    from tests import metrics3d_cases as MC

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    x, y = (t.to(dev) for t in MC.make_inputs("recon", BATCH))
    bank = MC.make_bank(BANK).to(dev)
    index = M.metrics.plan_pairs(BANK[0], PAIRS, 0).to(dev)
    kw = dict(betas=M.betas_for(SCALES), kernel_size=K, sigma=SIGMA)

    def torch_ms(p, q):
        return MC.ref_ms_ssim3d(MC.ref_terms3d(p, q, torch.float32, k=K, sigma=SIGMA, scales=SCALES, device=dev))

    forms = {
        "batch / library": lambda: M.ms_ssim3d(x, y, **kw),
        "batch / torch": lambda: torch_ms(x, y),
        "bank / library": lambda: M.pairwise_ms_ssim3d(bank, index, **kw)[0],
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
    reps = {label: min(a.max_reps, max(a.reps, int(a.window * 1e3 / timed(fn, 2)) + 1)) for label, fn in forms.items()}
    lines.append(f"device: {torch.cuda.get_device_name(dev)}; {a.rounds} alternating rounds, device events around {reps} calls; ms per call")
    times = {label: [] for label in forms}
    for _ in range(a.rounds):
        for label, fn in forms.items():
            times[label].append(timed(fn, reps[label]))
    for label, ts in times.items():
        lines.append(f"{label:16s} {' '.join(f'{t:9.3f}' for t in ts)} | mean {sum(ts) / len(ts):9.3f} spread {max(ts) - min(ts):.3f}")
    for what, pairs in (("batch", BATCH[0]), ("bank", PAIRS)):
        lib, ref = (sum(times[f"{what} / {f}"]) / a.rounds for f in ("library", "torch"))
        lines.append(f"{what}: {pairs / lib * 1e3:.1f} pairs/s (library) against {pairs / ref * 1e3:.2f} pairs/s (torch form): measured ratio {ref / lib:.1f}")
    # the main launch of scale 0 alone (with its small finish launch): 4 pairs = 1024 workgroups
    taps = M.metrics.gaussian_taps(K, SIGMA)
    d = KK.make_ssim3d_desc(BATCH[0], *BATCH[1:], BATCH[0], BATCH[0], taps, 0.01, 0.03, 1.0)
    sim, cs = torch.empty(BATCH[0], device=dev), torch.empty(BATCH[0], device=dev)
    one = lambda: KK.ssim3d_pairs(x, y, d, sim, cs)
    one()
    ts = [timed(one, 50) for _ in range(a.rounds)]
    b = compulsory_bytes(BATCH[0], 2 * BATCH[0], *BATCH[1:])
    lines.append(f"batch: the scale-0 launch pair alone (ssim3d_pairs_kernel<K=11, V=4> over 1024 workgroups + finish), back to back: "
                 f"{' '.join(f'{t * 1e3:.1f}' for t in ts)} us per call = {b['scale0'] / (sum(ts) / len(ts)) / 1e6:.1f} GB/s of its compulsory "
                 f"{b['scale0'] / 1e6:.1f} MB")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timing at least")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "metrics3d_bench.txt"))
    ap.add_argument("--plan", action="store_true", help="print shapes, bytes and kernel resources, touch no device")
    a = ap.parse_args()
    if a.plan:
        print("\n".join(plan_lines()))
        sys.exit(0)
    main(a)
