#!/usr/bin/env python3
"""Device time of precision_recall next to the plain-torch form of the same definition (the full distance matrices, topk, compare) on the same GPU,
in the same process, and the distance core alone as TFLOP/s (profiles/fidelity_bench.txt).

  python scripts/fidelity_bench.py [--n 10000 --m 10000 --d 2048 --knn 3] [--reps 5] [--rounds 3] [--out profiles/fidelity_bench.txt]   (on a ROCm device)
  python scripts/fidelity_bench.py --plan [--n ... --m ... --d ...]                                  (no device: splits, workspace, flops, kernel resources)

Default shape: N = M = 10 000 features of width 2048 (the reference script's Inception feature width), knn = 3.  Every time is the time between two
device events around back-to-back WHOLE calls (the host's launch gaps and the one host sync of precision_recall are inside), after a warm-up of
each form; the forms alternate over `rounds` rounds and every round is printed.  The torch form is the definition with the matrix materialised:
centre by the pivot, |x|^2 + |y|^2 - 2 x y^T, clamp, topk(knn + 1), (d < r).any -- four N x M fp32 matrices one after the other.  Before timing the two
forms' counts are compared.  The distance core alone: mf_feat_sqdist_f32 (the matrix IS written: an upper bound of the core's time), 2 N M D flops,
against the 157.3 TF fp32-matrix peak.  No ratio is promised: the file records what is measured."""
import argparse
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

PEAK_TF = 157.3


def plan(n: int, m: int, d: int, knn: int) -> dict:
    from medfusion_amd import fidelity as F
    splits = {"knn_real": F.plan_splits(n, n), "knn_fake": F.plan_splits(m, m), "precision": F.plan_splits(m, n), "recall": F.plan_splits(n, m)}
    ws = max(F.workspace_bytes(n, n, splits["knn_real"]), F.workspace_bytes(m, m, splits["knn_fake"]), F.workspace_bytes(n, m, splits["precision"]),
             F.workspace_bytes(m, n, splits["recall"]))
    return {"splits": splits, "workspace_bytes": ws, "matrix_bytes": n * m * 4, "flops": 2.0 * d * (n * n + m * m + 2 * n * m), "knn": knn}


def kernel_resources():
    """VGPRs, LDS and scratch of the kernels of fidelity.hip, from the device assembly the build's ISA lint keeps"""
    from medfusion_amd import build as B
    asm = B.OBJ / "lint" / "fidelity.s"
    if not asm.exists():
        B.lint_isa()
    rows, cur = [], {}
    for line in asm.read_text().splitlines():
        mt = re.match(r"\s*\.(name|vgpr_count|agpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size):\s*(\S+)", line)
        if not mt:
            continue
        cur[mt.group(1)] = mt.group(2)
        if mt.group(1) == "vgpr_count":
            rows.append(cur)
            cur = {}
    out = []
    for r in rows:
        name = re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", r.get("name", "?"))
        # every template argument of the instantiation, integers and bools (I Li4E Lb1E E): the first is the load width V of every kernel template here
        tmpl = re.match(r"[a-z0-9_]+I((?:L[ib]\d+E)+)E", name)
        args = [a[1:] if a[0] == "i" else ("false", "true")[int(a[1:])] for a in re.findall(r"L([ib]\d+)E", tmpl.group(1))] if tmpl else []
        short = re.match(r"[a-z0-9_]+", name).group(0) + (f"<V={', '.join(args)}>" if args else "")
        out.append(f"{short:32s} vgpr {r.get('vgpr_count'):>3s} (agpr {r.get('agpr_count', '0'):>2s})  sgpr {r.get('sgpr_count'):>3s}  "
                   f"lds {r.get('group_segment_fixed_size'):>6s} B  scratch {r.get('private_segment_fixed_size')} B")
    return out


def plan_lines(n, m, d, knn):
    p = plan(n, m, d, knn)
    lines = [f"precision_recall of real [{n}, {d}] and fake [{m}, {d}], knn = {knn}: splits {p['splits']}, workspace {p['workspace_bytes'] / 2 ** 20:.2f} MiB "
             f"(one materialised matrix: {p['matrix_bytes'] / 2 ** 20:.1f} MiB), {p['flops'] / 1e12:.3f} TFLOP in four tiled launches",
             "kernels of fidelity.hip (gfx950):"]
    return lines + ["  " + r for r in kernel_resources()]


def torch_form(real, fake, knn):
    """the same definition with every matrix materialised, fp32, on the device of the inputs -> (precision hits, recall hits) as a [2] tensor"""
    import torch
    c = real.double().mean(0).float()
    rt, ft = real - c, fake - c
    nr, nf = (rt.double() ** 2).sum(1).float(), (ft.double() ** 2).sum(1).float()

    def d2(a, na, b, nb):
        return ((na[:, None] + nb[None, :]) - 2 * (a @ b.t())).clamp_min_(0)

    def radii(a, na):
        own = d2(a, na, a, na)
        own.fill_diagonal_(0)
        return torch.topk(own, knn + 1, dim=1, largest=False).values[:, knn]

    r_real, r_fake = radii(rt, nr), radii(ft, nf)
    inside_real = (d2(rt, nr, ft, nf) < r_real[:, None]).any(0).sum()
    inside_fake = (d2(ft, nf, rt, nr) < r_fake[:, None]).any(0).sum()
    return torch.stack([inside_real, inside_fake])


def run(a):
    import torch

    import medfusion_amd as M
    from medfusion_amd import kernels as K
    from tests import fidelity_cases as FC

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.backends.cuda.matmul.allow_tf32 = False
    real, fake = (t.to(dev) for t in FC.make(0, a.n, a.m, a.d))
    lines = plan_lines(a.n, a.m, a.d, a.knn)

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n

    forms = {"library": lambda: M.precision_recall(real, fake, a.knn), "torch": lambda: torch_form(real, fake, a.knn).tolist()}
    outs = {}
    for label, fn in forms.items():
        for _ in range(2):
            outs[label] = fn()
        torch.cuda.synchronize()
    lib_counts = [round(outs["library"]["precision"] * a.m), round(outs["library"]["recall"] * a.n)]
    lines.append(f"counts at the timed size (fake inside real, real inside fake): library {lib_counts}, torch fp32 form {outs['torch']}")
    lines.append(f"device: {torch.cuda.get_device_name(dev)}; {a.rounds} alternating rounds, device events around {a.reps} whole calls; ms per call")
    times = {label: [] for label in forms}
    for _ in range(a.rounds):
        for label, fn in forms.items():
            times[label].append(timed(fn, a.reps))
    for label, ts in times.items():
        lines.append(f"{label:10s} {' '.join(f'{t:9.3f}' for t in ts)} | median {sorted(ts)[len(ts) // 2]:9.3f} min {min(ts):9.3f}")
    lib, ref = (sorted(times[f])[a.rounds // 2] for f in ("library", "torch"))
    flops = plan(a.n, a.m, a.d, a.knn)["flops"]
    lines.append(f"precision_recall: {lib:.3f} ms = {flops / lib / 1e9:.1f} TFLOP/s over the whole call; torch form {ref:.3f} ms: measured ratio {ref / lib:.2f}")
    if lib > ref:
        lines.append("the library call is SLOWER than the torch form at this size: the torch form's matrix products run on the vendor GEMM; see the core's rate below")
    pivot = K.feat_colmean(real)
    nr, nf = K.feat_norms(real, pivot), K.feat_norms(fake, pivot)
    core = lambda: K.feat_sqdist(real, nr, fake, nf, pivot)
    core()
    torch.cuda.synchronize()
    ts = [timed(core, a.reps) for _ in range(a.rounds)]
    tf = 2.0 * a.n * a.m * a.d / min(ts) / 1e9
    lines.append(f"distance core (mf_feat_sqdist_f32, the {a.n} x {a.m} matrix written): {' '.join(f'{t:8.3f}' for t in ts)} ms; best {tf:.1f} TFLOP/s = "
                 f"{100 * tf / PEAK_TF:.0f} % of the {PEAK_TF} TF fp32-matrix peak")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10000, help="real features")
    ap.add_argument("--m", type=int, default=10000, help="generated features")
    ap.add_argument("--d", type=int, default=2048, help="feature width")
    ap.add_argument("--knn", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fidelity_bench.txt"))
    ap.add_argument("--plan", action="store_true", help="print splits, workspace, flops and kernel resources, touch no device")
    a = ap.parse_args(argv)
    if a.plan:
        print("\n".join(plan_lines(a.n, a.m, a.d, a.knn)))
        return 0
    run(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
