#!/usr/bin/env python3
"""Device time of nearest_neighbours and density_coverage next to the plain-torch forms of the same definitions (the full distance matrix + topk,
and the matrix form of density / coverage) on the same GPU, in the same process (profiles/neighbours_bench.txt).

  python scripts/neighbours_bench.py [--n 10000 --m 10000 --d 2048 --k 1 10] [--reps 5] [--rounds 3] [--out profiles/neighbours_bench.txt]   (on a ROCm device)
  python scripts/neighbours_bench.py --plan [--n ... --m ... --d ...]                          (no device: splits, workspace, flops, kernel resources)

Default shape: N = 10 000 reference rows, M = 10 000 queries, D = 2048, k = 1 and 10.  Every time is the time between two device events around
back-to-back WHOLE calls, after a warm-up of each form; the forms alternate over `rounds` rounds and every round is printed.  The torch form of the
search: centre by the pivot, |x|^2 + |y|^2 - 2 x y^T, clamp, topk(k, largest=False) -- the M x N fp32 matrix materialised.  Before timing, the
indices of the two forms are compared (they may differ where two distances are within the error of either form: the share is printed).  No ratio
is promised: the file records what is measured."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(Path(__file__).resolve().parent))

NEW_KERNELS = ("nn_partial_kernel", "nn_finish_kernel", "pair_sqdist_kernel", "manifold_count_partial_kernel", "manifold_count_finish_kernel")


def plan(n: int, m: int, d: int, ks, knn: int = 5) -> dict:
    from medfusion_amd import fidelity as F
    splits = {"search": F.plan_splits(m, n), "radii": F.plan_splits(n, n), "counts": F.plan_splits(m, n), "coverage": F.plan_splits(n, m)}
    ws = max(F.nn_workspace_bytes(m, splits["search"]), F.workspace_bytes(n, n, splits["radii"]), F.nn_workspace_bytes(n, splits["coverage"]))
    return {"splits": splits, "workspace_bytes": ws, "matrix_bytes": n * m * 4, "search_flops": 2.0 * d * n * m, "dc_flops": 2.0 * d * (n * n + 2 * n * m),
            "k": list(ks), "knn": knn}


def plan_lines(n, m, d, ks, knn=5):
    from fidelity_bench import kernel_resources
    p = plan(n, m, d, ks, knn)
    lines = [f"nearest_neighbours of {m} queries in {n} reference rows, D = {d}, k in {p['k']}: splits {p['splits']['search']}, workspace "
             f"{p['workspace_bytes'] / 2 ** 20:.2f} MiB (one materialised matrix: {p['matrix_bytes'] / 2 ** 20:.1f} MiB), {p['search_flops'] / 1e12:.3f} TFLOP per search",
             f"density_coverage (knn = {knn}): splits {p['splits']}, {p['dc_flops'] / 1e12:.3f} TFLOP in three tiled launches",
             "new kernels of fidelity.hip (gfx950):"]
    return lines + ["  " + r for r in kernel_resources() if r.startswith(NEW_KERNELS)]


def torch_search(query, ref, k):
    import torch
    c = ref.double().mean(0).float()
    qt, rt = query - c, ref - c
    nq, nr = (qt.double() ** 2).sum(1).float(), (rt.double() ** 2).sum(1).float()
    d2 = ((nq[:, None] + nr[None, :]) - 2 * (qt @ rt.t())).clamp_min_(0)
    v, i = torch.topk(d2, k, dim=1, largest=False)
    return v.sqrt(), i


def torch_density_coverage(real, fake, knn):
    import torch
    c = real.double().mean(0).float()
    rt, ft = real - c, fake - c
    nr, nf = (rt.double() ** 2).sum(1).float(), (ft.double() ** 2).sum(1).float()
    own = ((nr[:, None] + nr[None, :]) - 2 * (rt @ rt.t())).clamp_min_(0)
    own.fill_diagonal_(0)
    r2 = torch.topk(own, knn + 1, dim=1, largest=False).values[:, knn]
    d2 = ((nr[:, None] + nf[None, :]) - 2 * (rt @ ft.t())).clamp_min_(0)
    inside = d2 < r2[:, None]
    return torch.stack([inside.sum(), (d2.min(1).values < r2).sum()])


def run(a):
    import torch

    import medfusion_amd as M
    from tests import fidelity_cases as FC

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.backends.cuda.matmul.allow_tf32 = False
    ref, query = (t.to(dev) for t in FC.make(0, a.n, a.m, a.d))
    lines = plan_lines(a.n, a.m, a.d, a.k, a.knn)
    lines.append(f"device: {torch.cuda.get_device_name(dev)}; {a.rounds} alternating rounds, device events around {a.reps} whole calls; ms per call")

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n

    def compare(title, forms, flops):
        outs = {}
        for label, fn in forms.items():
            for _ in range(2):
                outs[label] = fn()
            torch.cuda.synchronize()
        times = {label: [] for label in forms}
        for _ in range(a.rounds):
            for label, fn in forms.items():
                times[label].append(timed(fn, a.reps))
        for label, ts in times.items():
            lines.append(f"{title} {label:16s} {' '.join(f'{t:9.3f}' for t in ts)} | median {sorted(ts)[len(ts) // 2]:9.3f} min {min(ts):9.3f}")
        med = {label: sorted(ts)[len(ts) // 2] for label, ts in times.items()}
        first = next(iter(forms))
        lines.append(f"{title}: {first} {med[first]:.3f} ms = {flops / med[first] / 1e9:.1f} TFLOP/s over the whole call; torch form {med['torch']:.3f} ms: "
                     f"measured ratio {med['torch'] / med[first]:.2f}" + (" (the library call is SLOWER)" if med[first] > med["torch"] else ""))
        return outs

    p = plan(a.n, a.m, a.d, a.k, a.knn)
    for k in a.k:
        outs = compare(f"k={k}", {"library refined": lambda: M.nearest_neighbours(query, ref, k), "library unrefined": lambda: M.nearest_neighbours(query, ref, k, refine=False),
                                  "torch": lambda: torch_search(query, ref, k)}, p["search_flops"])
        same = float((outs["library unrefined"][1] == outs["torch"][1]).double().mean())
        lines.append(f"k={k}: share of indices equal between the unrefined library form and the torch form {same:.5f}")
    outs = compare(f"density_coverage knn={a.knn}", {"library": lambda: M.density_coverage(ref, query, a.knn), "torch": lambda: torch_density_coverage(ref, query, a.knn).tolist()},
                   p["dc_flops"])
    lib = outs["library"]
    lines.append(f"density_coverage: library (sum of counts, covered rows) = ({round(lib['density'] * a.knn * a.m)}, {round(lib['coverage'] * a.n)}), torch fp32 form {outs['torch']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10000, help="reference rows")
    ap.add_argument("--m", type=int, default=10000, help="query rows")
    ap.add_argument("--d", type=int, default=2048, help="feature width")
    ap.add_argument("--k", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--knn", type=int, default=5, help="neighbours of density / coverage")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "neighbours_bench.txt"))
    ap.add_argument("--plan", action="store_true", help="print splits, workspace, flops and kernel resources, touch no device")
    a = ap.parse_args(argv)
    if a.plan:
        print("\n".join(plan_lines(a.n, a.m, a.d, a.k, a.knn)))
        return 0
    run(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
