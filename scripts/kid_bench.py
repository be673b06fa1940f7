#!/usr/bin/env python3
"""Device time and peak extra memory of kid and mmd2 next to the plain-torch forms of the same definition (three kernel matrices, a pow pass and a
sum pass over each) on the same GPU, in the same process (profiles/kid_bench.txt).

  python scripts/kid_bench.py [--n 10000 --d 2048 --subsets 100 --subset-size 1000 --big 50000] [--reps 3] [--rounds 3] [--out profiles/kid_bench.txt]   (on a ROCm device)
  python scripts/kid_bench.py --plan [--n ... --d ... --subsets ... --subset-size ...]          (no device: launches, workgroups, workspace, kernel resources)

Three comparisons: kid at N = M = n rows with `subsets` x `subset_size`; mmd2 of the full sets at n rows; mmd2 at `big` rows, where the torch form
is chunked over row blocks (its matrices would take 3 x 10 GB at 50 000 rows), or reported as "does not fit" if it cannot allocate.  The torch
form of kid comes twice: the loop over the subsets (what a metrics package does) and the batched form (one bmm per term over all the gathered
subsets); both draw the same index lists inside the call, as kid does.  Every time is the time between two device events around back-to-back WHOLE calls, after a warm-up of each form; the forms alternate over
`rounds` rounds and every round is printed.  Peak extra memory: torch.cuda.max_memory_allocated over one call, above what was allocated before it
(the library's workspace is allocated inside its first call and counted).  No threshold is set in advance: the file records what is measured,
whichever way the ratio falls."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(Path(__file__).resolve().parent))

NEW_KERNELS = ("ksum_partial_kernel", "ksum_finish_kernel", "kernel_matrix_kernel")


def plan_lines(n, m, d, subsets, subset_size):
    from fidelity_bench import kernel_resources
    from medfusion_amd import fidelity as F
    lines = []
    for title, s, size in ((f"kid, {subsets} subsets of {subset_size}", subsets, subset_size), ("mmd2 of the full sets", None, None)):
        p = F.plan_kid(n, m, s, size)
        pairs = sum(p["workgroups"].values()) * F.TILE * F.TILE
        lines.append(f"{title}, real [{n}, {d}] fake [{m}, {d}]: {sum(p['workgroups'].values())} workgroups in 3 launches + 3 finish launches, workspace "
                     f"{p['workspace_bytes'] / 2 ** 10:.1f} KiB, index lists {p['index_bytes'] / 2 ** 10:.1f} KiB, {2.0 * d * pairs / 1e12:.3f} TFLOP executed "
                     f"(the materialised form: {p['matrix_bytes'] / 2 ** 20:.1f} MiB of fp32 matrices)")
        lines += ["  " + x for x in p["launches"]]
    lines.append("new kernels of fidelity.hip (gfx950):")
    return lines + ["  " + r for r in kernel_resources() if r.startswith(NEW_KERNELS)]


def _mmd2_of(kxx, kyy, kxy):
    n, m = kxx.shape[-1], kyy.shape[-1]
    sxx = kxx.sum((-2, -1), dtype=kxx.dtype) - kxx.diagonal(dim1=-2, dim2=-1).sum(-1)
    syy = kyy.sum((-2, -1)) - kyy.diagonal(dim1=-2, dim2=-1).sum(-1)
    return sxx / (n * (n - 1)) + syy / (m * (m - 1)) - 2 * kxy.sum((-2, -1)) / (n * m)


def torch_mmd2(x, y, gamma, degree=3, coef0=1.0):
    """the plain-torch form: three fp32 matrices, a pow pass and a sum pass over each"""
    return _mmd2_of(*((gamma * (a @ b.t()) + coef0) ** degree for a, b in ((x, x), (y, y), (x, y))))


def torch_mmd2_chunked(x, y, gamma, rows, degree=3, coef0=1.0):
    """the same sums over row blocks of `rows` rows, accumulated in fp64: no matrix larger than rows x N"""
    import torch
    n, m = x.shape[0], y.shape[0]
    s = torch.zeros(3, dtype=torch.float64, device=x.device)
    for t, (a, b, same) in enumerate(((x, x, True), (y, y, True), (x, y, False))):
        for lo in range(0, a.shape[0], rows):
            k = (gamma * (a[lo:lo + rows] @ b.t()) + coef0) ** degree
            s[t] += k.sum(dtype=torch.float64)
            if same:
                s[t] -= k.diagonal(offset=lo).sum(dtype=torch.float64)
    return s[0] / (n * (n - 1)) + s[1] / (m * (m - 1)) - 2 * s[2] / (n * m)


def torch_kid_loop(x, y, ia, ib, gamma):
    import torch
    v = torch.stack([torch_mmd2(x[a], y[b], gamma) for a, b in zip(ia, ib)])
    return torch.stack([v.mean(), v.std(unbiased=False)]).tolist()


def torch_kid_batched(x, y, ia, ib, gamma, degree=3, coef0=1.0):
    import torch
    xs, ys = x[ia], y[ib]                                                       # [S, s, D]
    v = _mmd2_of(*((gamma * torch.bmm(a, b.transpose(1, 2)) + coef0) ** degree for a, b in ((xs, xs), (ys, ys), (xs, ys))))
    return torch.stack([v.mean(), v.std(unbiased=False)]).tolist()


def run(a):
    import torch

    import medfusion_amd as M
    from medfusion_amd import fidelity as F

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.backends.cuda.matmul.allow_tf32 = False
    lines = plan_lines(a.n, a.n, a.d, a.subsets, a.subset_size)
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

    def compare(title, forms, reps):
        outs, mem, times = {}, {}, {}
        for label, fn in list(forms.items()):
            try:
                outs[label], mem[label] = peak(fn)                             # (the warm-up of the form as well)
                fn()
                torch.cuda.synchronize()
            except torch.cuda.OutOfMemoryError:
                lines.append(f"{title} {label:16s} does not fit")
                del forms[label]
                torch.cuda.empty_cache()
        for label in forms:
            times[label] = []
        for _ in range(a.rounds):
            for label, fn in forms.items():
                times[label].append(timed(fn, reps))
        for label, ts in times.items():
            lines.append(f"{title} {label:16s} {' '.join(f'{t:10.3f}' for t in ts)} | median {sorted(ts)[len(ts) // 2]:10.3f} min {min(ts):10.3f} ms; "
                         f"peak extra memory {mem[label] / 2 ** 20:10.2f} MiB; result {outs[label]}")
        med = {label: sorted(ts)[len(ts) // 2] for label, ts in times.items()}
        others = {label: t for label, t in med.items() if label != "library"}
        if others:
            best = min(others, key=others.get)
            lines.append(f"{title}: library {med['library']:.3f} ms, fastest torch form ({best}) {others[best]:.3f} ms: measured ratio torch / library "
                         f"{others[best] / med['library']:.2f}" + (" (the library call is SLOWER)" if med["library"] > others[best] else "")
                         + f"; peak extra memory {mem['library'] / 2 ** 20:.2f} MiB against {mem[best] / 2 ** 20:.2f} MiB")

    def banks(rows, seed):
        """non-negative rows of a five-mode mixture, the generated bank from two of the modes: drawn on the device"""
        g = torch.Generator(device=dev).manual_seed(seed)
        centres = 0.2 * torch.randn(5, a.d, device=dev, generator=g) + 0.1
        draw = lambda modes: (centres[torch.randint(0, modes, (rows,), device=dev, generator=g)]
                              + 0.35 * torch.randn(rows, a.d, device=dev, generator=g)).clamp_min_(0)
        return draw(5), draw(2)

    gamma = float(torch.tensor(1.0 / a.d, dtype=torch.float64).float())
    real, fake = banks(a.n, 0)
    def lists():
        """the draw of kid itself: every form pays it inside its call"""
        return tuple(t.to(dev).long() for t in F.draw_subsets(a.n, a.n, a.subsets, a.subset_size, 0))

    import time
    draws = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lists()
        torch.cuda.synchronize()
        draws.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"the index draw alone ({2 * a.subsets} host randperm({a.n}) and the upload; host clock): {' '.join(f'{t:.3f}' for t in draws)} ms -- inside every kid time below")
    compare(f"kid {a.n} x {a.n} x {a.d}, {a.subsets} x {a.subset_size}",
            {"library": lambda: [M.kid(real, fake, subsets=a.subsets, subset_size=a.subset_size)[key] for key in ("kid_mean", "kid_std")],
             "torch loop": lambda: torch_kid_loop(real, fake, *lists(), gamma), "torch batched": lambda: torch_kid_batched(real, fake, *lists(), gamma)}, a.reps)
    compare(f"mmd2 {a.n} x {a.n} x {a.d}", {"library": lambda: M.mmd2(real, fake).item(), "torch": lambda: torch_mmd2(real, fake, gamma).item()}, a.reps)
    del real, fake
    torch.cuda.empty_cache()
    if a.big:
        real, fake = banks(a.big, 1)
        compare(f"mmd2 {a.big} x {a.big} x {a.d}", {"library": lambda: M.mmd2(real, fake).item(),
                                                    "torch chunked": lambda: torch_mmd2_chunked(real, fake, gamma, a.chunk).item(),
                                                    "torch": lambda: torch_mmd2(real, fake, gamma).item()}, max(1, a.reps // 2))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10000, help="rows of either bank")
    ap.add_argument("--d", type=int, default=2048, help="feature width")
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--subset-size", type=int, default=1000)
    ap.add_argument("--big", type=int, default=50000, help="rows of the large mmd2 comparison (0: skip it)")
    ap.add_argument("--chunk", type=int, default=5000, help="rows of a block of the chunked torch form")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kid_bench.txt"))
    ap.add_argument("--plan", action="store_true", help="print launches, workgroups, workspace and kernel resources, touch no device")
    a = ap.parse_args(argv)
    if a.n < 2 or a.d < 1 or a.subsets < 1 or not 2 <= a.subset_size <= a.n or a.big < 0 or a.chunk < 1 or a.reps < 1 or a.rounds < 1:
        ap.error("--n >= 2, --d >= 1, --subsets >= 1, 2 <= --subset-size <= --n, --big >= 0, --chunk, --reps and --rounds >= 1")
    if a.plan:
        print("\n".join(plan_lines(a.n, a.n, a.d, a.subsets, a.subset_size)))
        return 0
    run(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
