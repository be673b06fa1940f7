#!/usr/bin/env python3
"""What the Inception features cost on the device (medfusion_amd.inception): whole calls between device events, the median of --reps after a warm-up,
seeded weights, --batch byte images (100: the reference script's batch) at 299 x 299 -- and, next to it, the plain-torch form of the same definition
(F.conv2d with the folded weights, the pools, fp32) on the same device in the same process, with the distance between the two results.  The
convolution launches are timed on their own (the library's launch timing) for their TFLOP/s against the 157.3 TF fp32-matrix peak.

  python scripts/inception_bench.py --plan                 # no device: launches, workgroups, bytes, flops, kernel resources
  python scripts/inception_bench.py --reps 5 --out profiles/inception_bench.txt"""
import argparse
import json
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

PEAK_TF = 157.3


def kernel_resources():
    """VGPRs, LDS, scratch and spills of the kernels of inception.hip and of the kernels of cnn_layers.hip the network runs (the convolution and the
    window-3 pool), from the device assembly the build's ISA lint keeps"""
    from medfusion_amd import build as B
    out, cur = [], {}
    for unit, used in (("cnn_layers.hip", ("conv_gemm_kernel", "pool_nhwc_kernel<3>")), ("inception.hip", None)):
        asm = B.OBJ / "lint" / (Path(unit).stem + ".s")
        if not asm.exists() or asm.stat().st_mtime < (B.CSRC / unit).stat().st_mtime:
            B.lint_isa()
        for line in asm.read_text().splitlines():
            mt = re.match(r"\s*\.(name|vgpr_count|agpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|sgpr_spill_count|vgpr_spill_count):\s*(\S+)", line)
            if not mt:
                continue
            cur[mt.group(1)] = mt.group(2)
            if mt.group(1) == "vgpr_spill_count":
                name = re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", cur.get("name", "?"))
                args = re.findall(r"Li(\d+)E", name.split("Ev")[0])
                short = re.match(r"[a-z0-9_]+kernel", name).group(0) + (f"<{', '.join(args)}>" if args else "")
                if used is None or any(short.startswith(u) for u in used):
                    out.append(f"{short:34s} vgpr {cur.get('vgpr_count'):>3s} (agpr {cur.get('agpr_count', '0'):>3s})  sgpr {cur.get('sgpr_count'):>3s}  lds {cur.get('group_segment_fixed_size'):>5s} B  "
                               f"scratch {cur.get('private_segment_fixed_size')} B  spilled sgprs {cur.get('sgpr_spill_count')} vgprs {cur.get('vgpr_spill_count')}")
                cur = {}
    return out


def torch_form(net, x, size):
    """the definition in plain torch on the device x lives on (fp32, NCHW): the library's resize, then F.conv2d / pools of ATen"""
    import torch
    import torch.nn.functional as F

    from medfusion_amd import inception as I
    from medfusion_amd import kernels as K
    from medfusion_amd import lib as L
    ws = getattr(net, "_torch_form", None)
    if ws is None:
        ws = net._torch_form = [tuple(t.to(x.device) for t in net.folded(i)) for i in range(len(I.LAYERS))]
    bufs = {"in": K.inception_prepare(x, size).permute(0, 3, 1, 2).contiguous()}
    parts = {}
    for op in I.OPS:
        if op[0] == "tap":
            if op[1] == "2048":
                return _whole(bufs, parts, op[2]).mean(dim=(2, 3))
            continue
        if op[0] == "conv":
            _, _, _, _, _, s, ph, pw = I.LAYERS[op[1]]
            src, dst, off = op[2], op[3], op[4]
            y = torch.relu(F.conv2d(_whole(bufs, parts, src), ws[op[1]][0], ws[op[1]][1], stride=s, padding=(ph, pw)))
        else:
            src, dst, off = op[1], op[2], op[6]
            xin = _whole(bufs, parts, src)
            y = F.max_pool2d(xin, 3, op[3], op[4]) if op[5] == L.POOL_MAX else F.avg_pool2d(xin, 3, op[3], op[4], count_include_pad=False)
        if I.WIDTH[dst] == y.shape[1]:
            bufs[dst] = y
        else:
            parts.setdefault(dst, []).append((off, y))


def _whole(bufs, parts, name):
    import torch
    if name not in bufs:
        bufs[name] = torch.cat([t for _, t in sorted(parts[name], key=lambda p: p[0])], dim=1)
    return bufs[name]


def plan_lines(batch, size):
    from medfusion_amd import inception as I
    p = I.plan(batch, size)
    tiles = {}
    for r in p["layers"]:
        if "tile" in r:
            tiles[r["tile"]] = tiles.get(r["tile"], 0) + 1
    lines = [f"plan: {batch} images at {size} x {size}: {p['launches']} launches per pass ({p['conv_launches']} mf_conv2d_gemm_f32 with the fc, "
             f"{p['launches'] - p['conv_launches'] - 2} pools, the resize, the mean), {p['workgroups']} convolution workgroups, {p['flops'] / 1e9:.1f} GFLOP, "
             f"activations {p['activation_bytes'] / 2 ** 20:.0f} MiB (largest {p['largest_activation_bytes'] / 2 ** 20:.0f} MiB), weights {p['weight_bytes'] / 2 ** 20:.1f} MiB, "
             f"at most {I.default_chunk(size)} images per pass by default ({-(-batch // I.default_chunk(size))} passes of equal size)",
             "tiles (1: 128 x 128, 2: 128 x 64, 3: 64 x 64): " + ", ".join(f"{k}: {v} layers" for k, v in sorted(tiles.items()))]
    return p, lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--plan", action="store_true", help="no device: the launches, bytes and flops of a pass and the kernels' resources")
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--size", type=int, default=299)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args(argv)
    p, lines = plan_lines(args.batch, args.size)
    lines += ["kernel resources (gfx950):"] + ["  " + r for r in kernel_resources()]
    row = {"batch": args.batch, "size": args.size, "launches": p["launches"], "conv_launches": p["conv_launches"], "gflop": round(p["flops"] / 1e9, 2)}
    if not args.plan:
        import torch

        from medfusion_amd import inception as I
        from medfusion_amd import lib as L
        dev = torch.device("cuda")
        net = I.InceptionNet.seeded(args.seed).to(dev)
        x = torch.randint(0, 256, (args.batch, 3, args.size, args.size), generator=torch.Generator().manual_seed(args.seed), dtype=torch.uint8).to(dev)

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = fn()
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            return sorted(ms)[len(ms) // 2], out

        ours_ms, ours = timed(lambda: net.features(x, size=args.size))
        torch_ms, theirs = timed(lambda: torch_form(net, x, args.size))
        rel = float((ours - theirs).abs().max() / theirs.abs().max())
        lib = L.load()
        lib.mf_prof_enable(1)
        lib.mf_prof_reset()
        net.features(x, size=args.size)
        torch.cuda.synchronize()
        import ctypes as C
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        lib.mf_prof_query(0, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by))
        lib.mf_prof_enable(0)
        conv_tf = fl.value / (ms.value * 1e-3) / 1e12 if ms.value > 0 else 0.0
        lines += [f"library: {ours_ms:.2f} ms per call, {args.batch / ours_ms * 1e3:.1f} images/s (median of {args.reps})",
                  f"plain torch (F.conv2d, fp32, same device, same process): {torch_ms:.2f} ms per call, {args.batch / torch_ms * 1e3:.1f} images/s; library / torch time = {ours_ms / torch_ms:.2f}",
                  f"max |library - torch| / max |torch| of the 2048 features: {rel:.3e}",
                  f"convolution launches: {n.value} launches, {ms.value:.2f} ms, {conv_tf:.1f} TFLOP/s = {100 * conv_tf / PEAK_TF:.1f} % of the {PEAK_TF} TF fp32-matrix peak"]
        row.update(library_ms=round(ours_ms, 3), torch_ms=round(torch_ms, 3), images_per_s=round(args.batch / ours_ms * 1e3, 2), torch_images_per_s=round(args.batch / torch_ms * 1e3, 2),
                   conv_ms=round(ms.value, 3), conv_tflops=round(conv_tf, 2), rel_diff=rel)
    lines.append(json.dumps(row))
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
