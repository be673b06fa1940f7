#!/usr/bin/env python3
"""What LPIPS costs on the device (medfusion_amd.lpips): whole calls between device events, after a warm-up, for both trunks at the default
arithmetic -- 100 pairs of 3 x 256 x 256 (the reference script's batch) and 4 pairs of 1 x 64 x 128 x 128 volumes, slice by slice -- and, next to
each, the plain-torch form of the same definition (F.conv2d, F.max_pool2d) on the same device in the same process with the same seeded weights, with
the distance between the two results.

  python scripts/lpips_bench.py --plan                 # no device: layers, launches, workspace, kernel resources
  python scripts/lpips_bench.py --reps 5 --out profiles/lpips_bench.txt"""
import argparse
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

IMAGES = (100, 3, 256, 256)
VOLUMES = (4, 1, 64, 128, 128)
NETS = ("vgg", "alex")
UNITS = ("lpips.hip", "cnn_layers.hip")
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)


def kernel_resources():
    """VGPRs, LDS and scratch of the kernels of lpips.hip and of the general layers of cnn_layers.hip (the trunk runs every one of them: the convolution
    under mf_conv2d_direct_f32, both pool windows, the ReLU), from the device assembly the build's ISA lint keeps"""
    from medfusion_amd import build as B
    out, cur = [], {}
    for unit in UNITS:
        asm = B.OBJ / "lint" / (Path(unit).stem + ".s")
        if not asm.exists() or asm.stat().st_mtime < (B.CSRC / unit).stat().st_mtime:
            B.lint_isa()
        for line in asm.read_text().splitlines():
            mt = re.match(r"\s*\.(name|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count):\s*(\S+)", line)
            if not mt:
                continue
            cur[mt.group(1)] = mt.group(2)
            if mt.group(1) == "vgpr_spill_count":
                name = re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", cur.get("name", "?"))
                flags = ", ".join(v if kind == "i" else ("false", "true")[int(v)] for kind, v in re.findall(r"L([bi])(\d+)E", name.split("Ev")[0]))
                short = re.match(r"[a-z0-9_]+kernel", name).group(0) + (f"<{flags}>" if flags else "")
                out.append(f"{short:32s} vgpr {cur.get('vgpr_count'):>3s}  sgpr {cur.get('sgpr_count'):>3s}  lds {cur.get('group_segment_fixed_size'):>5s} B  "
                           f"scratch {cur.get('private_segment_fixed_size')} B  spilled vgprs {cur.get('vgpr_spill_count')}")
                cur = {}
    return out


def plan_rows():
    from medfusion_amd import lpips as LP
    rows = []
    for net in NETS:
        for label, (h, w) in (("256 x 256 image", IMAGES[2:]), ("128 x 128 slice", VOLUMES[3:])):
            p = LP.plan(net, h, w)
            direct = [l["key"] for l in p["layers"] if l["kernel"] == "mf_conv2d_direct_f32"]
            step = max(1, LP.PIXEL_BUDGET // (h * w))
            rows.append(f"{net:4s} {label}: {p['launches']} launches per trunk pass, taps {p['taps']}, mf_conv2d_direct_f32 on {direct}, distance workspace "
                        f"{p['workspace_bytes']} B per pair, {step} pairs per pass by default (largest activation {step * p['activation_bytes'] / 2 ** 20:.0f} MiB)")
    return rows


def torch_form(net, x, y):
    """the definition in plain torch on the device the tensors live on (fp32, NCHW)"""
    import torch
    import torch.nn.functional as F
    from medfusion_amd.lpips import OPS

    def taps(t):
        if t.shape[1] == 1:
            t = t.expand(-1, 3, -1, -1)
        h = (t - torch.tensor(SHIFT, device=t.device).view(1, 3, 1, 1)) / torch.tensor(SCALE, device=t.device).view(1, 3, 1, 1)
        out, i = [], 0
        for op in OPS[net.net]:
            if op[0] == "conv":
                w, b = net._torch_convs[i]
                i += 1
                h = F.relu(F.conv2d(h, w, b, stride=op[5], padding=op[6]))
            elif op[0] == "pool":
                h = F.max_pool2d(h, op[1], op[2])
            else:
                out.append(h)
        return out

    total = 0
    for a, b, w in zip(taps(x), taps(y), net._torch_lins):
        an = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        bn = b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        total = total + ((an - bn).pow(2) * w.view(1, -1, 1, 1)).sum(1).mean((1, 2))
    return total


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return out, sorted(times)[len(times) // 2], min(times), max(times)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--plan", action="store_true", help="no device: the plan and the kernels' resources")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args(argv)
    lines = plan_rows() + ["kernels of lpips.hip and cnn_layers.hip (gfx950):"] + ["  " + r for r in kernel_resources()]
    if not args.plan:
        import torch
        from medfusion_amd import lpips as LP
        dev = torch.device("cuda")
        g = torch.Generator().manual_seed(0)
        for net_name in NETS:
            net = LP.LPIPSNet.seeded(net_name, 1, 0.05).to(dev)
            net._torch_convs = [(w.to(dev), b.to(dev)) for w, b in net.convs]
            net._torch_lins = [v.to(dev) for v in net.lins]
            for label, shape in (("100 pairs of 3 x 256 x 256", IMAGES), ("4 pairs of 1 x 64 x 128 x 128, slice by slice", VOLUMES)):
                x = (torch.rand(shape, generator=g) * 2 - 1).to(dev)
                y = (x + 0.3 * torch.randn(shape, generator=g).to(dev)).clamp(-1, 1)
                got, med, lo, hi = timed(lambda: LP.lpips(x, y, net), args.reps)

                def ref():
                    if x.dim() == 4:
                        return torch.cat([torch_form(net, x[i:i + 16], y[i:i + 16]) for i in range(0, x.shape[0], 16)])
                    return torch.stack([torch_form(net, x[i].transpose(0, 1), y[i].transpose(0, 1)).mean() for i in range(x.shape[0])])
                with torch.no_grad():
                    want, tmed, tlo, thi = timed(ref, args.reps)
                rel = float(((got.double() - want.double()).abs() / want.double()).max())
                lines.append(f"{net_name:4s} {label}: library {med:.1f} ms (min {lo:.1f}, max {hi:.1f}; {args.reps} calls after a warm-up), torch form {tmed:.1f} ms "
                             f"(min {tlo:.1f}, max {thi:.1f}); largest relative distance of the two results {rel:.2e}; mean LPIPS {float(got.mean()):.4f}")
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
