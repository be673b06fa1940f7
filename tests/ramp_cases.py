"""The launches of tests/test_conv_ramp_gpu.py.  Run as a script -- `python tests/ramp_cases.py OUT.pt` -- it executes every case on the library
the process loads (MEDFUSION_LIB selects a twin of medfusion_amd.build.build_variant) and saves every output tensor, so that two processes
on two libraries can be compared bit for bit.  Inputs are functions of the case alone.

The shapes are the smallest at which the ramp of the fp16-pair convolution kernels can go wrong (bounds fetched early, exponents carried
through the loop, the kernel argument read in two places); every sample and every source has its own scale, 2^10 apart or more, so that an
exponent taken from the wrong sample, the wrong source or a stale register changes the bits of the result."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

# ("conv", N, H, W, C1, C2, Cout, k, stride, ups, tile, split-K)
CONV_CASES = [
    ("conv", 4, 8, 8, 64, 0, 128, 3, 1, 0, 33, 1),      # two samples inside one 128-row tile: lanes of one wave read different bounds (TM = 2)
    ("conv", 4, 8, 8, 64, 0, 128, 3, 1, 0, 34, 1),      # ... TM = 1
    ("conv", 2, 16, 16, 32, 64, 128, 3, 1, 0, 53, 1),   # two sources, the switch in the middle of the K loop (it_sw = 9)
    ("conv", 2, 16, 16, 32, 64, 128, 3, 1, 0, 53, 2),   # ... and a split-K slice that STARTS in the second source (chunks [0, 1] | [2])
    ("conv", 2, 16, 16, 32, 64, 128, 3, 1, 0, 33, 1),
    ("conv", 3, 8, 8, 64, 0, 128, 3, 1, 0, 33, 1),      # M = 192 on 128-row tiles: rows past M (the clamp of the bound index)
    ("conv", 3, 8, 8, 64, 0, 128, 3, 1, 0, 34, 1),
    ("conv", 2, 8, 8, 32, 0, 128, 1, 1, 0, 53, 1),      # one chunk: nit < NST, the prologue's own vmcnt(0)
    ("conv", 2, 8, 8, 64, 0, 128, 1, 1, 0, 53, 1),      # two chunks
    ("conv", 2, 8, 8, 32, 0, 128, 1, 1, 0, 51, 1),      # (NST = 2)
    ("conv", 2, 16, 16, 128, 0, 128, 3, 2, 0, 53, 2),   # split-K tree, stride 2
    ("conv", 2, 16, 16, 128, 0, 128, 3, 2, 0, 53, 4),
    ("conv", 2, 8, 8, 64, 0, 128, 3, 1, 2, 53, 1),      # sub-pixel up-convolution 8 x 8 -> 16 x 16 (Cout = 64 has no tile at 8 x 8: BM | 64 and BN | 64)
    ("conv", 2, 16, 16, 64, 0, 64, 3, 1, 2, 54, 1),     # ... 64 -> 64 at the smallest source grid a 64-column tile takes
    ("conv", 1, 32, 32, 64, 0, 128, 3, 1, 0, 62, 1),    # halo tile <256,128,4,2,7>
    ("conv", 3, 16, 16, 64, 64, 128, 3, 1, 0, 62, 2),   # ... two sources, split-K, one whole image per tile
]
# ("wino", N, H, W, C1, C2, Cout): the component GEMMs run through the descriptor with upsample = 3 and wphase_rows
WINO_CASES = [("wino", 4, 8, 8, 64, 0, 128), ("wino", 4, 8, 8, 32, 64, 128), ("wino", 2, 16, 16, 64, 0, 128)]
# ("group", N, H, W, C1, C2, Cout, tile of the 3x3, its split-K, tile of conv_res): tests.util.GROUP_CASES
GROUP_CASES = [("group", 2, 16, 16, 64, 0, 128, 53, 1, 53), ("group", 2, 32, 32, 64, 64, 128, 62, 1, 36), ("group", 3, 16, 16, 64, 32, 128, 54, 2, 53)]
CASES = CONV_CASES + WINO_CASES + GROUP_CASES
GN_GROUPS = 8


def case_id(case) -> str:
    return "-".join(str(v) for v in case)


def operands(case):
    """(x1 NCHW, x2 NCHW or None, weight OIHW, bias) on the CPU: sample i of x1 is scaled by 2^(10 i - 5), x2 by another 2^-13"""
    import torch
    kind, n, h, w, c1, c2, co = case[:7]
    k = case[7] if kind == "conv" else 3
    g = torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(case_id(case))))
    sc = torch.tensor([2.0 ** (10 * i - 5) for i in range(n)]).view(n, 1, 1, 1)
    x1 = torch.randn((n, c1, h, w), generator=g) * sc
    x2 = torch.randn((n, c2, h, w), generator=g) * sc * 2.0 ** -13 if c2 else None
    wt = torch.randn((co, c1 + c2, k, k), generator=g) / float((c1 + c2) * k * k) ** 0.5
    b = torch.randn((co,), generator=g) * 0.1
    return x1, x2, wt, b


def run_case(case, dev) -> dict:
    import torch
    from medfusion_amd import kernels as K
    kind, n, h, w, c1, c2, co = case[:7]
    x1, x2, wt, b = operands(case)
    xd = K.nchw_to_nhwc(x1.to(dev))
    x2d = K.nchw_to_nhwc(x2.to(dev)) if c2 else None
    bd = b.to(dev)
    out = {}
    if kind == "conv":
        k, stride, ups, tile, sk = case[7:]
        pad = 1 if k == 3 else 0
        wp = K.pack_upconv_weight(wt.to(dev)) if ups == 2 else K.pack_conv_weight(wt.to(dev))
        wh = K.split_weight_f16x2(wp)
        d = K.make_conv_desc(n, h, w, c1, c2, co, k, stride, pad, ups, tile_hint=tile, splitk_hint=sk, precision=5)
        assert K.conv_f16x2_ok(d) and K.conv_plan(d) == (tile, sk), (case, K.conv_plan(d))
        y = K.conv2d_f16x2(xd, wh, bd, d, x2=x2d, measure_out=True)
        out["y"] = y
        if getattr(y, "_mf_slots", None) is not None:
            out["slots"] = y._mf_slots
        parts = K.conv_gn_parts(d, GN_GROUPS)
        if parts:
            y2, partial = K.conv2d_f16x2(xd, wh, bd, d, x2=x2d, gn_groups=GN_GROUPS, gn_parts=parts)
            out["y_gn"], out["records"] = y2, partial
    elif kind == "wino":
        uh = K.split_weight_f16x2(K.wino_pack_weight(wt.to(dev)))
        d = K.make_conv_desc(n, h, w, c1, c2, co, 3, 1, 1, 0, precision=5)
        assert K.wino_ok(d), case
        out["y"] = K.conv2d_wino_f16x2(xd, uh, bd, d, x2=x2d)
        parts = K.wino_gn_parts(d, GN_GROUPS)
        assert parts > 0, case
        y2, partial = K.conv2d_wino_f16x2(xd, uh, bd, d, x2=x2d, gn_groups=GN_GROUPS, gn_parts=parts)
        out["y_gn"], out["records"] = y2, partial
    else:
        ta, ska, tb = case[7:]
        g = torch.Generator().manual_seed(7)
        w1 = torch.randn((co, c1 + c2, 1, 1), generator=g) / float(c1 + c2) ** 0.5
        b1 = (torch.randn((co,), generator=g) * 0.1).to(dev)
        wh3, wh1 = K.split_weight_f16x2(K.pack_conv_weight(wt.to(dev))), K.split_weight_f16x2(K.pack_conv_weight(w1.to(dev)))
        da = K.make_conv_desc(n, h, w, c1, c2, co, 3, 1, 1, 0, tile_hint=ta, splitk_hint=ska, precision=5)
        db = K.make_conv_desc(n, h, w, c1, c2, co, 1, 1, 0, 0, tile_hint=tb, precision=5)
        pa, pb = K.pin_conv_plan(da), K.pin_conv_plan(db)
        parts = K.conv_gn_parts(da, GN_GROUPS)
        assert parts > 0 and pb[1] > 0 and K.conv_group_ok(da, GN_GROUPS, db, 0), case
        (y, part), r = K.conv2d_f16x2_group(xd, x2d, dict(w_split=wh3, bias=bd, d=da, gn_groups=GN_GROUPS, gn_parts=parts, pinned=pa),
                                            dict(w_split=wh1, bias=b1, d=db, pinned=pb))
        out.update(y=y, records=part, res=r, slots=r._mf_slots)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def main():
    sys.path.insert(0, str(ROOT))
    import torch
    dev = torch.device("cuda:0")
    res = {}
    for case in CASES:
        res[case_id(case)] = run_case(case, dev)
        print("ran", case_id(case), flush=True)
    torch.save(res, sys.argv[1])


if __name__ == "__main__":
    main()
