"""The launches of tests/test_pass_chain_gpu.py.  Run as a script -- `python tests/pass_chain_cases.py OUT.pt` -- it executes every case on the
library the process loads (MEDFUSION_LIB selects a twin of medfusion_amd.build.build_variant) and saves every output, so that two processes
on two libraries can be compared bit for bit.  Inputs are functions of the case alone; a tensor of more than 1 MB is saved as the SHA-256 of
its bytes.

The shapes are the smallest at which each code path of wino_tail_kernel and gn_apply_part_kernel (MF_PASS_CHAIN, csrc/split_f16.h) can go
wrong; every sample has its own scale, 2^6 apart, so that a bound, a residual row or a record taken from the wrong sample changes the bits.

The process sets MF_GN_BLOCKS_PER_CU=1 (the apply pass's grid cap, read once): with the product grid a workgroup of these small tensors would
never see a second round of x."""
import hashlib
import itertools
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

# ("tail", N, H, W, C, G): the rounds of phase 2 are H W (C / G) / 1024 -- 8 x 8 x 64 / 4: one round, three quarters of the threads idle in phases 1
# and 3; 16 x 16 x 128 / 8: exactly RJ = 4 rounds, nothing left for the loop behind them; 32 x 32 x 64 / 4: the 64 KB LDS edge, 16 rounds: the loop;
# 8 x 8 x 128 / 4: 32 channels per group
TAIL_CASES = [("tail", 2, 8, 8, 64, 4), ("tail", 1, 16, 16, 128, 8), ("tail", 1, 32, 32, 64, 4), ("tail", 2, 8, 8, 128, 4)]
# (residual kind, embedding, gamma / beta, fp32 output next to the pairs, V of the output) of the fp16-pair tail: every residual kind with every
# combination of outputs kernels.py asks for (conv2d_wino_gn_apply: pairs always; fp32 and V optional), embedding and affine on and off
TAIL_VARIANTS = [(r, e, a, f, v) for r, (e, a, f, v) in itertools.product(
    (None, "f32", "slots", "pairs"), ((True, True, True, True), (False, False, False, True), (True, False, True, False), (False, True, False, False)))]
# ... and 300 slots per sample, the largest of them behind the 256th: the first 256 come with the kernel's entry burst, the rest in a loop behind phase 1
TAIL_VARIANTS.append(("slots300", True, True, True, True))
# (residual, embedding, gamma / beta, V) of the fp32 tail (mf_wino_tail_f32: v_f32)
TAIL_F32_VARIANTS = [(None, False, False, True), ("f32", True, True, True), ("f32", False, True, False), (None, True, False, False)]
# ("apply", N, H, W, C, G, parts).  U (float4 per thread and round) is chosen by mf_gn_apply_from_partials_pairs_f32 from the workgroup count
# N H W C / 1024: 1 below 2048, 2 from 2048, 4 from 4096 -- the smallest tensor of each; with the grid cap of this process (256 / N workgroups per
# sample) the two large ones run 4 rounds per workgroup.  C = 96: 256 % (C / 4) != 0, the channel constants are fetched per element (G = 32:
# groups of 3 channels, a float4 spans two).  5 x 61 x 64 and 6 x 10 x 328 at N = 16: 16 workgroups per sample, a second round that is ragged
# (4880 = 4096 + 784 float4; 4920 = 4096 + 824).  parts = 9 > 256 / G = 8: a second record per thread.
APPLY_CASES = [("apply", 2, 16, 16, 64, 8, 3), ("apply", 2, 16, 16, 96, 8, 3), ("apply", 2, 16, 16, 96, 32, 3), ("apply", 16, 5, 61, 64, 8, 2),
               ("apply", 16, 6, 10, 328, 8, 3), ("apply", 2, 32, 32, 1024, 32, 9), ("apply", 4, 32, 32, 1024, 32, 9)]
# (residual kind, embedding, gamma / beta, fp32 output next to the pairs)
APPLY_VARIANTS = [(None, True, True, True), ("f32", False, True, False), ("slots", True, False, True), ("pairs", True, True, False), ("pairs", False, False, True),
                  ("slots", False, True, False), ("slots300", True, True, True)]
APPLY_VARIANTS_LARGE = [("pairs", True, True, False), ("slots", True, True, True)]
CASES = TAIL_CASES + APPLY_CASES


def case_id(case) -> str:
    return "-".join(str(v) for v in case)


def variants(case):
    if case[0] == "tail":
        return [("f16",) + v for v in TAIL_VARIANTS] + [("f32",) + v for v in TAIL_F32_VARIANTS]
    return APPLY_VARIANTS_LARGE if case[1] * case[2] * case[3] * case[4] >= 2048 * 1024 else APPLY_VARIANTS


def _gen(case):
    import torch
    return torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(case_id(case))))


def _keep(out: dict) -> dict:
    import torch
    torch.cuda.synchronize()
    res = {}
    for k, v in out.items():
        t = v.detach().cpu().contiguous()
        res[k] = t.clone() if t.numel() * t.element_size() <= (1 << 20) else (tuple(t.shape), str(t.dtype), hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest())
    return res


def _residual(kind, r, K, dev):
    """a fresh residual tensor of the kind: plain fp32 (its bound measured), a measured convolution output (bound still as slot maxima), pairs only"""
    import torch
    if kind is None:
        return None
    r = r.clone()
    if kind == "pairs":
        K.split_of(r)
        r._mf_pairs_only = True
    elif kind in ("slots", "slots300"):
        sl = torch.zeros((r.shape[0], 7 if kind == "slots" else 300), device=dev)
        sl[:, 3 if kind == "slots" else 290] = r.abs().amax(dim=(1, 2, 3))
        sl[:, 5] = 0.25 * sl.amax(dim=1)
        r._mf_slots = sl
        K._stamp(r)
    return r


def run_tail(case, dev) -> dict:
    import ctypes as C
    import torch
    from medfusion_amd import kernels as K, lib as L
    _, n, h, w, c, G = case
    g = _gen(case)
    cpg = c // G
    res = {}
    # ---- the fp16-pair tail behind its component GEMM (mf_conv2d_wino_gn_apply_f16x2).  The GEMM needs a tile whose rows divide a component's
    # N (H/2)(W/2) rows and whose columns divide C (64 channels: 128 rows): the two 8 x 8 cases run this entry at the smallest multiple of their N
    # the planner takes, and at their own N = 2 on the fp32 entry below, which takes M as it is
    nf = next(k * n for k in (1, 2, 4, 8, 16) if K.wino_tail_ok(K.make_conv_desc(k * n, h, w, c, 0, c, 3, 1, 1, 0, precision=5), G))
    sc = torch.tensor([2.0 ** (6 * i - 3) for i in range(nf)]).view(nf, 1, 1, 1)
    x = K.nchw_to_nhwc((torch.randn((nf, c, h, w), generator=g) * sc).to(dev))
    wt = torch.randn((c, c, 3, 3), generator=g) / float(c * 9) ** 0.5
    b = (torch.randn((c,), generator=g) * 0.1).to(dev)
    gamma, beta = (1.0 + 0.3 * torch.randn((c,), generator=g)).to(dev), (0.2 * torch.randn((c,), generator=g)).to(dev)
    r0 = (torch.randn((nf, h, w, c), generator=g) * 2.0 * sc.flip(0)).to(dev)
    emb = (torch.randn((nf, c + 8), generator=g) * 0.5 * sc.view(nf, 1)).to(dev)[:, 8:]     # (a row stride that is not C)
    uh = K.split_weight_f16x2(K.wino_pack_weight(wt.to(dev)))
    d = K.make_conv_desc(nf, h, w, c, 0, c, 3, 1, 1, 0, precision=5)
    assert K.wino_tail_ok(d, G), case
    for var in variants(case):
        if var[0] != "f16":
            continue
        _, rkind, has_emb, affine, out_fp32, want_v = var
        bconst = (float(gamma.abs().max()) * (h * w * cpg) ** 0.5 + float(beta.abs().max())) if affine else float((h * w * cpg) ** 0.5)
        got = K.conv2d_wino_gn_apply(x, uh, b, d, gamma if affine else None, beta if affine else None, G, 1e-5, act=1, residual=_residual(rkind, r0, K, dev),
                                     emb=emb if has_emb else None, emb_stride=emb.stride(0) if has_emb else 0, bconst=bconst, out_fp32=out_fp32, want_wino=want_v)
        out = {"pairs": got._mf_split, "out_bound": got._mf_bound}
        if out_fp32:
            out["y"] = got
        else:
            assert K.pairs_only(got)
        if want_v:
            out["v"], out["wino_bound"] = got._mf_wino, got._mf_wino_bound
        res[str(var)] = _keep(out)
    # ---- the fp32 tail (mf_wino_tail_f32) on an M of its own, at the case's N
    t = (h // 2) * (w // 2)
    sc = torch.tensor([2.0 ** (6 * i - 3) for i in range(n)]).view(1, n, 1, 1)
    m = (torch.randn((16, n, t, c), generator=g) * sc).to(dev)
    r1 = (torch.randn((n, h, w, c), generator=g) * 2.0).to(dev)
    emb1 = (torch.randn((n, c + 8), generator=g) * 0.5).to(dev)[:, 8:]
    for var in variants(case):
        if var[0] != "f32":
            continue
        _, rkind, has_emb, affine, want_v = var
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=dev)
        ov = torch.empty((16, n, t, c), dtype=torch.float32, device=dev) if want_v else None
        ptr = lambda a: None if a is None else a.data_ptr()
        rc = L.load().mf_wino_tail_f32(m.data_ptr(), b.data_ptr(), ptr(gamma if affine else None), ptr(beta if affine else None), ptr(r1 if rkind else None),
                                       ptr(emb1 if has_emb else None), emb1.stride(0) if has_emb else 0, out.data_ptr(), ptr(ov), n, h, w, c, G, 1, 1e-5, K.stream())
        L.check(rc, "mf_wino_tail_f32")
        o = {"y": out}
        if want_v:
            o["v"] = ov
        res[str(var)] = _keep(o)
    return res


def run_apply(case, dev) -> dict:
    import torch
    from medfusion_amd import kernels as K
    _, n, h, w, c, G, parts = case
    g = _gen(case)
    cpg, hw = c // G, h * w
    sc = torch.tensor([2.0 ** (6 * i - 3) for i in range(n)]).view(n, 1, 1, 1)
    y = (torch.randn((n, h, w, c), generator=g) * sc + 0.5 * sc).to(dev)
    # the records a convolution would have left: {sum, sum of squares} of `parts` pixel ranges per (sample, group), fp64
    yd = y.double().reshape(n, hw, G, cpg)
    cuts = [hw * k // parts for k in range(parts + 1)]
    rec = torch.stack([torch.stack([yd[:, a:b].sum(dim=(1, 3)), (yd[:, a:b] ** 2).sum(dim=(1, 3))], dim=-1) for a, b in zip(cuts, cuts[1:])], dim=1).contiguous()
    assert rec.shape == (n, parts, G, 2)
    del yd
    gamma, beta = (1.0 + 0.3 * torch.randn((c,), generator=g)).to(dev), (0.2 * torch.randn((c,), generator=g)).to(dev)
    r0 = (torch.randn((n, h, w, c), generator=g) * 2.0 * sc.flip(0)).to(dev)
    emb = (torch.randn((n, c + 8), generator=g) * 0.5 * sc.view(n, 1)).to(dev)[:, 8:]
    res = {}
    for var in variants(case):
        rkind, has_emb, affine, out_fp32 = var
        bconst = (float(gamma.abs().max()) * (hw * cpg) ** 0.5 + float(beta.abs().max())) if affine else float((hw * cpg) ** 0.5)
        got = K.gn_apply(y, K.GnPartials(rec, parts, 1e-5), gamma if affine else None, beta if affine else None, G, 1, _residual(rkind, r0, K, dev),
                         emb if has_emb else None, emb.stride(0) if has_emb else 0, split=True, bconst=bconst, out_fp32=out_fp32)
        out = {"pairs": got._mf_split, "out_bound": got._mf_bound}
        if out_fp32:
            out["y"] = got
        else:
            assert K.pairs_only(got)
        res[str(var)] = _keep(out)
    if case[1] * hw * c < 2048 * 1024:     # the pass without the pair mirror (SPLIT = false), once per small case
        res["plain"] = _keep({"y": K.gn_apply(y, K.GnPartials(rec, parts, 1e-5), gamma, beta, G, 1, r0.clone(), emb, emb.stride(0))})
    return res


def main():
    os.environ["MF_GN_BLOCKS_PER_CU"] = "1"
    sys.path.insert(0, str(ROOT))
    import torch
    dev = torch.device("cuda:0")
    res = {}
    for case in CASES:
        res[case_id(case)] = run_tail(case, dev) if case[0] == "tail" else run_apply(case, dev)
        print("ran", case_id(case), flush=True)
    torch.save(res, sys.argv[1])


if __name__ == "__main__":
    main()
