"""The 2-D convolutions (csrc/conv_f16x2.hip with its two bodies, csrc/conv.hip) at their edges: references, exact operands, the host rules
restated in Python and the case lists of tests/test_conv2d_cpu.py and tests/test_conv2d_gpu.py.  Plain Python and torch, no device.

Exact operands (tests/conv3d_cases.py has the argument; its dimension-free helpers are imported, not copied).  Three families:
  * "xlo" / "wlo": activations (weights) a + b 2^-13 with a in {-1, 0, 1}, |b| <= 3 carry a non-zero lo' part, the other operand is in {-1, 0, 1}: the
    lo.lo term the fp16-pair kernel drops is identically zero and hi.hi, hi.lo', lo'.hi are all exercised.  Exact on the pair arithmetic
    (precision 5), on the fp32 matrix cores (precision 0), on the fp32 fma chains of the direct kernels and -- split_bf16x3 below: x = a + b 2^-13
    splits into the bf16 terms (a, b 2^-13, 0), so the three products the triplet mode drops are zero -- on precision 3.
  * "int8": integer activations |x| <= 127 times the sample's scale, weights in {-1, 0, 1}, no lo part: exact on EVERY arithmetic, the single-term
    fp16 (precision 6: 7 bits fit the 11 of fp16) and the plain bf16 mode (precision 4: 7 bits fit the 8 of bf16) included.
Samples are scaled 2^0, 2^20, 2^-20; two-source cases take the conv3d construction (ratio +-20 or "mixed", the LARGER source sparse and alone
in carrying the lo part); the bias is k 2^20 on every third channel.  Every product is a whole multiple of the sample's output unit u and
sum |w||x| < 2^24 u, so every partial sum of every accumulator, slab and hand-off is exact in fp32 and the kernel must return float32(ref64) bit
for bit on every tile and split-K plan.  exact_budget() states the conditions on the form the kernel really multiplies (the four 2 x 2 phase
filters of the sub-pixel form included); the CPU test asserts them for every case of every family.

No constant of this file comes from a run of the kernels: tables restate the sources (the line each restates is named), sizes follow from
the launch arithmetic quoted next to them."""

import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests.conv3d_cases import (LO_BITS, RATIO_INSIDE, SAMPLE_EXPS, _ints, _is_multiple, _log2, _product_unit, _seed_of, _sparse, _unit_exp,  # noqa: F401
                                _with_lo, bias_add_rounds_once, pair_terms, real_operands, scale_exp)

# ---------------------------------------------------------------------------------------------------------------- the host rules, restated
# kTiles2 of conv_f16x2.hip: id -> (BM, BN, WM, WN, NST, HG)
TILES2 = {31: (128, 256, 2, 4, 3, 0), 32: (256, 128, 4, 2, 3, 0), 33: (128, 128, 2, 4, 3, 0), 34: (128, 128, 4, 2, 3, 0), 35: (256, 64, 4, 2, 3, 0),
          36: (128, 64, 4, 2, 3, 0), 37: (64, 256, 1, 8, 3, 0),
          51: (128, 128, 2, 2, 2, 0), 52: (128, 128, 2, 2, 3, 0), 53: (64, 128, 2, 2, 3, 0), 54: (128, 64, 2, 2, 3, 0),   # 4-wave workgroups, two per CU
          61: (256, 128, 4, 2, 3, 6), 62: (256, 128, 4, 2, 3, 7), 63: (128, 128, 2, 4, 3, 4), 64: (128, 128, 2, 4, 3, 5)}   # halo tiles (3x3 stride 1 pad 1)
F16X2_TILES = {t: v[:2] for t, v in TILES2.items()}                       # tile -> (BM, BN)
HALO_HG = {t: (v[5], v[2] * v[3]) for t, v in TILES2.items() if v[5]}     # tile -> (halo pieces per wave, waves)
# kCfgs of conv.hip: id -> (BM, BN, WM, WN, BK)
IGEMM_CFGS = {1: (128, 128, 2, 2, 32), 2: (128, 64, 2, 2, 32), 3: (64, 128, 2, 2, 32), 4: (64, 64, 2, 2, 32), 5: (128, 32, 4, 1, 32), 6: (64, 32, 2, 1, 32),
              7: (128, 128, 4, 2, 32), 8: (128, 128, 2, 4, 32), 9: (128, 256, 2, 4, 32), 10: (256, 128, 4, 2, 32),
              23: (64, 128, 2, 2, 64), 24: (64, 64, 2, 2, 64), 27: (128, 128, 4, 2, 64), 28: (128, 128, 2, 4, 64)}   # BK = 64: C1 and C2 multiples of 64, fp32 only
IGEMM_BN = {t: v[1] for t, v in IGEMM_CFGS.items()}
IGEMM_SPLIT_MODE_TILES = (1, 2, 3, 4, 6, 7, 8, 9, 10)                     # the switch of conv2d_impl for precision 3 and 4 (no 128 x 32, no BK = 64)
# dispatch_group of conv_f16x2.hip: (3x3 host tile, 1x1 guest tile)
GROUP_PAIRS = ((53, 53), (54, 53), (34, 36), (34, 37), (62, 36), (62, 37), (33, 36), (33, 37), (31, 36), (31, 37))

Case = namedtuple("Case", "name N H W C1 C2 Cout k stride pad ups")


def case(name, N, hw, C1, C2=0, Cout=64, k=3, stride=1, pad=None, ups=0):
    return Case(name, N, hw[0], hw[1], C1, C2, Cout, k, stride, k // 2 if pad is None else pad, ups)


def as_case(t):
    """the 9-tuples of tests/test_kernels_gpu.py (N, H, W, C1, C2, Cout, k, stride, ups), padded as monai does (k // 2)"""
    n, h, w, c1, c2, co, k, stride, ups = t
    return Case("t", n, h, w, c1, c2, co, k, stride, k // 2, ups)


def out_hw(c):
    """fill_geometry (conv_plan.h): the effective grid is the source x2 under upsample 1 | 2"""
    up = 1 if c.ups in (1, 2) else 0
    return ((c.H << up) + 2 * c.pad - c.k) // c.stride + 1, ((c.W << up) + 2 * c.pad - c.k) // c.stride + 1


def geometry_ok(c):
    """what fill_geometry admits of a case (NHWC, the precisions of this file)"""
    if c.k not in (1, 3) or c.stride not in (1, 2) or c.pad not in (0, 1) or c.ups not in (0, 1, 2) or min(c.N, c.H, c.W, c.C1, c.Cout) < 1 or c.C2 < 0:
        return False
    if c.ups == 2 and (c.k, c.stride, c.pad) != (3, 1, 1):
        return False
    return min(out_hw(c)) > 0


def halo_fits(c, tile):
    """halo_fits of conv_f16x2.hip: the tile is a block of whole rows of one image or of whole small images, its halo inside the HG pieces"""
    if tile not in HALO_HG:
        return True
    if (c.k, c.stride, c.pad, c.ups) != (3, 1, 1, 0):
        return False
    bm = F16X2_TILES[tile][0]
    hw = c.H * c.W
    if hw >= bm:
        if hw % bm or bm % c.W:
            return False
        r, segs = bm // c.W, 1
    else:
        if bm % hw:
            return False
        r, segs = c.H, bm // hw
    hg, nw = HALO_HG[tile]
    return segs * (r + 2) * (c.W + 2) <= 8 * nw * hg


def _halo_fits(t, tile):
    """halo_fits for a 9-tuple of tests/test_kernels_gpu.py"""
    return halo_fits(as_case(t), tile)


def halo_kind(c, tile):
    """which of the halo kernel's three geometries (c, tile) is"""
    bm, hw = F16X2_TILES[tile][0], c.H * c.W
    return "images_per_tile" if hw < bm else ("one_image" if hw == bm else "row_blocks")


def pair_path_ok(c):
    """pl->ok of make_plan2 before a tile is chosen: NHWC, 32-channel chunks, Cout % 64, nearest x2 only in its sub-pixel form (the sizes of
    this file are far inside the 4 GiB buffer ranges)"""
    return geometry_ok(c) and c.C1 % 32 == 0 and c.C2 % 32 == 0 and c.Cout % 64 == 0 and c.ups != 1


def tile_valid(c, tile):
    """valid() of make_plan2"""
    bm, bn = F16X2_TILES[tile]
    return c.Cout % bn == 0 and (c.ups != 2 or (c.H * c.W) % bm == 0) and halo_fits(c, tile)


def f16x2_ok(c, tile=0, sk=0):
    """mf_conv2d_f16x2_ok for tile hint `tile` and split-K hint `sk`.  Hint 0: the cost model picks among the valid tiles but 52 (an A/B form) and the
    128-row halo tiles; with none valid the plan is not ok -- and it tries the splits 1, 2, 4, ... up to the channel groups only, so next to tile
    hint 0 any other split-K hint is refused (with a tile hint every sk >= 1 is taken, clipped to the channel groups).  A hint whose BN does not
    divide Cout is an MF_REQUIRE (the query answers 0 as well)."""
    if not pair_path_ok(c):
        return False
    if tile:
        return tile in F16X2_TILES and tile_valid(c, tile)
    if sk and (sk & (sk - 1) or sk > min(32, (c.C1 + c.C2) // 32)):
        return False
    return any(tile_valid(c, t) for t in F16X2_TILES if t not in (52, 63, 64))


def f16x2_tiles(c):
    return [t for t in F16X2_TILES if f16x2_ok(c, t)]


def slices(c, sk):
    """(cgroups, cg_sw, cg_per_split, splitk) of make_plan2 for split-K hint sk >= 1: the 2-D kernel splits by CHANNEL GROUP of 32, every slice runs
    all taps of its groups; cg_sw is the first group of the second source"""
    cg = (c.C1 + c.C2) // 32
    s = min(sk, cg)
    per = -(-cg // s)
    return cg, (c.C1 // 32 if c.C2 else cg), per, -(-cg // per)


def slice_kinds(c, sk):
    """every slice [cg0, cg1) of the plan against the first channel group of the second source"""
    cg, sw, per, eff = slices(c, sk)
    kinds = []
    for z in range(eff):
        g0, g1 = z * per, min(cg, (z + 1) * per)
        assert g0 < g1
        if c.C2 == 0 or g1 < sw:
            kinds.append("before")
        elif g1 == sw:
            kinds.append("ends_at")
        elif g0 == sw:
            kinds.append("starts_at")
        elif g0 < sw:
            kinds.append("straddles")
        else:
            kinds.append("after")
    return kinds


def tree_possible(c, sk):
    """tree_possible: a power-of-two split meets inside the launch (the hand-off of these sizes is far inside 32-bit offsets); any other split
    writes slabs and runs the reducer pass"""
    eff = slices(c, sk)[3]
    return eff >= 2 and eff & (eff - 1) == 0


def distinct_sks(c):
    """the split-K hints that give different plans for this case"""
    seen, out = set(), []
    for sk in range(1, (c.C1 + c.C2) // 32 + 1):
        key = slices(c, sk)
        if key not in seen:
            seen.add(key)
            out.append(sk)
    return out


def chain_chunks(c, sk=1):
    """chain_ok of make_plan2: 32-channel chunks one accumulation chain runs through"""
    return slices(c, sk)[2] * (4 if c.ups == 2 else c.k * c.k)


def igemm_ok(c):
    """pl->igemm of make_plan (conv.hip), NHWC in and out"""
    return geometry_ok(c) and c.C1 % 32 == 0 and c.C2 % 32 == 0 and c.Cout % 32 == 0


def subpixel_ok(c):
    """mf_conv2d_subpixel_ok on the planner's own tile: the implicit-GEMM path and Hin Win % 64 == 0 (every tile the planner falls back to has 64 rows)"""
    return c.ups == 2 and igemm_ok(c) and (c.H * c.W) % 64 == 0


def igemm_tiles(c, precision):
    """the tile hints mf_conv2d_f32 takes for this case: BN divides Cout, BK divides both channel counts, the BK = 64 forms and 128 x 32 exist
    for fp32 only, and a sub-pixel tile lies inside one phase"""
    if not igemm_ok(c) or (c.ups == 2 and not subpixel_ok(c)):
        return []
    out = []
    for t, (bm, bn, _, _, bk) in IGEMM_CFGS.items():
        if c.Cout % bn or c.C1 % bk or c.C2 % bk or (precision != 0 and t not in IGEMM_SPLIT_MODE_TILES) or (c.ups == 2 and (c.H * c.W) % bm):
            continue
        out.append(t)
    return out


def igemm_slices(c, tile, sk):
    """(nk, nk_per_split, splitk) of make_plan: this kernel splits by ITERATION (tap x chunk of BK channels)"""
    nk = (4 if c.ups == 2 else c.k * c.k) * ((c.C1 + c.C2) // IGEMM_CFGS[tile][4])
    s = min(max(sk, 1), nk)
    per = -(-nk // s)
    return nk, per, -(-nk // per)


def split_bf16x3(x):
    """mf_split_conv_weight_bf16x3 / the in-kernel activation split: x = t0 + t1 + t2, each the bf16 rounding of what is left (round to nearest even)"""
    x = x.float()
    t0 = x.bfloat16().float()
    t1 = (x - t0).bfloat16().float()
    t2 = (x - t0 - t1).bfloat16().float()
    return t0.double(), t1.double(), t2.double()


# ---------------------------------------------------------------------------------------------------------------- references
def _cat_up(x1, x2, ups):
    x = torch.cat([x1, x2], 1) if x2 is not None else x1
    return F.interpolate(x, scale_factor=2.0, mode="nearest") if ups else x


def ref64(x1, x2, w, b, c):
    """fp64: torch.cat of the two sources, nearest x2 where upsampled, F.conv2d"""
    return F.conv2d(_cat_up(x1.double(), None if x2 is None else x2.double(), c.ups), w.double(), None if b is None else b.double(), c.stride, c.pad)


def want32(x1, x2, w, b, c):
    """float32(ref64) of an exact case, NCHW: the sums are exact in fp64 and the bias is added once, at the end (bias_add_rounds_once), whatever order
    F.conv2d would add it in"""
    y = ref64(x1, x2, w, None, c)
    return (y if b is None else y + b.double().view(1, -1, 1, 1)).float()


def sabs64(x1, x2, w, c):
    """sum |w||x| of every output, fp64"""
    return F.conv2d(_cat_up(x1.double().abs(), None if x2 is None else x2.double().abs(), c.ups), w.double().abs(), None, c.stride, c.pad)


def gather64(x1, x2, w, b, c):
    """The kernel's stated rule, tap by tap, without F.interpolate / F.conv2d: coordinate u of the effective grid reads pixel u >> up, taps outside
    [0, H << up) contribute zero."""
    x = (torch.cat([x1, x2], 1) if x2 is not None else x1).double()
    w = w.double()
    up = 1 if c.ups else 0
    ho, wo = out_hw(c)
    y = torch.zeros((x.shape[0], w.shape[0], ho, wo), dtype=torch.float64)

    def axis(n_out, extent, kk):
        u = torch.arange(n_out) * c.stride - c.pad + kk
        ok = (u >= 0) & (u < (extent << up))
        return (u.clamp(0, (extent << up) - 1) >> up), ok.double()

    for kh in range(c.k):
        iy, vy = axis(ho, c.H, kh)
        for kw in range(c.k):
            ix, vx = axis(wo, c.W, kw)
            patch = x[:, :, iy][:, :, :, ix] * (vy[:, None] * vx[None, :])
            y += torch.einsum("nchw,oc->nohw", patch, w[:, :, kh, kw])
    return y if b is None else y + b.double().view(1, -1, 1, 1)


def subpixel_phases(w):
    """The sub-pixel form of nearest x2 + 3x3 pad 1 (what pack_upconv_weight builds, up to its storage order): output (2i + a, 2j + b) reads the 2 x 2
    SOURCE pixels (i + a - 1 + t, j + b - 1 + s), t, s in {0, 1}; along an axis the three taps fold to (w0, w1 + w2) for phase 0 and (w0 + w1, w2) for
    phase 1.  -> {(a, b): [Cout, Cin, 2, 2]}"""
    w = w.double()
    fold = lambda v0, v1, v2, ph: (v0, v1 + v2) if ph == 0 else (v0 + v1, v2)
    out = {}
    for a in (0, 1):
        rows = fold(w[:, :, 0], w[:, :, 1], w[:, :, 2], a)              # two of [Cout, Cin, 3]
        for b in (0, 1):
            out[(a, b)] = torch.stack([torch.stack(fold(r[..., 0], r[..., 1], r[..., 2], b), -1) for r in rows], -2).contiguous()
    return out


def kernel_forms(c, w):
    """the filters the kernel really multiplies and where they sit: [(filter, (left, right, top, bottom) zero padding, stride)]"""
    if c.ups != 2:
        return [(w.double(), (c.pad,) * 4, c.stride)]
    return [(f, (1 - b, b, 1 - a, a), 1) for (a, b), f in subpixel_phases(w).items()]


def subpixel64(x1, x2, w, b, c):
    """ref64 of a sub-pixel case computed through its four phases"""
    x = (torch.cat([x1, x2], 1) if x2 is not None else x1).double()
    y = torch.zeros((x.shape[0], w.shape[0], 2 * c.H, 2 * c.W), dtype=torch.float64)
    for (a, bb), f in subpixel_phases(w).items():
        y[:, :, a::2, bb::2] = F.conv2d(F.pad(x, (1 - bb, bb, 1 - a, a)), f)
    return y if b is None else y + b.double().view(1, -1, 1, 1)


def _sabs_forms(xa, forms):
    """max over the outputs of sum |filter||x| through every form; xa = |x| [1, C, H, W], forms as kernel_forms gives them with |filter|"""
    return max(float(F.conv2d(F.pad(xa, pad), f, None, stride).max()) for f, pad, stride in forms)


# ---------------------------------------------------------------------------------------------------------------- cases
def _geoms():
    out = []
    for hw in ((4, 6), (5, 7)):          # (even and odd extents: stride 2 leaves a last window that ends inside, at and past the edge)
        for stride in (1, 2):
            for k, pad in ((3, 0), (3, 1), (1, 0)):
                out.append(case(f"{hw[0]}x{hw[1]}k{k}p{pad}s{stride}", 3, hw, 32, k=k, stride=stride, pad=pad))
    for hw in ((1, 1), (1, 6), (5, 1)):  # extents of 1: every k = 3 window hangs over both edges of such an axis
        for stride in (1, 2):
            out.append(case(f"{hw[0]}x{hw[1]}k3p1s{stride}", 3, hw, 32, k=3, stride=stride, pad=1))
        out.append(case(f"{hw[0]}x{hw[1]}k1", 3, hw, 32, k=1))
    out.append(case("3x3k3p0", 3, (3, 3), 32, k=3, pad=0))   # a single output pixel per sample
    return out


GEOM_CASES = _geoms()
# M = N H W at the edges of the 64-, 128- and 256-row tiles (k = 1: M is the input's pixel count).  Cout = 256 so that EVERY tile's BN divides it: the
# 64-row tiles of the pair kernel (37: 64 x 256, 53: 64 x 128) exist for no smaller Cout.
_M_SHAPES = ((3, (3, 7)), (4, (4, 4)), (5, (1, 13)), (127, (1, 1)), (2, (8, 8)), (3, (1, 43)), (5, (3, 17)), (4, (8, 8)), (1, (1, 257)))
M_EDGE_CASES = [case(f"M{n * h * w}", n, (h, w), 32, Cout=256, k=1) for n, (h, w) in _M_SHAPES]
# k = 3 where the last rows of a tile belong to the next sample (M = 81, 144, 125)
M_EDGE_CASES += [case(f"M{n * h * h}k3", n, (h, h), 32, Cout=256, k=3) for n, h in ((9, 3), (9, 4), (5, 5))]
COUT_EDGE_CASES = [case(f"Cout{co}", 2, (5, 7), 32, Cout=co, k=3) for co in (64, 128, 192, 256, 320)]
COUT_IGEMM_CASES = [case(f"Cout{co}", 2, (5, 7), 32, Cout=co, k=3) for co in (32, 96, 160)]   # no pair path (Cout % 64): implicit GEMM only
# the BK = 64 tiles of the implicit GEMM (23, 24, 27, 28) take channel counts that are multiples of 64 only
BK64_CASES = [case("bk64_c64", 3, (5, 7), 64, Cout=256, k=3), case("bk64_c64+64", 3, (4, 5), 64, 64, Cout=128, k=1)]
TWO_SOURCE_CASES = [case(f"c{c1}+{c2}k{k}", 3, (4, 5), c1, c2, k=k) for c1, c2 in ((32, 32), (64, 32), (32, 64), (96, 32), (96, 96), (128, 128)) for k in (3, 1)]
SK8_CASE = TWO_SOURCE_CASES[10]          # c128+128k3: 8 channel groups, K = 2304 (reduced density), split-K up to 8
# splitk_reduce_kernel's launch (conv_f16x2_impl): grid (min(ceil(p4 / 256), cdiv(2048, N)), N) of 256 threads over p4 = Ho Wo Cout / 4 float4s per
# sample.  N = 16: the grid stops at 128 blocks = 32768 float4s; 16 x 33 x 256 / 4 = 33792 gives the grid-stride loop a second trip.  sk = 3 (not a
# power of two) takes the slabs + reducer form.
REDUCER_CASE = case("reducer_second_trip", 16, (16, 33), 96, Cout=256, k=1)
REDUCER_SK = 3


def _halos():
    out = []
    # (16 x 32: the one shape of the list whose 256-row tile is a block of rows of a larger image)
    for n, hw in ((3, (8, 8)), (5, (8, 8)), (9, (4, 4)), (3, (8, 16)), (2, (4, 32)), (2, (16, 16)), (3, (16, 16)), (3, (2, 64)), (2, (16, 32))):
        out.append(case(f"halo{n}x{hw[0]}x{hw[1]}", n, hw, 32, Cout=128))
        if hw in ((8, 8), (8, 16), (16, 16)):
            out.append(case(f"halo{n}x{hw[0]}x{hw[1]}c32+32", n, hw, 32, 32, Cout=128))
    return out


HALO_CASES = _halos()
SUBPIXEL_CASES = [case(f"sub{n}x{h}x{w}", n, (h, w), 32, Cout=256, ups=2) for n, (h, w) in ((3, (8, 8)), (2, (1, 64)), (2, (64, 1)), (3, (2, 32)), (2, (8, 16)), (2, (16, 16)))]
SUBPIXEL_CASES.append(case("sub2x8x16c32+32", 2, (8, 16), 32, 32, Cout=256, ups=2))

# nearest x2 in its GATHER form (upsample = 1: coordinate u reads pixel u >> 1; conv.hip only -- the pair path takes the sub-pixel form alone), where
# tap validity is a matter of the EFFECTIVE extent: pad 0 and 1, stride 1 and 2, an extent of 1, and a source the sub-pixel form refuses (5 x 7)
GATHER_UP_CASES = [case(f"up{h}x{w}k{k}p{pad}s{stride}", 3, (h, w), 32, k=k, stride=stride, pad=pad, ups=1)
                   for (h, w) in ((4, 6), (5, 7), (1, 3)) for k, pad in ((3, 0), (3, 1), (1, 0)) for stride in (1, 2)]
GATHER_UP_CASES = [c for c in GATHER_UP_CASES if geometry_ok(c)]          # (1 x 3 upsampled is 2 x 6: no room for a 3 x 3 window without padding)
GATHER_UP_CASES.append(case("up4x5c32+32", 3, (4, 5), 32, 32, k=3, ups=1))

EXACT_F16X2_CASES = GEOM_CASES + M_EDGE_CASES + COUT_EDGE_CASES + TWO_SOURCE_CASES + HALO_CASES + SUBPIXEL_CASES
EXACT_IGEMM_CASES = GEOM_CASES + M_EDGE_CASES + COUT_EDGE_CASES + COUT_IGEMM_CASES + BK64_CASES + TWO_SOURCE_CASES + SUBPIXEL_CASES + GATHER_UP_CASES
EXACT_CASES = (GEOM_CASES + M_EDGE_CASES + COUT_EDGE_CASES + COUT_IGEMM_CASES + BK64_CASES + TWO_SOURCE_CASES + [REDUCER_CASE] + HALO_CASES + SUBPIXEL_CASES +
               GATHER_UP_CASES)

# DIRECT (conv.hip's kernels that are not implicit GEMM): (case, input layout, output layout); the layout pairs of test_conv_direct.  Cin <= 16 and
# Cout = 64 with NHWC out is the small-Cin kernel, a 1x1 of 32 k channels onto Cout <= 8 the out-1x1 kernel, everything else the generic one.
Direct = namedtuple("Direct", "c lin lout")


def _directs():
    out = []
    geoms = (("5x7k3s2", (5, 7), 3, 2, 1), ("5x7k3p0", (5, 7), 3, 1, 0), ("1x6k3", (1, 6), 3, 1, 1), ("5x1k3", (5, 1), 3, 1, 1), ("5x7k1", (5, 7), 1, 1, 0))
    for cin, co, lin, lout in ((8, 64, "nchw", "nhwc"), (3, 64, "nchw", "nhwc"), (16, 64, "nhwc", "nhwc"), (3, 5, "nchw", "nhwc"), (8, 3, "nhwc", "nchw"),
                               (16, 8, "nhwc", "nhwc"), (16, 5, "nchw", "nchw")):
        for name, hw, k, stride, pad in geoms:
            out.append(Direct(case(f"d{cin}>{co}_{name}_{lin}>{lout}", 3, hw, cin, Cout=co, k=k, stride=stride, pad=pad), lin, lout))
    for cin, co, lout in ((32, 8, "nchw"), (32, 3, "nchw"), (64, 5, "nhwc"), (96, 5, "nchw")):   # out-1x1: 1, 1, 2 lanes per pixel; 96: C / 32 no power of two
        out.append(Direct(case(f"d{cin}>{co}_5x7k1_nhwc>{lout}", 3, (5, 7), cin, Cout=co, k=1), "nhwc", lout))
    out.append(Direct(case("d8+8>64_5x7k3", 3, (5, 7), 8, 8, Cout=64, k=3), "nhwc", "nhwc"))     # the two-source small-Cin form
    out.append(Direct(case("d8+8>64_1x6k3s2", 3, (1, 6), 8, 8, Cout=64, k=3, stride=2), "nhwc", "nhwc"))
    out.append(Direct(case("d8+8>5_5x7k3p0", 3, (5, 7), 8, 8, Cout=5, k=3, pad=0), "nhwc", "nchw"))       # two sources through the generic kernel
    out.append(Direct(case("d8>5_up5x7k3s2", 3, (5, 7), 8, Cout=5, k=3, stride=2, ups=1), "nchw", "nhwc"))  # nearest x2, gather form
    out.append(Direct(case("d16>64_up1x6k3s2", 3, (1, 6), 16, Cout=64, k=3, stride=2, ups=1), "nhwc", "nhwc"))
    return out


DIRECT_CASES = _directs()


def variants(c):
    """the (family, ratio) operand sets of a case: ratio = log2 of the second source's scale against the first ("mixed": +20 / -20 by sample)"""
    if c.C2 == 0:
        return [("xlo", None), ("wlo", None), ("int8", None)]
    return [("xlo", "mixed"), ("wlo", 20), ("wlo", -20), ("int8", "mixed")]


# ---------------------------------------------------------------------------------------------------------------- exact operands
def density(c):
    """non-zero probability of each operand: the conv3d density 0.5 up to Cin taps = 1152, then lowered so that the expected sum |w||x| stays where it
    is at 1152 (the budget is asserted, not assumed: exact_budget)"""
    k = (c.C1 + c.C2) * c.k * c.k
    return 0.5 if k <= 1152 else 0.5 * math.sqrt(1152.0 / k)


def sample_exps(c, ratio):
    """per sample: (log2 scale of source 1, log2 scale of source 2)"""
    out = []
    for n in range(c.N):
        e = SAMPLE_EXPS[n % 3]
        r = 0 if ratio is None else ((20 if (n // 3 + n) % 2 == 0 else -20) if ratio == "mixed" else ratio)
        out.append((e, e + r))
    return out


def _int8(g, shape, p):
    """integers in [-127, 127], non-zero with probability p"""
    v = torch.randint(-127, 128, shape, generator=g).double()
    return v * (torch.rand(shape, generator=g, dtype=torch.float64) < p).double()


def exact_operands(c, family, ratio, seed=0):
    """(x1, x2, w, b, unit_exps): fp64 tensors whose values are fp32 values (NCHW, OIHW), and log2 of every sample's output unit"""
    g = torch.Generator().manual_seed(_seed_of(c.name, family, ratio, seed))
    cin = c.C1 + c.C2
    p = density(c)
    exps = sample_exps(c, ratio)
    nnz = 2 if c.ups else 8              # an upsampled pixel meets a 3 x 3 window up to 4 times: at most 8 products of the sparse source per output
    x1 = torch.zeros((c.N, c.C1, c.H, c.W), dtype=torch.float64)
    x2 = torch.zeros((c.N, c.C2, c.H, c.W), dtype=torch.float64) if c.C2 else None
    units = []
    w = _ints(g, (c.Cout, cin, c.k, c.k), p)
    if c.C2 == 0:
        if family == "wlo":
            w = _with_lo(g, w)
        for n, (e1, _) in enumerate(exps):
            a = _int8(g, x1.shape[1:], p) if family == "int8" else _ints(g, x1.shape[1:], p)
            a.view(-1)[0] = 1.0
            x1[n] = (_with_lo(g, a) if family == "xlo" else a) * 2.0 ** e1
            units.append(e1 if family == "int8" else e1 - LO_BITS)
    else:
        for n, (e1, e2) in enumerate(exps):
            big1 = e1 > e2
            dshape = (x2 if big1 else x1).shape[1:]
            dense = _int8(g, dshape, p) if family == "int8" else _ints(g, dshape, p)
            dense.view(-1)[0] = 1.0
            sparse = _sparse(g, (x1 if big1 else x2).shape[1:], nnz)
            if family == "xlo":
                sparse = _with_lo(g, sparse)
            x1[n] = (sparse if big1 else dense) * 2.0 ** e1
            x2[n] = (dense if big1 else sparse) * 2.0 ** e2
            units.append(min(e1, e2))
        if family == "wlo":   # the lo part in the weights of the larger (sparse) source's channels
            sl = slice(0, c.C1) if exps[0][0] > exps[0][1] else slice(c.C1, cin)
            w[:, sl] = _with_lo(g, w[:, sl])
    w.view(-1)[0] = 1.0
    b = torch.zeros(c.Cout, dtype=torch.float64)
    nb = len(b[::3])
    b[::3] = torch.randint(1, 3, (nb,), generator=g).double() * (torch.randint(0, 2, (nb,), generator=g).double() * 2 - 1) * 2.0 ** 20
    return x1, x2, w, b, units


def exact_budget(c, x1, x2, w, b, units):
    """The qualifying conditions of an exact case on the pair arithmetic, as a dict of figures (the CPU test asserts them), taken on the filters the
    kernel multiplies (kernel_forms: the four phase filters of a sub-pixel case, split under THEIR common maximum as split_weight_f16x2 does):
      lolo       -- max |lo'_x| max |lo'_w| (must be 0: one operand has lo = 0 in every product)
      unit_ok    -- the pair form reproduces both operands, every hi and lo' product is a multiple of the sample's output unit u, and so is the bias
      bits_m, bits_x, bits_all -- log2 of sum |terms| / u of the hi.hi accumulator, of the cross accumulator, and of sum |w||x| (each < 24)"""
    forms = kernel_forms(c, w)
    wb = max(float(f.abs().max()) for f, _, _ in forms)
    wexp = scale_exp(wb)
    wparts = []
    for f, pad, stride in forms:
        _, whi, wlo = pair_terms(f, wb)
        wparts.append((f, whi * 2.0 ** wexp, wlo * 2.0 ** wexp / 2048.0, pad, stride))
    lolo, bits_m, bits_x, bits_all, unit_ok = 0.0, -1e9, -1e9, -1e9, True
    grid = (lambda t: F.interpolate(t, scale_factor=2.0, mode="nearest")) if c.ups == 1 else (lambda t: t)   # (the gather form walks the x2 grid)
    for n in range(c.N):
        his, los = [], []
        for x in ([x1[n:n + 1]] + ([x2[n:n + 1]] if x2 is not None else [])):
            s, hi, lo = pair_terms(x, float(x.abs().max()))
            his.append(hi * 2.0 ** s)
            los.append(lo * 2.0 ** s / 2048.0)
            lolo = max(lolo, float(lo.abs().max()) * max(float(wl.abs().max()) for _, _, wl, _, _ in wparts))
        x = torch.cat([x1[n:n + 1]] + ([x2[n:n + 1]] if x2 is not None else []), 1)
        xh, xl = torch.cat(his, 1), torch.cat(los, 1)
        u = 2.0 ** units[n]
        unit_ok &= bool(torch.equal(xh + xl, x))
        x, xh, xl = grid(x), grid(xh), grid(xl)
        sm = _sabs_forms(xh.abs(), [(wh.abs(), pad, st) for _, wh, _, pad, st in wparts]) / u
        sx = max(float((F.conv2d(F.pad(xl.abs(), pad), wh.abs(), None, st) + F.conv2d(F.pad(xh.abs(), pad), wl.abs(), None, st)).max()) for _, wh, wl, pad, st in wparts) / u
        sa = _sabs_forms(x.abs(), [(f.abs(), pad, st) for f, _, _, pad, st in wparts]) / u
        bits_m, bits_x, bits_all = max(bits_m, _log2(sm)), max(bits_x, _log2(sx)), max(bits_all, _log2(sa))
        for f, wh, wl, _, _ in wparts:
            unit_ok &= bool(torch.equal(wh + wl, f))
            for xa, wa in ((xh, wh), (xl, wh), (xh, wl)):
                if bool((xa != 0).any()) and bool((wa != 0).any()):
                    unit_ok &= _product_unit_or_none(xa[0], wa) >= units[n]
        unit_ok &= _is_multiple(b, u)
    return dict(lolo=lolo, unit_ok=unit_ok, bits_m=bits_m, bits_x=bits_x, bits_all=bits_all)


def _product_unit_or_none(x, w):
    """_product_unit, 10^9 where no input channel has both a non-zero activation and a non-zero weight"""
    both = [ci for ci in range(x.shape[0]) if bool((x[ci] != 0).any()) and bool((w[:, ci] != 0).any())]
    return _product_unit(x, w) if both else 10 ** 9


def bf16x3_dropped(x1, x2, w):
    """largest magnitude among the operand terms whose products the triplet mode drops: it keeps t_i(x) t_j(w) for i + j <= 2, so the dropped
    products are t1.t2, t2.t1 and t2.t2 -- all zero when max(|t1(x)| |t2(w)|, |t2(x)| |t1(w)|, |t2(x)| |t2(w)|) is"""
    x = torch.cat([x1, x2], 1) if x2 is not None else x1
    _, x1t, x2t = split_bf16x3(x)
    _, w1t, w2t = split_bf16x3(w)
    m = lambda t: float(t.abs().max())
    return max(m(x1t) * m(w2t), m(x2t) * m(w1t), m(x2t) * m(w2t))


# ---------------------------------------------------------------------------------------------------------------- real-valued operands
def scaled_real_operands(c, cancelling=False, seed=0):
    """real_operands of conv3d_cases in 2-D form with the samples scaled 2^0, 2^20, 2^-20"""
    x1, x2, w, b = real_operands(c, seed=seed, cancelling=cancelling)
    sc = torch.tensor([2.0 ** SAMPLE_EXPS[n % 3] for n in range(c.N)], dtype=torch.float64).view(-1, 1, 1, 1)
    return x1 * sc, (None if x2 is None else x2 * sc), w, b


# C: element-wise bound on real operands.  2^-21 sum |w||x| for the pair arithmetic holds while one chain is <= 96 chunks (asserted by the CPU test).
BOUND_TWO_SOURCE = (TWO_SOURCE_CASES[6], 2)        # c96+32k3, sk = 2: slices [0, 2) and [2, 4) -- the second straddles the switch at group 3
BOUND_HALO = HALO_CASES[1]                         # 3 x 8 x 8, 32 + 32 channels: samples of three scales share a tile
BOUND_SUBPIXEL = SUBPIXEL_CASES[6]                 # two sources, sub-pixel
BOUND_CASES = GEOM_CASES + [BOUND_TWO_SOURCE[0], BOUND_HALO, BOUND_SUBPIXEL]
BOUND_DIRECT = [d for d in DIRECT_CASES if d.c.name in ("d8>64_5x7k3s2_nchw>nhwc", "d16>5_5x7k3p0_nchw>nchw", "d96>5_5x7k1_nhwc>nchw", "d32>8_5x7k1_nhwc>nchw", "d8+8>64_5x7k3")]

# D: covariance and the zero source.  (case, tile, sk): the 9-copy body and a halo tile, unsplit and at a straddling split
COV_CASE = case("cov_c96+32", 3, (8, 8), 96, 32, Cout=128, k=3)
COV_PLANS = ((52, 1), (52, 2), (63, 1), (63, 2), (0, 0))   # sk = 2 of 4 groups: slice [2, 4) straddles the switch at group 3
# E: non-finite confinement: a GEOM case, a HALO case with several images per tile, a SUBPIXEL case
NONFINITE_CASES = [GEOM_CASES[1], HALO_CASES[0], SUBPIXEL_CASES[4]]
# F: nothing written past the output: the M_EDGE cases and the ragged-N halo cases
GUARD_CASES = M_EDGE_CASES + [h for h in HALO_CASES if h.C2 == 0 and (h.H, h.W) in ((8, 8), (4, 4))]
GUARD_FLOATS = 64
# B: two convolutions in one launch, on the entries of dispatch_group a small shape reaches (3x3 host tile, 1x1 guest tile on the same input)
GROUP_SMALL = [(case("grp2x16x16", 2, (16, 16), 64, 0, Cout=128), 53, 53), (case("grp3x16x16", 3, (16, 16), 64, 32, Cout=128), 54, 53),
               (case("grp2x16x16c128", 2, (16, 16), 128, 0, Cout=256), 34, 37), (case("grp3x16x16c96", 3, (16, 16), 96, 0, Cout=128), 34, 36),
               (case("grp2x16x16h", 2, (16, 16), 64, 64, Cout=128), 62, 36), (case("grp2x16x16h256", 2, (16, 16), 64, 0, Cout=256), 62, 37),
               (case("grp3x8x16", 3, (8, 16), 64, 0, Cout=128), 33, 36), (case("grp3x8x16c256", 3, (8, 16), 32, 32, Cout=256), 33, 37),
               (case("grp2x8x16c256", 2, (8, 16), 64, 0, Cout=256), 31, 36), (case("grp5x8x16c256", 5, (8, 16), 64, 0, Cout=256), 31, 37)]
