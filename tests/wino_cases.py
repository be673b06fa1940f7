"""The Winograd F(2x2, 3x3) form (csrc/winograd.h, csrc/conv_f16x2_wino.inc) at its edges: references, operands that are exact IN THE TRANSFORM
DOMAIN, the host rules restated in Python and the case lists of tests/test_wino_edges_cpu.py and tests/test_wino_edges_gpu.py.  Plain Python and
torch, no device.  The dimension-free pieces are imported from tests/conv2d_cases.py, tests/conv3d_cases.py and tests/groupnorm_cases.py.

Exact operands.  y = A^T [sum_c U . V] A with U = G g G^T, V = B^T d B is the fp64 convolution, algebraically.  The kernels return float32(ref64)
bit for bit when
  (a) U and V reproduce in their fp16-pair form (U under max |U|, V of sample n under 4 bound(x[n])) and one of lo'(U), lo'(V) is zero in every
      product -- the lo.lo term the pair arithmetic drops is identically zero;
  (b) every hi and lo' product is a whole multiple of the sample's unit: the direct form's unit / 4, because G carries halves twice;
  (c) sum |U_k||V_k| over the input channels and the nine components an output reads, plus |bias|, stays below 2^24 units: every partial sum of
      every accumulator, of the split-K hand-off and of A^T M A is then an integer below 2^24 in that unit, exact in fp32 in any order.
The families of conv2d_cases.exact_operands do NOT meet (c) as they stand (a transform-domain value is a sum of up to 9 weights or 4 pixels):
wino_operands() thins them -- a Bernoulli mask of probability keep(Cin) on activations and weights, which keeps (a) and (b) -- and the two-source
cases take the scale ratio 2^+-13 instead of 2^+-20 (13: the lo part b 2^-13 of the larger source is then a whole multiple of the smaller
source's unit; any smaller ratio would lower the unit, any larger one costs budget bit for bit).  wino_budget() states (a) - (c) per case,
family and sample; the CPU test asserts them and runs restate_fp32(), the four steps in plain fp32 torch, to float32(ref64).

No constant of this file comes from a run of the kernels: tables restate the sources (the line each restates is named), sizes follow from the
launch arithmetic quoted next to them, the bound of section C is a count of roundings."""

import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests import conv2d_cases as CC
from tests.conv2d_cases import distinct_sks, exact_operands, ref64, scaled_real_operands, slices, tree_possible, want32  # noqa: F401
from tests.conv3d_cases import _is_multiple, _seed_of, pair_terms, scale_exp
from tests.groupnorm_cases import EPS, bound_E, ref_terms  # noqa: F401

U24 = 2.0 ** -24
# winograd.h:14
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)
# the tiles the component GEMM can run on (kTiles2 without the halo tiles: halo_fits refuses a 1x1): tile -> (BM, BN).  tests/test_winograd_gpu.py
# imports this table
TILES = {t: v for t, v in CC.F16X2_TILES.items() if t not in CC.HALO_HG}


def case(name, N, hw, C1, C2=0, Cout=64):
    return CC.case(name, N, hw, C1, C2, Cout=Cout, k=3)


def tiles_of(c):
    return (c.H // 2) * (c.W // 2)


# ---------------------------------------------------------------------------------------------------------------- the host rules, restated
def wino_shape_ok(c, precision=5):
    """wino_shape_ok (conv_f16x2_wino.inc:17-22) of a 3x3 stride-1 pad-1 NHWC case"""
    return (precision == 5 and (c.k, c.stride, c.pad, c.ups) == (3, 1, 1, 0) and c.N > 0 and c.H >= 2 and c.W >= 2 and c.H % 2 == 0 and c.W % 2 == 0 and
            c.C1 > 0 and c.C1 % 32 == 0 and c.C2 >= 0 and c.C2 % 32 == 0 and c.Cout % 64 == 0 and c.Cout <= 1024 and 256 % (c.Cout // 4) == 0 and
            c.N * 16.0 * tiles_of(c) < 2147483647.0)


def gemm_case(c):
    """wino_gemm_desc (conv_f16x2_wino.inc:7-16): 16 N pseudo-samples of T pixels, 1x1"""
    return CC.Case(c.name, 16 * c.N, 1, tiles_of(c), c.C1, c.C2, c.Cout, 1, 1, 0, 3)


def tile_holds_a_component(c, tile):
    """valid() of make_plan2 for upsample == 3 (conv_f16x2.hip:108): BN divides Cout and a tile lies inside one component, (N T) % BM == 0"""
    bm, bn = TILES[tile]
    return c.Cout % bn == 0 and (c.N * tiles_of(c)) % bm == 0


def wino_tiles(c):
    return [t for t in TILES if wino_shape_ok(c) and tile_holds_a_component(c, t)]


def wino_ok(c, tile=0, sk=0, precision=5):
    """mf_wino_ok (wino_plan, conv_f16x2_wino.inc:28-33) under the hints: the shape, a tile that holds a component, and a split-K that is 1 or meets
    inside the launch (a power of two).  Hint 0 lets the cost model choose among the tiles but 52 and among power-of-two splits only."""
    if not wino_shape_ok(c, precision):
        return False
    if tile:
        if tile not in TILES or not tile_holds_a_component(c, tile):
            return False
    else:
        if sk and (sk & (sk - 1) or sk > min(32, (c.C1 + c.C2) // 32)):
            return False
        if not any(tile_holds_a_component(c, t) for t in TILES if t != 52):
            return False
    if sk == 0:
        return True
    eff = slices(gemm_case(c), sk)[3]
    return eff == 1 or tree_possible(gemm_case(c), sk)


def wino_sks(c):
    """the distinct split-K hints the Winograd path admits (the reducer form of any other split is refused)"""
    return [sk for sk in distinct_sks(gemm_case(c)) if wino_ok(c, next(iter(wino_tiles(c)), 0) or 0, sk)]


def tiles_per_part(c):
    """wino_tiles_per_part (conv_f16x2_wino.inc:94-100)"""
    T, R = tiles_of(c), 256 // (c.Cout // 4)
    parts = max(1, min(64, T // R))
    return -(-(-(-T // parts)) // R) * R


def gn_parts(c, Gn, tile=0, sk=0):
    """mf_wino_gn_parts (conv_f16x2_wino.inc:101-104)"""
    if not wino_ok(c, tile, sk) or Gn <= 0 or Gn > 256 or c.Cout % Gn or (c.Cout // Gn) % 4:
        return 0
    return -(-tiles_of(c) // tiles_per_part(c))


def output_rounds(c):
    """(R, parts, rounds of the first part, tiles of the last part) of wino_output_kernel (winograd.h:184-190): R tile lanes side by side"""
    T, R, tpp = tiles_of(c), 256 // (c.Cout // 4), tiles_per_part(c)
    parts = -(-T // tpp)
    return R, parts, -(-min(tpp, T) // R), T - (parts - 1) * tpp


def tail_ok(c, Gn):
    """mf_wino_tail_ok (conv_f16x2_wino.inc:164-169)"""
    if not wino_ok(c) or Gn <= 0 or c.Cout % Gn:
        return False
    cpg = c.Cout // Gn
    if cpg % 8 or 256 % (cpg // 4):
        return False
    return c.H * c.W * cpg * 4 <= 64 * 1024


def f32_ok(c, Gn, precision):
    """mf_wino_f32_ok (conv_f16x2_wino.inc:266-276)"""
    if (precision not in (0, 3) or (c.k, c.stride, c.pad, c.ups) != (3, 1, 1, 0) or c.N <= 0 or c.H < 2 or c.W < 2 or c.H % 2 or c.W % 2 or c.C1 <= 0 or
            c.C1 % 32 or c.C2 < 0 or c.C2 % 32 or c.Cout % 64 or c.Cout > 1024 or Gn <= 0 or c.Cout % Gn):
        return False
    cpg = c.Cout // Gn
    if cpg % 4 or 256 % (cpg // 4):
        return False
    if c.H * c.W * cpg * 4 > 64 * 1024:
        return False
    rows = c.N * tiles_of(c)
    return rows % 64 == 0 and rows * 16.0 < 2147483647.0


def sync_words(c, tile, eff_sk):
    """mf_wino_sync_words (conv_f16x2_wino.inc:86-91) for the plan (tile, effective split-K)"""
    if eff_sk <= 1:
        return 0
    bm, bn = TILES[tile]
    return -(-(16 * c.N * tiles_of(c)) // bm) * (c.Cout // bn) * (eff_sk - 1)


def input_refused_4gb(N, H, W, C):
    """the refusal of mf_wino_input_f16x2 (conv_f16x2_wino.inc:117): the transformed tensor [16][N][T][C] of 4-byte pairs must stay under 4 GB"""
    return not (16.0 * N * (H // 2) * (W // 2) * C * 4.0 < 4294967040.0)


INPUT_GRID_CAP = 256 * 16           # conv_f16x2_wino.inc:121 / :283: workgroups of 256 threads, one thread per (sample, tile, 4 channels)


def input_grid(N, H, W, C):
    """(workgroups launched, trips of the busiest thread) of wino_input_kernel / wino_input_f32_kernel"""
    total = N * (H // 2) * (W // 2) * (C // 4)
    blocks = min(-(-total // 256), INPUT_GRID_CAP)
    return blocks, -(-total // (blocks * 256))


def xcd_renumber(lin, total):
    """the renumbering of wino_tail_kernel (winograd.h:298-301): workgroup `lin` runs on XCD lin % 8; XCD x takes a contiguous range of (n, g) pairs"""
    q, r, xcd, within = total >> 3, total & 7, lin & 7, lin >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + within


def tail_census(c, Gn, nslots=0):
    """what a tail case reaches in wino_tail_kernel (winograd.h:290-573), from its launch arithmetic"""
    cpg = c.Cout // Gn
    cq = cpg // 4
    nel, tcq, total = c.H * c.W * cq, tiles_of(c) * cq, Gn * c.N
    return dict(cq=cq, nel=nel, idle_phase2=nel < 256, idle_phase1=tcq < 256, unrolled_only=nel <= 1024, rest_loop=nel > 1024,
                ragged_rest=nel > 1024 and nel % 256 != 0, remainder=total % 8 != 0, below_8=total < 8,
                slots=("none" if nslots == 0 else "one" if nslots == 1 else "under_256" if nslots < 256 else "256" if nslots == 256 else "second_loop"),
                lds=c.H * c.W * cpg * 4, padded_everywhere=c.H == 2 or c.W == 2)


# ---------------------------------------------------------------------------------------------------------------- references
def U64(w):
    """G g G^T: [Cout, Cin, 3, 3] -> [16, Cout, Cin] fp64 (k = 4 i + j)"""
    return torch.einsum("ia,ocab,jb->ijoc", G, w.double(), G).reshape(16, w.shape[0], w.shape[1])


def V64(x):
    """B^T d B of NCHW x: -> [16, N, T, C] fp64, tiles row-major over (H/2, W/2)"""
    n, c, h, w = x.shape
    patches = F.pad(x.double(), (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)           # [n, c, h/2, w/2, 4, 4]
    return torch.einsum("ia,nctuab,jb->ijntuc", BT, patches, BT).reshape(16, n, (h // 2) * (w // 2), c)


def Vabs64(x):
    """|B^T| |d| |B|: the magnitude the roundings of V are relative to (>= |B^T d B| element-wise)"""
    n, c, h, w = x.shape
    patches = F.pad(x.double().abs(), (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)
    return torch.einsum("ia,nctuab,jb->ijntuc", BT.abs(), patches, BT.abs()).reshape(16, n, (h // 2) * (w // 2), c)


def _bt_d_b_f32(d):
    """wino_bt_d_b (winograd.h:63-74) in fp32, operation by operation: d [..., 4, 4] (row, column)"""
    d0, d1, d2, d3 = d[..., 0, :], d[..., 1, :], d[..., 2, :], d[..., 3, :]
    t = torch.stack([d0 - d2, d1 + d2, d2 - d1, d1 - d3], dim=-2)
    t0, t1, t2, t3 = t[..., 0], t[..., 1], t[..., 2], t[..., 3]
    return torch.stack([t0 - t2, t1 + t2, t2 - t1, t1 - t3], dim=-1)


def V32(x):
    """the input transform as the kernels add it, in fp32: NCHW fp32 -> [16, N, T, C] fp32"""
    n, c, h, w = x.shape
    patches = F.pad(x.float(), (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)
    return _bt_d_b_f32(patches).permute(4, 5, 0, 2, 3, 1).reshape(16, n, (h // 2) * (w // 2), c)


def output32(m, b, c):
    """A^T M A + bias in the association order of wino_output_kernel / wino_tail_kernel (winograd.h:203-209), fp32: m [16, N, T, Cout] -> NCHW"""
    mm = m.float()
    a0 = [(mm[cc] + mm[4 + cc]) + mm[8 + cc] for cc in range(4)]
    a1 = [(mm[4 + cc] - mm[8 + cc]) - mm[12 + cc] for cc in range(4)]
    be = torch.zeros(c.Cout) if b is None else b.float()
    y00, y01 = ((a0[0] + a0[1]) + a0[2]) + be, ((a0[1] - a0[2]) - a0[3]) + be
    y10, y11 = ((a1[0] + a1[1]) + a1[2]) + be, ((a1[1] - a1[2]) - a1[3]) + be
    th, tw = c.H // 2, c.W // 2
    y = torch.stack([torch.stack([y00, y01], -1), torch.stack([y10, y11], -1)], -2)      # [N, T, Cout, 2, 2]
    y = y.reshape(c.N, th, tw, c.Cout, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(c.N, c.Cout, c.H, c.W)
    return y


def restate_fp32(x1, x2, w, b, c):
    """the four steps in plain fp32 torch: U once rounded, V, the 16 products summed over Cin, A^T M A + bias in the kernel's order -> NCHW fp32"""
    u = U64(w).float()
    x = torch.cat([x1, x2], 1) if x2 is not None else x1
    v = V32(x.float())
    m = torch.einsum("kntc,koc->knto", v, u)
    return output32(m, b, c)


# the components each of the 2 x 2 outputs of a tile reads: rows i of A^T's row a times columns j of A^T's row b (nine of the sixteen)
_ROWS = {0: (0, 1, 2), 1: (1, 2, 3)}
OUT_COMPONENTS = {(a, b): [4 * i + j for i in _ROWS[a] for j in _ROWS[b]] for a in (0, 1) for b in (0, 1)}


def sabs_wino(x1, x2, w, c, vabs=None):
    """sum over the input channels and the nine components an output reads of |U_k| |V_k| (vabs: another magnitude for V), NCHW fp64"""
    x = torch.cat([x1, x2], 1) if x2 is not None else x1
    p = torch.einsum("kntc,koc->knto", V64(x).abs() if vabs is None else vabs, U64(w).abs())
    th, tw = c.H // 2, c.W // 2
    out = torch.zeros((c.N, c.Cout, c.H, c.W), dtype=torch.float64)
    for (a, b), ks in OUT_COMPONENTS.items():
        out[:, :, a::2, b::2] = p[ks].sum(0).reshape(c.N, th, tw, c.Cout).permute(0, 3, 1, 2)
    return out


# ---------------------------------------------------------------------------------------------------------------- A. exact cases
# rows = N T = 64 reached five ways (H = 2 or W = 2: every tap of some patch row or column is padding), then 128 and 256.  Cout = 256 so that both
# 64-row tiles (37: 64 x 256, 53: 64 x 128) exist
ROW_CASES = [case(f"rows{n * (h // 2) * (w // 2)}_{n}x{h}x{w}", n, (h, w), 32, Cout=256)
             for n, h, w in ((64, 2, 2), (16, 4, 4), (16, 2, 8), (4, 8, 8), (1, 16, 16), (8, 8, 8), (4, 16, 16))]
COUT_CASES = [case(f"Cout{co}", 8, (8, 8), 32, Cout=co) for co in (64, 128, 256, 512, 1024)]          # 1024: C4 = 256, R = 1, at Cin = 32
TWO_SOURCE_CASES = [case(f"c{c1}+{c2}", 8, (8, 8), c1, c2, Cout=256) for c1, c2 in ((32, 32), (64, 32), (32, 64), (96, 32))]
CIN_CASES = [case(f"Cin{ci}", 4, (8, 8), ci, Cout=128) for ci in (64, 128, 1024)]
K2048_CASE = case("K2048", 4, (8, 8), 1024, 1024, Cout=128)                                              # 64 channel groups: split-K up to 64 in the launch
EXACT_CASES = ROW_CASES + COUT_CASES + TWO_SOURCE_CASES + CIN_CASES + [K2048_CASE]
RATIO = 13                          # log2 of the two sources' scale ratio (module docstring)


def variants(c):
    """the (family, ratio) operand sets of a case"""
    if c.C2 == 0:
        return [("xlo", None), ("wlo", None), ("int8", None)]
    return [("xlo", RATIO), ("xlo", -RATIO), ("wlo", RATIO), ("wlo", -RATIO), ("int8", RATIO)]


def keep(c):
    """probability with which wino_operands keeps a non-zero of conv2d_cases.exact_operands: 1/2 at Cin = 32 (a transform-domain value adds up to 9
    weights / 4 pixels, the budget of the direct form is nearly full as it stands), lowered like 1/sqrt(Cin) so that the expected sum |U||V|
    stays where it is at Cin = 32; two-source cases halve it again for the 2^13 of the larger source.  (The budget is asserted, not assumed.)"""
    cin = c.C1 + c.C2
    p = 0.5 * math.sqrt(32.0 / cin)
    return p / 2 if c.C2 else p


def wino_operands(c, family, ratio, seed=0):
    """(x1, x2, w, b): conv2d_cases.exact_operands thinned by keep(c); fp64 tensors whose values are fp32 values (NCHW, OIHW).  The first element of
    every sample and of the weights stays 1 (the operands' scales are those of the direct families)"""
    x1, x2, w, b, _ = exact_operands(c, family, ratio, seed)
    g = torch.Generator().manual_seed(_seed_of(c.name, family, ratio, seed, "thin"))
    p = keep(c)

    def thin(t, per_sample):
        m = (torch.rand(t.shape, generator=g, dtype=torch.float64) < p).double()
        if per_sample:
            m.view(t.shape[0], -1)[:, 0] = 1.0
        else:
            m.view(-1)[0] = 1.0
        return t * m

    return thin(x1, True), (None if x2 is None else thin(x2, True)), thin(w, False), b


def _unit_exps(t, dim):
    """per index of `dim`: log2 of the largest power of two dividing every value of t there (10^9 where all are zero)"""
    t = t.double().movedim(dim, 0).reshape(t.shape[dim], -1)
    m, e = torch.frexp(t.abs())
    mi = (m * 2.0 ** 53).long()
    tz = (mi & -mi).double().log2()
    u = torch.where(t != 0, e.double() - 53 + tz, torch.full_like(t, 1e9))
    return u.amin(dim=1)


def wino_budget(c, x1, x2, w, b):
    """The conditions (a) - (c) as figures, per case and family (the CPU test asserts them):
      lolo     -- max |lo'(U)| max |lo'(V)| (0: no lo.lo product)
      pair_ok  -- U (under max |U|) and V (sample n, source s under 4 max |x_s[n]|) are hi + lo'/2048 exactly, U is an fp32 value
      units    -- per sample, log2 of the common unit of every hi and lo' product; bias_ok: the bias is a multiple of each
      bits     -- per sample, log2 of [max over outputs of sum over channels and the output's nine components of (|hi| + |lo|)(U) (|hi| + |lo|)(V)]
                  in that unit (< 24)
      bits16   -- the same summed loosely over all 16 components (the figure the direct families were measured with)
      bits_with_bias -- the worst sample's figure with |bias| added.  Under sample scales of 2^-20 and a bias of 2^20 it cannot stay below 24: the bias
                  is the LAST addition of an output (winograd.h:208-209), from an exactly summed operand, so it rounds once to float32(ref64)
                  wherever conv3d_cases.bias_add_rounds_once holds -- the CPU test asserts that instead, as the direct families do"""
    u = U64(w)
    pair_ok = bool(torch.equal(u.float().double(), u))
    ub = float(u.abs().max())
    us, uh, ul = pair_terms(u, ub)
    uh, ul = uh * 2.0 ** us, ul * 2.0 ** us / 2048.0
    pair_ok &= bool(torch.equal(uh + ul, u))
    uabs = uh.abs() + ul.abs()
    u_unit = torch.minimum(_unit_exps(uh, 2), _unit_exps(ul, 2))                   # per input channel
    lolo, units, bits, bits16, bias_ok, bits_b = 0.0, [], [], [], True, -1e9
    th, tw = c.H // 2, c.W // 2
    for n in range(c.N):
        vh_, vl_ = [], []
        for x in ([x1[n:n + 1]] + ([x2[n:n + 1]] if x2 is not None else [])):
            v = V64(x)
            vs, vh, vl = pair_terms(v, 4.0 * float(x.float().abs().max()))
            vh, vl = vh * 2.0 ** vs, vl * 2.0 ** vs / 2048.0
            pair_ok &= bool(torch.equal(vh + vl, v))
            # the source itself reproduces in the pair form the transform starts from, and the fp32 sums of four are exact
            xs, xh, xl = pair_terms(x, float(x.float().abs().max()))
            pair_ok &= bool(torch.equal((xh + xl / 2048.0) * 2.0 ** xs, x)) and bool(torch.equal(V32(x).double(), v))
            lolo = max(lolo, float(vl.abs().max()) * float(ul.abs().max()))
            vh_.append(vh)
            vl_.append(vl)
        vh, vl = torch.cat(vh_, 3), torch.cat(vl_, 3)
        v_unit = torch.minimum(_unit_exps(vh, 3), _unit_exps(vl, 3))
        both = (v_unit < 1e8) & (u_unit < 1e8)
        unit = float((v_unit + u_unit)[both].min())
        p = torch.einsum("kntc,koc->knto", vh.abs() + vl.abs(), uabs)[:, 0]         # [16, T, Cout]
        worst = max(float(p[ks].sum(0).max()) for ks in OUT_COMPONENTS.values())
        units.append(unit)
        bits.append(math.log2(worst / 2.0 ** unit))
        bits16.append(math.log2(float(p.sum(0).max()) / 2.0 ** unit))
        bias_ok &= _is_multiple(b, 2.0 ** unit)
        bits_b = max(bits_b, math.log2(max(float(max((p[ks].sum(0) + b.abs().view(1, -1)).max() for ks in OUT_COMPONENTS.values())), 1e-300) / 2.0 ** unit))
    return dict(lolo=lolo, pair_ok=pair_ok, units=units, bits=bits, bits16=bits16, bias_ok=bias_ok, bits_with_bias=bits_b)


def direct_units(c, family, ratio):
    """log2 of the direct form's output unit per sample, as conv2d_cases.exact_operands states it for ratio +-20; at the ratio of this file the two-source
    unit is that of the smaller source (13: the larger source's lo part is a whole multiple of it)"""
    exps = CC.sample_exps(c, ratio)
    if c.C2 == 0:
        return [e1 if family == "int8" else e1 - CC.LO_BITS for e1, _ in exps]
    return [min(e1, e2) for e1, e2 in exps]


# ---------------------------------------------------------------------------------------------------------------- B. GroupNorm records
# wino_output_kernel runs R = 256 / (Cout / 4) tile lanes; a part holds tiles_per_part tiles (output_rounds).  Cout = 64 has 128- and 256-row
# tiles only, so N T % 128 == 0 there (the shape (2, 66, 64, 32, 0, 64) has 2112 rows = 16.5 x 128: the library refuses it, the CPU test says so):
#   T<R            T = 1, R = 4: three idle tile lanes
#   one_round      T = 16, R = 4: 4 parts of one round
#   rounds_whole   4 x 66 x 64, Cout 64: T = 1056, R = 16, 64 parts wanted, cdiv(1056, 64) = 17 -> 32 tiles per part: 33 parts of two rounds
#   rounds_ragged  8 x 130 x 32, Cout 64: T = 1040 -> 32 per part: 33 parts, the last holds 16 tiles (one round where the others run two)
#   ragged_round   64 x 2 x 6, Cout 128: T = 3, R = 8: one part whose only round is ragged
#   R1             Cout = 1024: C4 = 256, R = 1, T = 16: 16 parts of one tile, at Cin = 32
RECORD_CASES = [case("T<R", 64, (2, 2), 32, Cout=256), case("one_round", 4, (8, 8), 32, Cout=256), case("rounds_whole", 4, (66, 64), 32, Cout=64),
                case("rounds_ragged", 8, (130, 32), 32, Cout=64), case("ragged_round", 64, (2, 6), 32, Cout=128), case("R1", 8, (8, 8), 32, Cout=1024)]
RECORD_GROUPS = {64: 8, 128: 8, 256: 32, 1024: 32}
ISSUE_EXAMPLE_REFUSED = case("issue_2x66x64", 2, (66, 64), 32, Cout=64)


# ---------------------------------------------------------------------------------------------------------------- C. the bound on real operands
def real_bound_c(c, sk=1):
    """|y - y64| <= c (sum |U_k| |B^T||d||B|_k + |bias|), in units of 2^-24, by counting roundings per product and per sum:
      2  the pair form of x (2^-23 |x|: tests/test_kernels_gpu.py::test_split_f16x2_format), carried through the +-1 sums: relative to |B^T||d||B|
      2  the two fp32 roundings of B^T d B (each relative to a partial sum <= |B^T||d||B|)
      2  the pair form of V
      1  the one fp32 rounding of U, 2 its pair form
      4  the dropped lo.lo term (|lo| <= 2^-11 of its operand each)
      2 per 32-channel chunk of one chain, + 2 for joining the two accumulators and + 2 per level of the split-K tree: fp32 accumulation of the
         matrix cores (truncating: a whole ulp per step), relative to the partial sum
      5  A^T M A + bias: four additions on the longest path to an output and the bias, each relative to a partial sum of |M| and |bias|
    The floor of the pair format (2^-50 of the sample's bound per value, on values far below the bound) is added separately (real_bound)."""
    chunks = -(-((c.C1 + c.C2) // 32) // sk)
    levels = max(0, int(math.log2(sk)))
    return 2 + 2 + 2 + 1 + 2 + 4 + 2 * chunks + 2 + 2 * levels + 5


def real_bound(x1, x2, w, b, c, sk=1):
    """the element-wise bound of real_bound_c, NCHW fp64: c 2^-24 (sum |U_k| |B^T||d||B|_k + |b|) + the format's floor 2^-50 x 16 bound(x) sum |U_k|"""
    x = torch.cat([x1, x2], 1) if x2 is not None else x1
    s = sabs_wino(x1, x2, w, c, vabs=Vabs64(x)) + b.double().abs().view(1, -1, 1, 1)
    floor = 2.0 ** -50 * 16.0 * x.abs().amax(dim=(1, 2, 3)).view(-1, 1, 1, 1) * U64(w).abs().sum(dim=(0, 2)).view(1, -1, 1, 1) * 2
    return real_bound_c(c, sk) * U24 * s + floor


REAL_CASES = [case("real_32x4x6", 32, (4, 6), 32, Cout=128), case("real_c64+32", 8, (8, 8), 64, 32, Cout=128), case("real_2x8x2", 32, (8, 2), 96, Cout=128)]

# ---------------------------------------------------------------------------------------------------------------- D. the transforms
INPUT_GEOMS = ((2, 2), (2, 8), (8, 2), (4, 6), (8, 12))
INPUT_CHANNELS = (8, 24, 40)
PACK_CASE = (24, 13)                 # Cout x Cin = 312: no multiple of the 256 threads of a workgroup
# the grid cap: N T C / 4 threads; (5, 64, 64, 1024) gives 5 x 1024 x 256 = 1 310 720 > 4096 x 256 = 1 048 576; one sample (262 144) stays under it
GRID_CAP_SHAPE = (5, 64, 64, 1024)
SENTINEL = 64                        # int32 / float words behind an output that must stay untouched

# ---------------------------------------------------------------------------------------------------------------- E. the tail
# Tail = (conv case, G, residual kind, nslots, emb, affine, act, out_fp32, want_wino)
Tail = namedtuple("Tail", "c G res nslots emb affine act out_fp32 want_wino")
TAIL_CASES = [
    Tail(case("nel8", 64, (2, 2), 32, Cout=128), 16, "f32", 0, True, True, 1, True, True),            # cq = 2, nel = 8: 248 idle threads; every tap row padded
    Tail(case("nel384", 8, (8, 12), 32, Cout=128), 8, "pairs", 0, True, True, 1, True, True),         # cq = 4, nel = 384 (the smallest published one)
    Tail(case("nel1024", 2, (16, 16), 32, Cout=128), 8, "slots", 7, True, True, 1, False, True),      # cq = 4: exactly the four unrolled rounds
    Tail(case("nel1152", 8, (16, 18), 32, Cout=128), 8, "pairs", 0, False, True, 1, False, True),     # nel = 1152 = 4 x 256 + 128: rest loop, ragged round
    Tail(case("nel1152f", 8, (16, 18), 32, Cout=128), 8, "f32", 0, True, False, 0, True, False),      # the same loop on an fp32 residual; no affine, no act
    Tail(case("lds64k", 2, (32, 32), 32, Cout=512), 32, "pairs", 0, True, True, 1, False, True),      # 1024 pixels x 16 channels x 4 bytes = 64 KB
    Tail(case("GN4", 4, (8, 8), 32, Cout=128), 1, "slots", 1, True, True, 1, True, True),             # cpg = Cout: cq = 32; G N = 4 < 8: q = 0, r = 4
    Tail(case("GN10", 5, (16, 16), 32, Cout=128), 2, None, 0, False, True, 1, True, False),           # G N = 10: q = 1, r = 2; cpg = 64, 64 KB
    Tail(case("slots256", 4, (8, 8), 32, Cout=128), 8, "slots", 256, True, True, 0, True, True),
    Tail(case("slots257", 4, (8, 8), 32, Cout=128), 8, "slots", 257, False, True, 1, True, False),
    Tail(case("slots600", 4, (8, 8), 32, Cout=128), 8, "slots", 600, True, False, 1, False, True),
    Tail(case("slots448", 4, (8, 8), 32, Cout=128), 8, "slots", 448, True, True, 1, True, False),
    Tail(case("H2", 16, (2, 8), 32, Cout=128), 8, "pairs", 0, True, True, 1, True, True),             # the V output at H = 2
]
TAIL_SCALES = 4                      # distinct sample scales, cycled: 2^(6 (n % 4) - 3)
TAIL_SCALE_STEP = 6
# where slot_table puts the true maximum, per slot count: the thread that alone reads that slot sits in wave 0, 0, 3, 0 (second loop), 1 (second
# loop), 2 (second loop) -- slot_reader() -- so a wave left out of the maximum of the four wave maxima (winograd.h:433) shows in some case
SLOT_MAX_AT = {1: 0, 7: 2, 256: 255, 257: 256, 600: 599, 448: 447}


def tail_scale_exps(n):
    """log2 of sample n's scale: 2^6 apart, cycled over TAIL_SCALES samples (groupnorm_cases.scales, kept inside fp32 at the batch of 64)"""
    return TAIL_SCALE_STEP * (n % TAIL_SCALES) - 3


def small_operands(c, bias=True, seed=0):
    """exact-y operands whose y is a SMALL integer in its unit (the tail cases and the GroupNorm records) -> (x1, w, b) fp64.  The integer family
    thinned (wino_operands) with every activation reduced to its sign times the sample's scale 2^(6 (n % 4) - 3), and a constant channel: channel 0 of every sample is its scale everywhere and the centre tap of its
    weights is m for every output channel, so every output of sample n is shifted by m times its scale, about half the spread of y
    (groupnorm_cases: a mean of half the scale).  y is then a small integer in the sample's unit (scale / 4): the fp32 sums of 16 values and of
    their squares the kernels form before they go to fp64 are exact (tail_sums_exact states it, the CPU test asserts it).
    bias: k 2^13, |k| <= 3, on every third channel -- a whole multiple of every sample's unit, so y stays exact; it breaks the premise of
    tail_sums_exact on the small samples, so the tests that need exact sums run without it"""
    assert c.C2 == 0
    x1, _, w, _ = wino_operands(c, "int8", None, seed)
    for n in range(c.N):
        x1[n] = torch.sign(x1[n]) * 2.0 ** tail_scale_exps(n)
        x1[n, 0] = 2.0 ** tail_scale_exps(n)
    p = keep(c)
    m = max(1.0, round(0.5 * math.sqrt(9.0 * (c.C1 - 1)) * 0.5 * p))                  # half the std of a sum of 9 (Cin - 1) (p / 2)^2 products of +-1
    w[:, 0] = 0.0
    w[:, 0, 1, 1] = m
    b = torch.zeros(c.Cout, dtype=torch.float64)
    if bias:
        g = torch.Generator().manual_seed(_seed_of(c.name, "tailbias", seed))
        top = tail_scale_exps(TAIL_SCALES - 1) - 2
        b[::3] = torch.randint(1, 4, (len(b[::3]),), generator=g).double() * (torch.randint(0, 2, (len(b[::3]),), generator=g).double() * 2 - 1) * 2.0 ** top
    return x1, w, b


def tail_sums_exact(y, c):
    """premise of exact statistics: per sample, y NCHW is a whole multiple of the unit u = scale / 4 and 16 max |y / u|^2 < 2^24: the fp32 sum of a
    tile's 4 pixels x 4 channels and the fp32 fma chain of their squares (winograd.h:393-400, :222-229) are exact, and so is every fp64 sum behind"""
    for n in range(c.N):
        u = 2.0 ** (tail_scale_exps(n) - 2)
        if not _is_multiple(y[n], u) or 16.0 * float((y[n] / u).abs().max()) ** 2 >= 2.0 ** 24:
            return False
    return True


def tail_side_operands(t, seed=0):
    """(gamma, beta, residual NHWC, wide [N, C + 8]) fp32 of a tail case, scaled per sample as groupnorm_cases.apply_inputs scales them: the residual
    by the FLIPPED scales (the largest residual meets the smallest y), the embedding by the sample's own"""
    c = t.c
    g = torch.Generator().manual_seed(_seed_of(c.name, "tailside", seed))
    sc = torch.tensor([2.0 ** tail_scale_exps(n) for n in range(c.N)])
    gamma = (1.0 + 0.3 * torch.randn((c.Cout,), generator=g)) if t.affine else None
    beta = 0.2 * torch.randn((c.Cout,), generator=g) if t.affine else None
    res = (torch.randn((c.N, c.H, c.W, c.Cout), generator=g) * 2.0 * sc.flip(0).view(-1, 1, 1, 1)) if t.res else None
    wide = (torch.randn((c.N, c.Cout + 8), generator=g) * 0.5 * sc.view(-1, 1)) if t.emb else None
    return gamma, beta, res, wide


def slot_reader(nslots, i):
    """the threads of wino_tail_kernel that read slot i of nslots (winograd.h:339, :412): thread min(tid, nslots - 1) reads the entry burst's slot, the
    loop behind it gives slot i >= 256 to thread i % 256 -> (first thread, last thread)"""
    if i >= 256:
        return i % 256, i % 256
    return (i, 255) if i == nslots - 1 else (i, i)


def slot_table(res, nslots, seed=0):
    """[N, nslots] slot maxima a convolution would have left for `res` NHWC: the true maximum sits in slot SLOT_MAX_AT[nslots], every other slot
    holds a smaller non-negative value"""
    n = res.shape[0]
    g = torch.Generator().manual_seed(_seed_of("slots", nslots, seed))
    mx = res.abs().amax(dim=(1, 2, 3))
    sl = torch.rand((n, nslots), generator=g) * 0.5 * mx.view(-1, 1)
    sl[:, SLOT_MAX_AT[nslots]] = mx
    return sl


def tail_bounds(t, gamma, beta, res_bound, emb):
    """(bconst, out_bound [N]) in the kernel's fp32 order (winograd.h:434): bconst + rb + eb"""
    c = t.c
    cpg = c.Cout // t.G
    from tests.groupnorm_cases import bconst_of
    bconst = bconst_of(gamma, beta, c.H * c.W, cpg)
    bc = torch.tensor(bconst, dtype=torch.float32)
    rb = res_bound.float() if res_bound is not None else torch.zeros(c.N)
    eb = emb.float().abs().amax(dim=1) if emb is not None else torch.zeros(c.N)
    return bconst, (bc + rb) + eb


# fp32 form (precision 0 and 3): (conv case, G) -- rows % 64 at its edge (64 rows), cpg = 4 (cq = 1), the published two-source shape scaled down
F32_CASES = [(case("f32_rows64", 4, (8, 8), 32, Cout=64), 16), (case("f32_rows128_2src", 8, (8, 8), 32, 32, Cout=128), 8), (case("f32_H2", 64, (2, 2), 32, Cout=64), 16)]
F32_REFUSED = [(case("f32_rows48", 3, (8, 8), 32, Cout=64), 16), (case("f32_cpg2", 4, (8, 8), 32, Cout=64), 32), (case("f32_lds", 1, (64, 64), 32, Cout=512), 32)]
