"""The 3-D convolution (csrc/conv3d.hip) at its edges: references, exact operands and the case lists of tests/test_conv3d_cpu.py and
tests/test_conv3d_gpu.py.  Plain Python and torch, no device.

Exact operands.  The kernel computes sum(w x) on fp16 pairs (x ~ hi + lo'/2048 under a per-sample power-of-two scale, three matrix terms, fp32
accumulators, split_f16.h).  Operands on which that arithmetic is EXACT make the kernel's result float32(ref64) bit for bit, in any summation
order, on every tile and split-K plan:
  * family "xlo": activations a + b 2^-13 (a in {-1, 0, 1}, |b| <= 3, b = 0 where a = 0) carry a non-zero lo', weights in {-1, 0, 1} have lo = 0;
    family "wlo" is the mirror.  lo.lo, the term the kernel drops, is identically zero; hi.hi, hi.lo' and lo'.hi are all exercised.
  * every product is a whole multiple of the sample's output unit u (a power of two) and sum |w||x| < 2^24 u, so every partial sum -- of either
    accumulator, of their combination, of the split-K slabs -- is an integer below 2^24 in that unit and exact in fp32.
  * two sources whose scales differ by 2^20 leave 4 bits above the smaller source's unit: the LARGER source of a sample is sparse (a few non-zero
    voxels, at most 8 products per output) and it alone carries the lo part; the smaller one holds plain integers.  In family "wlo" the lo part
    sits in the weights of the larger source's channels, so the ratio is the same for every sample of a case (+20 or -20).
  * samples are scaled 2^0, 2^20, 2^-20; the bias is k 2^20 on every third channel (a multiple of every sample's unit), zero elsewhere.  Where the
    bias lies far above the sample's values the final add rounds ONCE, from an exact operand: still float32(ref64) (bias_add_rounds_once).
exact_budget() states these conditions; the CPU test asserts them for every case of every list below."""

import math
from collections import namedtuple

import torch
import torch.nn.functional as F

SAMPLE_EXPS = (0, 20, -20)          # per-sample scales 2^e of the exact cases, cycled over the batch
LO_BITS = 13                        # the lo part: b 2^-13
SPLIT_KS = (1, 2, 4, 8, 16)
TILES = (1, 2, 3, 4)


# ---------------------------------------------------------------------------------------------------------------- references
def _cat_up(x1, x2, up):
    x = torch.cat([x1, x2], 1) if x2 is not None else x1
    if any(up):
        x = F.interpolate(x, scale_factor=tuple(2.0 if u else 1.0 for u in up), mode="nearest")
    return x


def ref64(x1, x2, w, b, stride, pad, up):
    """fp64: torch.cat of the two sources, nearest x2 per axis, F.conv3d"""
    return F.conv3d(_cat_up(x1.double(), None if x2 is None else x2.double(), up), w.double(), None if b is None else b.double(), stride, pad)


def sabs64(x1, x2, w, stride, pad, up):
    """sum |w||x| of every output, fp64"""
    return F.conv3d(_cat_up(x1.double().abs(), None if x2 is None else x2.double().abs(), up), w.double().abs(), None, stride, pad)


def out_dims(dhw, k, stride, pad, up):
    return tuple(((e << u) + 2 * p - k) // s + 1 for e, s, p, u in zip(dhw, stride, pad, up))


def gather64(x1, x2, w, b, stride, pad, up):
    """The kernel's stated rule, tap by tap, without F.interpolate / F.conv3d: coordinate u of the upsampled grid reads voxel u >> 1 (u where the
    axis is not upsampled), zero outside [0, D << ud)."""
    x = (torch.cat([x1, x2], 1) if x2 is not None else x1).double()
    w = w.double()
    n, _, *dhw = x.shape
    k = w.shape[2]
    od = out_dims(dhw, k, stride, pad, up)
    y = torch.zeros((n, w.shape[0], *od), dtype=torch.float64)

    def axis(a, kk):
        u = torch.arange(od[a]) * stride[a] - pad[a] + kk
        ok = (u >= 0) & (u < (dhw[a] << up[a]))
        return (u.clamp(0, (dhw[a] << up[a]) - 1) >> up[a]), ok.double()

    for kd in range(k):
        iz, vz = axis(0, kd)
        for kh in range(k):
            iy, vy = axis(1, kh)
            for kw in range(k):
                ix, vx = axis(2, kw)
                patch = x[:, :, iz][:, :, :, iy][:, :, :, :, ix] * (vz[:, None, None] * vy[None, :, None] * vx[None, None, :])
                y += torch.einsum("ncdhw,oc->nodhw", patch, w[:, :, kd, kh, kw])
    return y if b is None else y + b.double().view(1, -1, 1, 1, 1)


# ---------------------------------------------------------------------------------------------------------------- split_f16.h in torch
def scale_exp(bound: float) -> int:
    """scale_exp_of: floor(log2 bound) - 14 from the exponent field of the fp32 bound, clamped to +-100 (a zero bound: -100)"""
    bits = torch.tensor([bound], dtype=torch.float32).view(torch.int32).item()
    return max(-100, min(100, ((bits >> 23) & 0xFF) - 127 - 14))


def pair_terms(x, bound: float):
    """(s, hi, lo'): the fp16 pair of fp32 values x under `bound`: x 2^-s ~ hi + lo'/2048, hi = RN16(x 2^-s), lo' = RN16((x 2^-s - hi) 2048)"""
    s = scale_exp(bound)
    xs = x.float().double() * 2.0 ** -s
    hi = xs.float().half().double()          # (xs is an fp32 value times a power of two: the one rounding is the fp16 one)
    lo = ((xs - hi) * 2048.0).float().half().double()
    return s, hi, lo


# ---------------------------------------------------------------------------------------------------------------- cases
Case = namedtuple("Case", "name N dhw C1 C2 Cout k stride pad up")


def case(name, N, dhw, C1, C2, Cout, k, stride=(1, 1, 1), pad=None, up=(0, 0, 0)):
    return Case(name, N, tuple(dhw), C1, C2, Cout, k, tuple(stride), tuple(pad) if pad is not None else ((k // 2,) * 3), tuple(up))


def _s(t):
    return "".join(map(str, t))


def _geoms():
    out = []
    for dhw in ((4, 6, 8), (5, 7, 9)):
        for stride in ((1, 1, 1), (2, 2, 2), (1, 2, 2)):
            for up in ((0, 0, 0), (1, 1, 1), (0, 1, 1)):
                for pad in (0, 1, 2):
                    out.append(case(f"{_s(dhw)}k3p{pad}s{_s(stride)}u{_s(up)}", 3, dhw, 32, 0, 6, 3, stride, (pad,) * 3, up))
                out.append(case(f"{_s(dhw)}k1s{_s(stride)}u{_s(up)}", 3, dhw, 32, 0, 6, 1, stride, (0,) * 3, up))
    for dhw in ((1, 1, 1), (1, 5, 6), (3, 1, 4)):   # extents of 1: every k = 3 window hangs over both edges of such an axis
        for pad in (1, 2):
            out.append(case(f"{_s(dhw)}k3p{pad}", 3, dhw, 32, 0, 6, 3, pad=(pad,) * 3))
        out.append(case(f"{_s(dhw)}k3p1u111", 3, dhw, 32, 0, 6, 3, up=(1, 1, 1)))
        out.append(case(f"{_s(dhw)}k3p1u111s2", 3, dhw, 32, 0, 6, 3, (2, 2, 2), (1,) * 3, (1, 1, 1)))
        out.append(case(f"{_s(dhw)}k1", 3, dhw, 32, 0, 6, 1))
    # eight output voxels per sample, nine samples: a 32-lane fragment holds four samples, M = 72 crosses a 64-row tile
    out.append(case("n9_222k3", 9, (2, 2, 2), 32, 0, 6, 3))
    out.append(case("n9_222k1", 9, (2, 2, 2), 32, 0, 6, 1))
    out.append(case("n9_444k3s2", 9, (4, 4, 4), 32, 0, 6, 3, (2, 2, 2)))
    return out


GEOM_CASES = _geoms()
# M = N D H W at the edges of the 64- and 128-row tiles (k = 1: M is the input's voxel count)
M_EDGE_CASES = [case(f"M{n * d * h * w}", n, (d, h, w), 32, 0, 8, 1)
                for n, (d, h, w) in ((3, (1, 3, 7)), (2, (2, 4, 4)), (5, (1, 1, 13)), (127, (1, 1, 1)), (2, (4, 4, 4)), (3, (1, 1, 43)))]
COUT_EDGE_CASES = [case(f"Cout{co}", 2, (2, 3, 4), 32, 0, co, 3) for co in (1, 3, 4, 63, 64, 65, 127, 128, 129)]


def _two_source():
    out = []
    for c1, c2, k in ((32, 32, 3), (64, 32, 3), (32, 64, 3), (64, 64, 1)):
        out.append(case(f"c{c1}+{c2}k{k}", 3, (3, 4, 5), c1, c2, 8, k))
        out.append(case(f"c{c1}+{c2}k{k}u111", 3, (2, 3, 2), c1, c2, 8, k, up=(1, 1, 1)))
        out.append(case(f"c{c1}+{c2}k{k}s2", 3, (4, 5, 6), c1, c2, 8, k, (2, 2, 2)))
    out.append(case("c96+96k1", 3, (3, 4, 5), 96, 96, 8, 1))   # (k = 1: a split slice of two chunks that straddles the switch)
    return out


TWO_SOURCE_CASES = _two_source()
# the split-K reducer's grid stops at 8192 x 256 elements: M Cout = 8448 x 256 gives its grid-stride loop a second trip
REDUCER_CASE = case("reducer_second_trip", 1, (16, 16, 33), 64, 0, 256, 1)
# the weight pack's grid stops at 4096 x 256 elements: Cout taps cin_pad = 512 x 27 x 96 (Cin = 72 < cin_pad)
PACK_CASE = dict(Cout=512, Cin=72, k=3, cin_pad=96)
# mutation target of the weight pack: Cin == taps, so that swapping t and ci in the source index stays inside the tensor
PACK_SQUARE_CASE = dict(Cout=5, Cin=27, k=3, cin_pad=32)
EXACT_CASES = GEOM_CASES + M_EDGE_CASES + COUT_EDGE_CASES + TWO_SOURCE_CASES + [REDUCER_CASE]


def variants(c):
    """the (family, ratio) operand sets of a case: ratio = log2 of the second source's scale against the first ("mixed": +20 / -20 by sample)"""
    if c.C2 == 0:
        return [("xlo", None), ("wlo", None)]
    return [("xlo", "mixed"), ("wlo", 20), ("wlo", -20)]


# ---------------------------------------------------------------------------------------------------------------- split-K arithmetic
def slices(c, sk):
    """(nit, it_sw, it_per_split, effective slices) of mf_conv3d_f16x2 for split-K hint sk >= 1"""
    nit = (c.C1 + c.C2) // 32 * c.k ** 3
    it_sw = c.C1 // 32 * c.k ** 3 if c.C2 > 0 else nit
    s = min(sk, nit)
    per = -(-nit // s)
    return nit, it_sw, per, -(-nit // per)


def slice_kinds(c, sk):
    """every slice [it0, it1) of the plan against the first iteration of the second source"""
    nit, it_sw, per, eff = slices(c, sk)
    kinds = []
    for z in range(eff):
        it0, it1 = z * per, min(nit, (z + 1) * per)
        assert it0 < it1
        if c.C2 == 0 or it1 < it_sw:
            kinds.append("before")
        elif it1 == it_sw:
            kinds.append("ends_at")
        elif it0 == it_sw:
            kinds.append("starts_at")
        elif it0 < it_sw:
            kinds.append("straddles")
        else:
            kinds.append("after")
    return kinds


def distinct_sks(c):
    """the split-K hints of SPLIT_KS that give different plans for this case"""
    seen, out = set(), []
    for sk in SPLIT_KS:
        key = slices(c, sk)
        if key not in seen:
            seen.add(key)
            out.append(sk)
    return out


# ---------------------------------------------------------------------------------------------------------------- exact operands
def _ints(g, shape, p_nonzero=0.5):
    """values in {-1, 0, 1}, non-zero with probability p_nonzero"""
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return sign * (torch.rand(shape, generator=g, dtype=torch.float64) < p_nonzero).double()


def _with_lo(g, a):
    """a + b 2^-13, |b| <= 3, b = 0 where a = 0"""
    b = torch.randint(-3, 4, a.shape, generator=g).double()
    return a + b * (a != 0).double() * 2.0 ** -LO_BITS


def _sparse(g, shape, nnz):
    """nnz entries of +-1 at random places (one of them at the origin, so the tensor is never zero), zero elsewhere"""
    t = torch.zeros(shape, dtype=torch.float64)
    flat = t.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:nnz]
    idx[0] = 0
    flat[idx] = torch.randint(0, 2, (nnz,), generator=g).double() * 2 - 1
    return t


def sample_exps(c, ratio):
    """per sample: (log2 scale of source 1, log2 scale of source 2)"""
    out = []
    for n in range(c.N):
        e = SAMPLE_EXPS[n % 3]
        r = 0 if ratio is None else ((20 if (n // 3 + n) % 2 == 0 else -20) if ratio == "mixed" else ratio)
        out.append((e, e + r))
    return out


def exact_operands(c, family, ratio, seed=0):
    """(x1, x2, w, b, unit_exps): fp64 tensors whose values are fp32 values (NCDHW, OIDHW), and log2 of every sample's output unit"""
    g = torch.Generator().manual_seed(_seed_of(c.name, family, ratio, seed))
    cin = c.C1 + c.C2
    wshape = (c.Cout, cin, c.k, c.k, c.k)
    exps = sample_exps(c, ratio)
    nnz = 1 if any(c.up) else 8          # an upsampled voxel meets a k = 3 window up to 8 times
    x1 = torch.zeros((c.N, c.C1, *c.dhw), dtype=torch.float64)
    x2 = torch.zeros((c.N, c.C2, *c.dhw), dtype=torch.float64) if c.C2 else None
    units = []
    w = _ints(g, wshape)
    if c.C2 == 0:
        if family == "wlo":
            w = _with_lo(g, w)
        for n, (e1, _) in enumerate(exps):
            a = _ints(g, x1.shape[1:])
            a.view(-1)[0] = 1.0
            x1[n] = (_with_lo(g, a) if family == "xlo" else a) * 2.0 ** e1
            units.append(e1 - LO_BITS)
    else:
        for n, (e1, e2) in enumerate(exps):
            big1 = e1 > e2
            dense = _ints(g, (x2 if big1 else x1).shape[1:])
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
    w.view(-1)[0] = 1.0      # max |w| in [1, 2): the weights' own scale is 2^-14
    b = torch.zeros(c.Cout, dtype=torch.float64)
    b[::3] = torch.randint(1, 3, (len(b[::3]),), generator=g).double() * (torch.randint(0, 2, (len(b[::3]),), generator=g).double() * 2 - 1) * 2.0 ** 20
    return x1, x2, w, b, units


def _seed_of(*parts):
    h = 2166136261
    for ch in "|".join(map(str, parts)).encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h & 0x3FFFFFFF


def exact_budget(c, x1, x2, w, b, units):
    """The qualifying conditions of an exact case, as a dict of figures (the CPU test asserts them):
      lolo       -- max |lo'_x| max |lo'_w| over the pair forms (must be 0: one operand has lo = 0 in every product)
      unit_ok    -- every activation is a multiple of ux, every weight of uw, ux uw >= the sample's output unit u, and the bias a multiple of u
      bits_m, bits_x, bits_all -- log2 of sum |terms| / u of the hi.hi accumulator, of the cross accumulator, and of sum |w||x| (each < 24)"""
    wb = float(w.abs().max())
    _, whi, wlo = pair_terms(w, wb)
    wexp = scale_exp(wb)
    lolo, bits_m, bits_x, bits_all, unit_ok = 0.0, -1e9, -1e9, -1e9, True
    for n in range(c.N):
        xs = [(x1[n:n + 1],)] + ([(x2[n:n + 1],)] if x2 is not None else [])
        his, los = [], []
        for (x,) in xs:
            s, hi, lo = pair_terms(x, float(x.abs().max()))
            his.append(hi * 2.0 ** s)
            los.append(lo * 2.0 ** s / 2048.0)
            lolo = max(lolo, float(lo.abs().max()) * float(wlo.abs().max()))
        hi1, hi2 = his[0], (his[1] if x2 is not None else None)
        lo1, lo2 = los[0], (los[1] if x2 is not None else None)
        wh, wl = whi * 2.0 ** wexp, wlo * 2.0 ** wexp / 2048.0
        u = 2.0 ** units[n]
        sm = sabs64(hi1, hi2, wh, c.stride, c.pad, c.up).max() / u
        sx = (sabs64(lo1, lo2, wh, c.stride, c.pad, c.up) + sabs64(hi1, hi2, wl, c.stride, c.pad, c.up)).max() / u
        sa = sabs64(x1[n:n + 1], None if x2 is None else x2[n:n + 1], w, c.stride, c.pad, c.up).max() / u
        bits_m, bits_x, bits_all = max(bits_m, _log2(sm)), max(bits_x, _log2(sx)), max(bits_all, _log2(sa))
        # the pair form reproduces the operands (nothing was rounded away), and every product is a whole multiple of u
        x = torch.cat([x1[n:n + 1]] + ([x2[n:n + 1]] if x2 is not None else []), 1)
        unit_ok &= bool(torch.equal(torch.cat([h + l for h, l in zip(his, los)], 1), x)) and bool(torch.equal(wh + wl, w))
        cin_units = _product_unit(x[0], w)
        unit_ok &= cin_units >= units[n] and _is_multiple(b, u)
    return dict(lolo=lolo, unit_ok=unit_ok, bits_m=bits_m, bits_x=bits_x, bits_all=bits_all)


def _log2(v):
    v = float(v)
    return math.log2(v) if v > 0 else -1e9


def _is_multiple(t, u):
    q = t.double() / u
    return bool(torch.equal(q, q.round()))


def _unit_exp(t):
    """log2 of the largest power of two that divides every value of t (1e9 for an all-zero tensor)"""
    t = t[t != 0]
    if t.numel() == 0:
        return 10 ** 9
    m, e = torch.frexp(t.double().abs())            # t = m 2^e, m in [0.5, 1) with at most 53 bits
    mi = (m * 2.0 ** 53).long()
    tz = ((mi & -mi).double().log2()).long()        # trailing zeros of the 53-bit significand
    return int((e.long() - 53 + tz).min())


def _product_unit(x, w):
    """min over input channels of unit(x[ci]) + unit(w[:, ci]): log2 of a power of two that divides every product"""
    return min(_unit_exp(x[ci]) + _unit_exp(w[:, ci]) for ci in range(x.shape[0]) if bool((x[ci] != 0).any()) and bool((w[:, ci] != 0).any()))


def bias_add_rounds_once(y_nobias, b):
    """True where adding the bias to the exact fp32 value y rounds at most once to float32(y + b in fp64): either the fp64 sum is exact, or |y| lies
    below a quarter ulp of the bias (every correctly rounded path then returns the bias)"""
    bb = b.double().view(1, -1, *([1] * (y_nobias.dim() - 2))).expand_as(y_nobias)
    s = y_nobias + bb
    exact = (s - bb) == y_nobias
    tiny = y_nobias.abs() < bb.abs() * 2.0 ** -26
    return bool((exact | tiny).all())


# ---------------------------------------------------------------------------------------------------------------- real-valued operands
def real_operands(c, seed=0, cancelling=False):
    """random fp32-valued operands (fp64 tensors): N(0, 1) activations and 1/sqrt(K) weights, or -- cancelling -- activations 1 + 1e-3 noise and
    filters with zero mean, the construction of tests/test_kernels_gpu.py::test_conv_f16x2_cancelling_sums.  Any rank: a case with `dhw` is a
    volume, one with `H` and `W` (tests/conv2d_cases.py) an image"""
    g = torch.Generator().manual_seed(_seed_of(c.name, "real", seed, cancelling))
    cin = c.C1 + c.C2
    extents = tuple(c.dhw) if hasattr(c, "dhw") else (c.H, c.W)
    rank = len(extents)
    x = torch.randn((c.N, cin, *extents), generator=g, dtype=torch.float64)
    w = torch.randn((c.Cout, cin, *((c.k,) * rank)), generator=g, dtype=torch.float64) / math.sqrt(cin * c.k ** rank)
    b = torch.randn((c.Cout,), generator=g, dtype=torch.float64) * 0.1
    if cancelling:
        x = 1.0 + 1e-3 * x
        w = w - w.mean(dim=tuple(range(1, rank + 2)), keepdim=True)
    x, w, b = x.float().double(), w.float().double(), b.float().double()
    return x[:, :c.C1].contiguous(), (x[:, c.C1:].contiguous() if c.C2 else None), w, b


CANCEL_CASES = [case("cancel_c96", 2, (4, 5, 6), 96, 0, 64, 3), case("cancel_c64+32", 2, (4, 5, 6), 64, 32, 64, 3)]   # 81 chunks: within the 96 the bound is derived for
TILE_BITS_CASES = [case("tiles_c64k3", 2, (5, 7, 9), 64, 0, 129, 3), case("tiles_c32+32k3", 3, (3, 4, 5), 32, 32, 67, 3),
                   case("tiles_k1s2", 2, (4, 6, 8), 64, 0, 65, 1, (2, 2, 2))]
COVARIANCE_CASES = [(case("cov_c32", 3, (3, 4, 5), 32, 0, 48, 3), 0), (case("cov_c32+64", 3, (3, 4, 5), 32, 64, 48, 3), 0),
                    (case("cov_c32+64_sk4", 3, (3, 4, 5), 32, 64, 48, 3), 4)]   # (sk = 4: slice [21, 42) straddles the switch at 27)
# a zero (or tiny) source next to a large one: (case, split-K hints): sk = 1 and a plan with a straddling slice
ZERO_SOURCE_CASE = case("zero_c32+32", 3, (3, 4, 5), 32, 32, 48, 3)
ZERO_SOURCE_SKS = (1, 4)   # sk = 4: per = 14, slice [14, 28) straddles the switch at 27
# the largest ratio of the two sources' scale exponents the rescale at the switch is derived for: e1 - e2 <= 80
RATIO_INSIDE = 80
