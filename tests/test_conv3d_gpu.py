"""The 3-D fp16-pair convolution (csrc/conv3d.hip) held to exact and fp64 references at its edges, on a real MI355X.  tests/conv3d_cases.py has the
references, the operands on which the pair arithmetic is exact and the case lists; tests/test_conv3d_cpu.py proves their premises without a GPU.
Every test prints `[digest] <name> <sha256 of its outputs>`: two builds computed the same bits when the lines agree
(profiles/conv3d_parity_measured.txt)."""

import hashlib

import pytest
import torch
import torch.nn.functional as F

from medfusion_amd import kernels as K
from tests import conv3d_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Digest:
    def __init__(self, name):
        self.name, self.h = name, hashlib.sha256()

    def add(self, y):
        self.h.update(y.detach().cpu().contiguous().numpy().tobytes())
        return y

    def done(self):
        print(f"[digest] {self.name} {self.h.hexdigest()[:24]}")


def _ndhwc(x, dev):
    return None if x is None else x.float().to(dev).permute(0, 2, 3, 4, 1).contiguous()


def _operands(x1, x2, w, b, dev):
    """the device operands of fp64 NCDHW / OIDHW tensors: (x1, x2 or None) NDHWC fp32, the split packed weights, the bias"""
    return (_ndhwc(x1, dev), _ndhwc(x2, dev), K.split_weight_f16x2(K.pack_conv3d_weight(w.float().to(dev))), None if b is None else b.float().to(dev))


def _desc(c, tile=0, sk=0):
    return K.make_conv3d_desc(c.N, *c.dhw, c.C1, c.C2, c.Cout, c.k, c.stride, c.pad, c.up, tile_hint=tile, splitk_hint=sk)


def _run(ops, c, tile=0, sk=0):
    a1, a2, wh, b = ops
    d = _desc(c, tile, sk)
    assert K.conv3d_ok(d), (c, tile, sk)
    if tile and sk:
        assert K.conv3d_plan(d) == (tile, min(sk, CC.slices(c, sk)[0])), (c, tile, sk)
    return K.conv3d_f16x2(a1, wh, b, d, x2=a2)


def _want32(x1, x2, w, b, c):
    """float32(ref64) in the kernel's layout"""
    return CC.ref64(x1, x2, w, b, c.stride, c.pad, c.up).permute(0, 2, 3, 4, 1).contiguous().float()


def _plans(c):
    """(tile hint, split-K hint): every tile unsplit and the planner's own plan; a single source adds two split plans, two sources every split-K
    factor that gives another plan (tests/test_conv3d_cpu.py: among them slices that start at, end at and straddle the source switch) on every tile"""
    plans = [(0, 0)] + [(t, 1) for t in CC.TILES]
    if c.C2 == 0:
        return plans + [(1, 4), (4, 16)]
    return plans + [(t, sk) for sk in CC.distinct_sks(c) if sk > 1 for t in CC.TILES]


def _first_diff(y, want):
    bad = (y != want) & ~(y.isnan() & want.isnan())
    i = bad.nonzero()[0].tolist()
    return f"{int(bad.sum())} of {y.numel()} differ, first at {i}: got {y[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}"


# ------------------------------------------------------------------------------------------------ (a) exact, everywhere
@pytest.mark.parametrize("c", CC.GEOM_CASES + CC.M_EDGE_CASES + CC.COUT_EDGE_CASES + CC.TWO_SOURCE_CASES, ids=lambda c: c.name)
def test_exact_operands_give_float32_of_ref64_bit_for_bit(dev, c):
    dg = Digest(f"exact/{c.name}")
    for family, ratio in CC.variants(c):
        x1, x2, w, b, _ = CC.exact_operands(c, family, ratio)
        want = _want32(x1, x2, w, b, c).to(dev)
        ops = _operands(x1, x2, w, b, dev)
        for tile, sk in _plans(c):
            y = _run(ops, c, tile, sk)
            assert y.shape == want.shape
            assert torch.equal(y, want), (c.name, family, ratio, tile, sk, CC.slice_kinds(c, max(sk, 1)), _first_diff(y, want))
        dg.add(y)
    dg.done()


def test_the_split_k_reducer_takes_a_second_trip(dev):
    """M Cout = 8448 x 256 elements: past the 8192 x 256 the reducer's grid stops at, so its grid-stride loop runs twice for the first 256 x 256"""
    c = CC.REDUCER_CASE
    dg = Digest("exact/reducer")
    for family, ratio in CC.variants(c):
        x1, x2, w, b, _ = CC.exact_operands(c, family, ratio)
        want = _want32(x1, x2, w, b, c).to(dev)
        ops = _operands(x1, x2, w, b, dev)
        for tile, sk in ((0, 2), (1, 2), (4, 2), (4, 1)):
            y = _run(ops, c, tile, sk)
            assert torch.equal(y, want), (family, tile, sk, _first_diff(y, want))
        dg.add(y)
    dg.done()


@pytest.mark.parametrize("p", [CC.PACK_CASE, CC.PACK_SQUARE_CASE], ids=["second_trip", "cin_eq_taps"])
def test_the_weight_pack_is_permute_plus_zero_pad(dev, p):
    g = torch.Generator().manual_seed(7)
    w = torch.randn((p["Cout"], p["Cin"], p["k"], p["k"], p["k"]), generator=g)
    want = torch.zeros((p["Cout"], p["k"], p["k"], p["k"], p["cin_pad"]))
    want[..., :p["Cin"]] = w.permute(0, 2, 3, 4, 1)
    got = K.pack_conv3d_weight(w.to(dev), p["cin_pad"])
    assert got.shape == want.shape and torch.equal(got.cpu(), want)
    dg = Digest(f"pack/{p['Cout']}x{p['Cin']}")
    dg.add(got)
    dg.done()


# ------------------------------------------------------------------------------------------------ (b) the tile does not change the bits
@pytest.mark.parametrize("c", CC.TILE_BITS_CASES, ids=lambda c: c.name)
def test_the_tile_does_not_change_the_bits(dev, c):
    """unsplit, all four tiles walk the same (chunk, tap) iterations and feed every output's accumulators the same 16-channel steps in the same
    order: the outputs are equal bit for bit, on real-valued data as on exact data"""
    dg = Digest(f"tiles/{c.name}")
    sets = [CC.real_operands(c)] + [CC.exact_operands(c, f, r)[:4] for f, r in CC.variants(c)[:1]]
    for x1, x2, w, b in sets:
        ops = _operands(x1, x2, w, b, dev)
        ys = [_run(ops, c, t, 1) for t in CC.TILES]
        for t, y in zip(CC.TILES[1:], ys[1:]):
            assert torch.equal(y, ys[0]), (c.name, t, _first_diff(y, ys[0]))
        dg.add(ys[0])
    dg.done()


# ------------------------------------------------------------------------------------------------ (c) power-of-two covariance
@pytest.mark.parametrize("c,sk", CC.COVARIANCE_CASES, ids=lambda v: v.name if isinstance(v, CC.Case) else f"sk{v}")
def test_scaling_a_sample_by_a_power_of_two_scales_its_output_exactly(dev, c, sk):
    x1, x2, w, _ = CC.real_operands(c)
    a1, a2, wh, _ = _operands(x1, x2, w, None, dev)
    sc = torch.tensor([2.0 ** 40 if n % 2 == 0 else 2.0 ** -40 for n in range(c.N)], device=dev).view(-1, 1, 1, 1, 1)
    dg = Digest(f"covariance/{c.name}")
    for tile in (0, 1, 4):
        y = _run((a1, a2, wh, None), c, tile, sk)
        ys = _run((a1 * sc, None if a2 is None else a2 * sc, wh, None), c, tile, sk)
        assert bool(y.isfinite().all()) and float(y.abs().max()) > 0
        assert torch.equal(ys, y * sc), (c.name, tile, sk, _first_diff(ys, y * sc))
        dg.add(y)
        dg.add(ys)
    dg.done()


# ------------------------------------------------------------------------------------------------ (d) element-wise bound on cancelling sums
def _bound_ratio(y, y64, sabs):
    """max over the elements of |y - y64| / sum |w||x|, as a multiple of 2^-22"""
    return float(((y.double().cpu().permute(0, 4, 1, 2, 3) - y64).abs() / sabs).max()) * 2.0 ** 22


@pytest.mark.parametrize("c", CC.CANCEL_CASES, ids=lambda c: c.name)
def test_cancelling_sums_stay_within_the_formats_bound_element_by_element(dev, c):
    """activations 1 + 1e-3 noise, zero-mean filters: |y| << sum |w||x|, and |y - y64| <= 2^-21 sum |w||x| for EVERY element -- 2^-23 per operand
    plus the dropped lo.lo term below 2^-22; 81 chunks, within the 96 the fp32 accumulation of the matrix cores is derived to stay below it for.
    Measured (MI355X): see profiles/conv3d_parity_measured.txt."""
    x1, x2, w, _ = CC.real_operands(c, cancelling=True)
    y64 = CC.ref64(x1, x2, w, None, c.stride, c.pad, c.up)
    sabs = CC.sabs64(x1, x2, w, c.stride, c.pad, c.up)
    inner = (slice(None), slice(None), slice(1, -1), slice(1, -1), slice(1, -1))
    cancel = float((y64[inner].abs() / sabs[inner]).median())
    assert cancel < 5e-3, cancel                  # the sums really cancel away from the padded border
    ops = _operands(x1, x2, w, None, dev)
    dg = Digest(f"cancel/{c.name}")
    worst = 0.0
    for tile, sk in [(0, 0)] + [(t, 1) for t in CC.TILES] + [(0, 4)]:
        y = dg.add(_run(ops, c, tile, sk))
        r = _bound_ratio(y, y64, sabs)
        print(f"[measured] {c.name} tile {tile} sk {sk}: max |y - y64| / sum|w||x| = {r:.3f} x 2^-22 (median |y| / sum|w||x| = {cancel:.1e})")
        worst = max(worst, r)
        assert r <= 2.0, (c.name, tile, sk, r)
    dg.done()
    print(f"[measured] {c.name}: worst {worst:.3f} x 2^-22 (bound 2.0)")


# ------------------------------------------------------------------------------------------------ (e) non-finite operands
@pytest.mark.parametrize("c", [CC.GEOM_CASES[1], CC.TWO_SOURCE_CASES[3]], ids=lambda c: c.name)
def test_a_non_finite_voxel_reaches_exactly_the_outputs_that_read_it(dev, c):
    """one NaN, one +Inf and one -Inf voxel, one per sample, in otherwise exact data: the non-finite mask of y is that of ref64, and every other
    element keeps the bits of the clean run -- the sample's measured bound is the largest FINITE magnitude, so its scale does not move"""
    family, ratio = CC.variants(c)[0]
    x1, x2, w, b, _ = CC.exact_operands(c, family, ratio)
    clean = _run(_operands(x1, x2, w, b, dev), c)
    assert torch.equal(clean, _want32(x1, x2, w, b, c).to(dev))
    dg = Digest(f"nonfinite/{c.name}")
    d, h, wd = c.dhw
    for which in ((1, 2) if x2 is not None else (1,)):
        xs = [x1.clone(), None if x2 is None else x2.clone()]
        t = xs[which - 1]
        for n, v in enumerate((float("nan"), float("inf"), float("-inf"))):
            t[n, 5 + n, d // 2, (h // 2 + n) % h, (wd - 1 - n) % wd] = v
        want = _want32(xs[0], xs[1], w, b, c).to(dev)
        assert 0 < int((~want.isfinite()).sum()) < want.numel() // 2
        for tile, sk in ((0, 0), (1, 1), (4, 1), (2, 4)):
            y = dg.add(_run(_operands(xs[0], xs[1], w, b, dev), c, tile, sk))
            assert torch.equal(y.isfinite(), want.isfinite()), (c.name, which, tile, sk, int((y.isfinite() != want.isfinite()).sum()))
            keep = want.isfinite()
            assert torch.equal(y[keep], clean[keep]), (c.name, which, tile, sk, int((y[keep] != clean[keep]).sum()))
    dg.done()


# ------------------------------------------------------------------------------------------------ (f) a zero or tiny source next to a large one
def _zero_source_sets(seed_case):
    """three samples: x1 x 1e6 with x2 all zero; x1 all zero with x2 x 1e6; an ordinary one"""
    x1, x2, w, b = CC.real_operands(seed_case, seed=3)
    x1, x2 = x1.clone(), x2.clone()
    x1[0] *= 1e6
    x2[0] = 0.0
    x1[1] = 0.0
    x2[1] *= 1e6
    return x1.float().double(), x2.float().double(), w, b


def test_a_zero_source_next_to_a_large_one_3d(dev):
    """The accumulators are rescaled by 2^(e1 - e2) where the K loop meets the second source.  An all-zero source sample has the measured bound 0,
    whose exponent is the clamp -100: next to a sample of 1e6 the factor was 2^107 and the first source's partial sums left fp32's range.  A zero
    bound says nothing (zeros are stored as zeros under any scale), so such a source takes the other source's exponent and the factor is 1."""
    c = CC.ZERO_SOURCE_CASE
    x1, x2, w, b = _zero_source_sets(c)
    y64 = CC.ref64(x1, x2, w, b, c.stride, c.pad, c.up)
    sabs = CC.sabs64(x1, x2, w, c.stride, c.pad, c.up) + b.abs().view(1, -1, 1, 1, 1)
    ops = _operands(x1, x2, w, b, dev)
    dg = Digest("zero_source/3d")
    for sk in CC.ZERO_SOURCE_SKS:
        for tile in (0, 1, 4):
            y = dg.add(_run(ops, c, tile, sk))
            assert bool(y.isfinite().all()), (tile, sk, int((~y.isfinite()).sum()))
            r = _bound_ratio(y, y64, sabs)
            assert r <= 2.0, (tile, sk, r)
    # exact data: the same three samples on integers
    x1e, x2e, we, be, _ = CC.exact_operands(c, "xlo", "mixed")
    x1e[0], x2e[0], x1e[1], x2e[1] = x1e[0] * 2.0 ** 20, 0.0, 0.0, x2e[1] * 2.0 ** 20
    want = _want32(x1e, x2e, we, None, c).to(dev)
    assert torch.equal(want.double(), CC.ref64(x1e, x2e, we, None, c.stride, c.pad, c.up).permute(0, 2, 3, 4, 1).to(dev))
    opse = _operands(x1e, x2e, we, None, dev)
    for sk in CC.ZERO_SOURCE_SKS:
        for tile in CC.TILES:
            y = dg.add(_run(opse, c, tile, sk))
            assert torch.equal(y, want), (tile, sk, _first_diff(y, want))
    dg.done()


def test_two_sources_whose_scales_differ_by_2_to_the_80(dev):
    """just inside the ratio the rescale at the switch is derived for: e1 - e2 = 80, and the mirror"""
    c = CC.ZERO_SOURCE_CASE
    x1, x2, w, _ = CC.real_operands(c, seed=4)
    h = CC.RATIO_INSIDE // 2
    s1 = torch.tensor([2.0 ** h, 2.0 ** -h, 1.0]).view(-1, 1, 1, 1, 1).double()
    x1, x2 = x1 * s1, x2 / s1
    y64 = CC.ref64(x1, x2, w, None, c.stride, c.pad, c.up)
    sabs = CC.sabs64(x1, x2, w, c.stride, c.pad, c.up)
    ops = _operands(x1, x2, w, None, dev)
    e = [(CC.scale_exp(float(x1[n].abs().max())), CC.scale_exp(float(x2[n].abs().max()))) for n in range(3)]
    assert e[0][0] - e[0][1] == CC.RATIO_INSIDE and e[1][1] - e[1][0] == CC.RATIO_INSIDE, e
    dg = Digest("zero_source/ratio80")
    for sk in CC.ZERO_SOURCE_SKS:
        for tile in (0, 1, 4):
            y = dg.add(_run(ops, c, tile, sk))
            assert bool(y.isfinite().all())
            r = _bound_ratio(y, y64, sabs)
            assert r <= 2.0, (tile, sk, r)
    dg.done()


@pytest.mark.parametrize("tile", [52, 63], ids=["plain_body", "halo_body"])
def test_a_zero_source_next_to_a_large_one_2d(dev, tile):
    """the 2-D pair kernel has the same rescale (conv_f16x2_body.inc, conv_f16x2_halo_body.inc): three 8 x 8 images of 96 + 32 channels, unsplit and
    split in two (4 chunk groups of 32 channels: the second slice holds the last of the first source and the second source, so it straddles the switch)"""
    from tests.test_kernels_gpu import F16X2_TILES, _halo_fits
    n, hh, ww, c1, c2, co, k = 3, 8, 8, 96, 32, 256, 3
    assert _halo_fits((n, hh, ww, c1, c2, co, k, 1, 0), tile) and co % F16X2_TILES[tile][1] == 0
    c = CC.case("zero2d", n, (1, hh, ww), c1, c2, co, 3)
    x1, x2, w, b = _zero_source_sets(c)
    x1, x2, w2 = x1[:, :, 0], x2[:, :, 0], w[:, :, 1]
    y64 = F.conv2d(torch.cat([x1, x2], 1), w2, b, padding=1)
    sabs = F.conv2d(torch.cat([x1, x2], 1).abs(), w2.abs(), None, padding=1) + b.abs().view(1, -1, 1, 1)
    xd, x2d = K.nchw_to_nhwc(x1.float().to(dev)), K.nchw_to_nhwc(x2.float().to(dev))
    wh = K.split_weight_f16x2(K.pack_conv_weight(w2.float().to(dev)))
    dg = Digest(f"zero_source/2d_tile{tile}")
    for sk in (1, 2):
        d = K.make_conv_desc(n, hh, ww, c1, c2, co, k, 1, 1, 0, tile_hint=tile, splitk_hint=sk, precision=5)
        assert K.conv_f16x2_ok(d) and K.conv_plan(d)[0] == tile
        y = dg.add(K.conv2d_f16x2(xd, wh, b.float().to(dev), d, x2=x2d))
        assert bool(y.isfinite().all()), (tile, sk, int((~y.isfinite()).sum()))
        r = float(((K.nhwc_to_nchw(y).double().cpu() - y64).abs() / sabs).max()) * 2.0 ** 22
        assert r <= 2.0, (tile, sk, r)
    dg.done()
