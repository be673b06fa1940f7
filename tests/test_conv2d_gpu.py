"""The 2-D convolutions (csrc/conv_f16x2.hip with its plain and halo bodies, the group launch, csrc/conv.hip with its implicit-GEMM tiles and the
direct, small-Cin and out-1x1 kernels) held to exact and element-wise fp64 references at their edges, on a real MI355X.  tests/conv2d_cases.py has
the references, the exact operand families, the restated host rules and the case lists; tests/test_conv2d_cpu.py proves their premises without a
GPU.  Every test prints `[digest] <name> <sha256 of its outputs>` and `[combos] <name> <count>`: two builds computed the same bits when the digest
lines agree (profiles/conv2d_parity_measured.txt).

  A  exact operands give float32(ref64) bit for bit on every tile the restated rule admits and every distinct split-K -- and what the rule
     refuses the library refuses;
  B  the side outputs at the same edges: the measured bound, the pairs-out epilogue, the GroupNorm records (per sample), the group launch;
  C  an element-wise bound on real and on cancelling operands, B taken from the code;
  D  power-of-two covariance, a zero source next to a large one, and the tile does not change the bits;
  E  a non-finite pixel reaches exactly the outputs whose window reads it;
  F  nothing is written past the output."""

import pytest
import torch

from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from tests import conv2d_cases as CC
from tests.test_conv3d_gpu import Digest

pytestmark = pytest.mark.gpu
LAYOUT = {"nchw": L.LAYOUT_NCHW, "nhwc": L.LAYOUT_NHWC}
PAIR_BOUND = 2.0 ** -21      # |y - y64| <= 2^-21 sum |w||x|: tests/test_kernels_gpu.py::test_conv_f16x2_cancelling_sums derives it for chains <= 96 chunks


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _nhwc(x, dev):
    return None if x is None else x.float().permute(0, 2, 3, 1).contiguous().to(dev)


def _desc(c, tile=0, sk=0, precision=5, lin="nhwc", lout="nhwc"):
    return K.make_conv_desc(c.N, c.H, c.W, c.C1, c.C2, c.Cout, c.k, c.stride, c.pad, c.ups, LAYOUT[lin], LAYOUT[lout], tile_hint=tile, splitk_hint=sk,
                            precision=precision)


class Ops:
    """the device operands of fp64 NCHW / OIHW tensors: NHWC fp32 sources, the packed weights (the sub-pixel packing where upsampled) in every
    form a precision takes, the bias"""

    def __init__(self, c, x1, x2, w, b, dev):
        self.c, self.a1, self.a2 = c, _nhwc(x1, dev), _nhwc(x2, dev)
        self.b = None if b is None else b.float().to(dev)
        wd = w.float().to(dev)
        self.wp = K.pack_upconv_weight(wd) if c.ups == 2 else K.pack_conv_weight(wd)
        self._forms = {}

    def weights(self, precision):
        if precision not in self._forms:
            make = {0: lambda: self.wp, 3: lambda: K.split_conv_weight(self.wp), 4: lambda: K.convert_conv_weight_bf16(self.wp)}
            self._forms[precision] = make.get(precision, lambda: K.split_weight_f16x2(self.wp))()
        return self._forms[precision]

    def l1(self):
        """(largest filter L1 norm over the channels of x1, ... of x2) and max |bias|, as conv2d_f16x2_pairs_out takes them"""
        c1 = self.c.C1
        l2 = float(self.wp[..., c1:].abs().sum(dim=(-3, -2, -1)).max()) * (1 + 1e-5) if self.c.C2 else 0.0
        return (float(self.wp[..., :c1].abs().sum(dim=(-3, -2, -1)).max()) * (1 + 1e-5), l2), (0.0 if self.b is None else float(self.b.abs().max()))


def _pair(ops, tile=0, sk=0, precision=5, bias=True, **kw):
    c = ops.c
    d = _desc(c, tile, sk, precision)
    assert K.conv_f16x2_ok(d), (c, tile, sk)
    if tile and sk:
        assert K.conv_plan(d) == (tile, CC.slices(c, sk)[3]), (c, tile, sk)
    return K.conv2d_f16x2(ops.a1, ops.weights(precision), ops.b if bias else None, d, x2=ops.a2, **kw)


def _want(x1, x2, w, b, c, dev):
    """float32(ref64) in the kernel's layout"""
    return CC.want32(x1, x2, w, b, c).permute(0, 2, 3, 1).contiguous().to(dev)


def _first_diff(y, want):
    bad = (y != want) & ~(y.isnan() & want.isnan())
    i = bad.nonzero()[0].tolist()
    return f"{int(bad.sum())} of {y.numel()} differ, first at (n, oy, ox, co) = {tuple(i)}: got {y[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}"


def _pair_plans(c):
    """(tile hint, split-K hint) of a case on the pair path: the planner's own plan, then every tile x every distinct split.  Asserts on the way that
    the library refuses exactly the tiles the restated rule refuses: no combination is skipped silently."""
    plans = [(0, 0)]
    for prec in (5, 6):
        assert K.conv_f16x2_ok(_desc(c, precision=prec)) == CC.f16x2_ok(c) is True, c
    for t in CC.F16X2_TILES:
        ok = CC.f16x2_ok(c, t)
        assert K.conv_f16x2_ok(_desc(c, t)) == ok, (c, t)
        if ok:
            plans += [(t, sk) for sk in CC.distinct_sks(c)]
    if c.ups == 2:
        assert K.subpixel_ok(_desc(c, precision=0)) == CC.subpixel_ok(c)
    return plans


# ------------------------------------------------------------------------------------------------ A. exact, everywhere
@pytest.mark.parametrize("c", CC.EXACT_F16X2_CASES, ids=lambda c: c.name)
def test_exact_operands_give_float32_of_ref64_on_the_pair_path(dev, c):
    """precision 5 on every family, precision 6 (one fp16 term) on the integers"""
    dg, n = Digest(f"exact_pair/{c.name}"), 0
    plans = _pair_plans(c)
    for family, ratio in CC.variants(c):
        x1, x2, w, b, _ = CC.exact_operands(c, family, ratio)
        want = _want(x1, x2, w, b, c, dev)
        ops = Ops(c, x1, x2, w, b, dev)
        for prec in ((5, 6) if family == "int8" else (5,)):
            for tile, sk in plans:
                y = _pair(ops, tile, sk, prec)
                assert y.shape == want.shape
                assert torch.equal(y, want), (c.name, family, ratio, prec, tile, sk, CC.slice_kinds(c, max(sk, 1)), _first_diff(y, want))
                n += 1
            dg.add(y)
    dg.done()
    print(f"[combos] exact_pair/{c.name} {len(plans)} (case, tile, sk) x {len(CC.variants(c))} families (+ precision 6 on int8) = {n} launches")


def test_the_split_k_reducer_takes_a_second_trip(dev):
    """16 samples of 16 x 33 x 256 outputs: past the 128 blocks x 256 threads of float4s the reducer's grid stops at, so its grid-stride loop runs
    twice for the first 1024 float4s of every sample (tests/test_conv2d_cpu.py derives the size); with and without the bound it measures"""
    c, sk = CC.REDUCER_CASE, CC.REDUCER_SK
    assert not CC.f16x2_ok(c, 0, sk) and not K.conv_f16x2_ok(_desc(c, 0, sk))   # (the cost model only splits by powers of two: hint 0 refuses a 3)
    dg = Digest("exact_pair/reducer")
    for family, ratio in CC.variants(c):
        x1, x2, w, b, _ = CC.exact_operands(c, family, ratio)
        want = _want(x1, x2, w, b, c, dev)
        ops = Ops(c, x1, x2, w, b, dev)
        for tile in (36, 33, 37, 32):
            y = _pair(ops, tile, sk)
            assert K.conv_plan(_desc(c, tile, sk))[1] == 3 and torch.equal(y, want), (family, tile, _first_diff(y, want))
            ym = _pair(ops, tile, sk, measure_out=True)
            assert torch.equal(ym, want) and torch.equal(K.bound_of(ym), want.abs().amax(dim=(1, 2, 3))), (family, tile)
        dg.add(y)
    dg.done()


@pytest.mark.parametrize("c", CC.EXACT_IGEMM_CASES, ids=lambda c: c.name)
def test_exact_operands_give_float32_of_ref64_on_the_implicit_gemm(dev, c):
    """precision 0 (fp32 matrix cores) and 3 (bf16 triplets: the CPU test shows the dropped products are zero on every family) on every family,
    precision 4 (one bf16 term) on the integers; every tile the restated rule admits x split-K 1, 2, 3, plus the planner's own plan"""
    dg, n = Digest(f"exact_igemm/{c.name}"), 0
    assert K.conv_is_igemm(_desc(c, precision=0)) == CC.igemm_ok(c) is True
    for family, ratio in CC.variants(c):
        x1, x2, w, b, _ = CC.exact_operands(c, family, ratio)
        want = _want(x1, x2, w, b, c, dev)
        ops = Ops(c, x1, x2, w, b, dev)
        for prec in ((0, 3, 4) if family == "int8" else (0, 3)):
            for tile, sk in [(0, 0)] + [(t, s) for t in CC.igemm_tiles(c, prec) for s in (1, 2, 3)]:
                d = _desc(c, tile, sk, prec)
                if tile:
                    assert K.conv_plan(d) == (tile, CC.igemm_slices(c, tile, sk)[2]), (c.name, prec, tile, sk)
                y = K.conv2d(ops.a1, ops.weights(prec), ops.b, d, x2=ops.a2)
                assert torch.equal(y, want), (c.name, family, ratio, prec, tile, sk, _first_diff(y, want))
                n += 1
            dg.add(y)
    dg.done()
    print(f"[combos] exact_igemm/{c.name} {n} launches")


@pytest.mark.parametrize("dc", CC.DIRECT_CASES, ids=lambda d: d.c.name)
def test_exact_integers_through_the_direct_kernels_in_each_layout(dev, dc):
    """the generic direct kernel, the small-Cin kernel (one and two sources) and the out-1x1 kernel: fp32 fma chains, exact on the integers"""
    c = dc.c
    x1, x2, w, b, _ = CC.exact_operands(c, "int8", None if c.C2 == 0 else "mixed")
    want = CC.want32(x1, x2, w, b, c)
    d = _desc(c, precision=0, lin=dc.lin, lout=dc.lout)
    assert not K.conv_is_igemm(d)
    a1 = x1.float().to(dev) if dc.lin == "nchw" else _nhwc(x1, dev)
    y = K.conv2d(a1, K.pack_conv_weight(w.float().to(dev)), b.float().to(dev), d, x2=_nhwc(x2, dev))
    y = y if dc.lout == "nchw" else y.permute(0, 3, 1, 2)
    assert y.shape == want.shape
    assert torch.equal(y.cpu(), want), (c.name, _first_diff(y.cpu().permute(0, 2, 3, 1), want.permute(0, 2, 3, 1)))
    dg = Digest(f"exact_direct/{c.name}")
    dg.add(y.contiguous())
    dg.done()


# ------------------------------------------------------------------------------------------------ B. side outputs at the same edges
SIDE_CASES = CC.GEOM_CASES + CC.M_EDGE_CASES + CC.COUT_EDGE_CASES + CC.TWO_SOURCE_CASES + CC.HALO_CASES + CC.SUBPIXEL_CASES


@pytest.mark.parametrize("c", SIDE_CASES, ids=lambda c: c.name)
def test_the_side_outputs_at_the_same_edges(dev, c):
    """on the first exact family of the case, every plan, against the plain launch of the same plan (whether THAT is right is test A's business):
    measure_out returns the same y and gives bound_of(y) == max |y| per sample bit for bit (measured by the epilogue's
    slots where a tile tells samples apart, by the reducer behind a slab split, by a stand-alone pass otherwise); the pairs-out epilogue returns the
    same y and pairs that decode within 2^-23 |y| + 2^-50 bound (the claim of test_split_f16x2_format); the GroupNorm records (8 groups, no bias, so
    that the three samples keep their three scales) equal fp64 sums of the returned y within the tolerance test_conv_f16x2 uses, PER SAMPLE"""
    from tests.test_kernels_gpu import _decode_pairs
    family, ratio = CC.variants(c)[0]
    x1, x2, w, b, _ = CC.exact_operands(c, family, ratio)
    ops = Ops(c, x1, x2, w, b, dev)
    l1, bmax = ops.l1()
    G = 8
    dg, seen = Digest(f"side/{c.name}"), dict(slots=0, pairs=0, gn=0, plans=0)
    for tile, sk in _pair_plans(c):
        d = _desc(c, tile, sk)
        want = _pair(ops, tile, sk)
        amax = want.abs().amax(dim=(1, 2, 3))
        y = _pair(ops, tile, sk, measure_out=True)
        assert torch.equal(y, want), (c.name, tile, sk, _first_diff(y, want))
        seen["plans"] += 1
        seen["slots"] += int(getattr(y, "_mf_slots", None) is not None)
        assert torch.equal(K.bound_of(y), amax), (c.name, tile, sk, K.bound_of(y).tolist(), amax.tolist())
        if K.conv_pairs_out_ok(d):
            seen["pairs"] += 1
            got = K.conv2d_f16x2_pairs_out(ops.a1, ops.weights(5), ops.b, d, l1, bmax, x2=ops.a2)
            assert torch.equal(got, want), (c.name, tile, sk, _first_diff(got, want))
            bound = got._mf_bound.double().cpu()
            assert bool((bound >= amax.double().cpu()).all())
            scale = torch.tensor([2.0 ** CC.scale_exp(float(v)) for v in got._mf_bound.cpu()], dtype=torch.float64).view(-1, 1, 1, 1)
            err = (_decode_pairs(got._mf_split, tuple(want.shape)) * scale - want.double().cpu()).abs()
            tol = want.double().cpu().abs() * 2.0 ** -23 + (bound * 2.0 ** -50).view(-1, 1, 1, 1)
            assert bool((err <= tol).all()), (c.name, tile, sk, float((err / tol).max()))
            dg.add(got._mf_split)
        parts = K.conv_gn_parts(d, G)
        if parts:
            seen["gn"] += 1
            want0 = _pair(ops, tile, sk, bias=False)
            y2, partial = _pair(ops, tile, sk, bias=False, gn_groups=G, gn_parts=parts)
            assert torch.equal(y2, want0), (c.name, tile, sk, _first_diff(y2, want0))
            cnt = y2.shape[1] * y2.shape[2] * (c.Cout // G)
            yg = y2.double().cpu().reshape(c.N, -1, G, c.Cout // G)
            mean, msq = yg.sum(dim=(1, 3)) / cnt, (yg * yg).sum(dim=(1, 3)) / cnt
            got = partial.sum(1).cpu() / cnt
            for n in range(c.N):
                assert torch.allclose(got[n, :, 1], msq[n], rtol=1e-5, atol=0), (c.name, tile, sk, n)
                assert torch.allclose(got[n, :, 0], mean[n], rtol=0, atol=1e-5 * float(msq[n].max().sqrt())), (c.name, tile, sk, n)
            dg.add(partial)
    dg.done()
    print(f"[combos] side/{c.name} {seen}")
    assert seen["pairs"] > 0                                     # (every unsplit plan writes its pairs itself)


@pytest.mark.parametrize("g", CC.GROUP_SMALL, ids=lambda g: f"{g[0].name}_{g[1]}+{g[2]}")
def test_two_convolutions_in_one_launch_equal_the_single_launches(dev, g):
    """one 3x3 + 1x1 pair per entry of dispatch_group: outputs, GroupNorm records and bound slots bit-equal to the two launches, on samples of
    three scales; the 3x3 is also run split in two (in-launch tree) where its channel groups allow"""
    c, ta, tb = g
    c1x1 = c._replace(k=1, pad=0)
    G = 8
    x1, x2, w3, b3 = CC.scaled_real_operands(c)
    _, _, w1, b1 = CC.scaled_real_operands(c1x1, seed=1)
    a1, a2 = _nhwc(x1, dev), _nhwc(x2, dev)
    wh3, wh1 = K.split_weight_f16x2(K.pack_conv_weight(w3.float().to(dev))), K.split_weight_f16x2(K.pack_conv_weight(w1.float().to(dev)))
    b3, b1 = b3.float().to(dev), b1.float().to(dev)
    dg = Digest(f"group/{c.name}")
    for ska in (1, 2):
        if ska > (c.C1 + c.C2) // 32:
            continue
        da, db = _desc(c, ta, ska), _desc(c1x1, tb, 1)
        assert K.conv_f16x2_ok(da) and K.conv_f16x2_ok(db)
        pa, pb = K.pin_conv_plan(da), K.pin_conv_plan(db)
        parts = K.conv_gn_parts(da, G)
        assert parts > 0 and pb[1] > 0 and K.conv_group_ok(da, G, db, 0), (c, ta, tb, ska)
        y_ref, part_ref = K.conv2d_f16x2(a1, wh3, b3, da, x2=a2, gn_groups=G, gn_parts=parts, pinned=pa)
        r_ref = K.conv2d_f16x2(a1, wh1, b1, db, x2=a2, measure_out=True, pinned=pb)
        for rep in range(2):
            (y, part), r = K.conv2d_f16x2_group(a1, a2, dict(w_split=wh3, bias=b3, d=da, gn_groups=G, gn_parts=parts, pinned=pa), dict(w_split=wh1, bias=b1, d=db, pinned=pb))
            assert torch.equal(y, y_ref), (c.name, ska, rep, "3x3 output", _first_diff(y, y_ref))
            assert torch.equal(part, part_ref), (c.name, ska, rep, "GroupNorm records")
            assert torch.equal(r, r_ref), (c.name, ska, rep, "1x1 output", _first_diff(r, r_ref))
            assert torch.equal(r._mf_slots, r_ref._mf_slots), (c.name, ska, rep, "bound slots")
        dg.add(y)
        dg.add(r)
    dg.done()
    assert int(K.SyncWords.get(1, a1.device).abs().max()) == 0          # every split-K counter back at zero


# ------------------------------------------------------------------------------------------------ C. element-wise bound on real operands
def _ratio(y_nchw, y64, sabs, bound):
    """max over the elements of |y - y64| / (bound sum |w||x|)"""
    assert bool((sabs > 0).all())
    return float(((y_nchw.double().cpu() - y64).abs() / (bound * sabs)).max())


@pytest.mark.parametrize("c", CC.BOUND_CASES, ids=lambda c: c.name)
def test_real_and_cancelling_operands_stay_within_the_formats_bound_element_by_element(dev, c):
    """N(0, 1) and cancelling operands (activations 1 + 1e-3 noise, zero-mean filters), samples scaled 2^0, 2^20, 2^-20: |y - y64| <= B sum |w||x| for
    EVERY element -- a max-norm over the tensor would let the 2^-20 sample hide behind the 2^20 one.  B = 2^-21 on the pair arithmetic (2^-23 per
    operand + the dropped lo.lo term below 2^-22; chains <= 96 chunks: tests/test_conv2d_cpu.py), (K + 2) 2^-24 on the fp32 matrix cores, whose
    sum of K products and one bias is an fp32 fma chain in some order (gamma_{K + 1} < (K + 2) u).  Measured: profiles/conv2d_parity_measured.txt."""
    dg, worst = Digest(f"bound/{c.name}"), {5: 0.0, 0: 0.0}
    kk = (c.C1 + c.C2) * c.k * c.k
    for cancelling in (False, True):
        x1, x2, w, b = CC.scaled_real_operands(c, cancelling=cancelling)
        y64 = CC.ref64(x1, x2, w, b, c)
        sabs = CC.sabs64(x1, x2, w, c) + b.abs().view(1, -1, 1, 1)
        ops = Ops(c, x1, x2, w, b, dev)
        plans = [(t, s) for t, s in _pair_plans(c) if s <= 1]
        if c == CC.BOUND_TWO_SOURCE[0]:
            plans += [(t, CC.BOUND_TWO_SOURCE[1]) for t in CC.f16x2_tiles(c)]
        for tile, sk in plans:
            y = dg.add(_pair(ops, tile, sk))
            r = _ratio(y.permute(0, 3, 1, 2), y64, sabs, PAIR_BOUND)
            worst[5] = max(worst[5], r)
            assert r <= 1.0, (c.name, cancelling, tile, sk, r)
        for tile in [0] + CC.igemm_tiles(c, 0):
            y = dg.add(K.conv2d(ops.a1, ops.wp, ops.b, _desc(c, tile, 1 if tile else 0, 0), x2=ops.a2))
            r = _ratio(y.permute(0, 3, 1, 2), y64, sabs, (kk + 2) * 2.0 ** -24)
            worst[0] = max(worst[0], r)
            assert r <= 1.0, (c.name, cancelling, tile, r)
    dg.done()
    print(f"[measured] bound/{c.name}: pair arithmetic worst {worst[5]:.3f} x 2^-21 sum|w||x|; fp32 matrix cores worst {worst[0]:.3f} x (K + 2) 2^-24 sum|w||x|, K = {kk}")


@pytest.mark.parametrize("dc", CC.BOUND_DIRECT, ids=lambda d: d.c.name)
def test_real_operands_through_the_direct_kernels_stay_within_an_fma_chains_bound(dev, dc):
    """(chain length + 2) 2^-24 sum |w||x| per element: K products and the bias summed in fp32 in any order"""
    c = dc.c
    kk = (c.C1 + c.C2) * c.k * c.k
    worst = 0.0
    dg = Digest(f"bound_direct/{c.name}")
    for cancelling in (False, True):
        x1, x2, w, b = CC.scaled_real_operands(c, cancelling=cancelling)
        y64 = CC.ref64(x1, x2, w, b, c)
        sabs = CC.sabs64(x1, x2, w, c) + b.abs().view(1, -1, 1, 1)
        a1 = x1.float().to(dev) if dc.lin == "nchw" else _nhwc(x1, dev)
        y = dg.add(K.conv2d(a1, K.pack_conv_weight(w.float().to(dev)), b.float().to(dev), _desc(c, precision=0, lin=dc.lin, lout=dc.lout), x2=_nhwc(x2, dev)))
        r = _ratio(y if dc.lout == "nchw" else y.permute(0, 3, 1, 2), y64, sabs, (kk + 2) * 2.0 ** -24)
        worst = max(worst, r)
        assert r <= 1.0, (c.name, cancelling, r)
    dg.done()
    print(f"[measured] bound_direct/{c.name}: worst {worst:.3f} x (K + 2) 2^-24 sum|w||x|, K = {kk}")


# ------------------------------------------------------------------------------------------------ D. covariance and plan-independence
def test_scaling_a_sample_by_a_power_of_two_scales_its_output_exactly(dev):
    """real operands, two sources, on the 9-copy body and a halo tile, unsplit and with a slice that straddles the source switch: sample n scaled
    by 2^+-40 gives exactly the scaled output.  The two sources scaled APART by 2^40 and 2^-40 -- e1 - e2 = +-80, just inside the ratio the
    rescale at the switch is derived for -- stay finite and inside the element-wise bound (sums of two scales are not a scaling of y)."""
    c = CC.COV_CASE
    x1, x2, w, _ = CC.real_operands(c)
    ops = Ops(c, x1, x2, w, None, dev)
    sc = torch.tensor([2.0 ** 40 if n % 2 == 0 else 2.0 ** -40 for n in range(c.N)], dtype=torch.float64).view(-1, 1, 1, 1)
    scaled = Ops(c, x1 * sc, x2 * sc, w, None, dev)
    h = CC.RATIO_INSIDE // 2
    exps = lambda a, b: [(CC.scale_exp(float(a[n].abs().max())), CC.scale_exp(float(b[n].abs().max()))) for n in range(3)]
    e0 = [a - b for a, b in exps(x1, x2)]          # (the unscaled sources' own difference, a binade at most: taken out so that the ratio is 80 exactly)
    xa = x1 * torch.tensor([2.0 ** h, 2.0 ** -h, 1.0], dtype=torch.float64).view(-1, 1, 1, 1)
    xb = x2 * torch.tensor([2.0 ** (e0[0] - h), 2.0 ** (e0[1] + h), 1.0], dtype=torch.float64).view(-1, 1, 1, 1)
    e = exps(xa, xb)
    assert e[0][0] - e[0][1] == CC.RATIO_INSIDE and e[1][1] - e[1][0] == CC.RATIO_INSIDE, e
    apart = Ops(c, xa, xb, w, None, dev)
    y64, sabs = CC.ref64(xa, xb, w, None, c), CC.sabs64(xa, xb, w, c)
    dg = Digest("covariance/2d")
    for tile, sk in CC.COV_PLANS:
        y, ys = dg.add(_pair(ops, tile, sk)), dg.add(_pair(scaled, tile, sk))
        assert bool(y.isfinite().all()) and float(y.abs().max()) > 0
        assert torch.equal(ys, y * sc.float().to(dev).view(-1, 1, 1, 1)), (tile, sk, _first_diff(ys, y * sc.float().to(dev).view(-1, 1, 1, 1)))
        ya = dg.add(_pair(apart, tile, sk))
        assert bool(ya.isfinite().all()) and _ratio(ya.permute(0, 3, 1, 2), y64, sabs, PAIR_BOUND) <= 1.0, (tile, sk)
    dg.done()


def test_a_zero_source_next_to_a_large_one_equals_the_one_source_result(dev):
    """The case that broke before the rescale took a zero bound for what it is (split_f16.h: source_exps): sample 0 has x1 x 2^20 next to an
    all-zero x2, sample 1 the mirror, sample 2 is ordinary.  Exact integers: float32(ref64) of the two-source problem, which for samples 0 and 1 is
    the one-source result, bit for bit -- on the 9-copy body and a halo tile, unsplit and with a slice that straddles the switch; real operands x 1e6:
    finite and inside the element-wise bound."""
    c = CC.COV_CASE
    dg = Digest("zero_source/2d")
    x1, x2, w, b, _ = CC.exact_operands(c, "xlo", "mixed")
    x1[0], x2[0], x1[1], x2[1] = x1[0] * 2.0 ** 20, 0.0, 0.0, x2[1] * 2.0 ** 20
    want = _want(x1, x2, w, None, c, dev)
    one = CC.want32(x1[:1], None, w[:, :c.C1], None, c._replace(C2=0)).permute(0, 2, 3, 1).to(dev)
    assert torch.equal(want[:1], one) and bool(want.isfinite().all())
    ops = Ops(c, x1, x2, w, None, dev)
    for tile, sk in CC.COV_PLANS:
        y = dg.add(_pair(ops, tile, sk))
        assert torch.equal(y, want), (tile, sk, _first_diff(y, want))
    x1, x2, w, b = CC.real_operands(c, seed=3)
    x1, x2 = x1.clone(), x2.clone()
    x1[0] *= 1e6
    x2[0] = 0.0
    x1[1] = 0.0
    x2[1] *= 1e6
    x1, x2 = x1.float().double(), x2.float().double()
    y64 = CC.ref64(x1, x2, w, b, c)
    sabs = CC.sabs64(x1, x2, w, c) + b.abs().view(1, -1, 1, 1)
    ops = Ops(c, x1, x2, w, b, dev)
    for tile, sk in CC.COV_PLANS:
        y = dg.add(_pair(ops, tile, sk))
        assert bool(y.isfinite().all()), (tile, sk, int((~y.isfinite()).sum()))
        assert _ratio(y.permute(0, 3, 1, 2), y64, sabs, PAIR_BOUND) <= 1.0, (tile, sk)
    dg.done()


TILE_BITS_CASES = [CC.COV_CASE, CC.HALO_CASES[-1], CC.SUBPIXEL_CASES[5], CC.M_EDGE_CASES[10], CC.COUT_EDGE_CASES[3]._replace(stride=2)]


@pytest.mark.parametrize("c", TILE_BITS_CASES, ids=lambda c: c.name)
def test_the_tile_does_not_change_the_bits(dev, c):
    """Real operands without split-K give the same bits on every tile, halo tiles included -- on one fp16 term (what test_conv_f16_single_term claims)
    AND on the three-term pair arithmetic.  The code shows the chain order is tile-independent: both bodies walk channel groups outermost, the taps
    ky KW + kx inside, two 16-channel steps per tap, and feed hi.hi into one accumulator and hi.lo' then lo'.hi into the other (MFC2_MFMA, MFH_MFMA);
    taps outside the image add exact zeros; the tile only decides which wave holds which 32 x 32 block.  One epilogue combines them."""
    x1, x2, w, b = CC.scaled_real_operands(c)
    ops = Ops(c, x1, x2, w, b, dev)
    dg = Digest(f"tiles/{c.name}")
    tiles = CC.f16x2_tiles(c)
    assert len(tiles) >= 4
    for prec in (5, 6):
        ys = [_pair(ops, t, 1, prec) for t in tiles]
        for t, y in zip(tiles[1:], ys[1:]):
            assert torch.equal(y, ys[0]), (c.name, prec, tiles[0], t, _first_diff(y, ys[0]))
        dg.add(ys[0])
    dg.done()


# ------------------------------------------------------------------------------------------------ E. non-finite confinement
@pytest.mark.parametrize("c", CC.NONFINITE_CASES, ids=lambda c: c.name)
def test_a_non_finite_pixel_reaches_exactly_the_outputs_whose_window_reads_it(dev, c):
    """one NaN, one +Inf and one -Inf pixel, one per sample, in otherwise exact data: the non-finite outputs are exactly those whose window reads
    the pixel (every output channel of them), and every other element -- of the same sample, of the other samples of the same tile -- keeps the
    bits of the clean run: the sample's measured bound is its largest FINITE magnitude, so its scale does not move"""
    family, ratio = CC.variants(c)[0]
    x1, x2, w, b, _ = CC.exact_operands(c, family, ratio)
    xs = x1.clone()
    hit = torch.zeros((c.N, 1, c.H, c.W), dtype=torch.float64)
    for n, v in enumerate((float("nan"), float("inf"), float("-inf"))[:c.N]):
        xs[n, 5 + n, (c.H // 2 + n) % c.H, (c.W - 1 - n) % c.W] = v
        hit[n, 0, (c.H // 2 + n) % c.H, (c.W - 1 - n) % c.W] = 1.0
    reads = (CC.gather64(hit, None, torch.ones(1, 1, c.k, c.k), None, c._replace(C1=1, C2=0, Cout=1)) > 0).permute(0, 2, 3, 1).expand(-1, -1, -1, c.Cout).to(dev)
    want = _want(xs, x2, w, b, c, dev)
    assert torch.equal(~want.isfinite(), reads) and 0 < int(reads.sum()) < reads.numel() // 2
    ops, ops_clean = Ops(c, xs, x2, w, b, dev), Ops(c, x1, x2, w, b, dev)
    dg = Digest(f"nonfinite/{c.name}")
    for tile, sk in _pair_plans(c):
        clean = _pair(ops_clean, tile, sk)                        # (the clean run of the same plan: whether IT is right is test A's business)
        assert bool(clean.isfinite().all())
        y = dg.add(_pair(ops, tile, sk))
        assert torch.equal(~y.isfinite(), reads), (c.name, tile, sk, int((y.isfinite() == reads).sum()))
        assert torch.equal(y[~reads], clean[~reads]), (c.name, tile, sk, int((y[~reads] != clean[~reads]).sum()))
    dg.done()


# ------------------------------------------------------------------------------------------------ F. nothing written past the output
@pytest.mark.parametrize("c", CC.GUARD_CASES, ids=lambda c: c.name)
def test_nothing_is_written_past_the_output(dev, c):
    """`out` is a view into a NaN-filled buffer with 64 floats of padding on both sides: after every plan the padding is still NaN bit for bit and
    the view holds no NaN -- every output element was written, nothing beside them -- and equals what the same plan returns in a tensor of its own"""
    family, ratio = CC.variants(c)[2]
    x1, x2, w, b, _ = CC.exact_operands(c, family, ratio)
    ops = Ops(c, x1, x2, w, b, dev)
    shape = (c.N, *CC.out_hw(c), c.Cout)
    g, n = CC.GUARD_FLOATS, c.N * CC.out_hw(c)[0] * CC.out_hw(c)[1] * c.Cout
    sentinel = torch.full((n + 2 * g,), float("nan"), dtype=torch.float32, device=dev).view(torch.int32).clone()
    count = 0
    for tile, sk in _pair_plans(c):
        buf = sentinel.clone().view(torch.float32)
        out = buf[g:g + n].view(shape)
        y = _pair(ops, tile, sk, out=out)
        assert y.data_ptr() == out.data_ptr()
        assert not bool(out.isnan().any()), (c.name, tile, sk, int(out.isnan().sum()), "output elements were not written")
        own = _pair(ops, tile, sk)
        assert torch.equal(out, own), (c.name, tile, sk, _first_diff(out, own))
        edges = torch.cat([buf[:g], buf[g + n:]]).view(torch.int32)
        assert torch.equal(edges, torch.cat([sentinel[:g], sentinel[g + n:]])), (c.name, tile, sk, int((edges != sentinel[0]).sum()))
        count += 1
    print(f"[combos] guard/{c.name} {count}")


# ------------------------------------------------------------------------------------------------ kernels.check_conv2d on the device
def test_wrappers_refuse_what_the_kernels_would_misread(dev):
    c = CC.case("chk", 2, (4, 5), 32, 32, Cout=64, k=3)
    x1, x2, w, b, _ = CC.exact_operands(c, "int8", "mixed")
    ops = Ops(c, x1, x2, w, b, dev)
    wh, d = ops.weights(5), _desc(c)
    want = _want(x1, x2, w, b, c, dev)
    assert torch.equal(K.conv2d_f16x2(ops.a1, wh, ops.b, d, x2=ops.a2), want) and torch.equal(K.conv2d(ops.a1, ops.wp, ops.b, _desc(c, precision=0), x2=ops.a2), want)
    z = lambda *s, **k: torch.zeros(*s, device=dev, **k)
    for msg, call in (
        ("conv2d_f16x2: x1 holds", lambda: K.conv2d_f16x2(z(2, 4, 5, 64), wh, ops.b, d, x2=ops.a2)),
        ("conv2d_f16x2: x1 holds", lambda: K.conv2d_f16x2(ops.a1[:1], wh, ops.b, d, x2=ops.a2)),
        ("conv2d_f16x2: x2 holds", lambda: K.conv2d_f16x2(ops.a1, wh, ops.b, d, x2=z(2, 4, 5, 64))),
        ("conv2d_f16x2: the second source is missing", lambda: K.conv2d_f16x2(ops.a1, wh, ops.b, d)),
        ("conv2d_f16x2: the second source is given", lambda: K.conv2d_f16x2(ops.a1, wh, ops.b, _desc(c._replace(C2=0)), x2=ops.a2)),
        ("conv2d_f16x2: bias", lambda: K.conv2d_f16x2(ops.a1, wh, z(63), d, x2=ops.a2)),
        ("conv2d_f16x2: bias", lambda: K.conv2d_f16x2(ops.a1, wh, z(64, dtype=torch.float64), d, x2=ops.a2)),
        ("conv2d_f16x2: the weights hold", lambda: K.conv2d_f16x2(ops.a1, (wh[0][:, :, :, :32].contiguous(), wh[1]), ops.b, d, x2=ops.a2)),
        ("conv2d_f16x2: the weights hold", lambda: K.conv2d_f16x2(ops.a1, wh, ops.b, _desc(c._replace(ups=2)), x2=ops.a2)),
        ("conv2d_f16x2: out", lambda: K.conv2d_f16x2(ops.a1, wh, ops.b, d, x2=ops.a2, out=z(2, 4, 5, 63))),
        ("conv2d_f16x2: out", lambda: K.conv2d_f16x2(ops.a1, wh, ops.b, d, x2=ops.a2, out=z(2, 4, 64, 5).transpose(2, 3))),
        ("conv2d_f16x2: out", lambda: K.conv2d_f16x2(ops.a1, wh, ops.b, d, x2=ops.a2, out=z(2, 4, 5, 64, dtype=torch.float64))),
        ("conv2d_f16x2_pairs_out: x2 holds", lambda: K.conv2d_f16x2_pairs_out(ops.a1, wh, ops.b, d, (1.0, 1.0), 1.0, x2=ops.a1[:, :, :, :16])),
        ("conv2d_f16x2_pairs_out: bias", lambda: K.conv2d_f16x2_pairs_out(ops.a1, wh, z(65), d, (1.0, 1.0), 1.0, x2=ops.a2)),
        ("conv2d: x1 holds", lambda: K.conv2d(ops.a1[:, :3], ops.wp, ops.b, _desc(c, precision=0), x2=ops.a2)),
        ("conv2d: the weights hold", lambda: K.conv2d(ops.a1, ops.wp, ops.b, _desc(c, precision=3), x2=ops.a2)),
        ("conv2d: the weights hold", lambda: K.conv2d(ops.a1, ops.weights(3), ops.b, _desc(c, precision=0), x2=ops.a2)),
        ("conv2d: out", lambda: K.conv2d(ops.a1, ops.wp, ops.b, _desc(c, precision=0), x2=ops.a2, out=z(2, 4, 5, 32))),
        ("conv2d: x1 holds 480 values.*NCHW", lambda: K.conv2d(z(2, 12, 4, 5), z(8, 3, 3, 8), None, _desc(CC.case("n", 2, (4, 5), 8, Cout=8), precision=0, lin="nchw"))),
    ):
        with pytest.raises(RuntimeError, match=msg):
            call()
    # and a refusal leaves the library usable
    assert torch.equal(K.conv2d_f16x2(ops.a1, wh, ops.b, d, x2=ops.a2), want)
