"""The 3-D convolution's edge cases without a GPU (tests/conv3d_cases.py): the two references agree, every exact case qualifies, the split-K
arithmetic restated in Python is the library's, the case list holds the slices the GPU test relies on, the library refuses what it must before
it launches anything, and the wrapper's size checks (kernels.check_conv3d)."""

import ctypes as C

import pytest
import torch

from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from tests import conv3d_cases as CC

ALL_GEOMS = CC.EXACT_CASES + CC.CANCEL_CASES + CC.TILE_BITS_CASES + [c for c, _ in CC.COVARIANCE_CASES] + [CC.ZERO_SOURCE_CASE]


def _desc(c, tile=0, sk=0):
    return K.make_conv3d_desc(c.N, *c.dhw, c.C1, c.C2, c.Cout, c.k, c.stride, c.pad, c.up, tile_hint=tile, splitk_hint=sk)


def _small(c):
    """the geometry of c on few channels (the references' agreement is about coordinates, not about channel counts)"""
    return c._replace(N=min(c.N, 2), C1=2, C2=1 if c.C2 else 0, Cout=2)


@pytest.mark.parametrize("c", ALL_GEOMS, ids=lambda c: c.name)
def test_the_two_references_agree_and_the_library_names_the_same_output_size(c):
    s = _small(c)
    g = torch.Generator().manual_seed(5)
    x1 = torch.randint(-4, 5, (s.N, s.C1, *s.dhw), generator=g).double()
    x2 = torch.randint(-4, 5, (s.N, s.C2, *s.dhw), generator=g).double() if s.C2 else None
    w = torch.randint(-4, 5, (s.Cout, s.C1 + s.C2, s.k, s.k, s.k), generator=g).double()
    b = torch.randint(-4, 5, (s.Cout,), generator=g).double()
    a, e = CC.ref64(x1, x2, w, b, s.stride, s.pad, s.up), CC.gather64(x1, x2, w, b, s.stride, s.pad, s.up)
    assert a.shape == e.shape and torch.equal(a, e)          # (small integers: both are exact)
    assert bool((a != 0).any())
    assert K.conv3d_ok(_desc(c))
    assert K.conv3d_out_dims(_desc(c)) == CC.out_dims(c.dhw, c.k, c.stride, c.pad, c.up) == tuple(a.shape[2:])


def test_the_reference_where_interpolate_and_conv3d_meet_pads_and_even_extents():
    """hand-checked values of ref64: pad 0, pad 2 and stride 2 on an even extent, upsampled -- a 1-D problem along W, D = H = 1, k = 3 on the W axis
    only (the other taps are zero)"""
    x = torch.tensor([1.0, 10.0, 100.0, 1000.0]).view(1, 1, 1, 1, 4)
    w = torch.zeros(1, 1, 3, 3, 3)
    w[0, 0, 1, 1] = torch.tensor([1.0, 2.0, 4.0])
    # upsampled row: 1 1 10 10 100 100 1000 1000
    u = [1, 1, 10, 10, 100, 100, 1000, 1000]
    conv = lambda p, s: [sum(wt * (u[o * s - p + t] if 0 <= o * s - p + t < 8 else 0) for t, wt in enumerate((1, 2, 4))) for o in range((8 + 2 * p - 3) // s + 1)]
    for p, s in ((0, 1), (2, 1), (0, 2), (1, 2), (2, 2)):
        for f in (CC.ref64, CC.gather64):
            y = f(x, None, w, None, (1, 1, s), (1, 1, p), (0, 0, 1))
            assert y.view(-1).tolist() == [float(v) for v in conv(p, s)], (p, s, f.__name__)
    assert conv(0, 2) == [43, 430, 4300] and conv(2, 1)[:2] == [4, 6] and conv(2, 1)[-1] == 1000   # (pad 2: the first window holds one voxel)


def test_pair_terms_restate_the_split():
    x = torch.tensor([1.0 + 3 * 2.0 ** -13, -1.0 - 2.0 ** -13, 0.0, 1.0, 0.3])
    s, hi, lo = CC.pair_terms(x, float(x.abs().max()))
    assert s == -14 and hi[:4].tolist() == [16384.0, -16384.0, 0.0, 16384.0] and lo[:4].tolist() == [6.0 * 2048, -2.0 * 2048, 0.0, 0.0]
    assert abs(float((hi[4] + lo[4] / 2048) * 2.0 ** s) - float(x[4].float())) <= 2.0 ** -23 * 0.3
    assert CC.scale_exp(0.0) == -100 and CC.scale_exp(1e6) == 5 and CC.scale_exp(float("inf")) == 100 and CC.scale_exp(65504.0) == 1


@pytest.mark.parametrize("c", CC.EXACT_CASES, ids=lambda c: c.name)
def test_every_exact_case_qualifies(c):
    for family, ratio in CC.variants(c):
        x1, x2, w, b, units = CC.exact_operands(c, family, ratio)
        for t in (x1, x2, w, b):
            assert t is None or torch.equal(t.float().double(), t)          # fp32 values
        q = CC.exact_budget(c, x1, x2, w, b, units)
        print(f"[margin] {c.name} {family} ratio={ratio}: lo.lo = {q['lolo']}, log2 sum|terms|/unit: hi.hi {q['bits_m']:.2f}, cross {q['bits_x']:.2f}, "
              f"all {q['bits_all']:.2f} (< 24)")
        assert q["lolo"] == 0.0 and q["unit_ok"], (family, ratio, q)
        assert q["bits_m"] < 24 and q["bits_x"] < 24 and q["bits_all"] < 24, (family, ratio, q)
        # the family's lo part is really there, and both signs of the ratio occur in a mixed case
        lo_x = max(float(CC.pair_terms(x[n], float(x[n].abs().max()))[2].abs().max()) for x in (x1, x2) if x is not None for n in range(c.N))
        lo_w = float(CC.pair_terms(w, float(w.abs().max()))[2].abs().max())
        assert (lo_x > 0, lo_w > 0) == ((True, False) if family == "xlo" else (False, True))
        exps = CC.sample_exps(c, ratio)
        assert {e for e, _ in exps} == set(CC.SAMPLE_EXPS[:min(3, c.N)])
        if ratio == "mixed":
            assert {b2 - a for a, b2 in exps} == {20, -20}
        y0 = CC.ref64(x1, x2, w, None, c.stride, c.pad, c.up)
        assert torch.equal(y0.float().double(), y0)                        # the value before the bias is an fp32 value
        assert CC.bias_add_rounds_once(y0, b)
        assert bool((b != 0).any()) or c.Cout < 3
        for n in range(c.N):                                                   # a sample's output is not all bias
            assert bool((y0[n] != 0).any()) or c.dhw == (1, 1, 1)


@pytest.mark.parametrize("c", CC.EXACT_CASES + CC.CANCEL_CASES + [CC.ZERO_SOURCE_CASE], ids=lambda c: c.name)
def test_slices_restate_the_librarys_split_k(c):
    lib = L.load()
    for sk in CC.SPLIT_KS:
        nit, it_sw, per, eff = CC.slices(c, sk)
        d = _desc(c, 1, sk)
        m = c.N
        for o in CC.out_dims(c.dhw, c.k, c.stride, c.pad, c.up):
            m *= o
        assert lib.mf_conv3d_workspace_bytes(C.byref(d)) == (eff * m * c.Cout * 4 if eff > 1 else 0), (sk, eff)
        kinds = CC.slice_kinds(c, sk)
        assert len(kinds) == eff and (eff - 1) * per < nit <= eff * per       # no empty slice
        if c.C2 == 0:
            assert set(kinds) == {"before"}
    if (c.C1, c.C2, c.k) == (64, 32, 3):
        assert CC.slices(c, 16) == (81, 54, 6, 14)


def test_the_split_k_list_meets_the_source_switch_in_every_way():
    for k in (1, 3):
        hit = {}
        for c in CC.TWO_SOURCE_CASES:
            if c.k != k:
                continue
            for sk in CC.distinct_sks(c):
                for kind in CC.slice_kinds(c, sk):
                    if sk > 1 or kind != "straddles":
                        hit.setdefault(kind, []).append((c.name, sk))
        print(f"[slices] k = {k}: " + "; ".join(f"{kind}: {len(v)} plans, e.g. {v[0]}" for kind, v in sorted(hit.items())))
        for kind in ("starts_at", "ends_at", "straddles"):
            assert hit.get(kind), (k, kind)                                   # (straddles: counted under a real split, sk > 1)
    assert "straddles" in CC.slice_kinds(CC.COVARIANCE_CASES[2][0], CC.COVARIANCE_CASES[2][1])
    assert "straddles" in CC.slice_kinds(CC.ZERO_SOURCE_CASE, CC.ZERO_SOURCE_SKS[1])
    assert "straddles" in CC.slice_kinds(CC.CANCEL_CASES[1], 4)


def test_the_cap_cases_pass_their_caps():
    c = CC.REDUCER_CASE
    assert c.k == 1 and c.C1 == 64 and CC.slices(c, 2)[3] == 2
    assert c.N * c.dhw[0] * c.dhw[1] * c.dhw[2] * c.Cout > 8192 * 256
    p = CC.PACK_CASE
    assert p["Cout"] * p["k"] ** 3 * p["cin_pad"] > 4096 * 256 and p["cin_pad"] > p["Cin"]
    assert CC.PACK_SQUARE_CASE["Cin"] == CC.PACK_SQUARE_CASE["k"] ** 3


def test_the_library_refuses_before_it_launches():
    lib = L.load()
    fake = C.c_void_p(0x1000)   # never dereferenced: every refusal below precedes the launch
    c = CC.TWO_SOURCE_CASES[0]
    d = _desc(c, 1, 4)
    need = lib.mf_conv3d_workspace_bytes(C.byref(d))
    assert need > 0
    rc = lib.mf_conv3d_f16x2(fake, fake, fake, None, fake, None, None, 1.0, fake, need - 1, C.byref(d), None)
    assert rc == -4 and b"workspace" in lib.mf_last_error()
    rc = lib.mf_conv3d_f16x2(fake, fake, fake, None, fake, None, None, 1.0, None, need, C.byref(d), None)
    assert rc < 0 and b"workspace" in lib.mf_last_error()
    rc = lib.mf_conv3d_f16x2(fake, None, fake, None, fake, None, None, 1.0, fake, need, C.byref(d), None)
    assert rc < 0 and b"null pointer" in lib.mf_last_error()
    for k in (1, 3):
        dd = K.make_conv3d_desc(2, 4, 4, 4, 32, 0, 8, k, 1, k)
        assert not K.conv3d_ok(dd)
        rc = lib.mf_conv3d_f16x2(fake, None, fake, None, fake, None, None, 1.0, None, 0, C.byref(dd), None)
        assert rc == -2 and b"unsupported" in lib.mf_last_error()
    assert K.conv3d_ok(K.make_conv3d_desc(2, 4, 4, 4, 32, 0, 8, 3, 1, 2)) and not K.conv3d_ok(K.make_conv3d_desc(2, 4, 4, 4, 32, 0, 8, 3, 1, -1))
    rc = lib.mf_pack_conv3d_weight_f32(fake, fake, 4, 33, 3, 32, None)
    assert rc < 0 and b"pack_conv3d_weight" in lib.mf_last_error()


def test_check_conv3d_compares_every_size_with_the_descriptor():
    d = K.make_conv3d_desc(2, 3, 4, 5, 32, 64, 6, 3, (1, 2, 2), (1, 1, 1), (0, 1, 1))
    do, ho, wo = K.conv3d_out_dims(d)
    assert (do, ho, wo) == (3, 4, 5)
    x1, x2 = torch.zeros(2, 12, 5, 32), torch.zeros(2, 12, 5, 64)          # (the [N, D*H, W, C] view the 3-D blocks hold)
    wh = (torch.zeros(6, 3, 3, 3, 96, dtype=torch.int32), 1.0)
    bias, out = torch.zeros(6), torch.zeros(2, do * ho, wo, 6)
    K.check_conv3d(x1, x2, wh, bias, out, d)
    K.check_conv3d(x1, x2, wh, None, None, d)
    K.check_conv3d(x1.view(2, 3, 4, 5, 32), x2, wh, bias, out.view(2, do, ho, wo, 6), d)
    bad = [
        ("x1 holds", dict(x1=torch.zeros(2, 12, 5, 31))), ("x1 holds", dict(x1=torch.zeros(1, 12, 5, 32))), ("x1 holds", dict(x1=x2)),
        ("x2 holds", dict(x2=x1)), ("second source is missing", dict(x2=None)), ("bias", dict(bias=torch.zeros(5))), ("bias", dict(bias=torch.zeros(6, dtype=torch.float64))),
        ("split weights", dict(wh=(torch.zeros(6, 27, 64, dtype=torch.int32), 1.0))), ("split weights", dict(wh=(torch.zeros(6, 96, dtype=torch.int32), 1.0))),
        ("out", dict(out=torch.zeros(2, do * ho, wo, 5))), ("out", dict(out=torch.zeros(2, do * ho - 1, wo, 6))), ("out", dict(out=torch.zeros(2, do * ho, wo, 6, dtype=torch.float64))),
        ("out", dict(out=torch.zeros(2, do * ho, 6, wo).transpose(2, 3))),
    ]
    for msg, kw in bad:
        a = dict(x1=x1, x2=x2, wh=wh, bias=bias, out=out)
        a.update(kw)
        with pytest.raises(RuntimeError, match=msg):
            K.check_conv3d(a["x1"], a["x2"], a["wh"], a["bias"], a["out"], d)
    d1 = K.make_conv3d_desc(2, 3, 4, 5, 32, 0, 6, 1)
    with pytest.raises(RuntimeError, match="second source is given"):
        K.check_conv3d(x1, x1, (torch.zeros(6, 32, dtype=torch.int32), 1.0), bias, None, d1)
    # it is the first thing conv3d_f16x2 does: a wrong size raises before any device is asked for
    with pytest.raises(RuntimeError, match="out"):
        K.conv3d_f16x2(x1, wh, bias, d, x2=x2, out=torch.zeros(2, 3, 4, 5, 5))
