"""The Winograd F(2x2, 3x3) form (csrc/winograd.h, csrc/conv_f16x2_wino.inc) held to exact and element-wise fp64 references at its edges, on a real
MI355X.  tests/wino_cases.py has the references, the operands that are exact in the transform domain, the restated host rules and the case lists;
tests/test_wino_edges_cpu.py proves their premises without a GPU.  Every test prints `[digest] <name> <sha256 of its outputs>`: two builds computed
the same bits when the digest lines agree (profiles/wino_parity_measured.txt).

  A  the three transforms bit for bit: U = G g G^T, V = B^T d B as pairs and as fp32, on every padded-tap geometry, past the grid cap, with a
     non-finite pixel confined to the components that read it, and nothing written past an output;
  B  exact operands give float32(ref64) on every tile that holds a component and every split-K that meets inside the launch; the GroupNorm records
     EQUAL the fp64 sums; an all-zero second source changes no bit;
  C  an element-wise bound on real and cancelling operands, counted in the cases file; the tile does not change the bits;
  D  the tail: element-wise against fp64 on an exact y at every loop shape, workgroup numbering, slot count and residual kind; its side outputs
     exactly; bit for bit the three-launch form and -- without an activation -- an fp32 restatement; the constant group; non-finite confinement;
  E  the fp32 form (precision 0 and 3)."""

import ctypes as C

import pytest
import torch

from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from tests import groupnorm_cases as GC
from tests import wino_cases as WC
from tests.test_conv3d_gpu import Digest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _nhwc(x, dev):
    return None if x is None else x.float().permute(0, 2, 3, 1).contiguous().to(dev)


def _desc(c, tile=0, sk=0, precision=5):
    return K.make_conv_desc(c.N, c.H, c.W, c.C1, c.C2, c.Cout, c.k, c.stride, c.pad, c.ups, tile_hint=tile, splitk_hint=sk, precision=precision)


def _halves(pairs):
    """fp16-pair storage (int32 [..., C], groups of 8 channels as [hi x 8][lo' x 8]) -> (hi, lo') fp64 on the CPU, same shape"""
    raw = pairs.cpu().contiguous().view(torch.float16).double().reshape(-1, 2, 8)
    return raw[:, 0].reshape(pairs.shape), raw[:, 1].reshape(pairs.shape)


def _decode(pairs, bounds):
    """the values a pair tensor [rows, ...] stands for under its per-row bounds, by scale_exp_of's own rule (a zero bound included)"""
    hi, lo = _halves(pairs)
    s = torch.tensor([2.0 ** WC.scale_exp(float(b)) for b in bounds.cpu()], dtype=torch.float64).view(-1, *([1] * (pairs.dim() - 1)))
    return (hi + lo / 2048.0) * s


def _same_halves(a, b, where):
    """two pair tensors hold the same (hi, lo') at the channels `where` selects (a storage word holds two channels' hi or lo': compare decoded)"""
    (ah, al), (bh, bl) = _halves(a), _halves(b)
    return torch.equal(ah[where], bh[where]) and torch.equal(al[where], bl[where])


def _first_diff(y, want):
    bad = (y != want) & ~(y.isnan() & want.isnan())
    i = bad.nonzero()[0].tolist()
    return f"{int(bad.sum())} of {y.numel()} differ, first at {tuple(i)}: got {y[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}"


def _exact_x(shape, seed, zero_sample=None):
    """NCHW fp64: a + b 2^-13 (a in {-1, 0, 1}, |b| <= 3), samples scaled 2^0, 2^20, 2^-20: V = B^T d B of it is exact in fp32 and in the pair form"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-1, 2, shape, generator=g).double()
    x = a + torch.randint(-3, 4, shape, generator=g).double() * (a != 0).double() * 2.0 ** -13
    x.view(shape[0], -1)[:, 0] = 1.0
    x = x * torch.tensor([2.0 ** WC.CC.SAMPLE_EXPS[n % 3] for n in range(shape[0])], dtype=torch.float64).view(-1, 1, 1, 1)
    if zero_sample is not None:
        x[zero_sample] = 0.0
    return x


def _wino_input_raw(xs, xb, n, h, w, c, dev):
    """mf_wino_input_f16x2 into buffers with WC.SENTINEL words behind them -> (V [16, n, T, c] int32, vbound [16 n]); asserts the words stay"""
    t = (h // 2) * (w // 2)
    nv = 16 * n * t * c
    v = torch.full((nv + WC.SENTINEL,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    vb = torch.full((16 * n + WC.SENTINEL,), -7.0, dtype=torch.float32, device=dev)
    L.check(L.load().mf_wino_input_f16x2(xs.data_ptr(), xb.data_ptr(), v.data_ptr(), vb.data_ptr(), n, h, w, c, K.stream()), "mf_wino_input_f16x2")
    assert bool((v[nv:] == 0x5A5A5A5A).all()) and bool((vb[16 * n:] == -7.0).all()), (n, h, w, c)
    return v[:nv].view(16, n, t, c), vb[:16 * n]


# ------------------------------------------------------------------------------------------------ A. the transforms
def test_wino_pack_weight_is_fp64_rounded_once(dev):
    co, ci = WC.PACK_CASE
    g = torch.Generator().manual_seed(5)
    w = torch.randn((co, ci, 3, 3), generator=g)
    want = WC.U64(w).float()
    buf = torch.full((16 * co * ci + WC.SENTINEL,), -7.0, dtype=torch.float32, device=dev)
    L.check(L.load().mf_wino_pack_weight_f32(w.to(dev).data_ptr(), buf.data_ptr(), co, ci, K.stream()), "mf_wino_pack_weight_f32")
    got = buf[:16 * co * ci].view(16, co, ci).cpu()
    assert torch.equal(got, want), _first_diff(got, want)
    assert bool((buf[16 * co * ci:] == -7.0).all())
    assert torch.equal(K.wino_pack_weight(w.to(dev)).view(16, co, ci).cpu(), want)
    Digest("pack_weight").add(got)


@pytest.mark.parametrize("ch", WC.INPUT_CHANNELS)
@pytest.mark.parametrize("hw", WC.INPUT_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_wino_input_pairs_is_bt_d_b_exactly(dev, hw, ch):
    """samples scaled 2^0, 2^20, 2^-20 and an all-zero one: the decoded V equals B^T d B, vbound[k N + n] == 4 bound(x[n]) for all 16 k"""
    h, w = hw
    n = 4
    x = _exact_x((n, ch, h, w), 100 * h + 10 * w + ch, zero_sample=3)
    xd = _nhwc(x, dev)
    v, vb = _wino_input_raw(K.split_of(xd), K.bound_of(xd), n, h, w, ch, dev)
    xb = K.bound_of(xd).cpu()
    assert torch.equal(xb, x.abs().amax(dim=(1, 2, 3)).float())
    assert torch.equal(vb.cpu().view(16, n), (4.0 * xb).expand(16, n))
    got = _decode(v.reshape(16 * n, -1, ch), vb).view(16, n, -1, ch)
    want = WC.V64(x)
    assert torch.equal(got, want), _first_diff(got, want)
    assert not bool(v[:, 3].any())                                           # the zero sample: zero bits
    dg = Digest(f"wino_input/{h}x{w}x{ch}")
    dg.add(v)
    dg.done()


def _patch_components(h, w, py, px):
    """{(tile, k)}: the components of the tiles whose 4 x 4 patch holds pixel (py, px) that read it (B^T has a non-zero there)"""
    out = set()
    for ty in range(h // 2):
        for tx in range(w // 2):
            r, c = py - (2 * ty - 1), px - (2 * tx - 1)
            if 0 <= r < 4 and 0 <= c < 4:
                out |= {(ty * (w // 2) + tx, 4 * i + j) for i in range(4) for j in range(4) if WC.BT[i, r] != 0 and WC.BT[j, c] != 0}
    return out


def test_wino_input_confines_a_non_finite_pixel(dev):
    """a NaN and an Inf pixel in sample 1, under the bound of the clean tensor (a derived bound, as a producer hands it on): V is
    non-finite in exactly the components of the tiles whose patch holds the pixel and that read it, at that channel; every other value of the sample
    and every other sample keep their bits"""
    n, h, w, ch = 3, 8, 12, 24
    x = _exact_x((n, ch, h, w), 77)
    xd = _nhwc(x, dev)
    xb = K.bound_of(xd)
    clean, _ = _wino_input_raw(K.split_of(xd), xb, n, h, w, ch, dev)
    bad = xd.clone()
    spots = {(3, 4, 5): float("nan"), (0, 11, 17): float("inf")}
    for (py, px, c), val in spots.items():
        bad[1, py, px, c] = val
    v, vb = _wino_input_raw(K.split_f16x2(bad, xb), xb, n, h, w, ch, dev)
    hi, lo = _halves(v)
    finite = torch.isfinite(hi) & torch.isfinite(lo)
    want_bad = torch.zeros((16, n, (h // 2) * (w // 2), ch), dtype=torch.bool)
    for (py, px, c) in spots:
        for tile, k in _patch_components(h, w, py, px):
            want_bad[k, 1, tile, c] = True
    assert torch.equal(~finite, want_bad), (int((~finite).sum()), int(want_bad.sum()))
    assert _same_halves(v, clean, ~want_bad)


@pytest.mark.parametrize("hw", WC.INPUT_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_wino_input_f32_is_bt_d_b_exactly(dev, hw):
    h, w = hw
    n, ch = 3, 4
    x = _exact_x((n, ch, h, w), 7 * h + w)
    xd = _nhwc(x, dev)
    t = (h // 2) * (w // 2)
    buf = torch.full((16 * n * t * ch + WC.SENTINEL,), -7.0, dtype=torch.float32, device=dev)
    L.check(L.load().mf_wino_input_f32(xd.data_ptr(), buf.data_ptr(), n, h, w, ch, K.stream()), "mf_wino_input_f32")
    got, want = buf[:16 * n * t * ch].view(16, n, t, ch).cpu(), WC.V64(x).float()
    assert torch.equal(got, want), _first_diff(got, want)
    assert bool((buf[16 * n * t * ch:] == -7.0).all())
    assert torch.equal(K.wino_input_f32(xd).cpu(), want)
    Digest(f"wino_input_f32/{h}x{w}").add(got)


def test_the_input_transforms_past_their_grid_cap(dev):
    """(5, 64, 64, 1024): 1 310 720 threads of work on a grid capped at 4096 x 256, so the grid-stride loop takes a second trip for a quarter of the
    threads.  Every sample equals the transform of that sample alone (262 144 threads: under the cap) bit for bit, in both forms; sample 4 -- the one
    the second trip writes -- is also exact against B^T d B"""
    n, h, w, ch = WC.GRID_CAP_SHAPE
    assert WC.input_grid(n, h, w, ch) == (WC.INPUT_GRID_CAP, 2) and WC.input_grid(1, h, w, ch)[0] < WC.INPUT_GRID_CAP
    t = (h // 2) * (w // 2)
    g = torch.Generator(device=dev).manual_seed(9)
    a = torch.randint(-1, 2, (n, h, w, ch), generator=g, device=dev).float()
    xd = a + torch.randint(-3, 4, (n, h, w, ch), generator=g, device=dev).float() * (a != 0).float() * 2.0 ** -13
    xd[:, 0, 0, 0] = 1.0
    xd = (xd * torch.tensor([2.0 ** WC.CC.SAMPLE_EXPS[i % 3] for i in range(n)], device=dev).view(-1, 1, 1, 1)).contiguous()
    xs, xb = K.split_of(xd), K.bound_of(xd)
    v, vb = _wino_input_raw(xs, xb, n, h, w, ch, dev)
    vf = torch.empty((16, n, t, ch), dtype=torch.float32, device=dev)
    lib = L.load()
    L.check(lib.mf_wino_input_f32(xd.data_ptr(), vf.data_ptr(), n, h, w, ch, K.stream()), "mf_wino_input_f32")
    dg = Digest("grid_cap")
    for i in range(n):
        vi, vbi = _wino_input_raw(xs[i:i + 1], xb[i:i + 1], 1, h, w, ch, dev)
        assert torch.equal(v[:, i], vi[:, 0]) and torch.equal(vb.view(16, n)[:, i], vbi), i
        vfi = torch.empty((16, 1, t, ch), dtype=torch.float32, device=dev)
        L.check(lib.mf_wino_input_f32(xd[i:i + 1].data_ptr(), vfi.data_ptr(), 1, h, w, ch, K.stream()), "mf_wino_input_f32")
        assert torch.equal(vf[:, i], vfi[:, 0]), i
        dg.add(vi[:, 0, :8])
    for cs in (slice(0, 64), slice(ch - 64, ch)):                          # (the first and last channels of the sample: V is per channel)
        want = WC.V64(xd[n - 1:, :, :, cs].cpu().double().permute(0, 3, 1, 2))[:, 0]
        assert torch.equal(vf[:, n - 1, :, cs].cpu().double(), want)
        got = _decode(v[:, n - 1, :, cs].contiguous(), vb.view(16, n)[:, n - 1])
        assert torch.equal(got, want), _first_diff(got, want)
    dg.done()


# ------------------------------------------------------------------------------------------------ B. exact, everywhere
class Ops:
    """device operands of fp64 NCHW / OIHW tensors: NHWC fp32 sources (their V is cached on them by the first call), U as fp16 pairs, the bias"""

    def __init__(self, c, x1, x2, w, b, dev):
        self.c, self.a1, self.a2 = c, _nhwc(x1, dev), _nhwc(x2, dev)
        self.b = None if b is None else b.float().to(dev)
        self.u = K.wino_pack_weight(w.float().to(dev))
        self.uh = K.split_weight_f16x2(self.u)


def _wino(ops, tile=0, sk=0, bias=True, **kw):
    d = _desc(ops.c, tile, sk)
    assert K.wino_ok(d), (ops.c, tile, sk)
    return K.conv2d_wino_f16x2(ops.a1, ops.uh, ops.b if bias else None, d, x2=ops.a2, **kw)


def _plans(c):
    """(tile hint, split-K hint): the planner's own plan, then every tile that holds a component x every distinct split-K that meets inside the launch.
    Asserts on the way that the library refuses exactly the tiles and splits the restated rule refuses: no combination is skipped silently."""
    plans = [(0, 0)]
    for t in WC.TILES:
        if c.Cout % WC.TILES[t][1] == 0:
            assert K.wino_ok(_desc(c, t)) == WC.wino_ok(c, t), (c, t)
    tiles = WC.wino_tiles(c)
    assert tiles
    for sk in WC.distinct_sks(WC.gemm_case(c)):
        assert K.wino_ok(_desc(c, tiles[0], sk)) == WC.wino_ok(c, tiles[0], sk), (c, sk)
    return plans + [(t, sk) for t in tiles for sk in WC.wino_sks(c)]


def _want(x1, x2, w, b, c, dev):
    return WC.want32(x1, x2, w, b, c).permute(0, 2, 3, 1).contiguous().to(dev)


@pytest.mark.parametrize("c", WC.EXACT_CASES, ids=lambda c: c.name)
def test_exact_operands_give_float32_of_ref64_on_the_winograd_form(dev, c):
    dg, n = Digest(f"exact_wino/{c.name}"), 0
    plans = _plans(c)
    for family, ratio in WC.variants(c):
        x1, x2, w, b = WC.wino_operands(c, family, ratio)
        want = _want(x1, x2, w, b, c, dev)
        ops = Ops(c, x1, x2, w, b, dev)
        for tile, sk in plans:
            y = _wino(ops, tile, sk)
            assert y.shape == want.shape
            assert torch.equal(y, want), (c.name, family, ratio, tile, sk, WC.CC.slice_kinds(WC.gemm_case(c), max(sk, 1)), _first_diff(y, want))
            n += 1
        dg.add(y)
        y0 = _wino(ops, bias=False)                                       # the bias rounds once: without it the exact fp32 value before the add
        assert torch.equal(y0.double().cpu(), WC.ref64(x1, x2, w, None, c).permute(0, 2, 3, 1))
    dg.done()
    print(f"[combos] exact_wino/{c.name} {len(plans)} (tile, sk) x {len(WC.variants(c))} families = {n} launches")


def _zero_source_plans(c):
    """(tile, sk, one-source split or None) for an all-zero second source: every tile unsplit, the first tile on every split.  The one-source call
    whose slices cut at the same channel groups and meet in the same tree sums the same fp32 values in the same order (the second source's groups and
    slices add exact zeros); None where no such call exists (another association of the same sums)"""
    one = WC.case(c.name + "_one", c.N, (c.H, c.W), c.C1, 0, Cout=c.Cout)
    out = []
    for tile, sk in _plans(c)[1:]:
        if sk > 1 and tile != WC.wino_tiles(c)[0]:
            continue
        _, _, per, eff = WC.slices(WC.gemm_case(c), sk)
        eff1 = -(-(c.C1 // 32) // per)
        aligned = eff1 == 1 or (eff1 == eff and WC.slices(WC.gemm_case(one), eff1)[2] == per)
        out.append((tile, sk, eff1 if aligned else None))
    return one, out


def _zero_source_ops(c, dev):
    x1, _, w, b = WC.scaled_real_operands(c)
    one, plans = _zero_source_plans(c)
    x2 = torch.zeros((c.N, c.C2, c.H, c.W), dtype=torch.float64)
    return (x1, x2, w, b), Ops(one, x1, None, w[:, :c.C1].contiguous(), b, dev), Ops(c, x1, x2, w, b, dev), plans


@pytest.mark.parametrize("c", WC.TWO_SOURCE_CASES, ids=lambda c: c.name)
def test_an_all_zero_second_source_changes_no_bit(dev, c):
    """the rescale 2^(e1 - e2) at the switch with e2 = -100 (a zero bound): the one-source call on the first source's channels, bit for bit, on real
    operands (any difference shows), unsplit on every tile and on every split whose slices the one-source call can cut at the same groups"""
    _, ref, ops, plans = _zero_source_ops(c, dev)
    dg = Digest(f"zero_source/{c.name}")
    n_equal = 0
    for tile, sk, sk1 in plans:
        if sk1 is not None:
            y, base = _wino(ops, tile, sk), _wino(ref, tile, sk1)
            assert bool(torch.isfinite(y).all()) and torch.equal(y, base), (c.name, tile, sk, _first_diff(y, base))
            n_equal += 1
            dg.add(y)
    assert n_equal >= len(WC.wino_tiles(c)) + (1 if c.C1 <= c.C2 * 2 else 0)
    dg.done()


@pytest.mark.parametrize("c", WC.TWO_SOURCE_CASES, ids=lambda c: c.name)
def test_an_all_zero_second_source_within_the_counted_bound_on_every_split(dev, c):
    """every plan of the two-source call, the splits no one-source call sums in the same order included, element-wise within wino_cases.real_bound
    of the fp64 convolution (the zero source adds nothing to the bound: sum |U||V| over its channels is zero)"""
    (x1, x2, w, b), _, ops, plans = _zero_source_ops(c, dev)
    y64 = WC.ref64(x1, x2, w, b, c).permute(0, 2, 3, 1)
    for tile, sk, _ in plans:
        E = WC.real_bound(x1, x2, w, b, c, WC.slices(WC.gemm_case(c), sk)[3]).permute(0, 2, 3, 1)
        y = _wino(ops, tile, sk).cpu().double()
        assert bool(torch.isfinite(y).all()) and float(((y - y64).abs() / E).max()) < 1.0, (c.name, tile, sk)


@pytest.mark.parametrize("c", WC.RECORD_CASES, ids=lambda c: c.name)
def test_the_groupnorm_records_equal_the_fp64_sums(dev, c):
    """on small-integer outputs (wino_cases.small_operands, no bias: the CPU test asserts the premise) the fp32 sums of a tile's 16 values and of their
    squares are exact, so the records {sum, sum of squares} of every part equal the fp64 sums of the output: torch.equal, per sample and part"""
    G = WC.RECORD_GROUPS[c.Cout]
    x1, w, _ = WC.small_operands(c, bias=False)
    ops = Ops(c, x1, None, w, None, dev)
    parts = K.wino_gn_parts(_desc(c), G)
    assert parts == WC.gn_parts(c, G) > 0
    y, partial = _wino(ops, bias=False, gn_groups=G, gn_parts=parts)
    y64 = WC.ref64(x1, None, w, None, c).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(y.cpu().double(), y64)
    T, tpp, cpg = WC.tiles_of(c), WC.tiles_per_part(c), c.Cout // G
    tiles = y64.reshape(c.N, c.H // 2, 2, c.W // 2, 2, G, cpg).permute(0, 1, 3, 2, 4, 5, 6).reshape(c.N, T, 4, G, cpg)
    s, q = tiles.sum(dim=(2, 4)), (tiles * tiles).sum(dim=(2, 4))                                   # [N, T, G]
    want = torch.stack([torch.stack([s[:, p * tpp:min(T, (p + 1) * tpp)].sum(1), q[:, p * tpp:min(T, (p + 1) * tpp)].sum(1)], -1) for p in range(parts)], 1)
    assert partial.shape == want.shape == (c.N, parts, G, 2)
    assert torch.equal(partial.cpu(), want), (c.name, WC.output_rounds(c), _first_diff(partial.cpu(), want))
    assert torch.equal(_wino(ops, bias=False), y)
    dg = Digest(f"records/{c.name}")
    dg.add(partial)
    dg.done()


# ------------------------------------------------------------------------------------------------ C. real operands
@pytest.mark.parametrize("cancelling", [False, True], ids=["real", "cancelling"])
@pytest.mark.parametrize("c", WC.REAL_CASES, ids=lambda c: c.name)
def test_real_operands_within_the_counted_bound(dev, c, cancelling):
    """|y - y64| <= c 2^-24 (sum |U_k| |B^T||d||B|_k + |bias|) element by element (wino_cases.real_bound counts c), samples scaled 2^0 / 2^20 / 2^-20;
    and at a fixed split-K the tile does not change the bits"""
    x1, x2, w, b = WC.scaled_real_operands(c, cancelling=cancelling)
    ops = Ops(c, x1, x2, w, b, dev)
    y64 = WC.ref64(x1, x2, w, b, c).permute(0, 2, 3, 1)
    t, s = C.c_int32(), C.c_int32()
    L.load().mf_wino_plan_query(C.byref(_desc(c)), C.byref(t), C.byref(s))
    worst, by_sk = 0.0, {}
    dg = Digest(f"real/{c.name}/{cancelling}")
    for tile, sk in _plans(c):
        eff = s.value if tile == 0 else WC.slices(WC.gemm_case(c), sk)[3]
        E = WC.real_bound(x1, x2, w, b, c, eff).permute(0, 2, 3, 1)
        y = _wino(ops, tile, sk)
        r = float(((y.cpu().double() - y64).abs() / E).max())
        worst = max(worst, r)
        assert r < 1.0, (c.name, tile, sk, r)
        if tile:
            if sk in by_sk:
                assert torch.equal(y, by_sk[sk][1]), (c.name, sk, by_sk[sk][0], tile, _first_diff(y, by_sk[sk][1]))
            else:
                by_sk[sk] = (tile, y)
                dg.add(y)
    dg.done()
    print(f"[measured] wino real bound {c.name} cancelling={cancelling}: worst fraction of the bound {worst:.3f} (c = {WC.real_bound_c(c)} x 2^-24 unsplit)")


# ------------------------------------------------------------------------------------------------ D. the tail
class TailOps:
    """device operands of a tail case; residual() makes a fresh tensor of the case's kind (pairs only / slot maxima / plain fp32) for every call"""

    def __init__(self, t, dev, bias=True):
        self.t, self.dev = t, dev
        c = t.c
        self.x1, self.w, self.b = WC.small_operands(c, bias=bias)
        self.ops = Ops(c, self.x1, None, self.w, self.b if bias else None, dev)
        self.gamma, self.beta, self.res, self.wide = WC.tail_side_operands(t)
        self.gd, self.bd = (self.gamma.to(dev), self.beta.to(dev)) if t.affine else (None, None)
        self.emb = GC.emb_of(self.wide) if t.emb else None
        self.embd = GC.emb_of(self.wide.to(dev)) if t.emb else None
        self.y = WC.want32(self.x1, None, self.w, self.b if bias else None, c).permute(0, 2, 3, 1).contiguous()      # the exact y, NHWC fp32
        rb = self.res.abs().amax(dim=(1, 2, 3)) if t.res else None
        self.bconst, self.ob = WC.tail_bounds(t, self.gamma, self.beta, rb, self.emb)

    def residual(self, res=None):
        t = self.t
        if t.res is None:
            return None
        r = (self.res if res is None else res).to(self.dev)
        if t.res == "pairs":
            K.split_of(r)
            r._mf_pairs_only = True
        elif t.res == "slots":
            r._mf_slots = WC.slot_table(self.res, t.nslots).to(self.dev)
            K._stamp(r)
        return r

    def run(self, a1=None, residual="own", want_wino=None):
        t = self.t
        return K.conv2d_wino_gn_apply(self.ops.a1 if a1 is None else a1, self.ops.uh, self.ops.b, _desc(t.c), self.gd, self.bd, t.G, GC.EPS, act=t.act,
                                      residual=self.residual() if isinstance(residual, str) else residual, emb=self.embd,
                                      emb_stride=self.embd.stride(0) if t.emb else 0, bconst=self.bconst, out_fp32=t.out_fp32,
                                      want_wino=t.want_wino if want_wino is None else want_wino)

    def three_launch(self):
        t, d = self.t, _desc(self.t.c)
        parts = K.wino_gn_parts(d, t.G)
        y, partial = K.conv2d_wino_f16x2(self.ops.a1, self.ops.uh, self.ops.b, d, gn_groups=t.G, gn_parts=parts)
        return K.gn_apply(y, K.GnPartials(partial, parts, GC.EPS), self.gd, self.bd, t.G, t.act, self.residual(), self.embd, self.embd.stride(0) if t.emb else 0,
                          split=True, bconst=self.bconst, out_fp32=t.out_fp32)


def _values(out, fp32):
    """the values of a tail output [N, H, W, C] on the CPU, fp64: its fp32 form, or -- pairs only -- its decoded pairs"""
    return out.cpu().double() if fp32 else _decode(out._mf_split, out._mf_bound)


def _stand_alone_v(out, dev):
    n, h, w, c = out.shape
    return _wino_input_raw(out._mf_split, out._mf_bound, n, h, w, c, dev)


@pytest.mark.parametrize("t", WC.TAIL_CASES, ids=lambda t: t.c.name)
def test_the_tail_on_an_exact_y(dev, t):
    """y is exact (the CPU test asserts it), so the output is held element-wise to groupnorm_cases.bound_E of the fp64 chain on THAT y -- samples 2^6
    apart, the residual scaled the other way round -- and the side outputs exactly: out_bound == bconst + rb + eb in the kernel's fp32 order,
    wino_bound == 4 out_bound for all 16 k, the pair mirror == the pair form of the fp32 output, V == the stand-alone transform of the pair output"""
    c = t.c
    assert K.wino_tail_ok(_desc(c), t.G) and WC.tail_ok(c, t.G)
    o = TailOps(t, dev)
    got = o.run()
    tm = GC.ref_terms(o.y, t.G, o.gamma, o.beta, t.act, o.res, o.emb)
    E = GC.bound_E(tm, res_pairs=t.res == "pairs")
    vals = _values(got, t.out_fp32)
    if not t.out_fp32:
        assert K.pairs_only(got)
        E = E + 2.0 ** -23 * tm["out"].abs() + 2.0 ** -50 * o.ob.double().view(-1, 1, 1, 1)          # the pair form of the result (test_split_f16x2_format)
    ratios = GC.ratio_rows(vals, tm, E)
    print(f"[measured] wino tail {c.name}: worst fraction of bound_E per sample {max(ratios):.3f}")
    assert all(r < 1.0 for r in ratios), (c.name, ratios)
    assert torch.equal(got._mf_bound.cpu(), o.ob), (got._mf_bound.cpu(), o.ob)
    dg = Digest(f"tail/{c.name}")
    dg.add(got._mf_split)
    if t.out_fp32:
        dg.add(got)
        hi, lo = _halves(got._mf_split)
        for n in range(c.N):
            _, whi, wlo = WC.pair_terms(got[n].cpu(), float(o.ob[n]))
            assert torch.equal(hi[n], whi) and torch.equal(lo[n], wlo), (c.name, n)
    if t.want_wino:
        assert torch.equal(got._mf_wino_bound.cpu().view(16, c.N), (4.0 * o.ob).expand(16, c.N))
        v, vb = _stand_alone_v(got, dev)
        assert torch.equal(vb, got._mf_wino_bound) and torch.equal(v, got._mf_wino), (c.name, _first_diff(got._mf_wino, v))
        dg.add(v)
        off = o.run(want_wino=False)                                      # the other setting of want_wino: the same result, no V
        assert torch.equal(off._mf_split, got._mf_split) and getattr(off, "_mf_wino", None) is None
    else:
        assert getattr(got, "_mf_wino", None) is None
        on = o.run(want_wino=True)
        v, vb = _stand_alone_v(on, dev)
        assert torch.equal(on._mf_split, got._mf_split) and torch.equal(v, on._mf_wino) and torch.equal(vb, on._mf_wino_bound)
    dg.done()


@pytest.mark.parametrize("t", WC.TAIL_CASES, ids=lambda t: t.c.name)
def test_the_tail_equals_the_three_launch_form_bit_for_bit(dev, t):
    """Without the bias y is a small integer in its unit: S and Q are exact in both forms (wino_cases.tail_sums_exact, asserted on the CPU), both state
    mean = S / count, var = Q / count - mean mean, rstd = float(1 / sqrt(var + eps)) in fp64 and the same fp32 operations per element in the same order
    (winograd.h:426-431,479-492; groupnorm.hip:290-294,339-352).  Whether either contracts the variance was decided from the build flag
    -ffp-contract=off (build.py), which holds for every unit, and from a disassembly of the two code objects, which hold the same fp64
    instruction counts (12 v_fma_f64 and 6 v_div_fixup / v_div_fmas each -- the expansions of the divisions; 6 v_mul_f64, one more in the tail for
    its own count = HW cpg): the same source line compiled the same way in both, so bit for bit applies and there is no rstd allowance.  Without an activation (no device sigmoid) the same holds against an fp32 restatement in torch,
    whose mean is the fp64 mean rounded once."""
    c = t.c
    o = TailOps(t, dev, bias=False)
    got, ref = o.run(), o.three_launch()
    assert torch.equal(got._mf_bound, ref._mf_bound) and torch.equal(got._mf_split, ref._mf_split), (c.name, _first_diff(got._mf_split, ref._mf_split))
    if t.out_fp32:
        assert torch.equal(got, ref), (c.name, _first_diff(got, ref))
    if t.act == 0 and t.out_fp32 and t.res != "pairs":
        y = o.y.double().reshape(c.N, c.H * c.W, t.G, c.Cout // t.G)
        count = float(c.H * c.W * (c.Cout // t.G))
        mean_d = y.sum(dim=(1, 3)) / count
        var = ((y * y).sum(dim=(1, 3)) / count - mean_d * mean_d).clamp_min(0.0)
        rstd = (1.0 / torch.sqrt(var + GC.EPS)).float()
        rep = lambda v: v.repeat_interleave(c.Cout // t.G, dim=1).view(c.N, 1, 1, c.Cout)
        e = (o.y - rep(mean_d.float())) * rep(rstd)
        if t.affine:
            e = e * o.gamma.view(1, 1, 1, -1)
            e = e + o.beta.view(1, 1, 1, -1)
        if t.res:
            e = e + o.res
        if t.emb:
            e = e + o.emb.reshape(c.N, 1, 1, c.Cout)
        assert torch.equal(got.cpu(), e), (c.name, _first_diff(got.cpu(), e))
    dg = Digest(f"tail3/{c.name}")
    dg.add(got._mf_split)
    dg.done()


def test_the_tail_on_a_constant_group(dev):
    """zero weights and a constant bias: every group is constant, Q / count - mean^2 is a rounding residue of either sign and reaches the clamp; every
    output -- fp32, pairs, V -- is finite"""
    t = WC.TAIL_CASES[1]
    c = t.c
    o = TailOps(t, dev)
    o.ops = Ops(c, o.x1, None, torch.zeros_like(o.w), torch.full((c.Cout,), 0.1, dtype=torch.float64), dev)
    got = o.run()
    assert bool(torch.isfinite(got).all()) and all(bool(torch.isfinite(h).all()) for p in (got._mf_split, got._mf_wino) for h in _halves(p))
    assert torch.equal(got._mf_bound.cpu(), o.ob)


def test_the_tail_confines_non_finite_values(dev):
    """a NaN input pixel poisons its own sample only; a NaN residual element (under the clean residual's bound) poisons that element of the output,
    of the pair mirror and the V components that read it, nothing else"""
    t = WC.TAIL_CASES[1]._replace(res="f32")
    c = t.c
    o = TailOps(t, dev)
    clean = o.run()
    a1 = o.ops.a1.clone()
    a1[2, 3, 5, 7] = float("nan")
    got = o.run(a1=a1)
    others = [n for n in range(c.N) if n != 2]
    assert bool(got[2].isnan().all())
    for name in ("_mf_split", "_mf_bound"):
        assert torch.equal(getattr(got, name)[others], getattr(clean, name)[others]), name
    assert torch.equal(got[others], clean[others]) and torch.equal(got._mf_wino[:, others], clean._mf_wino[:, others])
    assert torch.equal(got._mf_wino_bound.view(16, c.N)[:, others], clean._mf_wino_bound.view(16, c.N)[:, others])
    # the residual
    n, py, px, ch = 1, 4, 7, 9
    r = o.res.clone()
    r[n, py, px, ch] = float("nan")
    rd = r.to(dev)
    K._attach(rd, bound=o.res.abs().amax(dim=(1, 2, 3)).to(dev))
    got = o.run(residual=rd)
    bad = torch.zeros(got.shape, dtype=torch.bool)
    bad[n, py, px, ch] = True
    assert torch.equal(got.isnan().cpu(), bad) and torch.equal(got[~bad.to(dev)], clean[~bad.to(dev)])
    hi, lo = _halves(got._mf_split)
    assert torch.equal(~(torch.isfinite(hi) & torch.isfinite(lo)), bad)
    assert _same_halves(got._mf_split, clean._mf_split, ~bad) and torch.equal(got._mf_bound, clean._mf_bound)
    vbad = torch.zeros(got._mf_wino.shape, dtype=torch.bool)
    for tile, k in _patch_components(c.H, c.W, py, px):
        vbad[k, n, tile, ch] = True
    hi, lo = _halves(got._mf_wino)
    assert torch.equal(~(torch.isfinite(hi) & torch.isfinite(lo)), vbad)
    assert _same_halves(got._mf_wino, clean._mf_wino, ~vbad)


def test_the_wrappers_refuse_sizes_that_disagree_with_the_descriptor(dev):
    """kernels.check_wino in front of the three wrappers, on device tensors (tests/test_wino_edges_cpu.py walks every size)"""
    t = WC.TAIL_CASES[1]
    o = TailOps(t, dev)
    d = _desc(t.c)
    with pytest.raises(RuntimeError, match="x1"):
        K.conv2d_wino_f16x2(o.ops.a1[:-1], o.ops.uh, o.ops.b, d)
    with pytest.raises(RuntimeError, match="residual"):
        K.conv2d_wino_gn_apply(o.ops.a1, o.ops.uh, o.ops.b, d, o.gd, o.bd, t.G, GC.EPS, residual=o.ops.a1)
    with pytest.raises(RuntimeError, match="emb_stride"):
        K.conv2d_wino_gn_apply(o.ops.a1, o.ops.uh, o.ops.b, d, o.gd, o.bd, t.G, GC.EPS, emb=o.embd, emb_stride=t.c.Cout)
    with pytest.raises(RuntimeError, match="weights"):
        K.conv2d_wino_gn_apply_f32(o.ops.a1, o.ops.u[:8], o.ops.b, _desc(t.c, precision=0), o.gd, o.bd, t.G, GC.EPS)


# ------------------------------------------------------------------------------------------------ E. the fp32 form
@pytest.mark.parametrize("prec", [0, 3])
@pytest.mark.parametrize("cg", WC.F32_CASES, ids=lambda cg: cg[0].name)
def test_the_fp32_form_on_exact_operands(dev, cg, prec):
    """precision 0 (fp32 matrix cores) and 3 (bf16 triplets: the three terms hold U and V of these families exactly and the dropped products are zero):
    the component GEMM returns float32 of the fp64 products bit for bit on every family, the tail's output lies within bound_E of the fp64 chain on the
    exact y, and its fp32 V equals wino_input_f32 of its output bit for bit.  rows % 64 at its edge (64 rows), cpg = 4 (cq = 1), H = W = 2"""
    c, G = cg
    assert K.wino_f32_ok(_desc(c, precision=prec), G)
    dg = Digest(f"f32/{c.name}/{prec}")
    T = WC.tiles_of(c)
    for family, ratio in WC.variants(c):
        x1, x2, w, b = WC.wino_operands(c, family, ratio)
        a1, a2 = _nhwc(x1, dev), _nhwc(x2, dev)
        u = K.wino_pack_weight(w.float().to(dev))
        up = K.split_conv_weight(u) if prec == 3 else u
        g = K.make_conv_desc(16 * c.N, 1, T, c.C1, c.C2, c.Cout, 1, 1, 0, 3, precision=prec)
        v1, v2 = K.wino_input_f32(a1), (K.wino_input_f32(a2) if a2 is not None else None)
        m = K.conv2d(v1.view(16 * c.N, 1, T, c.C1), up, None, g, x2=None if v2 is None else v2.view(16 * c.N, 1, T, c.C2))
        x = torch.cat([x1, x2], 1) if x2 is not None else x1
        m64 = torch.einsum("kntc,koc->knto", WC.V64(x), WC.U64(w))
        assert torch.equal(m.view(16, c.N, T, c.Cout).cpu().double(), m64), (c.name, family, ratio, prec)
        gamma, beta, res, wide = WC.tail_side_operands(WC.Tail(c, G, "f32", 0, True, True, 1, True, True))
        embd = GC.emb_of(wide.to(dev))
        got = K.conv2d_wino_gn_apply_f32(a1, up, b.float().to(dev), _desc(c, precision=prec), gamma.to(dev), beta.to(dev), G, GC.EPS, act=1, residual=res.to(dev),
                                         emb=embd, emb_stride=embd.stride(0), x2=a2, want_wino=True)
        y = WC.want32(x1, x2, w, b, c).permute(0, 2, 3, 1).contiguous()
        tm = GC.ref_terms(y, G, gamma, beta, 1, res, GC.emb_of(wide))
        ratios = GC.ratio_rows(got.cpu(), tm, GC.bound_E(tm))
        assert all(r < 1.0 for r in ratios), (c.name, family, prec, ratios)
        v = got._mf_wino_f32
        assert torch.equal(K.wino_input_f32(got.clone()), v)
        assert torch.equal(v.cpu(), WC.V32(got.cpu().permute(0, 3, 1, 2)))                # (the transform's own additions, in fp32)
        dg.add(got)
    dg.done()


def test_the_fp32_form_refuses_what_it_cannot_do(dev):
    for c, G in WC.F32_REFUSED:
        for prec in (0, 3):
            assert not K.wino_f32_ok(_desc(c, precision=prec), G) and not WC.f32_ok(c, G, prec), (c.name, prec)
    c, G = WC.F32_CASES[0]
    assert not K.wino_f32_ok(_desc(c, precision=5), G) and not K.wino_f32_ok(_desc(c, precision=4), G)
    lib = L.load()
    for (n, h, w, ch, G) in ((4, 8, 8, 64, 32), (1, 64, 64, 512, 32), (2, 32, 32, 256, 8)):   # cpg = 2; 64 x 64 x 16 channels; 32 x 32 x 32 channels
        m = torch.zeros((16, n, (h // 2) * (w // 2), ch), dtype=torch.float32, device=dev)
        out = torch.zeros((n, h, w, ch), dtype=torch.float32, device=dev)
        rc = lib.mf_wino_tail_f32(m.data_ptr(), None, None, None, None, None, 0, out.data_ptr(), None, n, h, w, ch, G, 1, 1e-5, K.stream())
        assert rc == -2 and not bool(out.any()), (n, h, w, ch, G, rc)
