"""The quantizer (csrc/vq.hip), the window kernels (csrc/window_ops.hip) and the held-out loss kernels (csrc/loss.hip) on a real MI355X at the
path boundaries their feature tests never reach, against the exact references of tests/small_edge_cases.py (premises proved in
tests/test_small_edges_cpu.py): every C of the search, every slicing regime, slices that are no whole number of chunks; grid-stride loops past
their 2048-workgroup cap on both load widths, 32 origins on an axis, dense covers; the loss rows' second finish block, grid.y = 65535, the
chunk regime above 2 Mi elements per row, pooling by 3, the sample index across 2^32.  Outputs that the wrappers let the caller provide lie
between sentinel floats; the ones the wrappers allocate land in a block that was filled with NaN just before.
Measured on an MI355X: profiles/small_edges_measured.txt."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import kernels as K
from medfusion_amd.window import WindowPlan
from oracle import restate as R
from tests import small_edge_cases as E
from tests import val_cases as V
from tests import window_cases as WC
from tests.util import offset_view

T_ = 1000
I32 = torch.int32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sch():
    return M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())


class Guarded:
    """an fp32 output of `shape` prefilled with the sentinel, four sentinel floats before it (one when `shifted`: the tensor then starts 4 bytes off
    a 16-byte boundary) and GUARD behind it"""

    def __init__(self, shape, dev, shifted=False):
        self.n, self.off = E.prod(shape), 1 if shifted else 4
        self.buf = torch.full((self.off + self.n + E.GUARD,), E.SENTINEL, device=dev)
        self.t = self.buf[self.off:self.off + self.n].view(tuple(shape))
        assert self.t.data_ptr() % 16 == (4 if shifted else 0) and self.t.is_contiguous()

    def intact(self) -> bool:
        return bool((torch.cat([self.buf[:self.off], self.buf[self.off + self.n:]]) == E.SENTINEL).all())

    def untouched(self) -> bool:
        return bool((self.buf == E.SENTINEL).all())


def poison(dev, numel):
    """fill a block of `numel` doubles with NaN and free it: the caching allocator hands it to the next request of that size, the [B, values]
    result a loss wrapper allocates -- a row the finish launch does not write then reads NaN"""
    torch.full((numel,), float("nan"), dtype=torch.float64, device=dev)


def bits(t):
    return t.contiguous().view(I32)


# ================================================================================================ 1. the quantizer
_VQ = {}


def vq_case(name):
    if name not in _VQ:
        c = E.vq_dyadic_case(name)
        c["rows"] = E.pixel_subset(c["P"])
        c["di"] = E.int_distances(c["zi"][c["rows"]], c["ci"])
        c["want"] = torch.argmin(c["di"], dim=1)                                           # the first minimum: the lowest index
        _VQ[name] = c
    return _VQ[name]


@pytest.mark.parametrize("name", list(E.VQ_CASES))
def test_quantizer_is_the_integer_argmin_on_the_dyadic_grid(dev, name):
    c = vq_case(name)
    n, ch, h, w = c["z"].shape
    z, cb = c["z"].to(dev), c["cb"].to(dev)
    zq, idx, sq = K.vector_quantize(z, cb, want_idx=True, want_sqerr=True)
    got = idx.cpu().long()
    assert idx.dtype == I32 and got.shape == (c["P"],) and int(got.min()) >= 0 and int(got.max()) < c["K"]
    wrong = int((got[c["rows"]] != c["want"]).sum())
    ties = int((c["di"] == c["di"].min(1, keepdim=True).values).sum(1).gt(1).sum())
    total = int(((c["ci"][got] - c["zi"]) ** 2).sum())
    print(f"[measured] vq exact {name}: S={c['S']} slices={c['slices']} {len(c['pairs'])} planted boundaries, {c['rows'].numel()} of {c['P']} pixels "
          f"checked, {ties} with an exact tie, {wrong} wrong indices; sqerr {float(sq)!r} vs {total / 4096.0!r}")
    assert wrong == 0
    zq_want = torch.moveaxis(c["cb"][got].view(n, h, w, ch), -1, 1)
    assert torch.equal(bits(zq.cpu()), bits(zq_want))                          # z + (e - z) is e itself on the grid, every pixel
    assert float(sq) == total / 4096.0                                           # multiples of 2^-12: the fp64 sum is exact in any order
    zq2, idx2, sq2 = K.vector_quantize(z, cb)
    assert idx2 is None and sq2 is None and torch.equal(bits(zq2), bits(zq))
    zq3, idx3, _ = K.vector_quantize(z, cb, want_idx=True)
    assert torch.equal(bits(zq3), bits(zq)) and torch.equal(idx3, idx)
    zq4, _, sq4 = K.vector_quantize(z, cb, want_sqerr=True)
    assert torch.equal(bits(zq4), bits(zq)) and torch.equal(sq4, sq)


RANDOM_VQ = [(k, c) for k in (1, 1000, 8192, 16384) for c in (1, 3, 4, 8, 16)] + [(65, 2), (200, 7), (8193, 13), (10000, 5), (1500, 11)]


@pytest.mark.parametrize("K_,C", RANDOM_VQ)
def test_quantizer_index_is_the_argmin_of_the_stated_arithmetic_near_ties_included(dev, K_, C):
    """random floats (the adversarial inputs of tests/test_vq_gpu.py): the header states the distance operation by operation, so the index is the
    first minimum of that chain evaluated on the CPU on EVERY finite pixel -- not only where the margin is clear"""
    z, cb = E.adversarial(K_, C, (3, C, 7, 11), 1000 * K_ + C)
    _, idx, _ = K.vector_quantize(z.to(dev), cb.to(dev), want_idx=True)
    d = E.cpu_formula(z, cb)
    want = torch.argmin(d, dim=1)
    finite = torch.isfinite(torch.moveaxis(z, 1, -1).reshape(-1, C)).all(1)
    got = idx.cpu().long()
    wrong = int((got[finite] != want[finite]).sum())
    print(f"[measured] vq random K={K_} C={C}: {int(finite.sum())} finite pixels, {wrong} indices differ from the argmin of the stated arithmetic")
    assert wrong == 0


# ================================================================================================ 2. the windows
def _plans(case, weight="tent"):
    return WindowPlan(case["canvas"], case["window"], case["stride"], weight), E.ref_plan(case, weight)


@pytest.mark.parametrize("name", list(E.GATHER_CASES))
def test_gather_is_slicing_bit_for_bit_on_both_load_widths(dev, name):
    case = E.GATHER_CASES[name]
    plan, ref = _plans(case)
    canvas = E.bits_input((case["B"], case["C"], *ref.canvas), 31)
    want = bits(WC.ref_gather(canvas, ref))
    d_canvas = canvas.to(dev)
    for shifted in (False, True):
        out = Guarded(want.shape, dev, shifted)
        got = K.window_gather(offset_view(d_canvas, shifted), plan, out=out.t)
        assert got.data_ptr() == out.t.data_ptr()
        wrong = int((bits(out.t.cpu()) != want).sum())
        print(f"[measured] window_gather {name} {'shifted' if shifted else 'aligned'}: {want.numel()} cells, {wrong} differ in bits")
        assert wrong == 0 and out.intact()


@pytest.mark.parametrize("weight", ["uniform", "tent"])
@pytest.mark.parametrize("name", list(E.MERGE_CASES))
def test_merge_is_the_correctly_rounded_quotient_on_the_dyadic_grid(dev, name, weight):
    """integer weights, p = k / 16: numerator and denominator are exact in fp32, so every cell is float32(acc / den) -- the fp64 merge rounded
    once -- bit for bit, on both load widths"""
    case = E.MERGE_CASES[name]
    plan, ref = _plans(case, weight)
    wins = E.dyadic_windows((case["B"] * ref.M, case["C"], *ref.window), 41)
    want = bits(WC.ref_merge(wins, ref, torch.float64).float())
    d_wins = wins.to(dev)
    for shifted in (False, True):
        out = Guarded(want.shape, dev, shifted)
        K.window_merge(offset_view(d_wins, shifted), plan, out=out.t)
        wrong = int((bits(out.t.cpu()) != want).sum())
        print(f"[measured] window_merge exact {name} / {weight} {'shifted' if shifted else 'aligned'}: {want.numel()} cells, cover up to {case['cover']}, "
              f"{wrong} differ from float32(acc / den)")
        assert wrong == 0 and out.intact()


@pytest.mark.parametrize("weight", ["uniform", "tent"])
@pytest.mark.parametrize("name", list(E.MERGE_CASES))
def test_merge_of_random_floats_within_the_bound_and_the_same_bits_on_both_widths(dev, name, weight):
    case = E.MERGE_CASES[name]
    plan, ref = _plans(case, weight)
    g = torch.Generator().manual_seed(43)
    wins = torch.randn((case["B"] * ref.M, case["C"], *ref.window), generator=g) * 1.7
    d_wins = wins.to(dev)
    got = K.window_merge(d_wins, plan)
    assert torch.equal(bits(K.window_merge(d_wins, plan)), bits(got))                       # a second launch
    out = Guarded(got.shape, dev, True)
    K.window_merge(offset_view(d_wins, True), plan, out=out.t)
    assert torch.equal(bits(out.t), bits(got)) and out.intact()                             # element by element
    worst = float(((got.cpu().double() - WC.ref_merge(wins, ref, torch.float64)).abs() / WC.merge_bound(wins, ref)).max())
    print(f"[measured] window_merge random {name} / {weight}: worst {worst:.3f} of (K + 2) 2^-24 max|p|")
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["cap", "clamped_vector", "clamped_element", "cover8_3d", "dense"])
def test_merge_copies_a_cell_under_one_window_bit_for_bit(dev, name):
    """windows of random BITS (NaN payloads, -0, infinities): a cover-1 cell is the window's word, no multiply, no divide"""
    case = E.MERGE_CASES[name]
    cover = E.ref_plan(case).cover()
    for weight in ("uniform", "tent"):
        plan, ref = _plans(case, weight)
        wins = E.bits_input((case["B"] * ref.M, case["C"], *ref.window), 47)
        want = torch.zeros((case["B"], case["C"], *ref.canvas))
        for b in range(case["B"]):
            for m in range(ref.M):
                want[(b, slice(None), *ref.slices(m))] = wins[b * ref.M + m]
        single = (cover == 1).expand_as(want)
        assert bool(single.any())
        for shifted in (False, True):
            out = Guarded(want.shape, dev, shifted)
            K.window_merge(offset_view(wins.to(dev), shifted), plan, out=out.t)
            assert torch.equal(bits(out.t.cpu())[single], bits(want)[single]) and out.intact(), (weight, shifted)


class TamperedPlan:
    """a plan whose descriptor is edited before the library sees it"""

    def __init__(self, plan, edit):
        self.plan, self.edit, self.canvas, self.window, self.M = plan, edit, plan.canvas, plan.window, plan.M

    def desc(self, B, C):
        d = self.plan.desc(B, C)
        self.edit(d)
        return d


def _set(**fields):
    def edit(d):
        for k, v in fields.items():
            if k == "origin2":
                for i, o in enumerate(v):
                    d.origin[2][i] = o
                d.count[2] = len(v)
            elif k in ("count2", "canvas0"):
                getattr(d, k[:-1])[int(k[-1])] = v
            else:
                setattr(d, k, v)
    return edit


# canvas (8, 24), window (8, 8), stride 8: origins (0, 8, 16) on the last axis
REFUSALS = [("origins33", _set(count2=33), r"axis 2: 33 origins \(1 \.\. 32\)"),
            ("gap", _set(origin2=(0, 16)), "axis 2: origins ascend strictly and leave no gap"),
            ("not_ascending", _set(origin2=(0, 8, 8, 16)), "axis 2: origins ascend strictly and leave no gap"),
            ("first_not_0", _set(origin2=(1, 8, 16)), "axis 2: the origins run from 0 to canvas - window"),
            ("last_not_at_the_edge", _set(origin2=(0, 8, 15)), "axis 2: the origins run from 0 to canvas - window"),
            ("dims4", _set(dims=4), r"dims=4 \(2 or 3\)"),
            ("leading_extent", _set(canvas0=2), "a 2-D descriptor has a leading extent of 1")]


@pytest.mark.parametrize("name,edit,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_descriptors_refusals_before_any_launch(dev, name, edit, message):
    plan = TamperedPlan(WindowPlan((8, 24), (8, 8), 8), edit)
    canvas, wins = torch.zeros((2, 3, 8, 24), device=dev), torch.zeros((6, 3, 8, 8), device=dev)
    out = Guarded(wins.shape, dev)
    with pytest.raises(RuntimeError, match=r"mf_window_gather_f32 failed \(code -1\): window_gather: " + message):
        K.window_gather(canvas, plan, out=out.t)
    assert out.untouched()
    out = Guarded(canvas.shape, dev)
    with pytest.raises(RuntimeError, match=r"mf_window_merge_f32 failed \(code -1\): window_merge: " + message):
        K.window_merge(wins, plan, out=out.t)
    assert out.untouched()


# ================================================================================================ 3. the held-out loss
def i32(values, dev):
    return torch.tensor(values, dtype=I32, device=dev)


def _diffuse_want(tb, x0, eps, ts):
    """fl32(fl32(a x) + fl32(c e)) with torch's separate fp32 ops; x_0 below 0, the draw from T on"""
    a, c = tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"]
    assert a.dtype == torch.float32 and c.dtype == torch.float32
    rows = []
    for b, t in enumerate(ts):
        if t < 0:
            rows.append(x0[b])
        elif t >= T_:
            rows.append(eps[b])
        else:
            p1, p2 = a[t] * x0[b], c[t] * eps[b]
            rows.append(p1 + p2)
    return torch.stack(rows)


DIFFUSE_T = [-1, T_, 0, T_ - 1]      # the rows of the second pass (the last ones) take a table row


@pytest.mark.parametrize("kind", ["vector", "vector_shifted", "element", "element_shifted"])
def test_diffuse_rows_past_the_grid_cap_bit_for_bit(dev, sch, kind):
    shape, shifted = E.DIFFUSE_CASES[kind.split("_")[0]], kind.endswith("shifted")
    g = torch.Generator().manual_seed(51)
    x0, eps = torch.randn(shape, generator=g) * 0.6, torch.randn(shape, generator=g)
    tbd = sch.device_tables(dev)
    want = bits(_diffuse_want(sch.host_tables(), x0, eps, DIFFUSE_T))
    out = Guarded(shape, dev, shifted)
    K.diffuse_rows(offset_view(x0.to(dev), shifted), i32(DIFFUSE_T, dev), tbd["sqrt_alphas_cumprod"], tbd["sqrt_one_minus_alphas_cumprod"],
                   eps=offset_view(eps.to(dev), shifted), out=out.t)
    wrong = int((bits(out.t.cpu()) != want).sum())
    print(f"[measured] diffuse_rows {kind} {shape}: {want.numel()} elements, t = {DIFFUSE_T}, {wrong} differ from fl(fl(a x) + fl(c e))")
    assert wrong == 0 and out.intact()


def test_diffuse_rows_draws_what_philox_normal_writes_past_the_cap(dev, sch):
    shape = E.DIFFUSE_CASES["vector"]
    g = torch.Generator().manual_seed(52)
    x0 = (torch.randn(shape, generator=g) * 0.6).to(dev)
    tbd = sch.device_tables(dev)
    a, c = tbd["sqrt_alphas_cumprod"], tbd["sqrt_one_minus_alphas_cumprod"]
    seed, draw, offset = 0x1234_5678_9ABC, 3, 11
    eps = K.philox_normal(torch.empty_like(x0), seed, draw, offset)
    want = bits(_diffuse_want(sch.host_tables(), x0.cpu(), eps.cpu(), DIFFUSE_T))
    out, stored = Guarded(shape, dev), Guarded(shape, dev)
    K.diffuse_rows(x0, i32(DIFFUSE_T, dev), a, c, philox=(seed, draw, offset), eps_out=stored.t, out=out.t)
    assert torch.equal(bits(stored.t), bits(eps)) and stored.intact()
    assert torch.equal(bits(out.t.cpu()), want) and out.intact()
    out2 = Guarded(shape, dev)
    K.diffuse_rows(x0, i32(DIFFUSE_T, dev), a, c, philox=(seed, draw, offset), out=out2.t)
    assert torch.equal(bits(out2.t), bits(out.t)) and out2.intact()


def test_the_sample_index_wraps_at_two_to_the_32(dev, sch):
    """mf_philox_normal_f32: sample_offset + b is taken mod 2^32, here and in every launch that regenerates the values -- rows 2 and 3 of a launch at
    offset 2^32 - 2 draw what rows 0 and 1 draw at offset 0"""
    shape = (4, 2, 4, 6)
    x0 = V.hash_rows("se.wrap", shape, 0.6).to(dev)
    tbd = sch.device_tables(dev)
    a, c = tbd["sqrt_alphas_cumprod"], tbd["sqrt_one_minus_alphas_cumprod"]
    t = i32([5, 900, 17, 400], dev)
    seed, draw, hi = 99, 4, 2 ** 32 - 2
    out, stored = Guarded(shape, dev), Guarded(shape, dev)
    K.diffuse_rows(x0, t, a, c, philox=(seed, draw, hi), eps_out=stored.t, out=out.t)
    low_e = torch.empty((2, *shape[1:]), device=dev)
    low = K.diffuse_rows(x0[2:], t[2:], a, c, philox=(seed, draw, 0), eps_out=low_e)
    assert torch.equal(bits(stored.t[2:]), bits(low_e)) and torch.equal(bits(out.t[2:]), bits(low)) and out.intact() and stored.intact()
    assert torch.equal(bits(stored.t), bits(K.philox_normal(torch.empty(shape, device=dev), seed, draw, hi)))
    assert torch.equal(bits(stored.t[:2]), bits(K.philox_normal(torch.empty((2, *shape[1:]), device=dev), seed, draw, hi)))
    assert not torch.equal(stored.t[:2], stored.t[2:])
    # the regenerated target of the error sums wraps the same way
    pred = V.hash_rows("se.wrap.p", shape).to(dev)
    whole = K.denoise_loss(pred, philox=(seed, draw, hi), target_shape=shape)
    assert torch.equal(whole, K.denoise_loss(pred, stored.t.clone()))
    assert torch.equal(whole[2:], K.denoise_loss(pred[2:], philox=(seed, draw, 0), target_shape=(2, *shape[1:])))


@pytest.mark.parametrize("per", list(E.ROW_SIZES))
def test_denoise_loss_is_exact_across_the_chunk_regimes(dev, per):
    """2 097 152: the last row of the 8192 regime, 256 partials; 2 097 156: chunk 9216, 228 partials, a last one of 5124, 16-byte loads;
    2 097 153: the same element by element, ending in a one-element quad.  On the grid both row sums are exact: bit for bit"""
    chunk, parts, last, tail = E.ROW_SIZES[per]
    shape = (2, *tail)
    pk, tk = E.dyadic_rows(shape, per), E.dyadic_rows(shape, per + 1)
    want = E.exact_loss_sums(pk, tk, 1)
    pred, target = (pk.float() * E.LOSS_GRID).to(dev), (tk.float() * E.LOSS_GRID).to(dev)
    poison(dev, 4)
    got = K.denoise_loss(pred, target)
    print(f"[measured] denoise_loss exact per={per}: chunk {chunk}, {parts} partials, last {last}; got {got.cpu().tolist()} want {want.tolist()}")
    assert torch.equal(got.cpu(), want)
    assert torch.equal(K.denoise_loss(offset_view(pred, True), offset_view(target, True)), got)


@pytest.mark.parametrize("shape,f", [((3, 2, 4, 4), 2), ((3, 2, 2, 2), 4), ((2, 2, 2, 2, 2), 2), ((2, 3, 1, 1, 1), 4)], ids=str)
def test_denoise_loss_is_exact_with_power_of_two_pooling(dev, shape, f):
    tshape = (*shape[:2], *(s * f for s in shape[2:]))
    pk, tk = E.dyadic_rows(shape, 61), E.dyadic_rows(tshape, 62)
    pred, target = (pk.float() * E.LOSS_GRID).to(dev), (tk.float() * E.LOSS_GRID).to(dev)
    for shifted in (False, True):
        assert torch.equal(K.denoise_loss(offset_view(pred, shifted), offset_view(target, shifted)).cpu(), E.exact_loss_sums(pk, tk, f))


@pytest.mark.parametrize("B", [65, E.ROWS_MAX])
def test_denoise_loss_rows_past_the_first_finish_block(dev, B):
    """one thread per row in blocks of 64: the second block, and the last admitted grid.y -- every row against its own exact sums"""
    shape = (B, 1, 2, 2)
    pk, tk = E.dyadic_rows(shape, 63), E.dyadic_rows(shape, 64)
    want = E.exact_loss_sums(pk, tk, 1)
    pred, target = (pk.float() * E.LOSS_GRID).to(dev), (tk.float() * E.LOSS_GRID).to(dev)
    poison(dev, 2 * B)
    got = K.denoise_loss(pred, target).cpu()
    wrong = (got != want).any(1).nonzero().flatten()
    print(f"[measured] denoise_loss B={B}: {wrong.numel()} rows differ from their exact sums (first {wrong[:4].tolist()})")
    assert got.shape == (B, 2) and wrong.numel() == 0


def test_more_rows_than_a_grid_admits_are_refused(dev):
    pred = torch.zeros((E.ROWS_MAX + 1, 1, 2, 2), device=dev)
    with pytest.raises(RuntimeError, match=r"mf_denoise_loss_f32 failed \(code -1\): denoise_loss: bad descriptor"):
        K.denoise_loss(pred, torch.zeros_like(pred))


@pytest.mark.parametrize("kind", ["unrelated", "close"])
@pytest.mark.parametrize("shape", [(2, 4, 3, 5), (2, 4, 2, 3, 5)], ids=str)
def test_denoise_loss_pooling_by_three(dev, shape, kind):
    """f = 3: the block mean is no exact division (held to loss_bound), and the Philox quads the regenerated target reads straddle block and row
    ends (rows of 15 values) -- stored and regenerated, aligned and shifted: the same bits"""
    f = 3
    tshape = (*shape[:2], *(s * f for s in shape[2:]))
    assert E.prod(tshape[1:]) % 4 == 0 and tshape[-1] % 4 != 0
    seed, draw, offset = 77, 2, 5
    target = K.philox_normal(torch.empty(tshape, device=dev), seed, draw, offset)
    noise = V.hash_rows(f"se.f3.{kind}", shape).to(dev)
    pool = torch.nn.functional.avg_pool2d if len(shape) == 4 else torch.nn.functional.avg_pool3d
    pred = noise if kind == "unrelated" else (pool(target, f) + 1e-3 * noise).contiguous()
    got = K.denoise_loss(pred, target)
    want, fields = V.loss_sums(pred.cpu(), target.cpu())
    ratio = float(((got.cpu() - want).abs() / V.loss_bound(fields)).max())
    print(f"[measured] denoise_loss {shape} f=3 {kind}: largest |sum - fp64| / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(K.denoise_loss(pred, philox=(seed, draw, offset), target_shape=tshape), got)
    assert torch.equal(K.denoise_loss(offset_view(pred, True), offset_view(target, True)), got)
    assert torch.equal(K.denoise_loss(offset_view(pred, True), philox=(seed, draw, offset), target_shape=tshape), got)
    assert torch.equal(K.denoise_loss(pred[1:2], philox=(seed, draw, offset + 1), target_shape=(1, *tshape[1:]))[0], got[1])


def _variance_inputs(shape, ts, tb, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda s=1.0: torch.randn(shape, generator=g) * s
    t = torch.tensor(ts)
    x0, xT, pv = r(0.5), r(), r(0.5).clamp(-1, 1)
    t_in = t.clamp(0, T_ - 1)                                   # (a row without a table row still needs an x_t to hand over)
    xt = V.diffuse(tb, x0, xT, t_in, torch.float32)
    return (x0, xt, xT, xT + 0.1 * r(), pv), t


def test_variance_loss_rows_past_the_first_finish_block(dev, sch):
    """B = 65: row 64 is the second finish block's; row 17 has no table row and is NaN -- every other row the bits of its own single-row call"""
    B, bad = 65, 17
    ts = [(37 * b) % T_ for b in range(B)]
    ts[bad] = T_
    args, t = _variance_inputs((B, 2, 4, 4), ts, sch.host_tables(), 71)
    tbd = sch.device_tables(dev)
    d_args, t32 = [v.to(dev) for v in args], t.to(dev, I32)
    poison(dev, 3 * B)
    got = K.variance_loss(*d_args, t32, tbd, 0, True)
    assert got.shape == (B, 3) and bool(got[bad].isnan().all())
    keep = [b for b in range(B) if b != bad]
    assert bool(got[keep].isfinite().all())
    for b in keep:
        assert torch.equal(K.variance_loss(*(v[b:b + 1] for v in d_args), t32[b:b + 1], tbd, 0, True)[0], got[b]), b


def test_variance_loss_above_two_mi_elements_per_row(dev, sch):
    """per-row length 2 097 156 (chunk 9216, 228 partials), held by the rule of tests/test_val_gpu.py: MARGIN x the distance of the fp32
    restatement from the fp64 one, computed here"""
    per = 2097156
    shape, ts = (1, *E.ROW_SIZES[per][3]), [417]
    tb, tbd = sch.host_tables(), sch.device_tables(dev)
    args, t = _variance_inputs(shape, ts, tb, 72)
    want64, want32 = (V.variance_sums(tb, *args, t, "x_T", True, d) for d in (torch.float64, torch.float32))
    d_args, t32 = [v.to(dev) for v in args], t.to(dev, I32)
    poison(dev, 3)
    got = K.variance_loss(*d_args, t32, tbd, 0, True)
    assert got.shape == (1, 3) and bool(got.isfinite().all())
    for k, what in enumerate(("kl", "nll", "var_scale")):
        d32, dk = float((want32[:, k].double() - want64[:, k]).abs().max()), float((got[:, k].cpu() - want64[:, k]).abs().max())
        print(f"[measured] variance_loss per={per} {what}: d32 {d32:.3e} kernel {dk:.3e} = {dk / (V.MARGIN * d32):.2e} of MARGIN x d32 (sum {float(want64[:, k].abs().max()):.6g})")
        assert dk <= V.MARGIN * d32, (what, dk, d32)
    assert torch.equal(K.variance_loss(*(offset_view(v, True) for v in d_args), t32, tbd, 0, True), got)
