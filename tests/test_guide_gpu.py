"""The guidance stage's kernels (mf_guide_f32: csrc/guide.hip) on a real MI355X, the library entry directly, on the seeded cases of
tests/guide_cases.py: the limit bit for bit against the exact order statistics of the fp32 x_0 chain, the rescale factor within one fp32 ulp of the
fp64 restatement, the prediction within the derived element bound (and bit for bit against the fp32 chain), the bare combine bit for bit, and the
same bits whatever the load path, the batch, the row's place or the launch.  Every comparison prints a [measured] line
(profiles/guide_parity_measured.txt holds one run's)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from tests import guide_cases as GC

CASES = GC.all_cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _place(rows, dev, offset):
    """[B][n] host rows -> a contiguous [B, n] device tensor that starts `offset` elements into its buffer (offset 1: a 4-byte offset, nothing is
    16-byte aligned, the element-wise path)"""
    B, n = len(rows), rows[0].numel()
    buf = torch.empty(B * n + offset + 3, dtype=torch.float32, device=dev)
    view = buf[offset: offset + B * n].view(B, n)
    view.copy_(torch.stack(rows))
    assert view.data_ptr() % 16 == (4 * offset) % 16 and view.is_contiguous()
    return view


def _stages(case, pair):
    return (L.GUIDE_RESCALE if (case["phi"] > 0 and pair) else 0) | (L.GUIDE_THRESHOLD if case["q"] is not None else 0)


def _table(case, dev, rows_before=0, g=None):
    row = L.MfGuideStep(case["g"] if g is None else g, case["phi"], 0.0 if case["q"] is None else case["q"], 0.0 if case["s_max"] is None else case["s_max"],
                        case["a"], case["b"], 500, 0)
    junk = L.MfGuideStep(float("nan"), 0.5, 0.125, 0.0, float("nan"), float("nan"), 0, 0)
    return K.guide_table([junk] * rows_before + [row], dev)


def _run(case, rows, dev, offset=None, in_place=False, step=0, table=None):
    """-> (out [B, n], scale [B], limit [B]) on the host"""
    offset = case["offset"] if offset is None else offset
    pair = rows[0][1] is not None
    pc = _place([r[0] for r in rows], dev, offset)
    pu = _place([r[1] for r in rows], dev, offset) if pair else None
    xt = _place([r[2] for r in rows], dev, offset)
    out = None if in_place else _place([torch.zeros_like(r[0]) for r in rows], dev, offset)
    B = len(rows)
    scale, limit = torch.full((B,), -7.0, device=dev), torch.full((B,), -7.0, device=dev)
    got = K.guide(pc, _table(case, dev) if table is None else table, pred_uncond=pu, x_t=xt, step=step, objective=case["objective"], stages=_stages(case, pair),
                  out=out, scale_out=scale, limit_out=limit)
    assert (got is pc) if in_place else (got is out)
    return got.cpu(), scale.cpu(), limit.cpu()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. exact limit, k within one ulp, the element bound
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_limit_is_exact_scale_within_one_ulp_prediction_within_its_bound(dev, case):
    rows = GC.case_rows(case)
    pair = rows[0][1] is not None
    stages = _stages(case, pair)
    out, scale, limit = _run(case, rows, dev)
    worst = 0.0
    for b, (pc, pu, xt) in enumerate(rows):
        rescale, thr = bool(stages & L.GUIDE_RESCALE), bool(stages & L.GUIDE_THRESHOLD)
        r = GC.restate(pc, pu, xt, case["g"], case["phi"] if rescale else 0.0, case["q"], case["s_max"], case["a"], case["b"], case["objective"])
        k = float(scale[b])
        if rescale:
            assert abs(k - r["k"]) <= GC.scale_bound(r["k"]), (case["name"], b, k, r["k"])
        else:
            assert k == 1.0
        want, s, _ = GC.chain32(pc, pu, xt, case["g"], k if rescale else None, case["q"], case["s_max"], case["a"], case["b"], case["objective"])
        if thr:
            # bit for bit: the fp32 rounding of the fp64 interpolation between the EXACT order statistics of the fp32 x_0 chain
            assert _same_bits(limit[b], s), (case["name"], b, float(limit[b]), float(s))
            assert float(limit[b]) >= 1.0 and (case["s_max"] is None or float(limit[b]) <= case["s_max"])
        else:
            assert float(limit[b]) == 0.0
        bound = GC.element_bound(r, pc, pu, xt, case["g"], case["a"], case["b"], case["objective"], rescale, thr)
        ratio = float(((out[b].double() - r["out"]).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (case["name"], b, ratio)
        assert _same_bits(out[b], want), (case["name"], b, "the fp32 chain", int((out[b] != want).sum()))
    print(f"[measured] guide {case['name']}: largest |pred_out - fp64| / bound {worst:.3f}; k {[round(float(v), 7) for v in scale]}, "
          f"s {[round(float(v), 7) for v in limit]}")


# ------------------------------------------------------------------------------------------------ 2. no stage: the bare combine
@pytest.mark.parametrize("n,B", GC.SHAPES)
def test_without_a_stage_the_combine_is_the_step_launches_chain_bit_for_bit(dev, n, B):
    case = dict(g=GC.f32(8.0), phi=0.0, q=None, s_max=None, objective=0, offset=1 if n in (36, 33) else 0, **GC.SCHED)
    rows = [GC.contents("normal", n, 77 + b) for b in range(B)]
    out, scale, limit = _run(case, rows, dev)
    g = torch.tensor(case["g"])
    for b, (pc, pu, _) in enumerate(rows):
        assert _same_bits(out[b], pu + g * (pc - pu))          # fl(pu + fl(g fl(pc - pu)))
    assert scale.tolist() == [1.0] * B and limit.tolist() == [0.0] * B
    single = [(pc, None, xt) for pc, _, xt in rows]           # without a pair the prediction passes through
    out, _, _ = _run(case, single, dev)
    assert _same_bits(out, torch.stack([r[0] for r in rows]))


# ------------------------------------------------------------------------------------------------ 3. the same bits, whatever surrounds the row
@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("n", sorted({n for n, _ in GC.SHAPES}))
def test_bits_do_not_depend_on_load_path_batch_place_launch_or_aliasing(dev, n, objective):
    case = dict(name="bits", n=n, B=3, kind="normal", objective=objective, g=GC.f32(8.0), phi=GC.f32(0.7), q=GC.f32(0.995), s_max=None, offset=0, **GC.SCHED)
    rows = GC.case_rows(case)
    base = _run(case, rows, dev, offset=0)
    again = _run(case, rows, dev, offset=0)
    for a, b in zip(base, again):
        assert _same_bits(a, b)                                                  # two launches
    shifted = _run(case, rows, dev, offset=1)                                   # nothing 16-byte aligned: element by element
    for a, b in zip(base, shifted):
        assert _same_bits(a, b)
    alias = _run(case, rows, dev, offset=0, in_place=True)                      # pred_out == pred
    for a, b in zip(base, alias):
        assert _same_bits(a, b)
    back = _run(case, rows[::-1], dev, offset=0)                                # the row's place
    for a, b in zip(base, back):
        assert _same_bits(a, b.flip(0))
    alone = _run(case, rows[1:2], dev, offset=0)                                # the batch
    for a, b in zip(base, alone):
        assert _same_bits(a[1:2], b)
    big = _run(case, rows + rows + rows[:1], dev, offset=0)
    for a, b in zip(base, big):
        assert _same_bits(a, b[:3]) and _same_bits(a, b[3:6])


# ------------------------------------------------------------------------------------------------ 4. the step index and the table
def test_the_step_comes_from_the_host_or_the_device_counter(dev):
    for n in (36, GC.ONE_WG + 4):
        case = dict(name="step", n=n, B=2, kind="normal", objective=0, g=GC.f32(3.0), phi=GC.f32(0.5), q=GC.f32(0.5), s_max=GC.f32(2.0), offset=0, **GC.SCHED)
        rows = GC.case_rows(case)
        want = _run(case, rows, dev)
        table = _table(case, dev, rows_before=2)                                  # rows 0 and 1 hold NaN scales and another quantile
        host = _run(case, rows, dev, step=2, table=table)
        word = torch.tensor([2, 0], dtype=torch.int32, device=dev)
        devc = _run(case, rows, dev, step=word[:1], table=table)
        assert word.tolist() == [2, 0]                                            # the stage reads the counter, it never advances it
        for a, b, c in zip(want, host, devc):
            assert _same_bits(a, b) and _same_bits(a, c)
        other = _run(case, rows, dev, table=_table(case, dev, g=GC.f32(5.0)))
        assert not _same_bits(other[0], want[0])


# ------------------------------------------------------------------------------------------------ 5. a NaN is one more large magnitude
@pytest.mark.parametrize("n", [36, GC.ONE_WG, 2 * GC.ONE_WG + 12])
def test_a_nan_sorts_above_infinity_and_does_not_poison_the_row(dev, n):
    case = dict(name="nan", n=n, B=1, kind="normal", objective=1, g=GC.f32(1.0), phi=0.0, q=GC.f32(0.5), s_max=None, offset=0, **GC.SCHED)
    pc, _, xt = GC.contents("normal", n, 9)
    pc = pc * 3.0
    clean, _, limit0 = _run(case, [(pc, None, xt)], dev)
    bad = pc.clone()
    top = int(pc.abs().argmax())
    bad[top] = float("nan")                     # the largest magnitude becomes a NaN: every rank below it keeps its value
    out, _, limit = _run(case, [(bad, None, xt)], dev)
    assert _same_bits(limit, limit0) and float(limit) > 1.0
    assert bool(torch.isnan(out[0, top])) and int(torch.isnan(out).sum()) == 1
    keep = torch.ones(n, dtype=torch.bool)
    keep[top] = False
    assert _same_bits(out[0][keep], clean[0][keep])
