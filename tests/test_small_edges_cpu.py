"""The premises and the restated host rules of tests/small_edge_cases.py, proved without a GPU: what tests/test_small_edges_gpu.py then holds the
quantizer, window and loss kernels to with no tolerance rests on these."""
import pytest
import torch

from medfusion_amd import lib as L
from medfusion_amd.window import WindowPlan
from tests import small_edge_cases as E
from tests import val_cases as V
from tests import window_cases as WC


# ------------------------------------------------------------------------------------------------ the quantizer
def test_plan_slices_restated_against_the_table():
    for (P, K), want in E.PLAN_TABLE.items():
        assert E.plan_slices(P, K) == want, (P, K)
    # the regimes the cases reach: 16 slices, the middle, one slice; whole and partial chunks; a one-code last slice
    counts = {name: E.vq_dyadic_case(name)["slices"] for name in ("C4", "K1", "K65", "K8193", "K10000", "three_slices", "one_slice")}
    assert counts == dict(C4=4, K1=1, K65=2, K8193=15, K10000=16, three_slices=3, one_slice=1)
    assert E.vq_chunks(10000, 640)[0] == [512, 128] and E.vq_chunks(10000, 640)[-1] == [400]
    assert E.vq_chunks(65, 64) == [[64], [1]] and E.vq_chunks(1500, 512)[-1] == [476] and E.vq_chunks(1100, 1152) == [[512, 512, 76]]
    assert E.vq_chunks(8193, 576)[-1] == [129] and E.vq_boundaries(1100, 1152) == [512, 1024] and E.vq_boundaries(65, 64) == [64]
    assert E.vq_boundaries(10000, 640)[:4] == [512, 640, 1152, 1280]
    P = 5 * 229 * 229
    assert E.cdiv(P, 256) == 1025 and P - 1024 * 256 == 61 and (229 * 229) % 256 != 0     # 61 live pixels in the last tile; tiles straddle samples
    assert E.cdiv(100000, 256) == 391


@pytest.mark.parametrize("name", list(E.VQ_CASES))
def test_on_the_dyadic_grid_the_kernels_formula_is_the_integer_distance(name):
    """every operation of (sum z^2 + sum e^2) - 2 sum z e is exact in fp32 on multiples of 2^-6 in [-2, 2] at C <= 16: the fp32 chain equals the
    int64 distance of the grid units, scaled by 2^-12 -- and the planted vectors tie exactly across every slice and chunk boundary"""
    c = E.vq_dyadic_case(name)
    rows = E.pixel_subset(c["P"])
    assert int(c["zi"].abs().max()) <= E.VQ_SPAN and int(c["ci"].abs().max()) <= E.VQ_SPAN and c["z"].shape[1] <= 16
    zrows = torch.moveaxis(c["z"], 1, -1).reshape(c["P"], -1)[rows]
    d32 = E.cpu_formula(zrows.t().reshape(1, -1, rows.numel(), 1), c["cb"])
    di = E.int_distances(c["zi"][rows], c["ci"])
    assert int(di.max()) < 2 ** 24 and int(di.min()) >= 0
    assert torch.equal(d32.double() * 4096.0, di.double())
    # the planted ties: both pixels of every boundary see distance 0 at b - 1 and at b, and the lowest index wins
    P, want = c["P"], torch.argmin(di, dim=1)
    where = {int(p): i for i, p in enumerate(rows.tolist())}
    for j, b in enumerate(c["pairs"]):
        for p in (1 + j, P - 2 - j):
            i = where[p]
            assert int(di[i, b - 1]) == 0 and int(di[i, b]) == 0 and int(want[i]) <= b - 1
    if c["K"] >= 8:
        i = where[E.VQ_TWIN_PIXEL]
        assert int(di[i, 4]) == 0 and int(di[i, 5]) == 0 and int(want[i]) <= 4
    # a distance of zero is +0: a sum of squares is +0 or positive and x - y is -0 only for x = -0, so the key of -0 is never formed
    assert not bool(torch.signbit(d32[d32 == 0]).any()) and bool((d32 == 0).any()) == bool((di == 0).any())
    # the squared error: a sum of multiples of 2^-12, far below 2^53 units
    assert c["P"] * c["z"].shape[1] * (2 * E.VQ_SPAN) ** 2 < 2 ** 53


def test_the_sqerr_tolerance_is_the_reordering_bound():
    assert E.sqerr_tolerance(1000, 3.0) == 2 * 1000 * 2.0 ** -53 * 3.0
    g = torch.Generator().manual_seed(1)
    v = (torch.rand(100000, generator=g) ** 2).double()
    a, b = float(v.sum()), float(v.flip(0).cumsum(0)[-1])          # a pairwise and a sequential sum of the same terms
    assert abs(a - b) <= E.sqerr_tolerance(v.numel(), a) < 1e-10 * a


# ------------------------------------------------------------------------------------------------ the windows
def _plans(case, weight="tent"):
    ref = E.ref_plan(case, weight)
    plan = WindowPlan(case["canvas"], case["window"], case["stride"], weight)
    assert plan.windows == ref.windows and plan.origins == ref.origins
    return plan, ref


def test_the_gather_cases_reach_their_paths():
    work = {}
    for name, case in E.GATHER_CASES.items():
        plan, ref = _plans(case)
        total = case["B"] * plan.M * case["C"] * E.prod(case["window"])
        work[name] = (E.vector_eligible(ref), total, max(len(o) for o in ref.origins))
    assert work["cap_vector"][0] and E.passes(work["cap_vector"][1] // 4) == 2 and work["cap_vector"][1] // 4 > 524288
    assert not work["cap_element"][0] and E.passes(work["cap_element"][1]) == 2
    ref = E.ref_plan(E.GATHER_CASES["cap_element"])
    assert ref.canvas[-1] % 4 == 0 and ref.window[-1] % 4 == 0 and ref.origins[-1] == (0, 130, 132)      # only an origin keeps it off the 16-byte path
    assert work["origins32_vector"][0] and work["origins32_vector"][2] == 32 == WC.MAX_PER_AXIS
    assert not work["origins32_element"][0] and work["origins32_element"][2] == 32
    assert work["vector3d"][0] and all(len(o) == 3 for o in E.ref_plan(E.GATHER_CASES["vector3d"]).origins)
    assert E.ref_plan(E.GATHER_CASES["whole_canvas"]).M == 1 and E.ref_plan(E.GATHER_CASES["one_cell"]).M == 35


@pytest.mark.parametrize("weight", ["uniform", "tent"])
@pytest.mark.parametrize("name", list(E.MERGE_CASES))
def test_on_the_dyadic_grid_the_merge_is_exact_and_its_quotient_correctly_rounded(name, weight):
    """integer weights times p = k / 16, |k| <= 128: every partial sum of the numerator is an integer below den * 128 < 2^24 sixteenths, so the
    fp32 chain (products, fmaf, den) is exact, and the fp64 quotient rounded to fp32 is the fp32 quotient"""
    case = E.MERGE_CASES[name]
    plan, ref = _plans(case, weight)
    den = E.merge_den(ref)
    assert int(ref.cover().max()) == case["cover"] and int(ref.cover().min()) == 1
    assert int(den.max()) * E.WIN_SPAN < 2 ** 24 and int(den.min()) >= 1
    assert torch.equal(ref.weights(torch.float32).double(), ref.weights(torch.int64).double())
    B = 1 if name == "cap" else case["B"]
    wins = E.dyadic_windows((B * ref.M, case["C"], *ref.window), 11)
    assert float(wins.abs().max()) == 8.0
    want = WC.ref_merge(wins, ref, torch.float64).float()
    got32 = WC.ref_merge(wins, ref, torch.float32)
    assert torch.equal(got32.view(torch.int32), want.view(torch.int32))
    # the numerator in integers: the fp64 merge above is itself exact
    w = ref.weights(torch.int64)
    acc = torch.zeros((B, case["C"], *ref.canvas), dtype=torch.int64)
    k = (wins.double() * 16).long()
    for m in range(ref.M):
        acc[(slice(None), slice(None), *ref.slices(m))] += w * k[m::ref.M]
    exact = (acc.double() / 16.0 / den.double()).float()
    assert torch.equal(torch.where(ref.cover() == 1, want, exact), want)


def test_the_merge_cases_reach_their_paths():
    cells = {name: (E.vector_eligible(E.ref_plan(c)), c["B"] * c["C"] * E.prod(c["canvas"])) for name, c in E.MERGE_CASES.items()}
    assert cells["cap"][0] and cells["cap"][1] // 4 > 524288 and E.passes(cells["cap"][1] // 4) == 2 and E.passes(cells["cap"][1]) == 5
    assert not cells["dense"][0] and cells["dense_vector"][0] and cells["origins32_vector"][0] and not cells["origins32_element"][0]
    assert cells["clamped_vector"][0] and not cells["clamped_element"][0] and cells["cover8_3d"][0] and cells["dense_3d"][0]
    assert E.ref_plan(E.MERGE_CASES["clamped_vector"]).origins[-1] == (0, 8, 12) and E.ref_plan(E.MERGE_CASES["clamped_element"]).origins[-1] == (0, 4, 5)
    assert len(E.ref_plan(E.MERGE_CASES["origins32_element"]).origins[-1]) == 32 == len(E.ref_plan(E.MERGE_CASES["origins32_vector"]).origins[-1])


# ------------------------------------------------------------------------------------------------ the held-out loss
def test_loss_chunk_and_parts_restated_against_the_library():
    lib = L.load()
    for per, (chunk, parts, last, shape) in E.ROW_SIZES.items():
        assert E.prod(shape) == per
        assert (E.loss_chunk(per), E.loss_parts(per), per - (parts - 1) * chunk) == (chunk, parts, last), per
        assert lib.mf_loss_parts(per) == parts
        assert chunk % E.QUAD_SPAN == 0                              # partial p begins 16-byte aligned
    for per in (1, 4, 8191, 8192, 8193, 9216, 2097151, 2097152, 2097153, 2097156, 2 * 2097152, 2 * 2097152 + 1, 3 * 10 ** 8, 1 << 30):
        assert lib.mf_loss_parts(per) == E.loss_parts(per) <= E.PARTS_MAX, per
        assert lib.mf_loss_workspace_bytes(3, per, 2) == 3 * E.loss_parts(per) * 16
    assert E.loss_parts(2097152) == E.PARTS_MAX and E.loss_parts(2097153) < E.PARTS_MAX < E.cdiv(2097153, E.CHUNK_MIN)
    assert E.cdiv(65, 64) == 2 and E.cdiv(E.ROWS_MAX, 64) == 1024     # the finish launch's blocks


@pytest.mark.parametrize("shape,f", [((2, 3, 5, 7), 1), ((2, 3, 4, 6), 2), ((2, 2, 3, 5), 4), ((2, 2, 2, 3, 5), 2), ((1, 2, 1, 2, 3), 4)], ids=str)
def test_on_the_dyadic_grid_the_loss_sums_are_exact(shape, f):
    """multiples of 2^-8 with |v| <= 4 and f a power of two: the fp32 emulation of the kernel (block summed one by one, divided, subtracted) equals
    the integer sums"""
    tshape = (*shape[:2], *(s * f for s in shape[2:]))
    pk, tk = E.dyadic_rows(shape, 3), E.dyadic_rows(tshape, 4)
    pred, target = pk.float() * E.LOSS_GRID, tk.float() * E.LOSS_GRID
    assert float(pred.abs().max()) == 4.0 == float(target.abs().max())
    want = E.exact_loss_sums(pk, tk, f)
    assert torch.equal(V.emulate_kernel_sums(pred, target), want)
    assert torch.equal(V.loss_sums(pred, target)[0], want)
    # d^2 <= 64 is at most 2^22 units of 2^-16; a row of the largest case stays below 2^44 units
    assert max(E.ROW_SIZES) * 2 ** 22 < 2 ** 44


def test_the_diffuse_cases_cross_the_cap_on_both_widths():
    v, e = E.DIFFUSE_CASES["vector"], E.DIFFUSE_CASES["element"]
    assert E.prod(v[1:]) % 4 == 0 and E.DIFFUSE_CAP < E.prod(v) // 4 <= E.DIFFUSE_CAP + 64
    assert E.prod(e[1:]) % 4 != 0 and E.DIFFUSE_CAP < E.prod(e) <= E.DIFFUSE_CAP + 64
