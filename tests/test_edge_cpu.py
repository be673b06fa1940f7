"""The yardsticks, case tables and refusals of tests/test_edge_gpu.py, checked without a GPU (tests/edge_cases.py): the restatements against torch,
every table row against the path its comment names (the census restates the launches' block counts and caps), and every refusal of the wrappers
on CPU tensors -- the check_* functions of medfusion_amd/kernels.py run ahead of any launch, so what they refuse here never reaches a kernel."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import restate as R
from tests import edge_cases as EC


# ---------------------------------------------------------------- inputs
def test_tagged_values_are_distinct_normal_numbers():
    t = EC.tagged(3, 5, 7)
    b = EC.bits(t).flatten()
    assert b[0] == 0x3F800000 and torch.equal(b, torch.arange(105, dtype=torch.int32) + 0x3F800000)
    assert bool(torch.isfinite(t).all()) and float(t.min()) == 1.0 and len(set(t.flatten().tolist())) == 105
    big = EC.tagged(4, start=0x3F000000 - 5)          # the largest pattern a case may reach is still a finite normal number
    assert bool(torch.isfinite(big).all()) and float(big.max()) < 3.4e38
    u = EC.tagged(2, 3, start=105)
    assert not set(EC.bits(u).flatten().tolist()) & set(b.tolist())
    # -0 and a NaN payload do not pass the int32 comparison
    assert EC.same_bits(torch.tensor([0.0]), torch.tensor([-0.0])) == 1 and bool(torch.tensor([0.0]) == torch.tensor([-0.0]))


def test_scaled_inputs_separate_samples_and_channels():
    x = EC.scaled("probe", (1,), (3, 1000, 2))
    rms = x.pow(2).mean(dim=1).sqrt()
    assert torch.allclose(torch.log2(rms[1] / rms[0]), torch.tensor(12.0), atol=0.3) and torch.allclose(torch.log2(rms[2] / rms[1]), torch.tensor(12.0), atol=0.3)
    assert torch.allclose(torch.log2(rms[:, 1] / rms[:, 0]), torch.tensor(6.0), atol=0.3)
    assert torch.equal(x, EC.scaled("probe", (1,), (3, 1000, 2)))       # a function of the case alone


# ---------------------------------------------------------------- A. layout
LAYOUT_PATHS = {      # (tiles along C, tiles along HW, N, C ragged, HW ragged)
    (1, 1, 1, 1): (1, 1, 1, True, True),
    (2, 31, 1, 33): (1, 2, 2, True, True),
    (3, 32, 4, 8): (1, 1, 3, False, False),
    (2, 33, 5, 13): (2, 3, 2, True, True),
    (1, 100, 3, 43): (4, 5, 1, True, True),
    (5, 3, 7, 11): (1, 3, 5, True, True),
    (65535, 1, 1, 1): (1, 1, 65535, True, True),
}


def test_layout_cases_reach_the_tile_edges_their_comments_name():
    assert set(LAYOUT_PATHS) == set(EC.LAYOUT_CASES)
    for case in EC.LAYOUT_CASES:
        assert EC.layout_grid(case) == LAYOUT_PATHS[case], case
    n, c, h, w = (2, 33, 5, 13)
    assert c == 32 + 1 and h * w == 2 * 32 + 1                       # one row and one column past a tile
    assert any(g[0] > 1 and g[1] > 1 and g[3] and g[4] for g in LAYOUT_PATHS.values())      # both plane dimensions ragged above 32
    assert max(c[0] for c in EC.LAYOUT_CASES) == 65535 == EC.LAYOUT_REFUSED_N - 1           # gridDim.z stops at 65535


# ---------------------------------------------------------------- B. resampling
@pytest.mark.parametrize("case", EC.POOL_CASES + [EC.POOL_CAP_CASE], ids=EC.case_id)
def test_avgpool_restatement_is_torchs_avg_pool2d_bit_for_bit(case):
    n, h, w, c, k, s, p = case
    x = EC.pool_input(case)
    got = EC.avgpool_restated(x, k, s, p)
    xn = EC.nchw(x)
    want = F.avg_pool2d(xn, k, s, p)
    assert want.shape[2:] == EC.pool_out_hw(case)
    assert EC.same_bits(got, EC.nhwc(want)) == 0, case
    want_cl = F.avg_pool2d(xn.contiguous(memory_format=torch.channels_last), k, s, p)
    assert EC.same_bits(got, EC.nhwc(want_cl)) == 0, case


def test_pool_cases_reach_the_windows_their_comments_name():
    """In floor mode (the only one the product has) no window passes the padded extent: hs + k <= H + p for the last window, so the min() that clips
    the divisor never acts and the divisor is k k everywhere -- while the SUM is clipped to the image wherever p > 0.  (A divisor taken after the
    clip to the image is therefore wrong in every case with padding.)"""
    for case in EC.POOL_CASES + [EC.POOL_CAP_CASE]:
        n, h, w, c, k, s, p = case
        div, cells = EC.pool_divisors(case)
        assert bool((div == k * k).all()), case
        assert bool((cells < div).any()) == (p > 0), case
        assert bool((cells >= 1).all()), case
    div, cells = EC.pool_divisors((2, 5, 6, 8, 2, 2, 1))             # 2 p = k: the corner windows hold ONE image cell of four
    assert float(cells[0, 0]) == 1 and float(cells[0, -1]) == 1 and float(div[0, 0]) == 4
    assert EC.pool_out_hw((1, 6, 5, 4, 2, 2, 0)) == (3, 2)           # W = 5, k = s = 2: the last column is dropped
    assert EC.pool_out_hw((1, 1, 1, 4, 3, 2, 1)) == (1, 1)
    assert sorted({c[3] for c in EC.POOL_CASES}) == [4, 8, 36]       # one float4 per pixel; two; nine


def test_upsample_expectation_is_nearest_exact():
    for case in EC.UP_CASES:
        x = EC.tagged(*case)
        want = EC.nhwc(F.interpolate(EC.nchw(x), scale_factor=2, mode="nearest-exact"))
        assert EC.same_bits(EC.upsample_expected(x), want) == 0, case


def test_shuffle_expectations_are_one_addition():
    for case in EC.UNSHUF_CASES:
        x, y = EC.unshuffle_inputs(case)
        n, h, w, c = case
        want = EC.unshuffle_expected(x, y)
        assert want.shape == (n, h // 2, w // 2, 4 * c)
        # y[n][h][w][c 4 + dy 2 + dx] += x[n][2 h + dy][2 w + dx][c], stated index by index
        again = y.clone()
        for dy in range(2):
            for dx in range(2):
                again[..., dy * 2 + dx::4] += x[:, dy::2, dx::2, :]
        assert EC.same_bits(want, again) == 0, case
    for case in EC.SHUF_CASES:
        x, y = EC.shuffle_inputs(case)
        want = EC.shuffle_expected(x, y)
        again = y.clone()
        for dy in range(2):
            for dx in range(2):
                again[:, dy::2, dx::2, :] += x[..., dy * 2 + dx::4]
        assert EC.same_bits(want, again) == 0, case
    assert [c[3] for c in EC.UNSHUF_CASES[:2]] == [1, 3] and EC.UNSHUF_CASES[2][1:3] == (2, 2)
    assert [c[3] // 4 for c in EC.SHUF_CASES[:2]] == [1, 3] and EC.SHUF_CASES[2][1:3] == (1, 1)


def test_only_the_cap_cases_cross_a_grid_stride_cap():
    table = [("avgpool", EC.POOL_CASES, EC.POOL_CAP_CASE), ("upsample", EC.UP_CASES, EC.UP_CAP_CASE), ("unshuffle", EC.UNSHUF_CASES, EC.UNSHUF_CAP_CASE),
             ("shuffle", EC.SHUF_CASES, EC.SHUF_CAP_CASE), ("add", EC.ADD_SIZES, EC.ADD_CAP_SIZE), ("gather", [(c[0], c[1], c[2], len(c[3])) for c in EC.GATHER_CASES],
             (*EC.GATHER_CAP_CASE[:3], len(EC.GATHER_CAP_CASE[3]))),
             ("gather_multi", [(c[0], c[1], c[2], len(c[3])) for c in EC.GATHER_MULTI_CASES], (*EC.GATHER_MULTI_CAP_CASE[:3], len(EC.GATHER_MULTI_CAP_CASE[3])))]
    for kernel, cases, cap_case in table:
        for case in cases:
            items, cap, blocks = EC.blocks_of(kernel, case)
            assert not EC.over_cap(kernel, case) and blocks == (items + 255) // 256, (kernel, case)
        items, cap, blocks = EC.blocks_of(kernel, cap_case)
        assert EC.over_cap(kernel, cap_case) and blocks == cap, (kernel, cap_case)
        assert 0 < items - cap * 256 <= 4, (kernel, cap_case, items)      # the smallest count past the cap: the first threads take a second item
    # the one-thread-per-element kernels have no cap; their cases cross a block edge with one element
    assert EC.blocks_of("embedding_add", 257) == (257, None, 2)
    rows, d, idx = EC.EMB_CASES[2]
    assert len(idx) * d == 257


# ---------------------------------------------------------------- C. embedding and tables
def test_embedding_cases_and_expectation():
    for case in EC.EMB_CASES + [EC.EMB_OOR_CASE]:
        table, idx, io = EC.emb_inputs(case)
        want = EC.emb_expected(table, idx, io)
        ok = (idx >= 0) & (idx < table.shape[0])
        if bool(ok.all()):
            assert EC.same_bits(want, io + table[idx]) == 0
        assert EC.same_bits(want[~ok], io[~ok]) == 0 and (case == EC.EMB_OOR_CASE) == (not bool(ok.all()))
    assert EC.EMB_CASES[0][1] == 1 and EC.EMB_CASES[1][1] == 65 and len(set(EC.EMB_CASES[1][2])) < len(EC.EMB_CASES[1][2])
    rows, d, idx = EC.EMB_CASES[3]
    assert set(idx) == {0, rows - 1}
    rows, d, idx = EC.EMB_OOR_CASE
    assert rows in idx and -1 in idx


@pytest.mark.parametrize("emb_dim", EC.SIN_DIMS)
def test_learned_sinusoidal_restatement_is_the_references_chain(emb_dim):
    t, w = EC.sin_inputs(emb_dim)
    ref, host, mask = EC.sin_reference(t, w, emb_dim)
    m = R.LearnedSinusoidalPosEmb(emb_dim)
    with torch.no_grad():
        m.weights.copy_(w)
        want = m(t)
    assert EC.same_bits(host, want) == 0                              # the fp32 angle chain ((t w) 2) pi and torch's sin / cos of it
    half = emb_dim // 2
    assert ref.shape == (len(EC.SIN_T), 1 + 2 * half + (emb_dim & 1)) and int(mask.sum()) == 2 * half
    assert torch.equal(ref[:, 0], t.double()) and (emb_dim % 2 == 0 or bool((ref[:, -1] == 0).all()))
    bound = EC.sin_bound(ref, host, mask)
    assert EC.U24 <= bound <= 4 * 2.0 ** -23                           # the host's functions are within 1 ulp of values <= 1


def test_gather_cases():
    assert sorted(c[2] for c in EC.GATHER_CASES) == [1, 4, 257]
    assert all(len(set(c[3])) < len(c[3]) for c in EC.GATHER_CASES)   # repeated columns
    assert [len(c[0]) for c in EC.GATHER_MULTI_CASES[:3]] == [1, 2, 3] and set(EC.GATHER_MULTI_CASES[2][0]) == {1, 64, 1280}
    tabs = EC.gather_tables((1, 64, 1280), 3, 2)
    allbits = torch.cat([EC.bits(t).flatten() for t in tabs])
    assert allbits.unique().numel() == allbits.numel()


# ---------------------------------------------------------------- D. VAE edge
@pytest.mark.parametrize("case", EC.DG_CASES, ids=EC.case_id)
def test_diag_gaussian_reference_and_bound_hold_the_fp32_cpu_chain(case):
    mom, noise = EC.dg_inputs(case)
    n, c, hw = case
    tm = EC.dg_terms(mom, noise)
    q = R.DiagonalGaussianDistribution()
    q.noise_fn = lambda shape, device: noise
    z, _ = q(mom)
    assert bool(((z.double() - tm["out"]).abs() <= tm["E"]).all()), case          # torch's own fp32 chain lies inside E
    lv = mom[:, c:].reshape(n, -1)
    k = min(len(EC.LOGVAR_PLANTS), c * hw)
    assert EC.same_bits(lv[0, :k], torch.tensor(EC.LOGVAR_PLANTS[:k])) == 0 and EC.same_bits(lv[-1, -k:], torch.tensor(EC.LOGVAR_PLANTS[:k])) == 0
    assert bool((mom[:, :c].reshape(n, -1)[0, :k] == 0).all())
    # a planted -31 gives what -30 gives, 21 what 20 gives
    if k >= 4:
        sd = (tm["out"] / noise.double()).reshape(n, -1)[0]
        assert math.isclose(float(sd[0]), math.exp(-15.0), rel_tol=1e-12) and math.isclose(float(sd[3]), math.exp(10.0), rel_tol=1e-12)
    assert EC.dg_inputs(EC.DG_CASES[1], hw_shape=(21, 3))[0].shape == (2, 8, 21, 3) and math.prod(EC.DG_5D_CASE[2:]) == EC.DG_CASES[1][2]


@pytest.mark.parametrize("case", EC.KL_CASES, ids=EC.case_id)
def test_kl_reference_and_bound_hold_the_fp32_cpu_chain(case):
    mom = EC.kl_inputs(case)
    tm = EC.kl_terms(mom)
    q = R.DiagonalGaussianDistribution()
    q.noise_fn = lambda shape, device: torch.zeros(shape)
    _, kl64 = q(mom.double())
    assert math.isclose(float(kl64), tm["out"], rel_tol=1e-12)
    assert tm["E"] > 0 and tm["E"] < 1e-5 * abs(tm["out"]) + 1e-6
    zero = EC.kl_terms(torch.zeros_like(mom))
    assert zero["out"] == 0.0
    assert sorted({c[1] * c[2] for c in EC.KL_CASES}) == [1, 1023, 1025, 5000] and {c[0] for c in EC.KL_CASES} == {1, 3}


def test_torch_clamp_keeps_a_nan_and_the_plants_are_distinct():
    v = torch.tensor(list(EC.NONFINITE) + [0.5])
    got = torch.clamp(v, -1.0, 1.0)
    assert math.isnan(float(got[0])) and got[1:].tolist() == [1.0, -1.0, 0.5]
    for numel in (3, 4, 63, 1536):
        pl = EC.clamp_plants(numel)
        assert len(pl) == 3 and max(pl) == numel - 1 and min(pl) >= 0 and set(map(str, pl.values())) == {"nan", "inf", "-inf"}


# ---------------------------------------------------------------- E. egress and pairs
def test_egress_inputs_sit_where_truncation_and_rounding_part():
    for case in EC.EGRESS0_CASES:
        x = EC.egress0_input(case)
        want = EC.egress0_expected(x)
        n, c, h, w = case
        assert want.shape == (n, h, w, c) and w % 2 == 1 and want.dtype == np.uint8
        v = (np.clip(x.numpy().reshape(n, -1)[:, :512], -1, 1) + 1) / 2 * 255
        assert (np.floor(v) != np.rint(v)).sum() > 100                # truncation and rounding disagree on many of the planted points
        assert set(np.floor(v).astype(int).flatten().tolist()) >= set(range(0, 255))
    assert {c[1] for c in EC.EGRESS0_CASES} == {1, 3}
    for name in EC.EGRESS1_CASES:
        x = EC.egress1_input(name)
        want = EC.egress1_expected(x)
        assert want.shape == (x.shape[0], x.shape[2], x.shape[3], x.shape[1]) and want.dtype == torch.uint8
    assert bool((EC.egress1_expected(EC.egress1_input("constant")) == 0).all())
    assert math.prod(EC.egress1_input("chw3").shape[1:]) == 3 and math.prod(EC.egress1_input("chw257").shape[1:]) == 257
    d = ((EC.egress1_input("disjoint") + 1) / 2).reshape(3, -1)
    assert float(d[0].max()) < float(d[1].min()) and float(d[1].max()) < float(d[2].min())
    o = EC.egress1_input("outside")
    assert float(o.abs().min()) > 1.0


def _split_on_cpu(x_nhwc, bound):
    """the fp16-pair form stated in torch: hi = fp16(x 2^-s), lo = fp16((x 2^-s - hi) 2048), groups of 8 channels [hi x 8][lo x 8]"""
    s = torch.floor(torch.log2(bound.double())) - 14
    v = (x_nhwc.double() * torch.exp2(-s).view(-1, 1, 1, 1)).float()
    hi = v.half()
    lo = ((v - hi.float()) * 2048.0).half()
    n, h, w, cp = x_nhwc.shape
    raw = torch.stack([hi.view(n, h, w, cp // 8, 8), lo.view(n, h, w, cp // 8, 8)], dim=4)      # [.., group, piece, 8]
    return raw.contiguous().view(torch.int16).view(n, h, w, cp * 2).view(torch.int32).view(n, h, w, cp)


def test_pair_decode_and_tolerance_hold_a_split_stated_in_torch():
    for case in EC.PACK_CASES:
        n, c, hw, cp = case
        x = EC.pack_input(case)
        if case == EC.PACK_ZERO_CASE:
            assert float(x[0].abs().max()) == 0 and float(x[1].abs().max()) > 1000
            x = x[1:]
        xp = torch.zeros((x.shape[0], hw, 1, cp))
        xp[..., :c] = x.permute(0, 2, 3, 1)
        bound = x.abs().amax(dim=(1, 2, 3))
        back, hi, lo = EC.decode_pairs(_split_on_cpu(xp, bound), bound)
        assert bool(((back - xp.double()).abs() <= EC.pack_tolerance(xp, bound)).all()), case
        assert bool((hi[..., c:] == 0).all()) and bool((lo[..., c:] == 0).all())
    assert any(c[1] % 8 for c in EC.PACK_CASES) and any(c[3] == 64 for c in EC.PACK_CASES)
    assert EC.PACK_REFUSED[1] * EC.PACK_REFUSED[2] == 2 ** 18 + 1


# ---------------------------------------------------------------- G. refusals, on CPU tensors
def _pairs_only(shape):
    t = torch.zeros(shape)
    t._mf_pairs_only = True
    return t


def _refused(match, fn, *args, **kw):
    with pytest.raises(RuntimeError, match=match):
        fn(*args, **kw)


def test_layout_refusals():
    from medfusion_amd import kernels as K
    x = torch.zeros((2, 3, 4, 5))
    K.check_layout("nhwc_to_nchw", x, copies=False)
    K.check_layout("nchw_to_nhwc", x.permute(0, 2, 1, 3), copies=True)             # (this direction copies a strided input itself)
    _refused("contiguous", K.check_layout, "nhwc_to_nchw", x.permute(0, 2, 1, 3), copies=False)
    for what, copies in (("nhwc_to_nchw", False), ("nchw_to_nhwc", True)):
        _refused("fp32", K.check_layout, what, x.double(), copies=copies)
        _refused("fp32", K.check_layout, what, x.long(), copies=copies)
        _refused("4 dimensions", K.check_layout, what, x[0], copies=copies)
        _refused("N <= 65535", K.check_layout, what, torch.zeros((EC.LAYOUT_REFUSED_N, 1, 1, 1)), copies=copies)
        K.check_layout(what, torch.zeros((65535, 1, 1, 1)), copies=copies)
    _refused("only as fp16 pairs", K.check_layout, "nhwc_to_nchw", _pairs_only((1, 2, 2, 8)), copies=False)
    _refused("only as fp16 pairs", K.check_layout, "nchw_to_nhwc", _pairs_only((1, 2, 2, 8)), copies=True)


def test_resampling_refusals():
    from medfusion_amd import kernels as K
    x = torch.zeros((2, 6, 8, 4))
    assert K.check_avgpool2d(x, 3, 2, 1) == (3, 4)
    _refused("fp32", K.check_avgpool2d, x.double(), 3, 2, 1)
    _refused("C % 4", K.check_avgpool2d, torch.zeros((2, 6, 8, 6)), 3, 2, 1)
    _refused("2 pad <= k", K.check_avgpool2d, x, 2, 2, 2)
    _refused("stride", K.check_avgpool2d, x, 2, 0, 0)
    _refused("empty output", K.check_avgpool2d, torch.zeros((1, 1, 1, 4)), 3, 1, 0)
    _refused("only as fp16 pairs", K.check_avgpool2d, _pairs_only((1, 4, 4, 8)), 2, 2, 0)
    K.check_upsample_nearest2x(x)
    _refused("fp32", K.check_upsample_nearest2x, x.to(torch.float16))
    _refused("C % 4", K.check_upsample_nearest2x, torch.zeros((1, 2, 2, 3)))
    _refused("4 dimensions", K.check_upsample_nearest2x, torch.zeros((2, 2, 4)))

    y = torch.zeros((2, 3, 4, 16))
    K.check_pixel_shuffle_pair("pixel_unshuffle2_add", x, y, unshuffle=True)
    K.check_pixel_shuffle_pair("pixel_unshuffle2_add", x.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3), y, unshuffle=True)   # (x is copied by the wrapper)
    _refused("does not unshuffle", K.check_pixel_shuffle_pair, "pixel_unshuffle2_add", x, torch.zeros((2, 3, 4, 4)), unshuffle=True)
    _refused("does not unshuffle", K.check_pixel_shuffle_pair, "pixel_unshuffle2_add", x, torch.zeros((2, 4, 3, 16)), unshuffle=True)
    _refused("does not unshuffle", K.check_pixel_shuffle_pair, "pixel_unshuffle2_add", torch.zeros((2, 5, 8, 4)), torch.zeros((2, 2, 4, 16)), unshuffle=True)
    _refused("y must be fp32", K.check_pixel_shuffle_pair, "pixel_unshuffle2_add", x, y.double(), unshuffle=True)
    _refused("x must be fp32", K.check_pixel_shuffle_pair, "pixel_unshuffle2_add", x.double(), y, unshuffle=True)
    _refused("y must be contiguous", K.check_pixel_shuffle_pair, "pixel_unshuffle2_add", x, torch.zeros((2, 4, 3, 16)).permute(0, 2, 1, 3), unshuffle=True)
    _refused("only as fp16 pairs", K.check_pixel_shuffle_pair, "pixel_unshuffle2_add", x, _pairs_only((2, 3, 4, 16)), unshuffle=True)
    xs, ys = torch.zeros((2, 3, 4, 8)), torch.zeros((2, 6, 8, 2))
    K.check_pixel_shuffle_pair("pixel_shuffle2_add", xs, ys, unshuffle=False)
    _refused("does not shuffle", K.check_pixel_shuffle_pair, "pixel_shuffle2_add", torch.zeros((2, 3, 4, 6)), ys, unshuffle=False)
    _refused("does not shuffle", K.check_pixel_shuffle_pair, "pixel_shuffle2_add", xs, torch.zeros((2, 6, 8, 8)), unshuffle=False)
    _refused("y must be fp32", K.check_pixel_shuffle_pair, "pixel_shuffle2_add", xs, ys.long(), unshuffle=False)
    _refused("y must be contiguous", K.check_pixel_shuffle_pair, "pixel_shuffle2_add", xs, torch.zeros((2, 8, 6, 2)).permute(0, 2, 1, 3), unshuffle=False)


def test_table_refusals():
    from medfusion_amd import kernels as K
    table, io = torch.zeros((5, 8)), torch.zeros((3, 8))
    idx = torch.tensor([0, 4, 2])
    K.check_embedding_add(table, idx, io)
    K.check_embedding_add(table, idx.int(), io)                       # (converted by the wrapper)
    _refused("idx must be int64", K.check_embedding_add, table, idx.float(), io)
    _refused("idx must be int64", K.check_embedding_add, table, idx.to(torch.int16), io)
    _refused("one index per row", K.check_embedding_add, table, idx[:2], io)
    _refused("table must be fp32", K.check_embedding_add, table.double(), idx, io)
    _refused("io must be fp32", K.check_embedding_add, table, idx, io.double())
    _refused("io must be contiguous", K.check_embedding_add, table, idx, torch.zeros((3, 16))[:, ::2])
    _refused("table must be contiguous", K.check_embedding_add, torch.zeros((8, 5)).t(), idx, io)
    _refused(r"\[B, D\]", K.check_embedding_add, table, idx, torch.zeros((3, 7)))
    _refused("2 dimensions", K.check_embedding_add, table, idx, torch.zeros((3, 2, 4)))

    t, w = torch.zeros(4), torch.zeros(8)
    K.check_learned_sinusoidal(t, w, 16)
    K.check_learned_sinusoidal(t.long(), w, 17)                       # (integer timesteps are converted by the wrapper)
    _refused("weights must be fp32", K.check_learned_sinusoidal, t, w.double(), 16)
    _refused("weights must have shape", K.check_learned_sinusoidal, t, w, 18)
    _refused("emb_dim", K.check_learned_sinusoidal, t, torch.zeros(0), 1)
    _refused(r"\[B\]", K.check_learned_sinusoidal, torch.zeros((4, 1)), w, 16)

    tab, cols = torch.zeros((4, 3, 5)), torch.tensor([2, 0, 2])
    step_dev = torch.zeros(1, dtype=torch.int32)
    for step in (0, 3, np.int64(2), step_dev):
        K.check_gather_step_rows([tab], step, cols)
    for step in (-1, 4, 1.0, True, None):
        _refused("host step", K.check_gather_step_rows, [tab], step, cols)
    _refused("device step must be int32", K.check_gather_step_rows, [tab], step_dev.long(), cols)
    _refused("cols must be int64", K.check_gather_step_rows, [tab], 0, cols.int())
    _refused("cols must be contiguous", K.check_gather_step_rows, [tab], 0, torch.tensor([2, 9, 0, 9, 2])[::2])
    _refused("cols must have 1 dimensions", K.check_gather_step_rows, [tab], 0, cols.view(3, 1))
    _refused("table 0 must be fp32", K.check_gather_step_rows, [tab.double()], 0, cols)
    _refused("table 0 must be contiguous", K.check_gather_step_rows, [torch.zeros((4, 5, 3)).transpose(1, 2)], 0, cols)
    _refused("table 0 must have 3 dimensions", K.check_gather_step_rows, [torch.zeros((4, 15))], 0, cols)
    _refused("table 1", K.check_gather_step_rows, [tab, torch.zeros((4, 2, 7))], 0, cols)
    _refused("table 1 must be fp32", K.check_gather_step_rows, [tab, torch.zeros((4, 3, 7), dtype=torch.float64)], 0, cols)
    _refused("one to three tables", K.check_gather_step_rows, [tab] * 4, 0, cols)
    _refused("one to three tables", K.check_gather_step_rows, [], 0, cols)
    K.check_gather_step_rows([tab, torch.zeros((4, 3, 1)), torch.zeros((4, 3, 64))], 3, cols)

    t1, out = torch.zeros(7), torch.zeros(5)
    K.check_broadcast_from_table(t1, step_dev, out)
    _refused("table must be fp32", K.check_broadcast_from_table, t1.double(), step_dev, out)
    _refused("device step must be int32", K.check_broadcast_from_table, t1, step_dev.long(), out)
    _refused("out must be fp32", K.check_broadcast_from_table, t1, step_dev, out.long())
    _refused("out must have 1 dimensions", K.check_broadcast_from_table, t1, step_dev, torch.zeros((5, 1)))
    _refused("out must be contiguous", K.check_broadcast_from_table, t1, step_dev, torch.zeros(10)[::2])
    _refused("table must have 1 dimensions", K.check_broadcast_from_table, torch.zeros((7, 1)), step_dev, out)


def test_add_refusals():
    from medfusion_amd import kernels as K
    a, b = torch.zeros((2, 3, 4)), torch.zeros((2, 3, 4))
    K.check_add(a, b)
    K.check_add(a, b, a)
    _refused("b must have shape", K.check_add, a, torch.zeros((2, 3, 5)))
    _refused("b must have shape", K.check_add, a, torch.zeros((2, 12)))
    _refused("out must have shape", K.check_add, a, b, torch.zeros((2, 3)))
    _refused("a must be fp32", K.check_add, a.double(), b)
    _refused("b must be fp32", K.check_add, a, b.long())
    _refused("out must be fp32", K.check_add, a, b, torch.zeros((2, 3, 4), dtype=torch.float64))
    _refused("a must be contiguous", K.check_add, torch.zeros((3, 2, 4)).transpose(0, 1), b)
    _refused("b must be contiguous", K.check_add, a, torch.zeros((3, 2, 4)).transpose(0, 1))
    _refused("out must be contiguous", K.check_add, a, b, torch.zeros((3, 2, 4)).transpose(0, 1))
    _refused("only as fp16 pairs", K.check_add, _pairs_only((2, 3, 4)), b)
    K.check_add(a, b, _pairs_only((2, 3, 4)))                         # (an output that is only written may be pairs-only storage: the writer fills it)
    po = _pairs_only((2, 3, 4))
    _refused("only as fp16 pairs", K.check_add, a, po, po)            # ... but not one that is read as well


def test_vae_edge_and_pair_refusals():
    from medfusion_amd import kernels as K
    mom, noise = torch.zeros((2, 8, 3, 5)), torch.zeros((2, 4, 3, 5))
    assert K.check_diag_gaussian("diag_gaussian_sample", mom, noise) == (2, 4, 15)
    assert K.check_diag_gaussian("diag_gaussian_kl", mom) == (2, 4, 15)
    _refused("moments must be fp32", K.check_diag_gaussian, "diag_gaussian_sample", mom.double(), noise)
    _refused("noise must be fp32", K.check_diag_gaussian, "diag_gaussian_sample", mom, noise.double())
    _refused("noise must have shape", K.check_diag_gaussian, "diag_gaussian_sample", mom, torch.zeros((2, 8, 3, 5)))
    _refused("noise must have shape", K.check_diag_gaussian, "diag_gaussian_sample", mom, torch.zeros((2, 4, 5, 3)))
    _refused("noise must be contiguous", K.check_diag_gaussian, "diag_gaussian_sample", mom, torch.zeros((2, 4, 5, 3)).transpose(2, 3))
    _refused("moments must be contiguous", K.check_diag_gaussian, "diag_gaussian_sample", torch.zeros((2, 8, 5, 3)).transpose(2, 3), noise)
    _refused(r"\[N, 2 C, H, W\]", K.check_diag_gaussian, "diag_gaussian_sample", torch.zeros((2, 7, 3, 5)), noise)
    _refused("4 dimensions", K.check_diag_gaussian, "diag_gaussian_sample", torch.zeros((2, 8, 3, 5, 1)), noise)
    _refused("moments must be fp32", K.check_diag_gaussian, "diag_gaussian_kl", mom.double())
    K.check_diag_gaussian("diag_gaussian_kl", torch.zeros((2, 8, 5, 3)).transpose(2, 3))      # (the KL wrapper copies a strided input itself)

    K.check_pack_nchw_pairs(torch.zeros((1, 8, 4, 4)), 32)
    _refused("x must be fp32", K.check_pack_nchw_pairs, torch.zeros((1, 8, 4, 4), dtype=torch.float64), 32)
    _refused("C <= cp", K.check_pack_nchw_pairs, torch.zeros((1, 33, 4, 4)), 32)
    _refused("multiple of 32", K.check_pack_nchw_pairs, torch.zeros((1, 8, 4, 4)), 40)
    n, c, hw, cp = EC.PACK_REFUSED
    _refused("2\\^18", K.check_pack_nchw_pairs, torch.zeros((n, c, hw, 1)), cp)
    K.check_pack_nchw_pairs(torch.zeros((1, 1, 2 ** 18, 1)), 32)
    _refused("x must be fp32", K.image_to_uint8, torch.zeros((1, 3, 4, 4), dtype=torch.float64))      # (refused before the device check)
