"""The layout kernels, the resampling / skip kernels of csrc/edge_ops.hip, the embedding and table kernels, the VAE edge of csrc/small_ops.hip, the
image egress and the network input's pair operand against exact references at their path edges, in-process on the product wrappers K.*.  Cases,
restatements, bounds and the census: tests/edge_cases.py (checked by tests/test_edge_cpu.py, which also proves every refusal on CPU tensors).
Every comparison prints a [measured] line (profiles/edge_parity_measured.txt holds one run's).

A. layout bit-equal with permute, N = 65535, N = 65536 refused      B. AvgPool / nearest x2 / PixelUnshuffle + add / PixelShuffle + add bit-equal, one
case per kernel past its grid-stride cap      C. embedding_add, learned_sinusoidal, the step gathers, broadcast_from_table, add      D. latent sampling
and KL against fp64 inside E      E. image egress at the points where truncation and rounding part; pack_nchw_pairs against a decode of its own
F. a NaN stays where torch.clamp leaves it      G. what the wrappers refuse, outputs untouched      S. sentinels: the mf_* entries write nothing
past their outputs"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import restate as R
from tests import edge_cases as EC

pytestmark = pytest.mark.gpu

REFUSED = RuntimeError


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import medfusion_amd  # noqa: F401  (loads libmedfusion_hip.so; raises if missing)
    return torch.device("cuda:0")


def _report(what, case, wrong, total):
    print(f"[measured] {what} {EC.case_id(case)}: {wrong} of {total} elements differ from the reference in their bits")


def _bit_equal(what, case, got, want):
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), (what, case, got.dtype, tuple(got.shape), tuple(want.shape))
    wrong = EC.same_bits(got.cpu(), want)
    _report(what, case, wrong, want.numel())
    assert wrong == 0, (what, case, (EC.bits(got.cpu()) != EC.bits(want)).nonzero()[:8].tolist())


# ---------------------------------------------------------------- A. layout
@pytest.mark.parametrize("case", EC.LAYOUT_CASES, ids=EC.case_id)
def test_layout_is_permute_bit_for_bit(dev, case):
    from medfusion_amd import kernels as K
    n, c, h, w = case
    x = EC.tagged(n, c, h, w)
    _bit_equal("nchw_to_nhwc", case, K.nchw_to_nhwc(x.to(dev)), x.permute(0, 2, 3, 1).contiguous())
    y = EC.tagged(n, h, w, c)
    _bit_equal("nhwc_to_nchw", case, K.nhwc_to_nchw(y.to(dev)), y.permute(0, 3, 1, 2).contiguous())
    xs = EC.tagged(n, c, w, h).transpose(2, 3)          # a strided NCHW input: this direction copies it first
    assert not xs.is_contiguous() or h == 1 or w == 1
    _bit_equal("nchw_to_nhwc (strided input)", case, K.nchw_to_nhwc(xs.to(dev)), xs.permute(0, 2, 3, 1).contiguous())


def test_layout_refuses_more_samples_than_grid_planes(dev):
    from medfusion_amd import kernels as K
    x = torch.zeros((EC.LAYOUT_REFUSED_N, 1, 1, 1), device=dev)
    with pytest.raises(REFUSED, match="N <= 65535"):
        K.nchw_to_nhwc(x)
    with pytest.raises(REFUSED, match="N <= 65535"):
        K.nhwc_to_nchw(x)


# ---------------------------------------------------------------- B. resampling and skip kernels
@pytest.mark.parametrize("case", EC.POOL_CASES + [EC.POOL_CAP_CASE], ids=EC.case_id)
def test_avgpool_bit_equal(dev, case):
    from medfusion_amd import kernels as K
    n, h, w, c, k, s, p = case
    x = EC.pool_input(case)
    _bit_equal("avgpool2d", case, K.avgpool2d(x.to(dev), k, s, p), EC.avgpool_restated(x, k, s, p))


@pytest.mark.parametrize("case", EC.UP_CASES + [EC.UP_CAP_CASE], ids=EC.case_id)
def test_upsample_nearest2x_bit_equal(dev, case):
    from medfusion_amd import kernels as K
    x = EC.tagged(*case)
    _bit_equal("upsample_nearest2x", case, K.upsample_nearest2x(x.to(dev)), EC.upsample_expected(x))


@pytest.mark.parametrize("case", EC.UNSHUF_CASES + [EC.UNSHUF_CAP_CASE], ids=EC.case_id)
def test_pixel_unshuffle_add_bit_equal(dev, case):
    from medfusion_amd import kernels as K
    x, y = EC.unshuffle_inputs(case)
    xd, yd = x.to(dev), y.to(dev)
    got = K.pixel_unshuffle2_add(xd, yd)
    assert got is yd
    _bit_equal("pixel_unshuffle2_add", case, got, EC.unshuffle_expected(x, y))
    assert EC.same_bits(xd.cpu(), x) == 0, case          # x is unchanged


@pytest.mark.parametrize("case", EC.SHUF_CASES + [EC.SHUF_CAP_CASE], ids=EC.case_id)
def test_pixel_shuffle_add_bit_equal(dev, case):
    from medfusion_amd import kernels as K
    x, y = EC.shuffle_inputs(case)
    xd, yd = x.to(dev), y.to(dev)
    got = K.pixel_shuffle2_add(xd, yd)
    assert got is yd
    _bit_equal("pixel_shuffle2_add", case, got, EC.shuffle_expected(x, y))
    assert EC.same_bits(xd.cpu(), x) == 0, case


# ---------------------------------------------------------------- C. embedding and table kernels
@pytest.mark.parametrize("case", EC.EMB_CASES + [EC.EMB_OOR_CASE], ids=lambda c: f"{c[0]}-{c[1]}-{len(c[2])}")
def test_embedding_add_bit_equal(dev, case):
    from medfusion_amd import kernels as K
    table, idx, io = EC.emb_inputs(case)
    want = EC.emb_expected(table, idx, io)
    for name, index in (("int64", idx), ("int32", idx.int())):
        iod = io.to(dev)
        got = K.embedding_add(table.to(dev), index.to(dev), iod)
        assert got is iod
        _bit_equal(f"embedding_add ({name} index)", (case[0], case[1], len(case[2])), got, want)


@pytest.mark.parametrize("emb_dim", EC.SIN_DIMS)
def test_learned_sinusoidal_against_fp64_of_the_fp32_angle(dev, emb_dim):
    from medfusion_amd import kernels as K
    t, w = EC.sin_inputs(emb_dim)
    ref, host, mask = EC.sin_reference(t, w, emb_dim)
    got = K.learned_sinusoidal(t.to(dev), w.to(dev), emb_dim).cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert EC.same_bits(got[:, 0].contiguous(), t) == 0                                   # column 0 is t bit for bit
    if emb_dim & 1:
        assert EC.same_bits(got[:, -1].contiguous(), torch.zeros(len(EC.SIN_T))) == 0     # the trailing column of an odd emb_dim is exactly +0
    err_k = float((got.double() - ref)[:, mask].abs().max())
    err_h = float((host.double() - ref)[:, mask].abs().max())
    bound = EC.sin_bound(ref, host, mask)
    print(f"[measured] learned_sinusoidal emb_dim {emb_dim}: kernel max |err| {err_k:.3e}, torch.sin / torch.cos (fp32, CPU) {err_h:.3e}, bound {bound:.3e}")
    assert err_k <= bound, (emb_dim, err_k, err_h, bound)


def _steps(S, dev):
    """host and device forms of the first and the last step"""
    return [(0, "host"), (S - 1, "host"), (torch.tensor([0], dtype=torch.int32, device=dev), "device"), (torch.tensor([S - 1], dtype=torch.int32, device=dev), "device")]


@pytest.mark.parametrize("case", EC.GATHER_CASES + [EC.GATHER_CAP_CASE], ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{len(c[3])}")
def test_gather_step_rows_bit_equal(dev, case):
    from medfusion_amd import kernels as K
    S, ncol, ln, cols = case
    table, colt = EC.tagged(S, ncol, ln), torch.tensor(cols, dtype=torch.int64)
    td, cd = table.to(dev), colt.to(dev)
    for step, where in _steps(S, dev):
        st = int(step.item()) if where == "device" else step
        _bit_equal(f"gather_step_rows ({where} step {st})", (S, ncol, ln, len(cols)), K.gather_step_rows(td, step, cd), table[st, colt])
    for bad in (-1, S):
        with pytest.raises(REFUSED, match="host step"):
            K.gather_step_rows(td, bad, cd)


@pytest.mark.parametrize("case", EC.GATHER_MULTI_CASES + [EC.GATHER_MULTI_CAP_CASE], ids=lambda c: f"{'x'.join(map(str, c[0]))}-{c[1]}-{c[2]}-{len(c[3])}")
def test_gather_step_rows_multi_bit_equal(dev, case):
    from medfusion_amd import kernels as K
    lens, S, ncol, cols = case
    tables, colt = EC.gather_tables(lens, S, ncol), torch.tensor(cols, dtype=torch.int64)
    tds, cd = [t.to(dev) for t in tables], colt.to(dev)
    for step, where in _steps(S, dev):
        st = int(step.item()) if where == "device" else step
        outs = K.gather_step_rows_multi(tds, step, cd)
        assert len(outs) == len(tables)
        for i, (o, t) in enumerate(zip(outs, tables)):
            _bit_equal(f"gather_step_rows_multi ({where} step {st}) table {i} of", (lens, S, ncol, len(cols)), o, t[st, colt])
    with pytest.raises(REFUSED, match="host step"):
        K.gather_step_rows_multi(tds, S, cd)


@pytest.mark.parametrize("case", EC.BROADCAST_CASES, ids=EC.case_id)
def test_broadcast_from_table_bit_equal(dev, case):
    from medfusion_amd import kernels as K
    S, n = case
    table = EC.tagged(S)
    td = table.to(dev)
    for st in sorted({0, S - 1}):
        out = torch.full((n,), EC.SENTINEL, device=dev)
        got = K.broadcast_from_table(td, torch.tensor([st], dtype=torch.int32, device=dev), out)
        assert got is out
        _bit_equal(f"broadcast_from_table (step {st})", case, got, table[st].expand(n).contiguous())


@pytest.mark.parametrize("n", EC.ADD_SIZES + (EC.ADD_CAP_SIZE,))
def test_add_bit_equal_and_aliased(dev, n):
    from medfusion_amd import kernels as K
    a, b = EC.scaled("add.a", (n,), (n,), channel_axis=None), EC.scaled("add.b", (n,), (n,), channel_axis=None)      # (neighbours 2^12 apart)
    ad, bd = a.to(dev), b.to(dev)
    _bit_equal("add", (n,), K.add(ad, bd), a + b)
    got = K.add(ad, bd, out=ad)          # out aliased to a
    assert got is ad
    _bit_equal("add (out = a)", (n,), got, a + b)
    assert EC.same_bits(bd.cpu(), b) == 0


# ---------------------------------------------------------------- D. VAE edge
def _within(what, case, got, tm):
    ratio = ((got.double().cpu() - tm["out"]).abs() / tm["E"].clamp_min(1e-300))
    ratio = torch.where((got.double().cpu() == tm["out"]), torch.zeros_like(ratio), ratio)
    worst = float(ratio.max())
    print(f"[measured] {what} {EC.case_id(case)}: largest |err| / E {worst:.4f}")
    assert worst <= 1.0, (what, case, worst)


@pytest.mark.parametrize("case", EC.DG_CASES, ids=EC.case_id)
def test_diag_gaussian_sample_is_within_E(dev, case):
    from medfusion_amd import kernels as K
    mom, noise = EC.dg_inputs(case)
    got = K.diag_gaussian_sample(mom.to(dev), noise.to(dev))
    assert got.shape == noise.shape and bool(torch.isfinite(got).all())
    _within("diag_gaussian_sample", case, got, EC.dg_terms(mom, noise))


def test_diag_gaussian_sample_5d_view(dev):
    """the NCDHW path of DiagonalGaussianDistribution.forward (medfusion_amd/vae.py): the per-voxel op on the [N, 2C, D H, W] view"""
    from medfusion_amd.vae import DiagonalGaussianDistribution
    n, c, d, h, w = EC.DG_5D_CASE
    mom, noise = EC.dg_inputs((n, c, d * h * w), hw_shape=(d * h, w))
    z, _ = DiagonalGaussianDistribution()(mom.view(n, 2 * c, d, h, w).to(dev), noise.view(n, c, d, h, w).to(dev))
    assert z.shape == (n, c, d, h, w)
    _within("diag_gaussian_sample (5-D view)", EC.DG_5D_CASE, z.reshape(n, c, d * h, w), EC.dg_terms(mom, noise))


@pytest.mark.parametrize("case", EC.KL_CASES, ids=EC.case_id)
def test_diag_gaussian_kl_is_within_E(dev, case):
    from medfusion_amd import kernels as K
    mom = EC.kl_inputs(case)
    tm = EC.kl_terms(mom)
    got = K.diag_gaussian_kl(mom.to(dev))
    assert got.shape == () and got.dtype == torch.float32
    err = abs(float(got.double()) - tm["out"])
    print(f"[measured] diag_gaussian_kl {EC.case_id(case)}: |err| / E {err / tm['E']:.4f} (kl {tm['out']:.6e})")
    assert err <= tm["E"], (case, float(got), tm)
    zero = K.diag_gaussian_kl(torch.zeros_like(mom).to(dev))
    assert EC.same_bits(zero.reshape(1), torch.zeros(1)) == 0, case      # the all-zero moments give exactly +0


# ---------------------------------------------------------------- E. image egress and the pair operand
@pytest.mark.parametrize("case", EC.EGRESS0_CASES, ids=EC.case_id)
def test_egress_truncates_where_the_dataset_script_does(dev, case):
    from medfusion_amd import kernels as K
    x = EC.egress0_input(case)
    got = K.image_to_uint8(x.to(dev)).cpu().numpy()
    want = EC.egress0_expected(x)
    assert got.shape == want.shape and got.dtype == np.uint8
    wrong = int((got != want).sum())
    print(f"[measured] image_to_uint8 mode 0 {EC.case_id(case)}: {wrong} of {want.size} bytes differ from the numpy chain")
    assert wrong == 0, (case, np.argwhere(got != want)[:8].tolist())


@pytest.mark.parametrize("name", EC.EGRESS1_CASES)
def test_egress_normalizes_each_image_like_save_image(dev, name):
    from medfusion_amd import kernels as K
    x = EC.egress1_input(name)
    got = K.image_to_uint8(x.to(dev), normalize_each=True).cpu()
    want = EC.egress1_expected(x)
    assert got.shape == want.shape and got.dtype == torch.uint8
    wrong = int((got != want).sum())
    print(f"[measured] image_to_uint8 mode 1 {name}: {wrong} of {want.numel()} bytes differ from the torchvision chain")
    assert wrong == 0, (name, (got != want).nonzero()[:8].tolist())


@pytest.mark.parametrize("case", EC.PACK_CASES, ids=EC.case_id)
def test_pack_nchw_pairs_against_its_decode(dev, case):
    from medfusion_amd import kernels as K
    n, c, hw, cp = case
    x = EC.pack_input(case)
    t = K.pack_nchw_pairs(x.to(dev), cp)
    assert K.pairs_only(t) and t.shape == (n, hw, 1, cp)
    bound = t._mf_bound.cpu()
    assert EC.same_bits(bound, x.abs().amax(dim=(1, 2, 3))) == 0, case          # the bound is max |x| bit for bit
    back, hi, lo = EC.decode_pairs(t._mf_split, bound)
    xp = torch.zeros((n, hw, 1, cp))
    xp[..., :c] = x.permute(0, 2, 3, 1)
    err, tol = (back - xp.double()).abs(), EC.pack_tolerance(xp, bound)
    worst = float(torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300)).max())
    print(f"[measured] pack_nchw_pairs {EC.case_id(case)}: largest |decode - x| / (2^-23 |x| + 2^-50 bound) {worst:.4f}, {float((err == 0).double().mean()):.3f} of the values exact")
    assert worst <= 1.0, (case, worst)
    pad16 = torch.stack([hi[..., c:], lo[..., c:]]).to(torch.float16).view(torch.int16)
    assert bool((pad16 == 0).all()), case                                        # the padded channels are exactly +0 in both pieces
    if case == EC.PACK_ZERO_CASE:
        z = torch.stack([hi[0], lo[0]]).to(torch.float16).view(torch.int16)
        assert float(bound[0]) == 0.0 and bool((z == 0).all())


def test_pack_nchw_pairs_refuses_more_than_one_workgroup_can_hold(dev):
    from medfusion_amd import kernels as K
    n, c, hw, cp = EC.PACK_REFUSED
    with pytest.raises(REFUSED, match="2\\^18"):
        K.pack_nchw_pairs(torch.zeros((n, c, hw, 1), device=dev), cp)


# ---------------------------------------------------------------- F. a NaN stays where the reference's is
def _planted(t: torch.Tensor, plants) -> torch.Tensor:
    out = t.clone()
    flat = out.view(-1)
    for pos, v in plants.items():
        flat[pos] = v
    return out


def _nan_aware(what, got, want_nan, want_bits_from, base, plants_mask):
    """isnan masks equal; bits equal to `want_bits_from` wherever the result is not NaN; every unplanted element bit-identical to `base`"""
    got = got.cpu()
    assert torch.equal(torch.isnan(got), want_nan), (what, (torch.isnan(got) != want_nan).nonzero()[:8].tolist())
    keep = ~want_nan
    assert torch.equal(EC.bits(got)[keep], EC.bits(want_bits_from)[keep]), what
    assert torch.equal(EC.bits(got)[~plants_mask], EC.bits(base.cpu())[~plants_mask]), what
    print(f"[measured] {what}: NaN at {int(want_nan.sum())} planted element(s) as torch.clamp leaves it, +-Inf clamped, {int((~plants_mask).sum())} other elements bit-identical")


@pytest.mark.parametrize("case", EC.DG_CASES[1:], ids=EC.case_id)
def test_a_nonfinite_logvar_comes_out_where_torch_clamp_puts_it(dev, case):
    from medfusion_amd import kernels as K
    n, c, hw = case
    mom, noise = EC.dg_inputs(case)
    lv = mom[:, c:].contiguous()
    plants = EC.clamp_plants(lv.numel())
    lvp = _planted(lv, plants)
    momp = torch.cat([mom[:, :c], lvp], dim=1).contiguous()
    mask = torch.zeros(lv.numel(), dtype=torch.bool)
    mask[list(plants)] = True
    mask = mask.view(noise.shape)
    # the reference's fp32 chain on the CPU decides where the NaN is; the kernel's own arithmetic on the CPU-clamped logvar gives the bits elsewhere
    q = R.DiagonalGaussianDistribution()
    q.noise_fn = lambda shape, device: noise
    zref, klref = q(momp)
    assert int(torch.isnan(zref).sum()) == 1 and bool(torch.isnan(klref))
    mom_cl = torch.cat([mom[:, :c], torch.clamp(lvp, -30.0, 20.0)], dim=1).contiguous()
    base = K.diag_gaussian_sample(mom.to(dev), noise.to(dev))
    on_clamped = K.diag_gaussian_sample(mom_cl.to(dev), noise.to(dev)).cpu()
    got = K.diag_gaussian_sample(momp.to(dev), noise.to(dev))
    _nan_aware(f"diag_gaussian_sample {EC.case_id(case)} with NaN / +Inf / -Inf logvar", got, torch.isnan(zref), on_clamped, base, mask)
    # KL: NaN with the NaN planted (as the reference's), and with the two infinities alone what the clamped logvar gives, inside E
    assert bool(torch.isnan(K.diag_gaussian_kl(momp.to(dev)).cpu()))
    inf_only = {p: v for p, v in plants.items() if v == v}
    mom_inf = torch.cat([mom[:, :c], _planted(lv, inf_only)], dim=1).contiguous()
    mom_inf_cl = torch.cat([mom[:, :c], torch.clamp(_planted(lv, inf_only), -30.0, 20.0)], dim=1).contiguous()
    kl_inf, kl_cl = K.diag_gaussian_kl(mom_inf.to(dev)).cpu(), K.diag_gaussian_kl(mom_inf_cl.to(dev)).cpu()
    tm = EC.kl_terms(mom_inf)
    assert EC.same_bits(kl_inf.reshape(1), kl_cl.reshape(1)) == 0 and abs(float(kl_inf.double()) - tm["out"]) <= tm["E"], (case, float(kl_inf), tm)
    print(f"[measured] diag_gaussian_kl {EC.case_id(case)}: NaN with a NaN logvar; with +-Inf alone |err| / E {abs(float(kl_inf.double()) - tm['out']) / tm['E']:.4f}")


@pytest.mark.parametrize("shape", [(3, 8, 8, 8), (2, 3, 7, 5)], ids=EC.case_id)
def test_rows_axpby_clamp_keeps_a_nan(dev, shape):
    from medfusion_amd import kernels as K
    x = EC.scaled("axpby", shape, shape, channel_axis=1) * 4096.0          # (values on both sides of [-1, 1])
    plants = EC.clamp_plants(x.numel())
    xp = _planted(x, plants)
    mask = torch.zeros(x.numel(), dtype=torch.bool)
    mask[list(plants)] = True
    want = torch.clamp(xp, -1.0, 1.0)
    assert int(torch.isnan(want).sum()) == 1 and float(x.abs().min()) < 1.0 < float(x.abs().max())
    base = K.rows_axpby(x.to(dev), clamp=(-1.0, 1.0))
    assert EC.same_bits(base.cpu(), torch.clamp(x, -1.0, 1.0)) == 0
    got = K.rows_axpby(xp.to(dev), clamp=(-1.0, 1.0))
    _nan_aware(f"rows_axpby clamp {EC.case_id(shape)}", got, torch.isnan(want), want, base, mask.view(shape))


# ---------------------------------------------------------------- G. refusals
def _pairs_only_tensor(K, dev, shape):
    """a tensor whose values exist only as fp16 pairs: the output of the GroupNorm-apply pass with out_fp32=False"""
    x = torch.randn(shape, device=dev)
    rec, parts = K.gn_stats_partial(x, 1)
    t = K.gn_apply(x, K.GnPartials(rec, parts, 1e-5), None, None, 1, 1, split=True, bconst=float(x[0].numel()) ** 0.5, out_fp32=False)
    assert K.pairs_only(t)
    return t


def _untouched(out):
    assert bool((out == EC.SENTINEL).all()), (out != EC.SENTINEL).nonzero()[:8].tolist()


def test_wrappers_refuse_what_the_kernels_would_misread(dev):
    from medfusion_amd import kernels as K
    S = EC.SENTINEL
    x = EC.tagged(2, 4, 6, 8).to(dev)
    # layout: a permuted view would be transposed by its storage, an fp64 tensor read as floats
    with pytest.raises(REFUSED, match="contiguous"):
        K.nhwc_to_nchw(x.permute(0, 2, 1, 3))
    for bad in (x.double(), x.long(), x.half()):
        with pytest.raises(REFUSED, match="fp32"):
            K.nhwc_to_nchw(bad)
        with pytest.raises(REFUSED, match="fp32"):
            K.nchw_to_nhwc(bad)
    po = _pairs_only_tensor(K, dev, (2, 4, 6, 8))
    for fn in (K.nhwc_to_nchw, K.nchw_to_nhwc, K.upsample_nearest2x, lambda t: K.avgpool2d(t, 2, 2, 0), lambda t: K.add(t, x), lambda t: K.add(x, t),
               lambda t: K.pixel_unshuffle2_add(t, torch.zeros((2, 2, 3, 32), device=dev)), lambda t: K.pixel_shuffle2_add(t, torch.zeros((2, 8, 12, 2), device=dev))):
        with pytest.raises(REFUSED, match="only as fp16 pairs"):
            fn(po)
    assert EC.same_bits(K.nhwc_to_nchw(x).cpu(), x.cpu().permute(0, 3, 1, 2).contiguous()) == 0      # (and what is right is still taken)

    with pytest.raises(REFUSED, match="fp32"):
        K.avgpool2d(x.double(), 2, 2, 0)
    with pytest.raises(REFUSED, match="2 pad <= k"):
        K.avgpool2d(x, 2, 2, 2)
    with pytest.raises(REFUSED, match="fp32"):
        K.upsample_nearest2x(x.double())

    # the shuffle pair: y of the wrong shape, dtype or strides stays untouched
    for fn, xs, good in ((K.pixel_unshuffle2_add, x, (2, 2, 3, 32)), (K.pixel_shuffle2_add, x, (2, 8, 12, 2))):
        for y, match in ((torch.full((2, 2, 3, 8), S, device=dev), "does not"), (torch.full(good, S, device=dev, dtype=torch.float64), "y must be fp32"),
                         (torch.full((good[0], good[2], good[1], good[3]), S, device=dev).permute(0, 2, 1, 3), "y must be contiguous")):
            with pytest.raises(REFUSED, match=match):
                fn(xs, y)
            _untouched(y)
        with pytest.raises(REFUSED, match="x must be fp32"):
            fn(xs.double(), torch.full(good, S, device=dev))

    # add: b and out
    a = EC.tagged(3, 5).to(dev)
    for b, out, match in ((torch.zeros((3, 4), device=dev), None, "b must have shape"), (torch.zeros((5, 3), device=dev).t(), None, "b must be contiguous"),
                          (a.double(), None, "b must be fp32"), (a, torch.full((3, 6), S, device=dev), "out must have shape"),
                          (a, torch.full((3, 5), S, device=dev, dtype=torch.float64), "out must be fp32"), (a, torch.full((5, 3), S, device=dev).t(), "out must be contiguous")):
        with pytest.raises(REFUSED, match=match):
            K.add(a, b, out=out)
        if out is not None:
            _untouched(out)

    # embedding_add
    table, idx = EC.tagged(4, 6).to(dev), torch.tensor([3, 0, 1], device=dev)
    for tb, ix, io, match in ((table, idx.float(), torch.full((3, 6), S, device=dev), "idx must be int64"), (table, idx[:2], torch.full((3, 6), S, device=dev), "one index per row"),
                              (table.double(), idx, torch.full((3, 6), S, device=dev), "table must be fp32"), (table, idx, torch.full((3, 6), S, device=dev, dtype=torch.float64), "io must be fp32"),
                              (table, idx, torch.full((3, 12), S, device=dev)[:, ::2], "io must be contiguous"), (table, idx, torch.full((3, 5), S, device=dev), r"\[B, D\]")):
        with pytest.raises(REFUSED, match=match):
            K.embedding_add(tb, ix, io)
        _untouched(io)

    # the step gathers and the broadcast
    tab, cols = EC.tagged(4, 3, 5).to(dev), torch.tensor([2, 0, 2], device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    for t, st, cl, match in ((tab.double(), 0, cols, "table 0 must be fp32"), (tab, 0, cols.int(), "cols must be int64"), (tab, 0, cols.view(3, 1), "cols must have 1 dimensions"),
                             (tab, 4, cols, "host step"), (tab, -1, cols, "host step"), (tab, step.long(), cols, "device step must be int32"),
                             (EC.tagged(4, 5, 3).to(dev).transpose(1, 2), 0, cols, "table 0 must be contiguous")):
        with pytest.raises(REFUSED, match=match):
            K.gather_step_rows(t, st, cl)
        with pytest.raises(REFUSED, match=match):
            K.gather_step_rows_multi([t], st, cl)
    with pytest.raises(REFUSED, match="table 1"):
        K.gather_step_rows_multi([tab, EC.tagged(4, 2, 5).to(dev)], 0, cols)
    t1 = EC.tagged(7).to(dev)
    for tb, st, out, match in ((t1.double(), step, torch.full((5,), S, device=dev), "table must be fp32"), (t1, step.long(), torch.full((5,), S, device=dev), "device step must be int32"),
                               (t1, step, torch.full((5,), S, device=dev, dtype=torch.float64), "out must be fp32"), (t1, step, torch.full((5, 1), S, device=dev), "out must have 1 dimensions"),
                               (t1, step, torch.full((10,), S, device=dev)[::2], "out must be contiguous")):
        with pytest.raises(REFUSED, match=match):
            K.broadcast_from_table(tb, st, out)
        _untouched(out)

    # the VAE edge, the learned embedding, the egress and the pair operand
    mom, noise = torch.zeros((2, 8, 3, 5), device=dev), torch.zeros((2, 4, 3, 5), device=dev)
    for m, nz, match in ((mom.double(), noise, "moments must be fp32"), (mom, noise.double(), "noise must be fp32"), (mom, torch.zeros((2, 4, 5, 3), device=dev), "noise must have shape"),
                         (mom, torch.zeros((2, 4, 5, 3), device=dev).transpose(2, 3), "noise must be contiguous"),
                         (torch.zeros((2, 8, 5, 3), device=dev).transpose(2, 3), noise, "moments must be contiguous")):
        with pytest.raises(REFUSED, match=match):
            K.diag_gaussian_sample(m, nz)
    with pytest.raises(REFUSED, match="moments must be fp32"):
        K.diag_gaussian_kl(mom.double())
    with pytest.raises(REFUSED, match="weights must be fp32"):
        K.learned_sinusoidal(torch.zeros(3, device=dev), torch.zeros(8, device=dev, dtype=torch.float64), 16)
    with pytest.raises(REFUSED, match="weights must have shape"):
        K.learned_sinusoidal(torch.zeros(3, device=dev), torch.zeros(8, device=dev), 18)
    with pytest.raises(REFUSED, match="x must be fp32"):
        K.image_to_uint8(torch.zeros((1, 3, 4, 4), device=dev, dtype=torch.float64))
    with pytest.raises(REFUSED, match="x must be fp32"):
        K.pack_nchw_pairs(torch.zeros((1, 3, 4, 4), device=dev, dtype=torch.float64))
    with pytest.raises(REFUSED, match="C <= cp"):
        K.pack_nchw_pairs(torch.zeros((1, 33, 4, 4), device=dev), 32)


# ---------------------------------------------------------------- S. sentinels: the entries write nothing past their outputs
def _padded(numel, dev, dtype=torch.float32, fill=EC.SENTINEL):
    return torch.full((numel + EC.PAD,), fill, dtype=dtype, device=dev)


def _tail_intact(what, buf, numel, fill=EC.SENTINEL):
    torch.cuda.synchronize()
    tail = buf[numel:].cpu()
    assert tail.numel() == EC.PAD and bool((tail == fill).all()), (what, (tail != fill).nonzero()[:8].tolist())


def test_entries_write_nothing_past_their_outputs(dev):
    """through the mf_* entries, every output allocated 64 elements longer than needed and filled with -7777: the tail is untouched and the head is what
    the wrapper returns.  Shapes with ragged last threads / blocks."""
    from medfusion_amd import kernels as K, lib as L
    lib, s = L.load(), K.stream()

    case = (2, 7, 9, 4, 3, 2, 1)
    n, h, w, c, k, st, p = case
    x = EC.pool_input(case).to(dev)
    ho, wo = EC.pool_out_hw(case)
    out = _padded(n * ho * wo * c, dev)
    L.check(lib.mf_avgpool2d_nhwc_f32(x.data_ptr(), out.data_ptr(), n, h, w, c, k, st, p, s), "mf_avgpool2d_nhwc_f32")
    _tail_intact("avgpool2d", out, n * ho * wo * c)
    assert torch.equal(out[:n * ho * wo * c].view(n, ho, wo, c), K.avgpool2d(x, k, st, p))

    case = (2, 3, 5, 36)
    x = EC.tagged(*case).to(dev)
    m = x.numel() * 4
    out = _padded(m, dev)
    L.check(lib.mf_upsample_nearest2x_nhwc_f32(x.data_ptr(), out.data_ptr(), *case, s), "mf_upsample_nearest2x_nhwc_f32")
    _tail_intact("upsample_nearest2x", out, m)
    assert torch.equal(out[:m].view(2, 6, 10, 36), K.upsample_nearest2x(x))

    case = (2, 6, 10, 5)
    xc, yc = EC.unshuffle_inputs(case)
    x, m = xc.to(dev), yc.numel()
    out = _padded(m, dev)
    out[:m] = yc.to(dev).view(-1)
    L.check(lib.mf_pixel_unshuffle2_add_nhwc_f32(x.data_ptr(), out.data_ptr(), *case, s), "mf_pixel_unshuffle2_add_nhwc_f32")
    _tail_intact("pixel_unshuffle2_add", out, m)
    assert EC.same_bits(out[:m].view(yc.shape).cpu(), EC.unshuffle_expected(xc, yc)) == 0

    case = (2, 2, 3, 12)
    xc, yc = EC.shuffle_inputs(case)
    x, m = xc.to(dev), yc.numel()
    out = _padded(m, dev)
    out[:m] = yc.to(dev).view(-1)
    L.check(lib.mf_pixel_shuffle2_add_nhwc_f32(x.data_ptr(), out.data_ptr(), *case, s), "mf_pixel_shuffle2_add_nhwc_f32")
    _tail_intact("pixel_shuffle2_add", out, m)
    assert EC.same_bits(out[:m].view(yc.shape).cpu(), EC.shuffle_expected(xc, yc)) == 0

    for name, fn, case in (("nchw_to_nhwc", lib.mf_nchw_to_nhwc_f32, (2, 33, 5, 13)), ("nhwc_to_nchw", lib.mf_nhwc_to_nchw_f32, (2, 33, 5, 13))):
        n, c, h, w = case
        xc = EC.tagged(n, c, h, w) if name == "nchw_to_nhwc" else EC.tagged(n, h, w, c)
        xd, out = xc.to(dev), _padded(xc.numel(), dev)
        L.check(fn(xd.data_ptr(), out.data_ptr(), n, c, h, w, s), name)
        _tail_intact(name, out, xc.numel())
        want = xc.permute(0, 2, 3, 1) if name == "nchw_to_nhwc" else xc.permute(0, 3, 1, 2)
        assert EC.same_bits(out[:xc.numel()].cpu(), want.contiguous().view(-1)) == 0

    table, idx, io = EC.emb_inputs(EC.EMB_CASES[1])
    m = io.numel()
    out = _padded(m, dev)
    out[:m] = io.to(dev).view(-1)
    tabd, idxd = table.to(dev), idx.to(dev)          # (kept alive until the launch has run)
    L.check(lib.mf_embedding_add_f32(tabd.data_ptr(), idxd.data_ptr(), out.data_ptr(), io.shape[0], io.shape[1], table.shape[0], s), "mf_embedding_add_f32")
    _tail_intact("embedding_add", out, m)
    assert EC.same_bits(out[:m].view(io.shape).cpu(), EC.emb_expected(table, idx, io)) == 0

    t, wts = EC.sin_inputs(33)
    td, wd = t.to(dev), wts.to(dev)
    m = t.shape[0] * 34
    out = _padded(m, dev)
    L.check(lib.mf_learned_sinusoidal_f32(td.data_ptr(), wd.data_ptr(), out.data_ptr(), t.shape[0], 33, s), "mf_learned_sinusoidal_f32")
    _tail_intact("learned_sinusoidal", out, m)
    assert torch.equal(out[:m].view(t.shape[0], 34), K.learned_sinusoidal(td, wd, 33))

    S_, ncol, ln, cols = EC.GATHER_CASES[2]
    tab, colt = EC.tagged(S_, ncol, ln), torch.tensor(cols, dtype=torch.int64)
    td, cd = tab.to(dev), colt.to(dev)
    m = len(cols) * ln
    out = _padded(m, dev)
    L.check(lib.mf_gather_step_rows_f32(td.data_ptr(), cd.data_ptr(), None, S_ - 1, ncol, ln, out.data_ptr(), len(cols), s), "mf_gather_step_rows_f32")
    _tail_intact("gather_step_rows", out, m)
    assert EC.same_bits(out[:m].view(len(cols), ln).cpu(), tab[S_ - 1, colt]) == 0

    lens, S_, ncol, cols = EC.GATHER_MULTI_CASES[2]
    tabs, colt = EC.gather_tables(lens, S_, ncol), torch.tensor(cols, dtype=torch.int64)
    tds, cd = [t_.to(dev) for t_ in tabs], colt.to(dev)
    outs = [_padded(len(cols) * ln, dev) for ln in lens]
    tp = (L.c_fp * 3)(*[t_.data_ptr() for t_ in tds])
    op = (L.c_fp * 3)(*[o.data_ptr() for o in outs])
    rl = (C.c_int64 * 3)(*lens)
    L.check(lib.mf_gather_step_rows3_f32(tp, rl, op, 3, cd.data_ptr(), None, 1, ncol, len(cols), s), "mf_gather_step_rows3_f32")
    for o, t_, ln in zip(outs, tabs, lens):
        _tail_intact("gather_step_rows3", o, len(cols) * ln)
        assert EC.same_bits(o[:len(cols) * ln].view(len(cols), ln).cpu(), t_[1, colt]) == 0

    tab = EC.tagged(3).to(dev)
    out = _padded(257, dev)
    stepd = torch.tensor([2], dtype=torch.int32, device=dev)
    L.check(lib.mf_broadcast_from_table_f32(tab.data_ptr(), stepd.data_ptr(), 0, out.data_ptr(), 257, s), "mf_broadcast_from_table_f32")
    _tail_intact("broadcast_from_table", out, 257)
    assert bool((out[:257] == tab[2]).all())

    a, b = EC.tagged(257).to(dev), EC.tagged(257, start=1000).to(dev)
    out = _padded(257, dev)
    L.check(lib.mf_add_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), 257, s), "mf_add_f32")
    _tail_intact("add", out, 257)
    assert torch.equal(out[:257], K.add(a, b))

    case = EC.DG_CASES[2]
    mom, noise = EC.dg_inputs(case)
    md, nd = mom.to(dev), noise.to(dev)
    m = noise.numel()
    out = _padded(m, dev)
    L.check(lib.mf_diag_gaussian_sample_f32(md.data_ptr(), nd.data_ptr(), out.data_ptr(), *case, s), "mf_diag_gaussian_sample_f32")
    _tail_intact("diag_gaussian_sample", out, m)
    assert torch.equal(out[:m].view(noise.shape), K.diag_gaussian_sample(md, nd))
    out = _padded(1, dev)
    L.check(lib.mf_diag_gaussian_kl_f32(md.data_ptr(), out.data_ptr(), *case, s), "mf_diag_gaussian_kl_f32")
    _tail_intact("diag_gaussian_kl", out, 1)
    assert torch.equal(out[:1].reshape(()), K.diag_gaussian_kl(md))

    for mode, xc in ((0, EC.egress0_input(EC.EGRESS0_CASES[1])), (1, EC.egress1_input("chw257"))):
        xd = xc.to(dev)
        n, c, h, w = xc.shape
        out = _padded(xc.numel(), dev, dtype=torch.uint8, fill=0xA5)
        ws = _padded(2 * n, dev)
        L.check(lib.mf_image_egress_u8(xd.data_ptr(), out.data_ptr(), ws.data_ptr(), n, c, h, w, mode, s), "mf_image_egress_u8")
        _tail_intact(f"image_egress mode {mode}", out, xc.numel(), fill=0xA5)
        _tail_intact(f"image_egress mode {mode} workspace", ws, 2 * n)
        assert torch.equal(out[:xc.numel()].view(n, h, w, c), K.image_to_uint8(xd, normalize_each=bool(mode)))

    case = (3, 3, 35, 32)
    n, c, hw, cp = case
    xd = EC.pack_input(case).to(dev)
    m = n * hw * cp
    pairs, bound = _padded(m, dev, dtype=torch.int32, fill=-7777), _padded(n, dev)
    L.check(lib.mf_pack_nchw_pairs_f32(xd.data_ptr(), pairs.data_ptr(), bound.data_ptr(), n, c, hw, cp, s), "mf_pack_nchw_pairs_f32")
    _tail_intact("pack_nchw_pairs", pairs, m, fill=-7777)
    _tail_intact("pack_nchw_pairs bound", bound, n)
    t = K.pack_nchw_pairs(xd, cp)
    assert torch.equal(pairs[:m].view(n, hw, 1, cp), t._mf_split) and torch.equal(bound[:n], t._mf_bound)
    print(f"[measured] sentinels: the {EC.PAD} elements behind every output of the entries of A to E untouched")
