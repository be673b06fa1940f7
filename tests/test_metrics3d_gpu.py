"""SSIM / MS-SSIM / MSE of volumes on a real MI355X (medfusion_amd/metrics3d.py, csrc/metrics3d.hip) against the fp64 plain-torch restatement of
the definition (tests/metrics3d_cases.py: F.conv3d on the full k^3 window, F.avg_pool3d).  The rule of every comparison: the kernel's distance
from fp64 is at most MARGIN = 4 times d32, the distance of the SAME restatement run in fp32 on the CPU, computed here for every case.  Then the
contract: banks and indices, determinism, independence of the batch, the two load paths giving the same bits, the axes, the refusals, the
volume meter, and nothing leaking into sample()."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import kernels as K
from medfusion_amd import metrics as MT
from medfusion_amd import metrics3d as M3
from oracle import restate as R
from oracle import synth as S
from tests import metrics3d_cases as MC
from tests.d3_cases import VAE_CASE
from tests.util import to_product_kwargs


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def kernel_terms(x, y, data_range=1.0, k=11, sigma=1.5, scales=1):
    """every per-scale sim_s / cs_s and the mse of the pairs (x[b], y[b]), as the library computes them"""
    mm = (K.rows_minmax(x), K.rows_minmax(y)) if data_range is None else None
    sim, cs, mse = M3._terms3d(M3.pyramid3d(x, scales), M3.pyramid3d(y, scales), None, None, x.shape[0], mm, data_range, MT.gaussian_taps(k, sigma),
                               0.01, 0.03, True)
    return dict(sim=sim, cs=cs, mse=mse)


def held(what, got, want64, want32, cap=None):
    d32, dk = MC.term_distance(want32, want64), MC.term_distance(got, want64)
    print(f"[measured] {what}: terms d32 {d32:.3e} kernel {dk:.3e}")
    assert dk <= MC.MARGIN * d32, (what, dk, d32)
    if cap is not None:
        assert dk <= cap, (what, dk, cap)


# ------------------------------------------------------------------------------------------------ 1. the single-scale kernel
@pytest.mark.parametrize("kind", ["recon", "flat"])
@pytest.mark.parametrize("name,win", MC.KERNEL_CASES, ids=[f"{n}-{w}" for n, w in MC.KERNEL_CASES])
def test_single_scale_kernel(dev, name, win, kind):
    shape, (k, sigma) = MC.KERNEL_SHAPES[name], MC.WINDOWS[win]
    x, y = (t.to(dev) for t in MC.make_inputs(kind, shape))
    want64, want32 = MC.references(kind, shape, 1.0, k, sigma, 1)
    got = kernel_terms(x, y, 1.0, k, sigma, 1)
    held(f"ssim3d {name} {win} {kind}", got, want64, want32, MC.FLAT_CAP_3D if kind == "flat" else None)
    value = M.ssim3d(x, y, kernel_size=k, sigma=sigma)
    assert torch.equal(value, got["sim"][:, 0]) and value.shape == (shape[0],)
    # mse3d(): d = x - y rounds once (2 ulp on d^2), a thread adds at most n = 4 squares in fp32 (the group of four voxels it stages per plane;
    # one rounding each), fp64 from there, one final rounding: at most (2 + 4 + 1) * 2^-24 of the value
    mse64 = want64["mse"]
    bound = (2 + MC.MSE_FP32_SQUARES + 1) * 2.0 ** -24
    for got_mse in (M.mse3d(x, y), got["mse"]):
        assert float(((got_mse.cpu().double() - mse64).abs() / mse64).max()) <= bound
    if k == min(11, (min(shape[2:]) - 1) // 2 * 2 + 1):
        assert torch.equal(M.mse3d(x, y), got["mse"])


# ------------------------------------------------------------------------------------------------ 2. MS-SSIM
@pytest.mark.parametrize("data_range", [1.0, None], ids=["range1", "rangeNone"])
@pytest.mark.parametrize("kind", ["recon", "flat", "inverted"])
@pytest.mark.parametrize("name", list(MC.MS_CASES))
def test_ms_ssim3d(dev, name, kind, data_range):
    shape, k, sigma, scales = MC.MS_CASES[name]
    betas = M.betas_for(scales)
    x, y = (t.to(dev) for t in MC.make_inputs(kind, shape))
    want64, want32 = MC.references(kind, shape, data_range, k, sigma, scales)
    what = f"ms_ssim3d {name} {kind} data_range={data_range}"
    got = kernel_terms(x, y, data_range, k, sigma, scales)
    held(what, got, want64, want32, MC.FLAT_CAP_3D if kind == "flat" else None)
    if data_range is None:                                          # L of every pair: max - min of the fp32 volumes, exact up to one subtraction
        want_L = torch.maximum(x.flatten(1).amax(1) - x.flatten(1).amin(1), y.flatten(1).amax(1) - y.flatten(1).amin(1))
        assert torch.equal(M.pair_range3d(x, y), want_L) and torch.equal(want_L.cpu(), want32["L"])
    kw = dict(data_range=data_range, betas=betas, kernel_size=k, sigma=sigma)
    value, terms = M.ms_ssim3d(x, y, return_terms=True, **kw)
    assert value.shape == (shape[0],) and terms.shape == (shape[0], scales)
    assert torch.equal(terms, torch.cat([got["cs"][:, :-1], got["sim"][:, -1:]], 1)) and torch.equal(value, M.ms_ssim3d(x, y, **kw))
    t64 = MC.ms_terms(want64)
    v64, v32 = MC.ref_ms_ssim3d(want64), MC.ref_ms_ssim3d(want32)
    raw = M.ms_ssim3d(x, y, normalize=None, **kw)
    if kind != "inverted":
        assert float(t64.min()) >= MC.MIN_TERM                     # no clamp anywhere near: the relative comparison means something
        r32, rk = MC.rel_distance(v32, v64), MC.rel_distance(value, v64)
        print(f"[measured] {what}: value {float(v64[0]):.6f} rel d32 {r32:.3e} kernel {rk:.3e}")
        assert rk <= MC.MARGIN * r32, (what, rk, r32)
        if kind == "flat":
            assert rk <= MC.FLAT_CAP_3D / float(t64.min()), (what, rk)
        assert torch.equal(raw, value)                               # relu changes nothing here
    else:
        assert bool((t64.min(dim=1).values <= -0.5).all())         # a clearly negative term in EVERY row: relu makes the value EXACTLY 0 ...
        assert bool((value == 0).all()) and bool((v64 == 0).all())
        raw64 = MC.ref_ms_ssim3d(want64, normalize=None)             # ... and without it a negative base under a fractional power is NaN, in both
        assert bool(torch.isnan(raw64).all()) and bool(torch.isnan(raw).all())


@pytest.mark.parametrize("name", ["odd", "k7s3"])
def test_pyramid3d_is_avg_pool3d(dev, name):
    shape, _, _, scales = MC.MS_CASES[name]
    x = MC.make_inputs("recon", shape)[0].to(dev)
    levels = M.pyramid3d(x, scales)
    assert len(levels) == scales and torch.equal(levels[0], x)
    for lo, hi in zip(levels[:-1], levels[1:]):
        want = F.avg_pool3d(lo, 2, 2)
        assert hi.shape == want.shape == (*lo.shape[:2], lo.shape[2] // 2, lo.shape[3] // 2, lo.shape[4] // 2)
        ulp = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
        worst = float(((hi - want).abs() / ulp).max())
        print(f"[measured] pyramid3d {name} level {tuple(hi.shape)}: {worst:.1f} ulp from F.avg_pool3d, bit-equal {torch.equal(hi, want)}")
        assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 3. banks and indices
BANK = ((4, 1, 20, 22, 24), 5, 1.0, 3)


@pytest.fixture(scope="module")
def bank(dev):
    return MC.make_bank(BANK[0]).to(dev)


def _kw(data_range=1.0):
    _, k, sigma, scales = BANK
    return dict(data_range=data_range, betas=M.betas_for(scales), kernel_size=k, sigma=sigma)


def test_pairwise_is_ms_ssim3d_on_the_gathered_pairs(dev, bank):
    pairs = MC.all_pairs(4)
    ix, iy = [p[0] for p in pairs], [p[1] for p in pairs]
    values, index = M.pairwise_ms_ssim3d(bank, **_kw())
    assert index.tolist() == [list(p) for p in pairs] and index.device == bank.device
    assert torch.equal(values, M.ms_ssim3d(bank[ix], bank[iy], **_kw()))
    cpu = bank.cpu()
    ref = dict(k=BANK[1], sigma=BANK[2], scales=BANK[3])
    want64, want32 = MC.ref_terms3d(cpu[ix], cpu[iy], torch.float64, **ref), MC.ref_terms3d(cpu[ix], cpu[iy], torch.float32, **ref)
    assert float(MC.ms_terms(want64).min()) >= MC.MIN_TERM
    r32, rk = MC.rel_distance(MC.ref_ms_ssim3d(want32), MC.ref_ms_ssim3d(want64)), MC.rel_distance(values, MC.ref_ms_ssim3d(want64))
    print(f"[measured] pairwise3d bank of 4: value {float(values[0]):.4f} rel d32 {r32:.3e} kernel {rk:.3e}")
    assert rk <= MC.MARGIN * r32
    assert torch.equal(M.pairwise_ms_ssim3d(bank, chunk=4, **_kw())[0], values)            # chunks of 4 + 2 pairs
    assert torch.equal(M.pairwise_ms_ssim3d(bank, chunk=1, **_kw())[0], values)
    assert torch.equal(M.pairwise_ms_ssim3d(bank, **_kw(None))[0], M.ms_ssim3d(bank[ix], bank[iy], **_kw(None)))


def test_explicit_and_drawn_pairs(dev, bank):
    chosen = torch.tensor([[0, 1], [3, 0], [0, 2], [3, 0]])                     # volume 0 four times, a pair twice, one in (j, i) order
    values, index = M.pairwise_ms_ssim3d(bank, chosen, **_kw())
    assert index.tolist() == chosen.tolist()
    assert torch.equal(values, M.ms_ssim3d(bank[chosen[:, 0]], bank[chosen[:, 1]], **_kw())) and torch.equal(values[1], values[3])
    assert torch.equal(M.pairwise_ms_ssim3d(bank, chosen.to(dev), **_kw())[0], values)
    v1, i1 = M.pairwise_ms_ssim3d(bank, 3, seed=5, **_kw())
    v2, i2 = M.pairwise_ms_ssim3d(bank, 3, seed=5, **_kw())
    assert torch.equal(i1, i2) and torch.equal(v1, v2) and i1.shape == (3, 2)
    with pytest.raises(ValueError, match="pairs"):
        M.pairwise_ms_ssim3d(bank, torch.tensor([[0, 4]]), **_kw())


def test_an_index_outside_its_bank_is_nan_for_that_pair_only(dev, bank):
    taps = MT.gaussian_taps(5, 1.0)
    n, c, d, h, w = bank.shape
    good = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    desc = K.make_ssim3d_desc(3, c, d, h, w, n, n, taps, 0.01, 0.03, 1.0, indexed=3, want_mse=True)
    out = [torch.empty(3, device=dev) for _ in range(6)]
    K.ssim3d_pairs(bank, bank, desc, out[0], out[1], out[2], good, torch.tensor([1, 2, 3], dtype=torch.int32, device=dev))
    K.ssim3d_pairs(bank, bank, desc, out[3], out[4], out[5], good, torch.tensor([1, 4, 3], dtype=torch.int32, device=dev))
    for ok, bad in zip(out[:3], out[3:]):
        assert bool(torch.isfinite(ok).all()) and bool(torch.isnan(bad[1])) and torch.equal(bad[[0, 2]], ok[[0, 2]])
    K.ssim3d_pairs(bank, bank, desc, out[3], out[4], out[5], torch.tensor([-1, 1, 2], dtype=torch.int32, device=dev),
                   torch.tensor([1, 2, 3], dtype=torch.int32, device=dev))
    assert bool(torch.isnan(out[3][0])) and torch.equal(out[3][1:], out[0][1:])


# ------------------------------------------------------------------------------------------------ 4. determinism, independence of the batch
def test_same_bits_every_launch_and_whatever_the_batch(dev):
    shape, k, sigma, scales = MC.MS_CASES["one_window_last"]
    kw = dict(betas=M.betas_for(scales), kernel_size=k, sigma=sigma)
    x, y = (t.to(dev) for t in MC.make_inputs("recon", shape))
    first = M.ms_ssim3d(x, y, return_terms=True, **kw)
    again = M.ms_ssim3d(x, y, return_terms=True, **kw)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    alone = M.ms_ssim3d(x[1:2], y[1:2], return_terms=True, **kw)                          # row 1 of P = 3 against P = 1
    assert torch.equal(alone[0], first[0][1:2]) and torch.equal(alone[1], first[1][1:2])
    assert torch.equal(M.mse3d(x[1:2], y[1:2]), M.mse3d(x, y)[1:2])
    assert torch.equal(M.ms_ssim3d(x, y, data_range=None, **kw)[1:2], M.ms_ssim3d(x[1:2], y[1:2], data_range=None, **kw))


def _misaligned(t):
    """the same values, contiguous, one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


# many volumes per case: a path-dependent rounding of a sum shows in a few volumes of many, not in every one
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", [(32, 1, 16, 24, 32), (8, 2, 24, 43, 76)], ids=["16x24x32", "24x43x76"])
def test_the_two_load_paths_give_the_same_bits(dev, shape, seed):
    """sim, cs and mse of an aligned call (16-byte loads) and of the same values one float further on (element by element), bit for bit"""
    for kind in ("recon", "flat"):
        x, y = (t.to(dev) for t in MC.make_inputs(kind, shape, seed))
        assert x.data_ptr() % 16 == 0 and shape[4] % 4 == 0
        xm, ym = _misaligned(x), _misaligned(y)
        a, b = kernel_terms(x, y), kernel_terms(xm, ym)
        for key in ("sim", "cs", "mse"):
            assert torch.equal(a[key], b[key]), (kind, key)
        assert torch.equal(M.ssim3d(x, y), M.ssim3d(xm, y)) and torch.equal(M.mse3d(x, y), M.mse3d(xm, ym)) and torch.equal(M.mse3d(x, y), M.mse3d(x, ym))
        kw = dict(data_range=None, betas=M.betas_for(2), kernel_size=7, sigma=1.0)
        a, b = M.ms_ssim3d_and_mse(x, y, **kw), M.ms_ssim3d_and_mse(xm, ym, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ 5. the axes
def test_permuted_axes_and_non_contiguous_inputs(dev):
    """(D, H, W) -> (W, D, H): swapped extents in the descriptor would show against the oracle of the permuted volumes"""
    shape = MC.KERNEL_SHAPES["edges_scalar"]
    x, y = MC.make_inputs("recon", shape)
    xp, yp = x.permute(0, 1, 4, 2, 3), y.permute(0, 1, 4, 2, 3)
    want64, want32 = MC.ref_terms3d(xp, yp, torch.float64), MC.ref_terms3d(xp, yp, torch.float32)
    gx, gy = x.to(dev).permute(0, 1, 4, 2, 3), y.to(dev).permute(0, 1, 4, 2, 3)
    assert not gx.is_contiguous()
    got = dict(sim=M.ssim3d(gx, gy)[:, None], mse=M.mse3d(gx, gy))
    held("ssim3d edges_scalar permuted (W, D, H)", got, want64, want32)
    assert torch.equal(got["sim"][:, 0], M.ssim3d(gx.contiguous(), gy.contiguous()))


# ------------------------------------------------------------------------------------------------ 6. refusals on device tensors
def test_refusals_on_device_tensors(dev):
    x = torch.zeros(2, 1, 44, 44, 48, device=dev)
    b3 = M.betas_for(3)
    with pytest.raises(ValueError, match="y:"):
        M.ms_ssim3d(x, x[:, :, :43], betas=b3)
    with pytest.raises(ValueError, match=r"at least 44.*43 x 44 x 48.*at most 2 scale"):
        M.ms_ssim3d(x[:, :, :43], x[:, :, :43], betas=b3)
    with pytest.raises(ValueError, match="at least 176"):
        M.ms_ssim3d(x, x)                                                         # the 2-D defaults: five scales
    with pytest.raises(ValueError, match="2-D function"):
        M.ssim3d(x[0], x[0])
    with pytest.raises(ValueError, match="5-D"):
        M.ssim(x, x)                                                              # the 2-D function keeps refusing volumes
    assert M.ms_ssim3d(x.transpose(2, 3), x.transpose(2, 3), betas=b3).shape == (2,)          # non-contiguous inputs are made contiguous
    assert bool((M.ms_ssim3d(x, x, betas=b3) == 1).all()) and bool((M.mse3d(x, x) == 0).all())
    r = MC.make_inputs("recon", MC.MS_CASES["k7s3"][0])[0].to(dev)
    assert bool((M.ms_ssim3d(r, r, betas=b3, kernel_size=7, sigma=1.0) == 1).all()) and bool((M.mse3d(r, r) == 0).all())


# ------------------------------------------------------------------------------------------------ 7. the volume meter
METER = dict(betas=M3.betas_for(2), kernel_size=5)
METER_SHAPE = (4, 1, 16, 16, 16)      # the tiny 3-D VAE takes multiples of 8 per side; min_side3d(2, 5) = 10: 16 is the smallest


def test_volume_reconstruction_meter(dev):
    assert M.min_side3d(2, 5) == 10
    emb = M.VAE(**VAE_CASE)
    S.synth_state_dict(emb, "metrics3d.VAE.")
    emb = emb.to(dev).eval()
    x = (MC.make_inputs("recon", METER_SHAPE)[0] * 2 - 1).to(dev)
    src, bare = M.PhiloxDeviceNoise(11), M.PhiloxDeviceNoise(11)
    torch.manual_seed(3)
    want_out = [emb(x[i:i + 2], noise=bare)[0].clamp(-1, 1) for i in (0, 2)]
    state_bare = torch.get_rng_state()
    torch.manual_seed(3)
    meter = M.VolumeReconstructionMeter(emb, noise=src, **METER)
    meter.update(x[:2])
    meter.update(x[2:])
    assert src.draw_index == bare.draw_index and bare.draw_index is not None     # the meter draws nothing of its own
    assert torch.equal(torch.get_rng_state(), state_bare)
    ms, err = meter.values()
    a, b = (x + 1) / 2, (torch.cat(want_out) + 1) / 2
    kw = dict(data_range=None, sigma=1.5, **METER)
    assert torch.equal(ms, torch.cat([M.ms_ssim3d(a[i:i + 2], b[i:i + 2], **kw) for i in (0, 2)]))
    assert torch.equal(err, torch.cat([M3.ms_ssim3d_and_mse(a[i:i + 2], b[i:i + 2], **kw)[1] for i in (0, 2)]))
    want_mse = ((a - b).double() ** 2).flatten(1).mean(1)
    assert float(((err.double() - want_mse).abs() / want_mse).max()) <= (2 + MC.MSE_FP32_SQUARES + 1) * 2.0 ** -24
    assert float(((M.mse3d(a, b).double() - want_mse).abs() / want_mse).max()) <= (2 + MC.MSE_FP32_SQUARES + 1) * 2.0 ** -24
    out = meter.compute()
    assert out["count"] == 4
    for key, t in (("ms_ssim", ms), ("mse", err)):
        assert out[f"{key}_mean"] == float(t.mean()) and out[f"{key}_std"] == float(torch.std(t))
    print(f"[measured] volume meter VAE: MS-SSIM {out['ms_ssim_mean']:.4f} ± {out['ms_ssim_std']:.4f}, MSE {out['mse_mean']:.3e}")
    assert bool(torch.isfinite(ms).all())
    # without a source the embedder keeps its default (keyed from torch's generator): the generator ends where a bare embedder(x) leaves it
    torch.manual_seed(7)
    bare_out = emb(x[:2])[0].clamp(-1, 1)
    state_bare = torch.get_rng_state()
    torch.manual_seed(7)
    default = M.VolumeReconstructionMeter(emb, **METER)
    default.update(x[:2])
    assert torch.equal(torch.get_rng_state(), state_bare) and default.embedder is emb
    assert torch.equal(default.values()[1], M3.ms_ssim3d_and_mse(a[:2], (bare_out + 1) / 2, **kw)[1])


def test_volume_reconstruction_meter_on_a_known_map(dev):
    """an "embedder" whose reconstruction is known: the meter's figures are the metric's, and not the clamp's 0"""
    shape = (4, 2, 20, 22, 24)
    x = (MC.make_inputs("recon", shape)[0] * 2 - 1).to(dev)
    y = (MC.make_inputs("recon", shape)[1] * 2 - 1).to(dev)
    rows = iter((y[:3] * 1.5, y[3:] * 1.5))                           # (scaled past [-1, 1]: the meter clamps)
    meter = M.VolumeReconstructionMeter(lambda t: (next(rows), None), **METER)
    meter.update(x[:3])
    meter.update(x[3:])
    ms, err = meter.values()
    a, b = (x + 1) / 2, ((y * 1.5).clamp(-1, 1) + 1) / 2
    t64 = MC.ref_terms3d(a.cpu(), b.cpu(), torch.float64, data_range=None, k=5, sigma=1.5, scales=2)
    t32 = MC.ref_terms3d(a.cpu(), b.cpu(), torch.float32, data_range=None, k=5, sigma=1.5, scales=2)
    want, want32 = MC.ref_ms_ssim3d(t64), MC.ref_ms_ssim3d(t32)
    assert float(want.min()) > 0.3 and float(MC.ms_terms(t64).min()) >= MC.MIN_TERM
    r32, rk = MC.rel_distance(want32, want), MC.rel_distance(ms, want)
    print(f"[measured] volume meter known map: value {float(want[0]):.4f} rel d32 {r32:.3e} kernel {rk:.3e}")
    assert rk <= MC.MARGIN * r32
    want_mse = t64["mse"]
    assert float(((err.cpu().double() - want_mse).abs() / want_mse).max()) <= (2 + MC.MSE_FP32_SQUARES + 1) * 2.0 ** -24
    out = meter.compute()
    assert out["ms_ssim_mean"] == float(ms.mean()) and out["ms_ssim_std"] == float(torch.std(ms)) > 0 and out["count"] == 4


# ------------------------------------------------------------------------------------------------ 8. nothing leaks into sampling
def test_sampling_is_untouched_by_the_volume_metrics(dev):
    ukw = R.tiny_unet_kwargs(3, "none")
    pipe = M.DiffusionPipeline(M.GaussianNoiseScheduler, M.UNet, None, R.published_scheduler_kwargs(), to_product_kwargs(ukw), clip_x0=False)
    S.synth_state_dict(pipe.noise_estimator, "metrics3d.unet.")
    pipe.to(dev).eval()

    def run():
        pipe.last_cmdlist_launches = 0
        return pipe.sample(2, (8, 8, 8), steps=6, noise=M.PhiloxDeviceNoise(5), loop="cmdlist"), pipe.last_cmdlist_launches

    before, launches = run()
    shape, k, sigma, scales = MC.MS_CASES["one_window_last"]
    x, y = (t.to(dev) for t in MC.make_inputs("recon", shape))
    M.ms_ssim3d(x, y, data_range=None, betas=M.betas_for(scales), kernel_size=k, sigma=sigma)
    M.pairwise_ms_ssim3d(x, 2, betas=M.betas_for(scales), kernel_size=k, sigma=sigma)
    after, launches_after = run()
    assert torch.equal(before, after) and launches == launches_after > 0
