"""SSIM / MS-SSIM / MSE on a real MI355X (medfusion_amd/metrics.py, csrc/metrics.hip) against the fp64 plain-torch restatement of the definition
(tests/metrics_cases.py).  The rule of every comparison: the kernel's distance from fp64 is at most MARGIN = 4 times d32, the distance of the SAME
restatement run in fp32 on the CPU, computed here for every case.  Then the contract: banks and indices, determinism, independence of the batch,
the two load paths giving the same bits, the reconstruction meter, and nothing leaking into sample()."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import kernels as K
from medfusion_amd import metrics as MT
from oracle import restate as R
from oracle import synth as S
from tests import metrics_cases as MC
from tests import vq_restate as V
from tests.util import to_product_kwargs


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def kernel_terms(x, y, data_range=1.0, k=11, sigma=1.5, scales=5):
    """every per-scale sim_s / cs_s and the mse of the pairs (x[b], y[b]), as the library computes them"""
    mm = (K.rows_minmax(x), K.rows_minmax(y)) if data_range is None else None
    sim, cs, mse = MT._terms(MT.pyramid(x, scales), MT.pyramid(y, scales), None, None, x.shape[0], mm, data_range, MT.gaussian_taps(k, sigma), 0.01, 0.03, True)
    return dict(sim=sim, cs=cs, mse=mse)


def held(what, got, want64, want32, cap=None):
    d32, dk = MC.term_distance(want32, want64), MC.term_distance(got, want64)
    print(f"[measured] {what}: terms d32 {d32:.3e} kernel {dk:.3e}")
    assert dk <= MC.MARGIN * d32, (what, dk, d32)
    if cap is not None:
        assert dk <= cap, (what, dk, cap)


# ------------------------------------------------------------------------------------------------ 1. the single-scale kernel
@pytest.mark.parametrize("kind", ["recon", "flat"])
@pytest.mark.parametrize("win", list(MC.WINDOWS))
@pytest.mark.parametrize("name", list(MC.KERNEL_SHAPES))
def test_single_scale_kernel(dev, name, win, kind):
    shape, (k, sigma) = MC.KERNEL_SHAPES[name], MC.WINDOWS[win]
    x, y = (t.to(dev) for t in MC.make_inputs(kind, shape))
    want64, want32 = MC.references(kind, shape, 1.0, k, sigma, 1)
    got = kernel_terms(x, y, 1.0, k, sigma, 1)
    held(f"ssim {name} {win} {kind}", got, want64, want32, MC.FLAT_CAP if kind == "flat" else None)
    assert torch.equal(M.ssim(x, y, kernel_size=k, sigma=sigma), got["sim"][:, 0])
    # mse(): d = x - y rounds once (2 ulp on d^2), a thread adds at most eight squares in fp32 (one rounding each), fp64 from there, one final
    # rounding: at most (2 + 8 + 1) * 2^-24 = 6.6e-7 of the value
    mse64 = want64["mse"]
    assert float(((M.mse(x, y).cpu().double() - mse64).abs() / mse64).max()) <= 11 * 2.0 ** -24
    if k == 11:
        assert torch.equal(M.mse(x, y), got["mse"])
    assert M.ssim(x, y, kernel_size=k, sigma=sigma).shape == (shape[0],)


# ------------------------------------------------------------------------------------------------ 2. MS-SSIM
@pytest.mark.parametrize("data_range", [1.0, None], ids=["range1", "rangeNone"])
@pytest.mark.parametrize("kind", ["recon", "flat", "unrelated"])
@pytest.mark.parametrize("name", list(MC.MS_SHAPES))
def test_ms_ssim(dev, name, kind, data_range):
    shape = MC.MS_SHAPES[name]
    x, y = (t.to(dev) for t in MC.make_inputs(kind, shape))
    want64, want32 = MC.references(kind, shape, data_range)
    what = f"ms_ssim {name} {kind} data_range={data_range}"
    got = kernel_terms(x, y, data_range)
    held(what, got, want64, want32, MC.FLAT_CAP if kind == "flat" else None)
    if data_range is None:                                          # L of every pair: max - min of the fp32 images, exact up to one subtraction
        want_L = torch.maximum(x.flatten(1).amax(1) - x.flatten(1).amin(1), y.flatten(1).amax(1) - y.flatten(1).amin(1))
        assert torch.equal(MT.pair_range(x, y), want_L) and torch.equal(want_L.cpu(), want32["L"])
        mm = K.rows_minmax(x)
        assert torch.equal(mm[:, 0], x.flatten(1).amin(1)) and torch.equal(mm[:, 1], x.flatten(1).amax(1))
    value, terms = M.ms_ssim(x, y, data_range=data_range, return_terms=True)
    assert value.shape == (shape[0],) and terms.shape == (shape[0], 5)
    assert torch.equal(terms, torch.cat([got["cs"][:, :-1], got["sim"][:, -1:]], 1)) and torch.equal(value, M.ms_ssim(x, y, data_range=data_range))
    t64 = MC.ms_terms(want64)
    v64, v32 = MC.ref_ms_ssim(want64), MC.ref_ms_ssim(want32)
    raw = M.ms_ssim(x, y, data_range=data_range, normalize=None)
    if kind != "unrelated":
        assert float(t64.min()) >= MC.MIN_TERM                     # no clamp anywhere near: the relative comparison means something
        r32, rk = MC.rel_distance(v32, v64), MC.rel_distance(value, v64)
        print(f"[measured] {what}: value {float(v64[0]):.6f} rel d32 {r32:.3e} kernel {rk:.3e}")
        assert rk <= MC.MARGIN * r32, (what, rk, r32)
        if kind == "flat":
            assert rk <= MC.FLAT_CAP / float(t64.min()), (what, rk)
        assert torch.equal(raw, value)                               # relu changes nothing here
    else:
        neg = t64.min(dim=1).values < -0.01                          # a clearly negative cs_s: relu makes the value EXACTLY 0
        assert bool(neg.any())
        assert bool((value.cpu()[neg] == 0).all()) and bool((v64[neg] == 0).all())
        raw64 = MC.ref_ms_ssim(want64, normalize=None)
        assert torch.equal(torch.isnan(raw.cpu()), torch.isnan(raw64))   # a negative base under a fractional power, in both
        ok = t64.min(dim=1).values >= MC.MIN_TERM
        if bool(ok.any()):
            r32 = MC.rel_distance(MC.ref_ms_ssim(want32, normalize=None)[ok], raw64[ok])
            assert MC.rel_distance(raw.cpu()[ok], raw64[ok]) <= MC.MARGIN * r32


def test_refusals_on_device_tensors(dev):
    x = torch.zeros(2, 1, 176, 176, device=dev)
    with pytest.raises(ValueError, match="y:"):
        M.ms_ssim(x, x[:, :, :175])
    with pytest.raises(ValueError, match="at least 176"):
        M.ms_ssim(x[:, :, :175], x[:, :, :175])
    with pytest.raises(ValueError, match="5-D"):
        M.ssim(x[None], x[None])
    assert M.ms_ssim(x.transpose(2, 3), x.transpose(2, 3)).shape == (2,)          # non-contiguous inputs are made contiguous
    assert bool((M.ms_ssim(x, x) == 1).all()) and bool((M.mse(x, x) == 0).all())


# ------------------------------------------------------------------------------------------------ 3. banks and indices
@pytest.fixture(scope="module")
def bank(dev):
    return MC.make_bank((4, 1, 176, 176)).to(dev)


def test_pairwise_is_ms_ssim_on_the_gathered_pairs(dev, bank):
    pairs = MC.all_pairs(4)
    ix, iy = [p[0] for p in pairs], [p[1] for p in pairs]
    values, index = M.pairwise_ms_ssim(bank)
    assert index.tolist() == [list(p) for p in pairs] and index.device == bank.device
    gathered = M.ms_ssim(bank[ix], bank[iy])
    assert torch.equal(values, gathered)
    cpu = bank.cpu()
    want64, want32 = MC.ref_terms(cpu[ix], cpu[iy], torch.float64), MC.ref_terms(cpu[ix], cpu[iy], torch.float32)
    assert float(MC.ms_terms(want64).min()) >= MC.MIN_TERM
    r32, rk = MC.rel_distance(MC.ref_ms_ssim(want32), MC.ref_ms_ssim(want64)), MC.rel_distance(values, MC.ref_ms_ssim(want64))
    print(f"[measured] pairwise bank of 4: value {float(values[0]):.4f} rel d32 {r32:.3e} kernel {rk:.3e}")
    assert rk <= MC.MARGIN * r32
    assert torch.equal(M.pairwise_ms_ssim(bank, chunk=4)[0], values)            # chunks of 4 + 2 pairs
    assert torch.equal(M.pairwise_ms_ssim(bank, data_range=None)[0], M.ms_ssim(bank[ix], bank[iy], data_range=None))


def test_explicit_and_drawn_pairs(dev, bank):
    chosen = torch.tensor([[0, 1], [3, 0], [0, 2], [3, 0]])                     # image 0 four times, a pair twice, one in (j, i) order
    values, index = M.pairwise_ms_ssim(bank, chosen)
    assert index.tolist() == chosen.tolist()
    assert torch.equal(values, M.ms_ssim(bank[chosen[:, 0]], bank[chosen[:, 1]])) and torch.equal(values[1], values[3])
    assert torch.equal(M.pairwise_ms_ssim(bank, chosen.to(dev))[0], values)
    v1, i1 = M.pairwise_ms_ssim(bank, 3, seed=5)
    v2, i2 = M.pairwise_ms_ssim(bank, 3, seed=5)
    assert torch.equal(i1, i2) and torch.equal(v1, v2) and i1.shape == (3, 2)
    rows = {tuple(r) for r in i1.tolist()}
    assert len(rows) == 3 and all(0 <= i < j < 4 for i, j in rows)
    with pytest.raises(ValueError, match="pairs"):
        M.pairwise_ms_ssim(bank, torch.tensor([[0, 4]]))
    with pytest.raises(ValueError, match="pairs"):
        M.pairwise_ms_ssim(bank, 7)


# ------------------------------------------------------------------------------------------------ 4. determinism, independence of the batch
def test_same_bits_every_launch_and_whatever_the_batch(dev):
    x, y = (t.to(dev) for t in MC.make_inputs("recon", MC.MS_SHAPES["min176"]))
    first = M.ms_ssim(x, y, return_terms=True)
    again = M.ms_ssim(x, y, return_terms=True)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    alone = M.ms_ssim(x[1:2], y[1:2], return_terms=True)                          # row 1 of P = 3 against P = 1
    assert torch.equal(alone[0], first[0][1:2]) and torch.equal(alone[1], first[1][1:2])
    assert torch.equal(M.mse(x[1:2], y[1:2]), M.mse(x, y)[1:2])
    assert torch.equal(M.ms_ssim(x, y, data_range=None)[1:2], M.ms_ssim(x[1:2], y[1:2], data_range=None))


def _misaligned(t):
    """the same values, contiguous, one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


# many images per case: a path-dependent rounding of a sum shows in a few images of a hundred, not in every one
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", [(128, 1, 64, 96), (48, 2, 43, 76), (16, 1, 12, 44), MC.MS_SHAPES["min176"]], ids=["64x96", "43x76", "12x44", "ms176"])
def test_the_two_load_paths_give_the_same_bits(dev, shape, seed):
    """sim, cs and mse of an aligned call (16-byte loads) and of the same values one float further on (element by element), bit for bit"""
    for kind in ("recon", "flat"):
        x, y = (t.to(dev) for t in MC.make_inputs(kind, shape, seed))
        assert x.data_ptr() % 16 == 0 and shape[3] % 4 == 0
        xm, ym = _misaligned(x), _misaligned(y)
        a, b = kernel_terms(x, y, scales=1), kernel_terms(xm, ym, scales=1)
        for key in ("sim", "cs", "mse"):
            assert torch.equal(a[key], b[key]), (kind, key)
        assert torch.equal(M.ssim(x, y), M.ssim(xm, y)) and torch.equal(M.mse(x, y), M.mse(xm, ym)) and torch.equal(M.mse(x, y), M.mse(x, ym))
        if shape[2] >= 176:
            a, b = M.ms_ssim(x, y, return_terms=True), M.ms_ssim(xm, ym, return_terms=True)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            a, b = MT.ms_ssim_and_mse(x, y, data_range=None), MT.ms_ssim_and_mse(xm, ym, data_range=None)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_rows_minmax_returns_a_nan_like_torch(dev):
    x = MC.make_inputs("recon", (3, 1, 43, 75))[0].clone()
    x[1, 0, 17, 33] = float("nan")
    x = x.to(dev)
    mm = K.rows_minmax(x)
    assert torch.equal(mm[[0, 2], 0], x[[0, 2]].flatten(1).amin(1)) and torch.equal(mm[[0, 2], 1], x[[0, 2]].flatten(1).amax(1))
    assert bool(torch.isnan(mm[1]).all()) and bool(torch.isnan(x.flatten(1).amin(1)[1]))
    L = MT.pair_range(x, x)
    assert bool(torch.isnan(L[1])) and bool(torch.isfinite(L[[0, 2]]).all())
    assert bool(torch.isnan(M.ssim(x, x, data_range=None)[1]))


# ------------------------------------------------------------------------------------------------ 5. the reconstruction meter
def _embedder(kind, dev):
    if kind == "VAE":
        m = M.VAE(**R.tiny_vae_kwargs())
    else:
        m = M.VQVAE(**V.tiny_vq_kwargs(num_embeddings=100, deep_supervision=0))
    S.synth_state_dict(m, f"metrics.{kind}.")
    return m.to(dev).eval()


@pytest.mark.parametrize("kind", ["VAE", "VQVAE"])
def test_reconstruction_meter(dev, kind):
    emb = _embedder(kind, dev)
    x = (MC.make_inputs("recon", (4, 3, 176, 176))[0] * 2 - 1).to(dev)
    src, bare = M.PhiloxDeviceNoise(11), M.PhiloxDeviceNoise(11)
    torch.manual_seed(3)
    want_out = [emb(x[i:i + 2], noise=bare)[0].clamp(-1, 1) for i in (0, 2)]
    state_bare = torch.get_rng_state()
    torch.manual_seed(3)
    meter = M.ReconstructionMeter(emb, noise=src)
    meter.update(x[:2])
    meter.update(x[2:])
    # the meter draws nothing of its own (a VQVAE never begins its source: no draw_index on either)
    assert getattr(src, "draw_index", None) == getattr(bare, "draw_index", None) == (1 if kind == "VAE" else None)
    assert torch.equal(torch.get_rng_state(), state_bare)
    ms, err = meter.values()
    a, b = (x + 1) / 2, (torch.cat(want_out) + 1) / 2
    assert torch.equal(ms, torch.cat([M.ms_ssim(a[i:i + 2], b[i:i + 2], data_range=None) for i in (0, 2)]))
    assert torch.equal(err, torch.cat([M.mse(a[i:i + 2], b[i:i + 2]) for i in (0, 2)]))
    want_mse = ((a - b).double() ** 2).flatten(1).mean(1)
    assert float(((err.double() - want_mse).abs() / want_mse).max()) < 1e-6
    out = meter.compute()
    assert out["count"] == 4
    for key, t in (("ms_ssim", ms), ("mse", err)):
        assert out[f"{key}_mean"] == float(t.mean()) and out[f"{key}_std"] == float(torch.std(t))
    print(f"[measured] meter {kind}: MS-SSIM {out['ms_ssim_mean']:.4f} ± {out['ms_ssim_std']:.4f}, MSE {out['mse_mean']:.3e}")
    assert bool(torch.isfinite(ms).all())
    # without a source the embedder keeps its default (keyed from torch's generator): the generator ends where a bare embedder(x) leaves it
    torch.manual_seed(7)
    bare_out = emb(x[:2])[0].clamp(-1, 1)
    state_bare = torch.get_rng_state()
    torch.manual_seed(7)
    default = M.ReconstructionMeter(emb)
    default.update(x[:2])
    assert torch.equal(torch.get_rng_state(), state_bare) and default.embedder is emb
    assert torch.equal(default.values()[1], M.mse(a[:2], (bare_out + 1) / 2))


def test_reconstruction_meter_on_a_known_map(dev):
    """an "embedder" whose reconstruction is known: the meter's figures are the metric's, and not the clamp's 0"""
    x = (MC.make_inputs("recon", (4, 3, 176, 176))[0] * 2 - 1).to(dev)
    y = (MC.make_inputs("recon", (4, 3, 176, 176))[1] * 2 - 1).to(dev)
    rows = iter((y[:3] * 1.5, y[3:] * 1.5))                           # (scaled past [-1, 1]: the meter clamps)
    meter = M.ReconstructionMeter(lambda t: (next(rows), None))
    meter.update(x[:3])
    meter.update(x[3:])
    ms, err = meter.values()
    a, b = (x + 1) / 2, ((y * 1.5).clamp(-1, 1) + 1) / 2
    assert torch.equal(ms, torch.cat([M.ms_ssim(a[:3], b[:3], data_range=None), M.ms_ssim(a[3:], b[3:], data_range=None)]))
    assert torch.equal(err, torch.cat([M.mse(a[:3], b[:3]), M.mse(a[3:], b[3:])]))
    want = MC.ref_ms_ssim(MC.ref_terms(a, b, torch.float64, data_range=None))
    assert float(want.min()) > 0.3 and float(((ms.cpu().double() - want).abs() / want).max()) < 1e-4
    out = meter.compute()
    assert out["ms_ssim_mean"] == float(ms.mean()) and out["ms_ssim_std"] == float(torch.std(ms)) > 0 and out["count"] == 4


# ------------------------------------------------------------------------------------------------ 6. nothing leaks into sampling
def test_sampling_is_untouched_by_the_metrics(dev):
    ukw = R.tiny_unet_kwargs(3, "none")
    pipe = M.DiffusionPipeline(M.GaussianNoiseScheduler, M.UNet, None, R.published_scheduler_kwargs(), to_product_kwargs(ukw), clip_x0=False)
    S.synth_state_dict(pipe.noise_estimator, "metrics.unet.")
    pipe.to(dev).eval()

    def run():
        pipe.last_cmdlist_launches = 0
        return pipe.sample(2, (8, 8, 8), steps=6, noise=M.PhiloxDeviceNoise(5), loop="cmdlist"), pipe.last_cmdlist_launches

    before, launches = run()
    x, y = (t.to(dev) for t in MC.make_inputs("recon", MC.MS_SHAPES["min176"]))
    M.ms_ssim(x, y, data_range=None)
    M.pairwise_ms_ssim(x, 2)
    after, launches_after = run()
    assert torch.equal(before, after) and launches == launches_after > 0
