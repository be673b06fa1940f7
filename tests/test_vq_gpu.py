"""The codebook quantizer (csrc/vq.hip) and the VQVAE / VQGAN / VAEGAN embedders on a real MI355X: the kernel against a CPU fp32 evaluation of
the reference's formula (latent_embedders.py:49-56) on adversarial inputs, the models against the reference's fixtures (tests/golden/vq_*), a
tiny VQGAN pipeline end to end, and pipeline checkpoints naming a VQGAN or VAEGAN."""

import pytest
import torch

import medfusion_amd as M
from medfusion_amd import kernels as K
from oracle import restate as R
from oracle import synth as S
from tests import vq_restate as V
from tests.small_edge_cases import adversarial, check_quantizer, cpu_formula, sqerr_tolerance
from tests.test_vq_cpu import KEYS, _embedder, _write_pipeline
from tests.util import T, gold, oracle_noise, relerr, to_product_kwargs

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(params=[(5, 1, 1), (5, 2, 1), (1, 1, 0), (1, 1, 2), (0, 1, 1)], ids=["f16x2", "f16x2_winograd_everywhere", "split3", "split3_winograd_everywhere", "fp32mfma"])
def conv_precision(request):
    """the fp32-class convolution arithmetics of the parity suite (tests/test_parity_gpu.py::conv_precision), for the models' convolutions"""
    from medfusion_amd import blocks as BLK
    old = BLK.CONV_PRECISION, BLK.WINOGRAD, BLK.WINOGRAD_F32
    BLK.CONV_PRECISION, BLK.WINOGRAD, BLK.WINOGRAD_F32 = request.param
    yield request.param[0]
    BLK.CONV_PRECISION, BLK.WINOGRAD, BLK.WINOGRAD_F32 = old


# ----------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("K_", [1, 1000, 8192, 16384])
@pytest.mark.parametrize("C", [1, 3, 4, 8, 16])
def test_quantizer_kernel_matches_the_reference_formula(dev, K_, C):
    shape = (3, C, 7, 11)                               # 231 pixels: not a multiple of the 256-pixel tile
    z, cb = adversarial(K_, C, shape, 1000 * K_ + C)
    zq, idx, sq = K.vector_quantize(z.to(dev), cb.to(dev), want_idx=True, want_sqerr=True)
    assert zq.shape == z.shape and idx.dtype == torch.int32 and idx.shape == (231,)
    clear, near = check_quantizer(z, cb, zq, idx, sq)
    print(f"[measured] vq K={K_} C={C}: {clear} pixels decided by margin, {near} near-ties within tau")
    if K_ > 8:
        assert int(idx[0]) not in (7, K_ - 1) and int(idx[1]) not in (7, K_ - 1)   # of three equal rows, never the higher two
    # two runs: bit-identical
    zq2, idx2, sq2 = K.vector_quantize(z.to(dev), cb.to(dev), want_idx=True, want_sqerr=True)
    assert torch.equal(zq, zq2) and torch.equal(idx, idx2) and torch.equal(sq, sq2)


def test_quantizer_kernel_nan_empty_and_refusals(dev):
    z, cb = adversarial(1000, 4, (2, 4, 17, 13), 5)     # 442 pixels
    z[1, 2, 3, 4] = float("nan")
    zq, idx, _ = K.vector_quantize(z.to(dev), cb.to(dev), want_idx=True)
    check_quantizer(z, cb, zq, idx)
    assert int(idx[17 * 13 + 3 * 13 + 4]) == 0          # every distance NaN: the first one
    cb2 = cb.clone()
    cb2[600, 1] = float("nan")                          # a NaN code: the first NaN distance beats every number, for every pixel
    z2 = z.clone()
    z2[1, 2, 3, 4] = 0.0
    zq, idx, _ = K.vector_quantize(z2.to(dev), cb2.to(dev), want_idx=True)
    assert bool((idx.cpu() == 600).all())
    assert bool((torch.argmin(cpu_formula(z2, cb2), dim=1) == 600).all())
    # N = 0: nothing launched, an empty result
    zq, idx, sq = K.vector_quantize(torch.empty((0, 4, 8, 8), device=dev), cb.to(dev), want_idx=True, want_sqerr=True)
    assert zq.shape == (0, 4, 8, 8) and idx.numel() == 0
    with pytest.raises(RuntimeError, match="code -2"):
        K.vector_quantize(torch.zeros((1, 17, 2, 2), device=dev), torch.zeros((5, 17), device=dev))
    with pytest.raises(RuntimeError, match="channels"):
        K.vector_quantize(torch.zeros((1, 4, 2, 2), device=dev), torch.zeros((5, 3), device=dev))


def test_quantizer_at_the_benchmark_shape(dev):
    """B = 16, 4 x 32 x 32, K = 8192 (VQGAN's default codebook): the split over codebook slices at a grid of 64 pixel tiles"""
    g = torch.Generator().manual_seed(3)
    cb = (torch.rand((8192, 4), generator=g) * 2 - 1) / 8192 * 4096
    z = torch.randn((16, 4, 32, 32), generator=g)
    zq, idx, sq = K.vector_quantize(z.to(dev), cb.to(dev), want_idx=True, want_sqerr=True)
    rows = [0, 15]                                      # the CPU check on two samples (pixels are independent); the loss over all
    check_quantizer(z[rows], cb, zq[rows], idx.view(16, -1)[rows].reshape(-1))
    zf = torch.moveaxis(z, 1, -1).reshape(-1, 4)
    want_sq = float(((cb[idx.cpu().long()] - zf) ** 2).double().sum())
    assert abs(float(sq) - want_sq) <= sqerr_tolerance(zf.numel(), want_sq)      # two fp64 sums of the same fp32 squares


# ----------------------------------------------------------------------------- the models against the reference's fixtures
@pytest.mark.parametrize("name,cls,kwtag,prefix", [("vq_vqvae_tiny", M.VQVAE, "VQVAE_tiny", "vqvae_tiny."),
                                                    ("vq_vqgan_tiny", M.VQGAN, "VQGAN_tiny", "vqgan_tiny.")])
def test_vq_models_against_the_reference(dev, conv_precision, name, cls, kwtag, prefix):
    """decode and forward of a tiny VQVAE (32 groups over 32 channels: one channel per group) and VQGAN against what the REFERENCE returns"""
    g = gold(name)
    m = cls(**KEYS["kwargs"][kwtag])
    S.synth_state_dict(m, prefix)
    m.to(dev).eval()
    vq = m.vqvae if hasattr(m, "vqvae") else m
    _, idx, _ = K.vector_quantize(T(g["z"]).to(dev), vq.quantizer.embedder.weight, want_idx=True)
    assert torch.equal(idx.cpu(), T(g["idx_dec"]))
    assert relerr(m.decode(T(g["z"]).to(dev)), T(g["x_dec"])) < TOL
    ze = m.encode(T(g["img"]).to(dev))
    assert relerr(ze, T(g["z_enc"])) < TOL
    _, idx, _ = K.vector_quantize(ze, vq.quantizer.embedder.weight, want_idx=True)
    assert torch.equal(idx.cpu(), T(g["idx_fwd"]))
    out, hor, loss = m(T(g["img"]).to(dev))
    assert out.shape == (2, 3, 32, 32) and len(hor) == 2
    assert relerr(out, T(g["out"])) < TOL
    assert relerr(hor[0], T(g["hor0"])) < TOL and relerr(hor[1], T(g["hor1"])) < TOL
    assert abs(float(loss) - float(g["emb_loss"][0])) <= 1e-5 * abs(float(g["emb_loss"][0]))


def test_vaegan_against_the_reference(dev, conv_precision):
    g = gold("vq_vaegan_tiny")
    m = M.VAEGAN(**V.tiny_vaegan_kwargs())
    S.synth_state_dict(m, "vaegan_tiny.")
    m.to(dev).eval()
    assert relerr(m.decode(T(g["z"]).to(dev)), T(g["x_dec"])) < TOL
    out, hor, kl = m(T(g["img"]).to(dev), noise=oracle_noise(int(g["seed"])))
    assert relerr(out, T(g["out"])) < TOL and len(hor) == 2
    assert relerr(hor[0], T(g["hor0"])) < TOL and relerr(hor[1], T(g["hor1"])) < TOL
    assert abs(float(kl) - float(g["emb_loss"][0])) <= 1e-5 * abs(float(g["emb_loss"][0]))


# ----------------------------------------------------------------------------- end to end
def test_vqgan_pipeline_end_to_end(dev):
    g = gold("vq_pipeline_tiny")
    ukw = R.tiny_unet_kwargs(None, "none", in_ch=4, out_ch=4)
    vkw = V.tiny_vq_kwargs(num_embeddings=1000, deep_supervision=0)
    pipe = M.DiffusionPipeline(noise_scheduler=M.GaussianNoiseScheduler, noise_estimator=M.UNet, latent_embedder=M.VQGAN(**vkw),
                               noise_scheduler_kwargs=R.published_scheduler_kwargs(), noise_estimator_kwargs=to_product_kwargs(ukw), clip_x0=False)
    S.synth_state_dict(pipe.noise_estimator, "vq_pipe.unet.")
    S.synth_state_dict(pipe.latent_embedder, "vq_pipe.vqgan.")
    pipe.to(dev).eval()
    n, size, steps, seed = int(g["n"]), tuple(int(v) for v in g["size"]), int(g["steps"]), int(g["seed"])
    noise = oracle_noise(seed)
    lat = pipe.sample(n, size, steps=steps, use_ddim=True, noise=noise, decode=False)
    assert noise.draw_index == int(g["draws"])
    assert lat.shape == (n, *size) and relerr(lat, T(g["latents"])) < TOL
    img = pipe.sample(n, size, steps=steps, use_ddim=True, noise=oracle_noise(seed))
    assert img.shape == (n, 3, 8 * size[1], 8 * size[2])
    # the decoder against the restated one, both fed the PRODUCT's own z_q (a near-tie after upstream drift is not a quantizer failure)
    cb = pipe.latent_embedder.vqvae.quantizer.embedder.weight
    zq, idx, _ = K.vector_quantize(lat, cb, want_idx=True)
    check_quantizer(lat.cpu(), cb.cpu(), zq, idx)
    ora = V.VQGAN(**vkw).eval()
    S.synth_state_dict(ora, "vq_pipe.vqgan.")
    with torch.no_grad():
        want = ora.vqvae.decode_quantized(zq.cpu())
    assert relerr(img, want) < TOL
    agree = float((idx.cpu() == T(g["idx"])).float().mean())
    print(f"[measured] vq pipeline: latents {relerr(lat, T(g['latents'])):.1e}, image vs restated decoder {relerr(img, want):.1e}, "
          f"indices equal to the reference's {agree:.4f} (fixture margin {float(g['margin']):.1e})")
    if float(g["margin"]) > 1e-3:
        assert agree == 1.0 and relerr(img, T(g["image"])) < TOL


@pytest.mark.parametrize("cls_name", ["VQGAN", "VAEGAN"])
def test_load_from_checkpoint_returns_images(dev, tmp_path, cls_name):
    kw = V.tiny_vq_kwargs(num_embeddings=100, deep_supervision=1) if cls_name == "VQGAN" else V.tiny_vaegan_kwargs()
    emb = _embedder(cls_name, kw, f"vqckpt_gpu.{cls_name}.")
    _write_pipeline(tmp_path, cls_name, kw, emb, baked="runs/gone/embedder.ckpt", embedder_ckpt=False)
    pipe = M.DiffusionPipeline.load_from_checkpoint(tmp_path / "last.ckpt").to(dev)
    assert type(pipe.latent_embedder) is getattr(M, cls_name)
    img = pipe.sample(2, (4, 8, 8), steps=2, use_ddim=True, noise=oracle_noise(3))
    assert img.shape == (2, 3, 64, 64) and bool(torch.isfinite(img).all())
