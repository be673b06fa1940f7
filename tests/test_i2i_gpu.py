"""Image-conditioned sampling (DiffusionPipeline.sample_from: img2img and masked inpainting) on a real MI355X: the new kernels bit for bit against
ATen and against their un-fused forms, every reference fixture of tests/golden/i2i_* through the product API, and the properties of the contract
(no mask == all-ones mask == estimate_x_t + today's loop; the three loop forms give the same bits; shard invariance; kept cells are z0).

Tolerance of the fixture parity: max-norm relative error <= 1e-4, on all three fp32-class arithmetics."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from oracle import restate as R
from oracle import synth as S
from tests import i2i_cases as I
from tests.test_oracle_cpu import build_oracle_pipe
from tests.util import T, ckpt_runs, gold, oracle_noise, relerr, to_product_kwargs

ROOT = Path(__file__).resolve().parents[1]
TOL = 1e-4
DRIFT_FACTOR = 2.0     # an ill-conditioned case is held to max(TOL, 2 x the fp32 oracle's distance from its own fp64 evaluation), measured in the test


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(params=[(5, 1, 1), (1, 1, 0), (0, 1, 1)], ids=["f16x2", "split3", "fp32mfma"])
def conv_precision(request):
    """the three fp32-class conv arithmetics (MF_CONV_FP32_F16X2, MF_CONV_FP32_SPLIT3_W3, MF_CONV_FP32), as shipped"""
    from medfusion_amd import blocks as BLK
    old = BLK.CONV_PRECISION, BLK.WINOGRAD, BLK.WINOGRAD_F32
    BLK.CONV_PRECISION, BLK.WINOGRAD, BLK.WINOGRAD_F32 = request.param
    yield request.param[0]
    BLK.CONV_PRECISION, BLK.WINOGRAD, BLK.WINOGRAD_F32 = old


def _rand(name, shape, scale=1.0):
    return S.synth_input("i2i." + name, shape, scale)


def product_pipe(unet_kw, vae_kw, tag, dev, clip_x0=False, objective="x_T", estimate_variance=False, centering=False):
    pipe = M.DiffusionPipeline(noise_scheduler=M.GaussianNoiseScheduler, noise_estimator=M.UNet, latent_embedder=None,
                               noise_scheduler_kwargs=R.published_scheduler_kwargs(), noise_estimator_kwargs=to_product_kwargs(unet_kw),
                               estimator_objective=objective, estimate_variance=estimate_variance, clip_x0=clip_x0, do_input_centering=centering)
    S.synth_state_dict(pipe.noise_estimator, f"{tag}.unet.")
    if vae_kw:
        pipe.latent_embedder = M.VAE(**vae_kw)
        S.synth_state_dict(pipe.latent_embedder, f"{tag}.vae.")
    return pipe.to(dev).eval()


def tiny_pipe(dev, ncls=3, vae=True, **kw):
    return product_pipe(R.tiny_unet_kwargs(ncls, "none"), R.tiny_vae_kwargs() if vae else None, "pipe_tiny", dev, **kw)


# ------------------------------------------------------------------------------------------------ kernels
def _sched_setup(dev, steps=7, use_ddim=True):
    osch = R.GaussianNoiseScheduler(**R.published_scheduler_kwargs())
    psch = M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())
    ts, _ = psch.loop_timesteps(steps, use_ddim)
    return osch, psch, ts, psch.upload_records(psch.step_records(ts, use_ddim), dev)


def _known(osch, z0, eps0, t_next):
    """ATen's chain for the kept cells: estimate_x_t at t_next (two products rounded separately, then the sum); z0 for t_next < 0"""
    return osch.estimate_x_t(z0, torch.full((z0.shape[0],), t_next), eps0)


@pytest.mark.parametrize("mask_kind", ["random", "zeros", "ones"])
@pytest.mark.parametrize("shape", [(3, 8, 8, 8), (2, 3, 5, 7), (2, 4, 3, 5, 6)], ids=["c8", "c3_35cells", "c4_3d_90cells"])
@pytest.mark.parametrize("objective,clip", [("x_T", False), ("x_T", True), ("x_0", True), ("x_0", False)])
def test_blended_step_bit_exact(dev, objective, clip, shape, mask_kind):
    """mf_sched_step_blend_f32 against the ATen chain of test_sched_step_bit_exact followed by torch.where with the ATen-evaluated known latent:
    first, middle (DDIM mode) and last iteration (posterior mode, coefficients (1, 0)); x0 / xT stay the un-blended estimates.  Channel counts 3, 4
    and 8, cell counts 64, 35 and 90 (not multiples of the vector width)."""
    osch, psch, ts, table = _sched_setup(dev)
    rev = list(reversed(ts))
    coef = psch.blend_records(ts, 0).to(dev)
    n = shape[0]
    cells = int(np.prod(shape[2:]))
    mshape = (n, 1, *shape[2:])
    m = {"random": _rand(f"bm{shape}", mshape) > 0.1, "zeros": torch.zeros(mshape, dtype=torch.bool), "ones": torch.ones(mshape, dtype=torch.bool)}[mask_kind]
    z0, e0 = _rand("bz", shape), _rand("be", shape)
    dz, de, dm = z0.to(dev), e0.to(dev), m.to(torch.uint8).to(dev)
    for i in (0, 3, 6):
        t = torch.full((n,), rev[i], dtype=torch.long)
        x_t, pc, pu = _rand(f"bx{i}", shape), _rand(f"bp{i}", shape), _rand(f"bu{i}", shape)
        npost, nddim = _rand(f"bn{i}", shape), _rand(f"bd{i}", shape)
        g = 8.0
        pred = pu + g * (pc - pu)
        osch.noise_fn = lambda like: npost
        if objective == "x_T":
            prior, x0 = osch.estimate_x_t_prior_from_x_T(x_t, t, pred, clip_x0=clip)
            xT = pred
        else:
            prior, x0 = osch.estimate_x_t_prior_from_x_0(x_t, t, pred, clip_x0=clip)
            xT = osch.estimate_x_T(x_t, x_0=pred, t=t, clip_x0=clip)
        want = prior
        if i < 6:
            alpha, alpha_next = osch.alphas_cumprod[rev[i]], osch.alphas_cumprod[ts[7 - i - 2]]
            sigma = 1 * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
            c = (1 - alpha_next - sigma ** 2).sqrt()
            want = x0 * alpha_next.sqrt() + c * xT + sigma * nddim
        want = torch.where(m, want, _known(osch, z0, e0, rev[i + 1] if i < 6 else -1))
        d = [v.to(dev) for v in (x_t, pc, pu, npost, nddim)]
        out, x0o, xTo = (torch.empty(shape, device=dev) for _ in range(3))
        a = L.MfSchedArgs(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), None, d[3].data_ptr(), d[4].data_ptr(), 0, out.data_ptr(),
                          x0o.data_ptr(), xTo.data_ptr(), table.data_ptr(), None, i, 0 if objective == "x_T" else 1, int(clip), g, out.numel())
        bl = L.MfSchedBlend(dz.data_ptr(), de.data_ptr(), dm.data_ptr(), coef.data_ptr(), cells, shape[1], 0)
        K.sched_step_blend(a, bl)
        assert torch.equal(x0o.cpu(), x0), (i, "x0")
        assert torch.equal(xTo.cpu(), xT), (i, "xT")
        assert torch.equal(out.cpu(), want), (i, "x_t")
        if i == 6:
            assert torch.equal(out.cpu()[~m.expand(shape)], z0[~m.expand(shape)])


def test_blended_step_learned_variance(dev):
    """the learned-variance posterior under the select: the regenerated cells are mf_sched_step_f32's own values (its expf is the device's), the
    kept cells ATen's known latent, bit for bit"""
    osch, psch, _, _ = _sched_setup(dev)
    shape, tval = (2, 8, 4, 4), 5
    ts = [2, tval]
    table = psch.upload_records(psch.step_records(ts, False), dev)
    coef = psch.blend_records(ts, 0).to(dev)
    x_t, pred, pv, npost, z0, e0 = (_rand(k, shape, 0.5 if k == "vv" else 1.0).to(dev) for k in ("vx", "vp", "vv", "vn", "vz", "ve"))
    m = _rand("vm", (2, 1, 4, 4)) > 0
    dm = m.to(torch.uint8).to(dev)
    plain, blended, x0a, x0b = (torch.empty(shape, device=dev) for _ in range(4))
    mk = lambda out, x0: L.MfSchedArgs(x_t.data_ptr(), pred.data_ptr(), None, pv.data_ptr(), npost.data_ptr(), None, 0, out.data_ptr(), x0.data_ptr(), None,
                                       table.data_ptr(), None, 0, 0, 0, 1.0, out.numel())
    K.sched_step(mk(plain, x0a))
    K.sched_step_blend(mk(blended, x0b), L.MfSchedBlend(z0.data_ptr(), e0.data_ptr(), dm.data_ptr(), coef.data_ptr(), 16, 8, 0))
    want = torch.where(m, plain.cpu(), _known(osch, z0.cpu(), e0.cpu(), 2))
    assert torch.equal(blended.cpu(), want) and torch.equal(x0a, x0b)


@pytest.mark.parametrize("objective,use_ddim,cfg", [("x_T", True, False), ("x_T", True, True), ("x_0", True, False), ("x_T", False, False)])
def test_blended_loop_tail_in_one_launch_equals_its_unfused_form(dev, objective, use_ddim, cfg):
    """mf_sched_step_philox_blend_f32 against mf_philox_normal_f32 x 2 + mf_sched_step_f32 + mf_rows_axpby_f32 (the known latent) +
    mf_select_cells_f32 + mf_counter_add_i32 over a whole 7-iteration loop driven by the device counter: bit-identical at every iteration, the
    counter advances by one per launch, the ticket word returns to zero; with a row offset (a shard of a larger batch)."""
    _, psch, ts, table = _sched_setup(dev, 7, use_ddim)
    steps = len(ts)
    coef_h = psch.blend_records(ts, 0)
    coef = coef_h.to(dev)
    B, shape, seed, off, base = 5, (5, 8, 16, 24), 0x1234567890ABCDEF, 3, 1
    stride = 2 if use_ddim else 1
    xa = _rand("lt_x", shape).to(dev)
    xb = xa.clone()
    z0, e0 = _rand("lt_z", shape).to(dev), _rand("lt_e", shape).to(dev)
    dm = (_rand("lt_m", (5, 1, 16, 24)) > -0.2).to(torch.uint8).to(dev)
    x0a, x0b = torch.empty_like(xa), torch.empty_like(xa)
    n_post, n_ddim = torch.empty_like(xa), torch.empty_like(xa)
    ca = torch.zeros(1, dtype=torch.int32, device=dev)
    cb = torch.zeros(2, dtype=torch.int32, device=dev)
    obj, g = 0 if objective == "x_T" else 1, 3.0
    bl = L.MfSchedBlend(z0.data_ptr(), e0.data_ptr(), dm.data_ptr(), coef.data_ptr(), 16 * 24, 8, 0)
    for i in range(steps):
        pred = _rand(f"lt_p{i}", shape).to(dev)
        pu = _rand(f"lt_u{i}", shape).to(dev) if cfg else None
        K.philox_normal(n_post, seed, base, off, step_dev=ca, draw_stride=stride)
        if use_ddim:
            K.philox_normal(n_ddim, seed, base + 1, off, step_dev=ca, draw_stride=stride)
        a = L.MfSchedArgs(xa.data_ptr(), pred.data_ptr(), None if pu is None else pu.data_ptr(), None, n_post.data_ptr(), n_ddim.data_ptr() if use_ddim else None, 0,
                          xa.data_ptr(), x0a.data_ptr(), None, table.data_ptr(), ca.data_ptr(), 0, obj, 0, g, xa.numel())
        K.sched_step(a, outputs=(xa, x0a))
        known = K.rows_axpby(z0, coef_h[i, 0].expand(B).contiguous().to(dev), e0, coef_h[i, 1].expand(B).contiguous().to(dev))
        K.select_cells(dm, xa, known, out=xa)
        K.counter_add(ca, 1)
        b = L.MfSchedArgs(xb.data_ptr(), pred.data_ptr(), None if pu is None else pu.data_ptr(), None, None, None, 0, xb.data_ptr(), x0b.data_ptr(), None,
                          table.data_ptr(), cb.data_ptr(), 0, obj, 0, g, xb.numel())
        K.sched_step_philox_blend(b, bl, seed, base, stride, off, B, cb, outputs=(xb, x0b))
        assert torch.equal(xa, xb) and torch.equal(x0a, x0b), (i, objective, use_ddim)
        assert cb.tolist() == [i + 1, 0] and int(ca.item()) == i + 1
    keep = (dm == 0).expand(shape)
    assert torch.equal(xb[keep], z0[keep]) and bool(xb.isfinite().all())


@pytest.mark.parametrize("shape,factors", [((3, 1, 64, 64), (8, 8)), ((2, 1, 30, 20), (3, 5)), ((2, 1, 8, 16, 16), (2, 4, 8)), ((1, 1, 6, 10), (1, 1))])
@pytest.mark.parametrize("kind", ["bool", "uint8", "float"])
def test_mask_maxpool_bit_exact(dev, shape, factors, kind):
    raw = _rand(f"mp{shape}", shape)
    m = {"bool": raw > 0.8, "uint8": (raw > 0.8).to(torch.uint8) * 200, "float": raw.clamp(0, 1)}[kind]
    pool = torch.nn.functional.max_pool2d if len(factors) == 2 else torch.nn.functional.max_pool3d
    want = pool(m.float(), factors) > 0.5 if kind == "float" else pool((m != 0).float(), factors) > 0.5
    got = K.mask_maxpool(m.to(dev), factors)
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got.cpu(), want.to(torch.uint8))
    with pytest.raises(ValueError):
        K.mask_maxpool(m.to(dev), tuple(f + 1 if f > 1 else 7 for f in factors))


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (3, 8, 5, 7), (2, 4, 3, 5, 6), (1, 1, 4, 4)])
def test_select_cells_bit_exact(dev, shape):
    a, b = _rand(f"sa{shape}", shape), _rand(f"sb{shape}", shape)
    m = _rand(f"sm{shape}", (shape[0], 1, *shape[2:])) > 0
    got = K.select_cells(m.to(torch.uint8).to(dev), a.to(dev), b.to(dev))
    assert torch.equal(got.cpu(), torch.where(m, a, b))
    da = a.to(dev)
    assert K.select_cells(m.to(torch.uint8).to(dev), da, b.to(dev), out=da) is da and torch.equal(da.cpu(), torch.where(m, a, b))


@pytest.mark.parametrize("shape", [(2, 64, 64, 3), (1, 17, 23, 1), (3, 8, 8, 4)])
def test_image_ingress_bit_exact(dev, shape):
    """uint8 NHWC -> fp32 NCHW by (x / 255 - 0.5) / 0.5, every byte value, against torch's chain; egress mode 0 of the result is defined"""
    n = int(np.prod(shape))
    x = (torch.arange(n, dtype=torch.int64) * 37 % 256).to(torch.uint8).reshape(shape)
    want = ((x.permute(0, 3, 1, 2) / 255) - 0.5) / 0.5
    mean, std = torch.tensor([0.5]).view(-1, 1, 1), torch.tensor([0.5]).view(-1, 1, 1)
    assert torch.equal(want, (x.permute(0, 3, 1, 2) / 255).sub(mean).div(std))
    got = K.image_ingress(x.to(dev))
    assert got.shape == want.shape and torch.equal(got.cpu(), want.contiguous())
    assert float(got.min()) >= -1.0 and float(got.max()) <= 1.0
    assert K.image_to_uint8(got).shape == x.shape


# ------------------------------------------------------------------------------------------------ fixtures through sample_from
def _case_call(name, dev):
    c = I.CASES[name]
    x, mask, is_latent = I.case_inputs(name)
    kw = dict(steps=c["steps"], use_ddim=c["use_ddim"], is_latent=is_latent, composite=c["mask"] == "pixels")
    if mask is not None:
        kw["mask"] = mask.to(dev)
    if "condition" in c:
        kw.update(condition=torch.tensor(c["condition"], device=dev), guidance_scale=c["guidance_scale"], un_cond=None)
    if "enc_seed" in c:
        kw["encode_noise"] = oracle_noise(c["enc_seed"])
    return c, x, mask, kw


@pytest.mark.parametrize("name", list(I.CASES))
def test_fixture_through_sample_from(dev, name, conv_precision):
    """every reference fixture with the oracle's injected noise: the result and every traced x_0 within 1e-4 (max-norm relative); the same number
    of draws as the reference; the kept cells of the final latent are z0, with composite=True the kept pixels are the input's"""
    g = gold(name)
    c, x, mask, kw = _case_call(name, dev)
    unet_kw, vae_kw, tag, flags = I.pipe_args(name)
    pipe = product_pipe(unet_kw, vae_kw, tag, dev, centering=c.get("centering", False), **flags)
    noise, trace = oracle_noise(c["seed"]), []
    out = pipe.sample_from(x.to(dev), c["strength"], noise=noise, trace=trace, **kw)
    assert noise.draw_index == int(g["draws"]) and len(trace) == int(g["executed"])
    e_out = relerr(out, T(g["result"]))
    e_lat = relerr(trace[-1][1], T(g["latent"]))
    e_x0 = [relerr(trace[i][0], T(g["x0_trace"][i])) for i in range(len(trace))]
    print(f"[measured] i2i {name} arithmetic {conv_precision}: result {e_out:.1e} latent {e_lat:.1e} x0 per iteration {' '.join(f'{e:.1e}' for e in e_x0)} (tolerance {TOL:.0e})")
    tol = TOL
    if max([e_out, e_lat] + e_x0) >= TOL:      # the project's rule for an ill-conditioned case: measure the oracle's own fp64 drift on the composed loop
        tol = max(TOL, DRIFT_FACTOR * _oracle_drift(name))
        print(f"[measured] i2i {name}: fp32 oracle vs its fp64 evaluation -> tolerance {tol:.1e}")
    assert e_out < tol and e_lat < tol and max(e_x0) < tol
    if mask is not None:
        if kw["is_latent"]:
            z0 = x.to(dev)
        else:
            z0 = pipe.sample_from(x.to(dev), 1.0, steps=1, decode=False, mask=torch.zeros_like(mask).to(dev), noise=oracle_noise(c["seed"]),
                                  encode_noise=oracle_noise(c["enc_seed"]))    # (nothing regenerated: the latent that comes back is z0)
        keep = ~I.cell_mask(mask, z0.shape).to(dev).expand_as(z0)
        assert torch.equal(trace[-1][1][keep], z0[keep])
        if kw["composite"]:
            pix = mask.to(dev).expand_as(out)
            assert torch.equal(out[~pix], x.to(dev)[~pix])


def _oracle_drift(name):
    """fp32 oracle against its own fp64 evaluation on the composed loop of a case (tests/util.oracle_fp64_drift's method)"""
    import copy
    from tests.test_i2i_cpu import oracle_case

    class N64:
        def __init__(self, s):
            self.f = S.PhiloxNoise(s)

        def __call__(self, like):
            return self.f(like).double()

    c = I.CASES[name]
    ora, x, _, kw = oracle_case(name)
    w32, _ = I.composed_loop(ora, ora._randn_like, x, **kw)
    o64 = copy.deepcopy(ora).double()
    o64.set_noise_fn(N64(c["seed"]))
    enc = S.PhiloxNoise(c.get("enc_seed", 0))
    o64.latent_embedder.quantizer.noise_fn = lambda shape, device: enc(torch.empty(shape)).double()
    torch.set_default_dtype(torch.float64)
    try:
        w64, _ = I.composed_loop(o64, o64._randn_like, x.double(), **kw)
    finally:
        torch.set_default_dtype(torch.float32)
    return relerr(w32, w64)


# ------------------------------------------------------------------------------------------------ properties of the contract
@pytest.mark.parametrize("use_ddim,cond", [(True, True), (False, False)], ids=["ddim_cfg", "ddpm"])
def test_no_mask_equals_all_ones_mask_equals_estimate_x_t_plus_the_loop(dev, use_ddim, cond):
    pipe = tiny_pipe(dev)
    z0 = _rand("p.z0", (2, 8, 8, 8)).to(dev)
    extra = dict(condition=torch.tensor([2, 0], device=dev), guidance_scale=4.0, un_cond=None) if cond else {}
    steps, strength = 10, 0.6
    kw = dict(is_latent=True, steps=steps, use_ddim=use_ddim, decode=False, **extra)
    plain = pipe.sample_from(z0, strength, noise=M.PhiloxDeviceNoise(11), **kw)
    ones = pipe.sample_from(z0, strength, noise=M.PhiloxDeviceNoise(11), mask=torch.ones((2, 1, 8, 8), device=dev), **kw)
    assert torch.equal(plain, ones)
    # estimate_x_t + the last k iterations of today's loop, driven step by step through the existing single-launch API on the sliced lists
    sch = pipe.noise_scheduler
    ts, _ = sch.loop_timesteps(steps, use_ddim)
    s, k = pipe._strength_span(len(ts), strength)
    rev, recs = list(reversed(ts))[s:], sch.step_records(ts, use_ddim)[s:]
    table = sch.upload_records(recs, dev)
    src = M.PhiloxDeviceNoise(11)
    src.begin(2, dev)
    x_t = sch.estimate_x_t(z0, torch.full((2,), rev[0]), noise=src.draw((2, 8, 8, 8)))
    x0 = torch.empty_like(x_t)
    for i, t in enumerate(rev):
        pred, pu, pv = pipe._predict(x_t, torch.full((2,), float(t), device=dev), extra.get("condition"), None, extra.get("guidance_scale", 1.0), None)
        n_post = src.draw((2, 8, 8, 8))
        n_ddim = src.draw((2, 8, 8, 8)) if recs[i].mode == 1 else None
        a = L.MfSchedArgs(x_t.data_ptr(), pred.data_ptr(), None if pu is None else pu.data_ptr(), None, n_post.data_ptr(), None if n_ddim is None else n_ddim.data_ptr(),
                          0, x_t.data_ptr(), x0.data_ptr(), None, table.data_ptr(), None, i, 0, 0, float(extra.get("guidance_scale", 1.0)), x_t.numel())
        K.sched_step(a, outputs=(x_t, x0))
    assert torch.equal(plain, x_t)
    assert src.draw_index == (2 * k if use_ddim else 1 + k)


@pytest.mark.parametrize("masked", [False, True], ids=["img2img", "inpaint"])
@pytest.mark.parametrize("use_ddim,cond", [(True, True), (False, False)], ids=["ddim_cfg", "ddpm"])
def test_the_three_loop_forms_are_bit_identical(dev, use_ddim, cond, masked):
    pipe = tiny_pipe(dev)
    z0 = _rand("l.z0", (2, 8, 8, 8)).to(dev)
    extra = dict(condition=torch.tensor([1, 2], device=dev), guidance_scale=4.0, un_cond=None) if cond else {}
    m = (_rand("l.m", (2, 1, 8, 8)) > 0).to(dev) if masked else None
    kw = dict(is_latent=True, steps=12, use_ddim=use_ddim, mask=m, **extra)
    eager = pipe.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(7), loop="eager", **kw)
    pipe.last_cmdlist_launches = 0
    listed = pipe.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(7), loop="cmdlist", **kw)
    launches = pipe.last_cmdlist_launches
    graph = pipe.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(7), loop="graph", **kw)
    default = pipe.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(7), **kw)
    assert eager.shape == (2, 3, 64, 64) and bool(eager.isfinite().all())
    assert torch.equal(eager, listed) and torch.equal(eager, graph) and torch.equal(eager, default)
    assert launches > 20 and pipe.last_cmdlist_launches == launches      # the default IS the command list, the blend did not leave it
    if masked:
        lat = pipe.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(7), decode=False, **kw)
        keep = ~m.expand_as(z0)
        assert torch.equal(lat[keep], z0[keep]) and not torch.equal(lat[~keep], z0[~keep])
    with pytest.raises(ValueError):      # the replayable rule applies to k: 3 iterations of 12 are too few to record and replay
        pipe.sample_from(z0, 0.25, noise=M.PhiloxDeviceNoise(7), loop="cmdlist", **kw)


def test_mask_at_image_resolution_and_refused_shapes(dev):
    pipe = tiny_pipe(dev, centering=True)
    img = _rand("r.img", (2, 3, 64, 64), 0.5).to(dev)
    pix = torch.zeros((2, 1, 64, 64), dtype=torch.bool, device=dev)
    pix[:, :, 9:30, 17:41] = True
    kw = dict(steps=8, noise=M.PhiloxDeviceNoise(5), encode_noise=M.PhiloxDeviceNoise(6))
    a = pipe.sample_from(img, 0.5, mask=pix, decode=False, **kw)
    cells = torch.nn.functional.max_pool2d(pix.float(), 8) > 0.5
    b = pipe.sample_from(img, 0.5, mask=cells, decode=False, **kw)
    c = pipe.sample_from(img, 0.5, mask=cells.float(), decode=False, **kw)
    assert torch.equal(a, b) and torch.equal(a, c)
    out = pipe.sample_from(img, 0.5, mask=pix, composite=True, **kw)
    assert torch.equal(out[~pix.expand_as(out)], img[~pix.expand_as(img)])
    for bad in ((2, 1, 16, 16), (2, 3, 64, 64), (1, 1, 8, 8), (2, 8, 8)):
        with pytest.raises(ValueError):
            pipe.sample_from(img, 0.5, mask=torch.ones(bad, device=dev), **kw)
    with pytest.raises(ValueError):      # composite needs the mask at image resolution
        pipe.sample_from(img, 0.5, mask=cells, composite=True, **kw)
    with pytest.raises(TypeError):
        pipe.sample_from(img, 0.5, eta=0.0, **kw)


@pytest.mark.parametrize("embedder", ["latents", "vqvae"])
def test_shards_concatenate_to_the_unsharded_call(dev, embedder):
    """shard=(0, 2) ++ shard=(1, 2) == the unsharded call, bit for bit (Philox source): latents in, and images through a codebook embedder, whose
    encode draws nothing.  (VAE.encode begins its own source at row 0: with a stochastic embedder a sharded caller encodes first.)"""
    cond = torch.tensor([2, 0, 1], device=dev)
    if embedder == "latents":
        pipe = tiny_pipe(dev)
        x = _rand("s.z0", (3, 8, 8, 8)).to(dev)
        m = (_rand("s.m", (3, 1, 8, 8)) > 0).to(dev)
        kw = dict(is_latent=True)
    else:
        from tests import vq_restate as V
        pipe = tiny_pipe(dev, vae=False)
        pipe.latent_embedder = M.VQVAE(**V.tiny_vq_kwargs(num_embeddings=100, emb_channels=8, deep_supervision=0))
        S.synth_state_dict(pipe.latent_embedder, "i2i.vq.")
        pipe.to(dev).eval()
        x = _rand("s.img", (3, 3, 64, 64), 0.5).to(dev)
        m = (_rand("s.pm", (3, 1, 64, 64)) > 0.9).to(dev)
        kw = dict(composite=True)
    kw.update(steps=10, condition=cond, guidance_scale=4.0, un_cond=None, mask=m)
    full = pipe.sample_from(x, 0.6, noise=M.PhiloxDeviceNoise(21), **kw)
    parts = [pipe.sample_from(x, 0.6, noise=M.PhiloxDeviceNoise(21), shard=(r, 2), **kw) for r in range(2)]
    assert parts[0].shape[0] + parts[1].shape[0] == 3
    assert torch.equal(torch.cat(parts), full)
    # more ranks than samples: the empty shard launches nothing and returns no rows of the right shape, like sample()
    none = pipe.sample_from(x[:1], 0.6, noise=M.PhiloxDeviceNoise(21), shard=(1, 2), **dict(kw, condition=cond[:1], mask=m[:1]))
    assert none.shape == (0, *full.shape[1:])
    lat = pipe.sample_from(x[:1], 0.6, noise=M.PhiloxDeviceNoise(21), shard=(1, 2), **dict(kw, condition=cond[:1], mask=m[:1], composite=False, decode=False))
    assert lat.shape == (0, 8, 8, 8)


def test_a_rerun_of_the_loop_keeps_eps0(dev, monkeypatch):
    """K.with_fused_fallback re-runs the loop after rewinding the noise source: sample_from enters it after draw #0, so the re-run starts at draw
    #1 and eps0 is kept.  The re-run is driven here on the host (the wrapper replaced by one that always runs the loop, rewinds, runs it again);
    nothing on the device is made to fail."""
    pipe = tiny_pipe(dev)
    z0 = _rand("rr.z0", (2, 8, 8, 8)).to(dev)
    m = (_rand("rr.m", (2, 1, 8, 8)) > 0).to(dev)
    kw = dict(is_latent=True, steps=10, mask=m, decode=False)
    want_trace, got_trace = [], []
    want = pipe.sample_from(z0, 0.6, noise=M.PhiloxDeviceNoise(13), trace=want_trace, **kw)
    listed = pipe.sample_from(z0, 0.6, noise=M.PhiloxDeviceNoise(13), **kw)
    runs = []

    def twice(device, fn, rewind=None):
        if rewind is None:
            return fn()
        runs.append(fn())
        rewind()
        return fn()

    monkeypatch.setattr(K, "with_fused_fallback", twice)
    src = M.PhiloxDeviceNoise(13)
    got = pipe.sample_from(z0, 0.6, noise=src, trace=got_trace, **kw)
    assert len(runs) == 1 and torch.equal(runs[0], want) and torch.equal(got, want)
    assert len(got_trace) == len(want_trace) == 6 and src.draw_index == 12           # the trace of the first run was dropped, 2k draws in all
    assert torch.equal(pipe.sample_from(z0, 0.6, noise=M.PhiloxDeviceNoise(13), **kw), listed) and torch.equal(listed, want)


def test_three_dimensional_latents(dev):
    """spatial_dims=3 (tiny 3-D UNet + VAE of tests/d3_cases.py): the step is element-wise, NCDHW latents run through the same code.  Loop forms
    bit-identical, kept cells equal z0, all-ones mask == no mask, latent-resolution and image-resolution masks agree."""
    from tests.d3_cases import VAE_CASE, unet_kwargs
    kw = to_product_kwargs(unet_kwargs([1, 2, 2, 2], in_ch=4))
    pipe = M.DiffusionPipeline(M.GaussianNoiseScheduler, M.UNet, None, R.published_scheduler_kwargs(), kw, estimator_objective="x_T", clip_x0=False,
                               do_input_centering=False)
    S.synth_state_dict(pipe.noise_estimator, "d3.i2i.unet.")
    pipe.latent_embedder = M.VAE(**dict(VAE_CASE, emb_channels=4))
    S.synth_state_dict(pipe.latent_embedder, "d3.i2i.vae.")
    pipe.to(dev).eval()
    z0 = _rand("d3.z0", (2, 4, 4, 4, 4)).to(dev)
    m = (_rand("d3.m", (2, 1, 4, 4, 4)) > 0).to(dev)
    call = lambda **k: pipe.sample_from(z0, 0.75, is_latent=True, steps=8, noise=M.PhiloxDeviceNoise(9), decode=False, **k)
    eager, listed, graph = call(mask=m, loop="eager"), call(mask=m, loop="cmdlist"), call(mask=m, loop="graph")
    assert torch.equal(eager, listed) and torch.equal(eager, graph) and pipe.last_cmdlist_launches > 20
    keep = ~m.expand_as(z0)
    assert torch.equal(eager[keep], z0[keep]) and not torch.equal(eager[~keep], z0[~keep])
    assert torch.equal(call(), call(mask=torch.ones_like(m)))
    img = _rand("d3.img", (2, 1, 32, 32, 32), 0.5).to(dev)
    pix = torch.zeros((2, 1, 32, 32, 32), dtype=torch.bool, device=dev)
    pix[:, :, 3:12, 9:20, 15:31] = True
    cells = torch.nn.functional.max_pool3d(pix.float(), pipe.latent_embedder.scale3) > 0.5
    run = lambda mk, **k: pipe.sample_from(img, 0.5, steps=8, mask=mk, noise=M.PhiloxDeviceNoise(9), encode_noise=M.PhiloxDeviceNoise(10), **k)
    assert torch.equal(run(pix, decode=False), run(cells, decode=False))
    out = run(pix, composite=True)
    assert out.shape == img.shape and torch.equal(out[~pix], img[~pix])


def test_published_size_inpainting_against_the_oracle(dev):
    """the published architecture at the benchmarked size, once: B = 2, latent (8, 32, 32), 150 DDIM steps, strength 0.5 (75 iterations), a
    rectangular mask, against the oracle's composed loop on the host CPU with identical injected noise."""
    ora = build_oracle_pipe(R.published_unet_kwargs(2), None, "published")
    pipe = product_pipe(R.published_unet_kwargs(2), None, "published", dev)
    z0 = _rand("pub.z0", (2, 8, 32, 32))
    m = torch.zeros((2, 1, 32, 32), dtype=torch.bool)
    m[0, :, 6:20, 9:27] = True
    m[1, :, 15:32, 0:11] = True
    cond = torch.tensor([1, 0])
    torch.set_num_threads(min(32, torch.get_num_threads()))
    ora.set_noise_fn(S.PhiloxNoise(77))
    tr_o, tr_p = [], []
    want, _ = I.composed_loop(ora, ora._randn_like, z0, 0.5, 150, True, mask=m, trace=tr_o, condition=cond, guidance_scale=1.0)
    got = pipe.sample_from(z0.to(dev), 0.5, condition=cond.to(dev), mask=m.to(dev), is_latent=True, steps=150, noise=oracle_noise(77), trace=tr_p)
    assert len(tr_p) == len(tr_o) == 75
    errs = [relerr(tr_p[i][0], tr_o[i][0]) for i in range(0, 75, 5)] + [relerr(tr_p[-1][0], tr_o[-1][0])]
    e = relerr(got, want)
    print(f"[measured] i2i published size, 75 of 150 DDIM iterations, rectangular mask: x0 rel-err every 5 iterations {' '.join(f'{v:.1e}' for v in errs)} | latent {e:.1e}")
    tol = TOL
    if max(errs + [e]) >= TOL:
        import copy
        o64 = copy.deepcopy(ora).double()
        src = S.PhiloxNoise(77)
        o64.set_noise_fn(lambda like: src(like).double())
        torch.set_default_dtype(torch.float64)
        try:
            w64, _ = I.composed_loop(o64, o64._randn_like, z0.double(), 0.5, 150, True, mask=m, condition=cond, guidance_scale=1.0)
        finally:
            torch.set_default_dtype(torch.float32)
        tol = max(TOL, DRIFT_FACTOR * relerr(want, w64))
        print(f"[measured] i2i published size: fp32 oracle vs its fp64 evaluation {relerr(want, w64):.1e} -> tolerance {tol:.1e}")
    assert max(errs) < tol and e < tol
    keep = ~m.expand_as(z0)
    assert torch.equal(got.cpu()[keep], z0[keep])


def test_img2img_script_matches_sample_from(dev, tmp_path):
    """scripts/img2img.py in a child process on the checkpoint fixture: a PNG and a mask PNG in, PNG files out; the fp32 tensor it saves equals
    sample_from called directly with the same arguments, and its kept pixels are the ingress of the input bytes"""
    from PIL import Image
    runs = ckpt_runs(tmp_path)
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    rgb = (S.synth_input("i2i.png", (64, 64, 3)).abs() * 140).clamp(0, 255).to(torch.uint8)
    Image.fromarray(rgb.numpy()).save(src / "scan.png")
    mk = torch.zeros((64, 64), dtype=torch.uint8)
    mk[12:40, 20:52] = 255
    Image.fromarray(mk.numpy()).save(tmp_path / "mask.png")
    cmd = [sys.executable, str(ROOT / "scripts" / "img2img.py"), "--checkpoint", str(runs / "tiny_diffusion" / "last.ckpt"), "--images", str(src),
           "--mask", str(tmp_path / "mask.png"), "--out", str(out), "--strength", "0.6", "--steps", "8", "--seed", "3", "--save-tensor"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    assert (out / "scan.png").exists()
    saved = torch.load(out / "result.pt")
    pipe = M.DiffusionPipeline.load_from_checkpoint(str(runs / "tiny_diffusion" / "last.ckpt")).to(dev).eval()
    x = K.image_ingress(rgb.unsqueeze(0).to(dev))
    m = (mk > 0).reshape(1, 1, 64, 64).to(dev)
    want = pipe.sample_from(x, 0.6, mask=m, steps=8, composite=True, noise=M.PhiloxDeviceNoise(3), encode_noise=M.PhiloxDeviceNoise(4))
    assert torch.equal(saved.to(dev), want)
    assert torch.equal(want[~m.expand_as(want)], x[~m.expand_as(x)])
    assert np.asarray(Image.open(out / "scan.png")).shape[:2] == (64, 64)
