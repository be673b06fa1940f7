"""The held-out denoising loss on a real MI355X (csrc/loss.hip, DiffusionPipeline.validation_step / denoising_profile, ValidationMeter): the forward
process with a timestep per row against rows_axpby and philox_normal bit for bit, the error sums against their fp64 definition within the bound
derived in tests/val_cases.py, the learned-variance sums within MARGIN x the distance of their own fp32 restatement, the bits that must not depend
on the load path, the batch or the stored / regenerated target -- and the pipeline against the reference's own `_step` (tests/golden/val_*)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import kernels as K
from oracle import restate as R
from oracle import synth as S
from tests import val_cases as V
from tests.test_solver_gpu import DRIFT_FACTOR, TOL, product_pipe
from tests.util import gold, oracle_noise, to_product_kwargs

T_ = 1000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sch():
    return M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())


def shifted(t):
    """the same values 4 bytes off a 16-byte boundary: every kernel takes its element-wise path"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def i32(values, dev):
    return torch.tensor(values, dtype=torch.int32, device=dev)


# pred shape, pooling factor: aligned; a row of 30 (no multiple of 4); one partial plus a tail that is no whole quad (two partials per row, element-wise only);
# two whole partials on 16-byte loads; factors 2 and 4 onto 8 x 8 and 4 x 4 x 4 targets
LOSS_SHAPES = [((2, 4, 4, 4), 1), ((3, 3, 2, 5), 1), ((2, 1, 97, 95), 1), ((2, 9, 32, 32), 1), ((3, 2, 4, 4), 2), ((3, 2, 2, 2), 4), ((2, 2, 2, 2, 2), 2),
               ((2, 3, 1, 1, 1), 4)]
DIFFUSE_SHAPES = [(2, 4, 4, 4), (3, 3, 2, 5), (3, 1, 97, 95), (3, 9, 32, 32), (3, 2, 4, 4, 4)]


# ------------------------------------------------------------------------------------------------ 1. the forward process
@pytest.mark.parametrize("shape", DIFFUSE_SHAPES, ids=str)
def test_diffuse_rows_is_rows_axpby_on_gathered_coefficients(dev, sch, shape):
    B = shape[0]
    x0, eps = V.hash_rows("dr.x0", shape, 0.6).to(dev), V.hash_rows("dr.eps", shape).to(dev)
    tb = sch.device_tables(dev)
    a, c = tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"]
    for ts in ([0, 1, T_ - 1][:B] + [500] * (B - 3), [999, 0, 1][:B]):
        t = i32(ts, dev)
        want = sch.estimate_x_t(x0, t.long(), x_T=eps)                       # rows_axpby with the coefficients gathered on the host
        got = K.diffuse_rows(x0, t, a, c, eps=eps)
        assert torch.equal(got, want)
        assert torch.equal(K.diffuse_rows(shifted(x0), t, a, c, eps=shifted(eps), out=shifted(torch.empty_like(x0))), want)     # element by element
        x_t, drawn = sch.diffuse_rows(x0, t, eps)
        assert torch.equal(x_t, want) and drawn is eps
    # rows outside [0, T): x_0 itself below, the draw itself above (gaussian_scheduler.py:68-75)
    t = i32([-1, T_, 5][:B] if B >= 3 else [-3, T_ + 7], dev)
    for xs, es in ((x0, eps), (shifted(x0), shifted(eps))):
        got = K.diffuse_rows(xs, t, a, c, eps=es)
        assert torch.equal(got[0], x0[0]) and torch.equal(got[1], eps[1])
        if B >= 3:
            assert torch.equal(got[2], sch.estimate_x_t(x0, torch.tensor([5] * B), x_T=eps)[2])


@pytest.mark.parametrize("shape", DIFFUSE_SHAPES, ids=str)
def test_diffuse_rows_draws_what_philox_normal_writes(dev, sch, shape):
    B, per = shape[0], 1
    for s in shape[1:]:
        per *= s
    x0 = V.hash_rows("dp.x0", shape, 0.6).to(dev)
    tb = sch.device_tables(dev)
    a, c = tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"]
    t = i32([0, 1, T_ - 1][:B], dev)
    seed, draw, offset = 0x1234_5678_9ABC, 3, 11
    if per % 4:
        with pytest.raises(RuntimeError, match="multiple of 4"):
            K.diffuse_rows(x0, t, a, c, philox=(seed, draw, offset))
        src = M.PhiloxDeviceNoise(seed)
        src.begin(B, dev)
        with pytest.raises(RuntimeError, match="multiple of 4"):     # the scheduler method falls back to the source's own draw, which refuses the same shapes
            sch.diffuse_rows(x0, t, src)
        return
    eps = K.philox_normal(torch.empty_like(x0), seed, draw, offset)
    want = K.diffuse_rows(x0, t, a, c, eps=eps)
    stored = torch.empty_like(x0)
    assert torch.equal(K.diffuse_rows(x0, t, a, c, philox=(seed, draw, offset), eps_out=stored), want) and torch.equal(stored, eps)
    assert torch.equal(K.diffuse_rows(x0, t, a, c, philox=(seed, draw, offset)), want)
    with pytest.raises(RuntimeError, match="16-byte"):                 # the refusals of the solver step's draw
        K.diffuse_rows(shifted(x0), t, a, c, philox=(seed, draw, offset))
    src = M.PhiloxDeviceNoise(seed)
    src.begin(B, dev, sample_offset=offset)
    src.draw_index = draw
    x_t, kept = sch.diffuse_rows(x0, t, src, want_eps=True)
    assert torch.equal(x_t, want) and torch.equal(kept, eps) and src.draw_index == draw + 1
    x_t, kept = sch.diffuse_rows(shifted(x0), t, src)                  # an unaligned input: the source draws, the tensor form runs -- the next draw
    assert kept is not None and src.draw_index == draw + 2 and torch.equal(kept, K.philox_normal(torch.empty_like(x0), seed, draw + 1, offset))


# ------------------------------------------------------------------------------------------------ 2. the error sums
def _target_shape(shape, f):
    return (*shape[:2], *(s * f for s in shape[2:]))


@pytest.mark.parametrize("kind", ["unrelated", "close"])
@pytest.mark.parametrize("shape,f", LOSS_SHAPES, ids=str)
def test_denoise_loss_within_the_derived_bound_and_the_same_bits_everywhere(dev, shape, f, kind):
    """Largest measured |sum - fp64 sum| / bound on an MI355X: see profiles/val_parity_measured.txt."""
    tshape = _target_shape(shape, f)
    B = shape[0]
    seed, draw, offset = 77, 2, 5
    per_t = 1
    for s in tshape[1:]:
        per_t *= s
    if per_t % 4 == 0:      # the target IS a stored Philox draw, so that it can be regenerated
        target = K.philox_normal(torch.empty(tshape, device=dev), seed, draw, offset)
    else:
        target = V.hash_rows(f"dl.{kind}.t", tshape).to(dev)
    noise = V.hash_rows(f"dl.{kind}.p", shape).to(dev)
    if kind == "unrelated":
        pred = noise
    else:                   # a good prediction: d is a thousandth of the data, the pooled mean's rounding shows
        pool = torch.nn.functional.avg_pool2d if len(shape) == 4 else torch.nn.functional.avg_pool3d
        pred = ((pool(target, f) if f > 1 else target) + 1e-3 * noise).contiguous()
    got = K.denoise_loss(pred, target)
    assert got.dtype == torch.float64 and got.shape == (B, 2)
    want, fields = V.loss_sums(pred.cpu(), target.cpu())
    bound = V.loss_bound(fields)
    ratio = float(((got.cpu() - want).abs() / bound).max())
    print(f"[measured] denoise_loss {shape} f={f} {kind}: largest |sum - fp64| / bound {ratio:.3f} (sum |d| {float(want[:, 0].max()):.4g}, bound {float(bound[:, 0].max()):.3g})")
    assert ratio <= 1.0
    # the two load paths
    assert torch.equal(K.denoise_loss(shifted(pred), shifted(target)), got)
    assert torch.equal(K.denoise_loss(pred, shifted(target)), got) and torch.equal(K.denoise_loss(shifted(pred), target), got)
    # the batch and the row's place in it
    for b in range(B):
        assert torch.equal(K.denoise_loss(pred[b:b + 1], target[b:b + 1])[0], got[b])
    flip = torch.arange(B - 1, -1, -1, device=dev)
    assert torch.equal(K.denoise_loss(pred[flip].contiguous(), target[flip].contiguous()), got[flip])
    big = torch.cat([pred] * 3), torch.cat([target] * 3)
    assert torch.equal(K.denoise_loss(*big), torch.cat([got] * 3))
    # the stored and the regenerated target
    if per_t % 4 == 0:
        assert torch.equal(K.denoise_loss(pred, philox=(seed, draw, offset), target_shape=tshape), got)
        assert torch.equal(K.denoise_loss(shifted(pred), philox=(seed, draw, offset), target_shape=tshape), got)
        assert torch.equal(K.denoise_loss(pred[1:2], philox=(seed, draw, offset + 1), target_shape=(1, *tshape[1:]))[0], got[1])
    else:
        with pytest.raises(RuntimeError, match="multiple of 4"):
            K.denoise_loss(pred, philox=(seed, draw, offset), target_shape=tshape)


def test_denoise_loss_refuses_what_it_cannot_describe(dev):
    pred = torch.zeros((2, 3, 3, 3), device=dev)
    with pytest.raises(ValueError, match="multiple"):
        K.denoise_loss(pred, torch.zeros((2, 3, 8, 8), device=dev))
    with pytest.raises(ValueError, match="every side"):
        K.denoise_loss(pred, torch.zeros((2, 3, 6, 9), device=dev))
    with pytest.raises(RuntimeError, match="fp32"):
        K.denoise_loss(pred.double(), torch.zeros((2, 3, 3, 3), device=dev))
    lib = M.load_library()
    assert lib.mf_loss_parts(8192) == 1 and lib.mf_loss_parts(8193) == 2 and lib.mf_loss_parts(9216) == 2 and lib.mf_loss_parts(1 << 30) <= 256
    assert lib.mf_loss_workspace_bytes(16, 8192, 2) == 16 * 16 and lib.mf_loss_workspace_bytes(3, 9215, 3) == 3 * 2 * 24


# ------------------------------------------------------------------------------------------------ 3. the learned-variance terms
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("objective", ["x_T", "x_0"])
@pytest.mark.parametrize("shape,ts", [((3, 4, 4, 4), [0, 1, T_ - 1]), ((3, 3, 2, 5), [T_ - 1, 0, 1]), ((2, 1, 97, 95), [500, 0]), ((2, 9, 32, 32), [0, 250])], ids=str)
def test_variance_loss_against_fp64_within_four_times_fp32(dev, sch, shape, ts, objective, clip):
    """Measured on an MI355X: see profiles/val_parity_measured.txt."""
    B = shape[0]
    tb, tbd = sch.host_tables(), sch.device_tables(dev)
    t = torch.tensor(ts)
    x0, xT, pv = V.hash_rows("vl.x0", shape, 0.5), V.hash_rows("vl.xT", shape), V.hash_rows("vl.pv", shape, 0.5).clamp(-1, 1)
    xt = V.diffuse(tb, x0, xT, t, torch.float32)
    pred = (x0 if objective == "x_0" else xT) + 0.1 * V.hash_rows("vl.pred", shape)
    args = (x0, xt, xT, pred, pv)
    want64, want32 = (V.variance_sums(tb, *args, t, objective, clip, d) for d in (torch.float64, torch.float32))
    d_args = [v.to(dev) for v in args]
    t32 = t.to(dev, torch.int32)
    got = K.variance_loss(*d_args, t32, tbd, 0 if objective == "x_T" else 1, clip)
    assert got.dtype == torch.float64 and got.shape == (B, 3) and bool(got.isfinite().all())
    for k, what in enumerate(("kl", "nll", "var_scale")):
        d32, dk = float((want32[:, k].double() - want64[:, k]).abs().max()), float((got[:, k].cpu() - want64[:, k]).abs().max())
        print(f"[measured] variance_loss {shape} t={ts} {objective} clip={clip} {what}: d32 {d32:.3e} kernel {dk:.3e} (sum {float(want64[:, k].abs().max()):.4g})")
        assert dk <= V.MARGIN * d32, (what, dk, d32)
    # the same bits on the other load path, in another batch, at another place
    assert torch.equal(K.variance_loss(*(shifted(v) for v in d_args), t32, tbd, 0 if objective == "x_T" else 1, clip), got)
    for b in range(B):
        assert torch.equal(K.variance_loss(*(v[b:b + 1] for v in d_args), t32[b:b + 1], tbd, 0 if objective == "x_T" else 1, clip)[0], got[b])
    flip = torch.arange(B - 1, -1, -1, device=dev)
    assert torch.equal(K.variance_loss(*(v[flip].contiguous() for v in d_args), t32[flip].contiguous(), tbd, 0 if objective == "x_T" else 1, clip), got[flip])
    # a row without a table row says so and reads nothing
    bad = t32.clone()
    bad[0] = T_
    out = K.variance_loss(*d_args, bad, tbd, 0, clip)
    assert bool(out[0].isnan().all()) and torch.equal(out[1:], K.variance_loss(*d_args, t32, tbd, 0, clip)[1:])


# ------------------------------------------------------------------------------------------------ 4. the pipeline against the reference's `_step`
def build(name, dev):
    case = V.CASES[name]
    if not case.get("unet"):
        return product_pipe(case, dev, vae=bool(case.get("image")))
    unet_kw, vae_kw, tag, flags = V.pipe_args(case)          # (product_pipe's construction with the case's extra UNet arguments)
    pipe = M.DiffusionPipeline(noise_scheduler=M.GaussianNoiseScheduler, noise_estimator=M.UNet, latent_embedder=None,
                               noise_scheduler_kwargs=R.published_scheduler_kwargs(), noise_estimator_kwargs=to_product_kwargs(unet_kw),
                               estimator_objective=flags.get("objective", "x_T"), clip_x0=flags.get("clip_x0", False),
                               estimate_variance=flags.get("estimate_variance", False))
    S.synth_state_dict(pipe.noise_estimator, f"{tag}.unet.")
    return pipe.to(dev).eval()


def step(pipe, name, dev, noise, **kw):
    case = V.CASES[name]
    kw.setdefault("t", torch.tensor(case["t"]))
    enc = oracle_noise(case["enc_seed"]) if case.get("image") else None
    return pipe.validation_step(V.case_input(name).to(dev), V.case_condition(name, dev), noise=noise, loss=case["loss"], is_latent=not case.get("image"),
                                encode_noise=enc, **kw)


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("name", list(V.CASES))
def test_validation_step_matches_the_reference_step(dev, name, source):
    """TOL; a scalar over it is held to DRIFT_FACTOR x the distance of the reference's fp32 run from its own fp64 run (tests/test_solver_gpu.py).
    source=host: the reference's x_T uploaded (the tensor-target path); device: the same Philox stream drawn in registers."""
    case, g = V.CASES[name], gold(name)
    pipe = build(name, dev)
    noise = oracle_noise(case["seed"]) if source == "host" else M.PhiloxDeviceNoise(case["seed"])
    r = step(pipe, name, dev, noise)
    assert noise.draw_index == 1
    keys = [k for k in V.SCALARS if k in g]
    assert set(keys) == set(r) and ("variance_loss" in r) == pipe.estimate_variance
    for k in keys:
        assert r[k].dtype == torch.float64 and r[k].dim() == 0 and r[k].is_cuda
        want32, want64 = float(g[k][0]), float(g[k + "64"][0])
        e, bound = abs(float(r[k]) - want32) / abs(want32), TOL
        line = f"[measured] validation_step {name} {source} {k}: {float(r[k]):.8g} vs {want32:.8g}, {e:.1e}"
        if e >= TOL:
            drift = abs(want32 - want64) / abs(want64)
            bound = max(TOL, DRIFT_FACTOR * drift)
            line += f" (the reference's fp32 run vs its fp64 run: {drift:.1e})"
        print(f"{line}; bound {bound:.1e}")
        assert e < bound


@pytest.mark.parametrize("name", ["val_2d_xT_ds_l1", "val_2d_var_x0", "val_3d_xT"])
def test_draws_seeds_rows_and_paths(dev, name):
    case = V.CASES[name]
    pipe, B = build(name, dev), len(case["t"])
    a = step(pipe, name, dev, M.PhiloxDeviceNoise(9), per_sample=True)
    b = step(pipe, name, dev, M.PhiloxDeviceNoise(9), per_sample=True)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)                               # the same seed, the same bits
    assert not torch.equal(a["loss"], step(pipe, name, dev, M.PhiloxDeviceNoise(10))["loss"])
    assert a["t"].tolist() == case["t"] and a["t"].dtype == torch.long and a["loss_rows"].shape == (B,) and a["loss_rows"].dtype == torch.float64
    for mean, rows in (("loss", "loss_rows"), ("L1", "l1_rows"), ("L2", "l2_rows")) + ((("variance_loss", "variance_rows"),) if pipe.estimate_variance else ()):
        assert torch.equal(a[mean], a[rows].mean())
    # the stored draw (a host source replaying the device's values) gives the bits of the draw that was never stored
    eps = K.philox_normal(torch.empty((B, *V.LATENT[case["dims"]]), device=dev), 9, 0, 0).cpu()
    replay = lambda rows: M.HostNoise(lambda shape: eps[rows])
    c = step(pipe, name, dev, replay(slice(None)), per_sample=True)
    assert all(torch.equal(a[k], c[k]) for k in a)
    # t drawn by the method: torch's CPU generator, one randint; a fresh Philox key after it
    torch.manual_seed(3)
    want_t = torch.randint(0, T_, (B,))
    torch.manual_seed(3)
    d = step(pipe, name, dev, None, t=None, per_sample=True)
    assert d["t"].tolist() == want_t.tolist()
    # the rows' order: the same bits; the batch size: the estimator's convolutions are planned per batch size (tile and split-K change the order of
    # their sums), so a row's prediction moves in its last bits and the row's figures with it -- within fp32 rounding of the estimator, 1e-5
    x, cond, t = V.case_input(name).to(dev), V.case_condition(name, dev), torch.tensor(case["t"])
    flip = list(range(B - 1, -1, -1))
    f = pipe.validation_step(x[flip].contiguous(), None if cond is None else cond[flip], t=t[flip], noise=replay(flip), loss=case["loss"], is_latent=True, per_sample=True)
    for k in ("loss_rows", "l1_rows", "l2_rows"):
        assert torch.equal(f[k], a[k][flip])
    one = pipe.validation_step(x[1:2], None if cond is None else cond[1:2], t=t[1:2], noise=replay(slice(1, 2)), loss=case["loss"], is_latent=True, per_sample=True)
    for k in ("loss_rows", "l1_rows", "l2_rows"):
        e = abs(float(one[k][0]) - float(a[k][1])) / abs(float(a[k][1]))
        print(f"[measured] {name} {k}: row 1 alone vs in its batch of {B}: {e:.1e}")
        assert e < 1e-5


def test_the_ema_switch_is_honoured(dev):
    name = "val_2d_xT_ds_l1"
    pipe = build(name, dev)
    raw = step(pipe, name, dev, M.PhiloxDeviceNoise(4))
    pipe.ema_model = M.EMAModel(pipe.noise_estimator)
    S.synth_state_dict(pipe.ema_model.averaged_model, "val_ema.unet.")
    pipe.ema_model.to(dev)
    assert all(torch.equal(step(pipe, name, dev, M.PhiloxDeviceNoise(4))[k], raw[k]) for k in raw)     # use_ema is off: the raw weights
    pipe.use_ema = True
    ema = step(pipe, name, dev, M.PhiloxDeviceNoise(4))
    other = build(name, dev)
    S.synth_state_dict(other.noise_estimator, "val_ema.unet.")
    other.to(dev)
    want = step(other, name, dev, M.PhiloxDeviceNoise(4))
    assert all(torch.equal(ema[k], want[k]) for k in want) and not torch.equal(ema["loss"], raw["loss"])


class _DrawAt(M.PhiloxDeviceNoise):
    """a device source whose next draw after begin() is number `first`"""

    def __init__(self, seed, first):
        super().__init__(seed)
        self.first = first

    def begin(self, *a, **k):
        super().begin(*a, **k)
        self.draw_index = self.first


@pytest.mark.parametrize("name", ["val_2d_xT_ds_l1", "val_3d_xT"])
def test_denoising_profile_is_validation_step_over_a_grid(dev, name):
    case = V.CASES[name]
    pipe = build(name, dev)
    x, cond = V.case_input(name).to(dev), V.case_condition(name, dev)
    N, ts, draws = x.shape[0], [10, 400, 990], 2
    src = M.PhiloxDeviceNoise(21)
    prof = pipe.denoising_profile(x, cond, timesteps=ts, draws=draws, noise=src, loss=case["loss"], is_latent=True)
    assert src.draw_index == len(ts) * draws and prof["t"].tolist() == ts
    assert all(prof[k].shape == (len(ts), N) and prof[k].dtype == torch.float64 and not prof[k].is_cuda for k in ("loss", "L1", "L2"))
    for k, tk in enumerate(ts):
        acc = {key: torch.zeros(N, dtype=torch.float64, device=dev) for key in ("loss_rows", "l1_rows", "l2_rows")}
        for d in range(draws):
            r = pipe.validation_step(x, cond, t=torch.full((N,), tk), noise=_DrawAt(21, k * draws + d), loss=case["loss"], is_latent=True, per_sample=True)
            for key in acc:
                acc[key] += r[key]
        for key, rows in (("loss", "loss_rows"), ("L1", "l1_rows"), ("L2", "l2_rows")):
            assert torch.equal(prof[key][k], (acc[rows] / draws).cpu())
    assert torch.equal(prof["score"], prof["loss"].mean(0))
    # rows per estimator pass: a row keeps its sample index, so only the estimator's batch-size planning moves a figure (see above)
    split = pipe.denoising_profile(x, cond, timesteps=ts, draws=draws, noise=M.PhiloxDeviceNoise(21), loss=case["loss"], is_latent=True, batch=N - 1)
    assert float(((split["loss"] - prof["loss"]).abs() / prof["loss"].abs()).max()) < 1e-5
    default = pipe.denoising_profile(x, cond, noise=M.PhiloxDeviceNoise(21), loss=case["loss"], is_latent=True)
    assert default["t"].tolist() == pipe.noise_scheduler.loop_timesteps(20, True, "logsnr")[0] and default["loss"].shape[1] == N


def test_the_meter_is_the_mean_of_its_updates(dev):
    name = "val_2d_var_xT"
    case = V.CASES[name]
    pipe = build(name, dev)
    x = V.case_input(name).to(dev)
    meter = M.ValidationMeter(pipe, bins=4, loss=case["loss"])
    calls = [(x, torch.tensor([0, 500, 998]), 31), (x[:2], torch.tensor([249, 250]), 32), (x[1:], torch.tensor([999, 750]), 33)]
    rows = []
    for xs, t, seed in calls:
        meter.update(xs, t=t, noise=M.PhiloxDeviceNoise(seed), is_latent=True)
        rows.append(pipe.validation_step(xs, t=t, noise=M.PhiloxDeviceNoise(seed), loss=case["loss"], is_latent=True, per_sample=True))
    got = meter.compute()
    assert got["n"] == 7 and got["bins"]["edges"] == [0, 250, 500, 750, 1000] and got["bins"]["count"] == [2, 1, 1, 3]
    for mean, key in (("loss", "loss_rows"), ("L1", "l1_rows"), ("L2", "l2_rows"), ("variance_loss", "variance_rows")):
        every = torch.cat([r[key] for r in rows]).cpu()
        assert got[mean] == float(every.mean())
        t_all = torch.cat([r["t"] for r in rows]).cpu()
        for i in range(4):
            sel = every[(t_all * 4) // T_ == i]
            assert got["bins"][mean][i] == pytest.approx(float(sel.mean()), rel=1e-14)
    meter.reset()
    with pytest.raises(RuntimeError):
        meter.compute()
