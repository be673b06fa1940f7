"""The deterministic few-step samplers (sampler="ddim0" / "dpmpp2m", spacing="logsnr") on a real MI355X: the solver step's kernel (front half bit
for bit against mf_sched_step_f32, back half against fp64 under a derived bound, history slots, device counter), parity with the reference at
eta = 0 (tests/golden/solver_ddim0_*), DPM-Solver++(2M) end to end against the oracle's CPU composition, and the properties of the contract
(three loop forms, one draw, inpainting, sharding, nothing leaks into the default path)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from oracle import restate as R
from oracle import synth as S
from tests import solver_cases as SC
from tests.test_oracle_cpu import build_oracle_pipe
from tests.util import T, gold, oracle_noise, relerr, to_product_kwargs

TOL = 1e-4             # the tolerance of every model-level parity test here (tests/test_parity_gpu.py, tests/test_3d_gpu.py)
DRIFT_FACTOR = 2.0     # an ill-conditioned case is held to max(TOL, 2 x the fp32 oracle's distance from its own fp64 evaluation), as in tests/test_i2i_gpu.py
SAMPLERS = ("ddim0", "dpmpp2m")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rand(name, shape, scale=1.0):
    return S.synth_input("solver." + name, shape, scale)


def product_pipe(case, dev, vae=True, **flags):
    unet_kw, vae_kw, tag, cflags = SC.pipe_args(case)
    cflags = {**cflags, **flags}
    pipe = M.DiffusionPipeline(noise_scheduler=M.GaussianNoiseScheduler, noise_estimator=M.UNet, latent_embedder=None,
                               noise_scheduler_kwargs=R.published_scheduler_kwargs(), noise_estimator_kwargs=to_product_kwargs(unet_kw),
                               estimator_objective=cflags.get("objective", "x_T"), clip_x0=cflags.get("clip_x0", False),
                               estimate_variance=cflags.get("estimate_variance", False), use_self_conditioning=cflags.get("self_cond", False))
    S.synth_state_dict(pipe.noise_estimator, f"{tag}.unet.")
    if vae_kw and vae:
        pipe.latent_embedder = M.VAE(**vae_kw)
        S.synth_state_dict(pipe.latent_embedder, f"{tag}.vae.")
    return pipe.to(dev).eval()


def oracle_pipe(case):
    unet_kw, vae_kw, tag, flags = SC.pipe_args(case)
    return build_oracle_pipe(unet_kw, vae_kw, tag, **flags)


def _sched(dev, steps, sampler, spacing=None, start=0):
    sch = M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())
    ts, _ = sch.loop_timesteps(steps, True, spacing)
    rows = sch.solver_records(ts, sampler, start=start)
    return sch, ts, rows, sch.upload_solver_records(rows, dev)


def _args(x_t, pred, pu, out, x0, xT, hist, table, objective, clip, g, step=0, counter=None, step_dev=None):
    p = lambda t: None if t is None else t.data_ptr()
    return L.MfSolverArgs(p(x_t), p(pred), p(pu), p(out), p(x0), p(xT), p(hist), p(table), p(counter), None if counter is None else counter.data_ptr() + 4,
                          p(step_dev), step, objective, clip, g, x_t.numel())


# ------------------------------------------------------------------------------------------------ 1. the kernel's front half
@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_front_half_is_the_scheduler_steps_bit_for_bit(dev, sampler, objective, cfg, clip):
    sch, ts, rows, table = _sched(dev, 7, sampler)
    old = sch.upload_records(sch.step_records(ts, True), dev)
    n = 2 * 8 * 8 * 8
    x_t, pred, pu = (_rand(f"f.{k}", (n,), 1.3).to(dev) for k in ("xt", "pred", "pu"))
    for step in (0, 3, 6):
        want = [torch.empty_like(x_t) for _ in range(3)]
        a = L.MfSchedArgs(x_t.data_ptr(), pred.data_ptr(), pu.data_ptr() if cfg else None, None, None, None, 0, want[0].data_ptr(), want[1].data_ptr(),
                          want[2].data_ptr(), old.data_ptr(), None, step, objective, clip, 3.5, n)
        K.sched_step(a)
        got = [torch.empty_like(x_t) for _ in range(3)]
        hist = torch.full((2, n), float("nan"), device=dev)
        if step > 0:
            hist[(step + 1) & 1] = _rand("f.prev", (n,)).to(dev)
        K.solver_step(_args(x_t, pred, pu if cfg else None, got[0], got[1], got[2], hist, table, objective, clip, 3.5, step=step))
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), (sampler, step)
        assert torch.equal(hist[step & 1], want[1])          # the history slot of this step holds the same x_0
        assert bool(got[0].isfinite().all())
        if clip:
            _nonfinite_pass(dev, sch, ts, table, old, x_t, pred, pu if cfg else None, step, objective, sampler)


def _nan_equal(got, want, what):
    """isnan masks equal, bits equal wherever the expected value is not NaN"""
    got, want = got.cpu(), want.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (what, "NaN mask", (torch.isnan(got) != torch.isnan(want)).nonzero()[:8].tolist())
    keep = ~torch.isnan(want)
    assert torch.equal(got.contiguous().view(torch.int32)[keep], want.contiguous().view(torch.int32)[keep]), what


def _nonfinite_pass(dev, sch, ts, table, old, x_t, pred, pu, step, objective, sampler):
    """second pass of the front half, clip_x0 only: `pred` holds a NaN and a +Inf inside a group of four and a -Inf in the last element -- at m = 1023 the
    scalar tail of the kernel.  The oracle's fp32 chain on the CPU (x_0.clamp(-1, 1) keeps a NaN) decides x_0 and x_T; mf_sched_step_f32 must agree too."""
    osch = R.GaussianNoiseScheduler(**R.published_scheduler_kwargs())
    g, t_now = 3.5, list(reversed(ts))[step]
    for m in (x_t.numel(), x_t.numel() - 1):
        xs, ps = x_t[:m].clone(), pred[:m].clone()
        us = None if pu is None else pu[:m].clone()
        for pos, v in ((5, float("nan")), (6, float("inf")), (m - 1, float("-inf"))):
            ps[pos] = v
        xc, pc_ = xs.cpu(), ps.cpu()
        pc = pc_ if us is None else us.cpu() + g * (pc_ - us.cpu())
        t = torch.full((1,), t_now, dtype=torch.long)
        if objective == 0:
            x0 = osch.estimate_x_0(xc[None], pc[None], t, clip_x0=True)[0]
            xT = pc
        else:
            x0 = pc.clamp(-1, 1)
            xT = osch.estimate_x_T(xc[None], x_0=pc[None], t=t, clip_x0=True)[0]
        assert int(torch.isnan(x0).sum()) == 1 and bool(torch.isnan(x0[5])) and bool(torch.isfinite(x0[6])) and bool(torch.isfinite(x0[m - 1]))
        want = [torch.empty_like(xs) for _ in range(3)]
        a = L.MfSchedArgs(xs.data_ptr(), ps.data_ptr(), None if us is None else us.data_ptr(), None, None, None, 0, want[0].data_ptr(), want[1].data_ptr(),
                          want[2].data_ptr(), old.data_ptr(), None, step, objective, 1, g, m)
        K.sched_step(a)
        got = [torch.empty_like(xs) for _ in range(3)]
        hist = torch.full((2, m), float("nan"), device=dev)
        if step > 0:
            hist[(step + 1) & 1] = _rand("f.prev", (x_t.numel(),)).to(dev)[:m]
        K.solver_step(_args(xs, ps, us, got[0], got[1], got[2], hist, table, objective, 1, g, step=step))
        for who, res in (("solver_step", got), ("sched_step", want)):
            _nan_equal(res[1], x0, (who, sampler, step, m, "x0"))
            _nan_equal(res[2], xT, (who, sampler, step, m, "xT"))
        _nan_equal(hist[step & 1], x0, (sampler, step, m, "history slot"))
        assert bool(torch.isnan(got[0][5])), (sampler, step, m)          # the NaN reaches the next latent, as in the reference


# ------------------------------------------------------------------------------------------------ 2. the kernel's back half
def back_half_bound(r, xi, e0, eT, prev):
    """the fp64 value of a non-final row's back half from the fp64 copies of x_t, x_0, x_T and the previous x_0, and the bound the test below
    derives for it -> (want, 4 * 2^-24 * the sum of the terms' magnitudes, that sum)"""
    if r.mode == L.SOLVER_DDIM0:
        terms = [r.B * e0, r.A * eT]
    elif r.mode == L.SOLVER_ORDER1:
        terms = [r.A * xi, r.B * e0]
    else:
        terms = [r.A * xi, r.B * e0, r.C * prev]
    want, mag = sum(terms), sum(t.abs() for t in terms)
    return want, 4 * 2.0 ** -24 * mag, mag


@pytest.mark.parametrize("n", [4096, 1023, 4098, 3])
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_back_half_against_fp64_history_slots_and_device_counter(dev, sampler, n):
    """|got - want| <= 4 * 2^-24 * (|A x_t| + |B x_0| + |C x_0_prev|): three products and two sums, each rounded once, the sums of magnitudes
    bounded by the sum of the terms' magnitudes (the DDIM chain B x_0 + A x_T is the two-term case).  want: fp64 on the CPU from the kernel's
    own fp32 x_0 / x_T (test 1 pins those).  n = 1023, 4098, 3: not whole 16-byte vectors (or a second history slot that is not aligned)."""
    sch, ts, rows, table = _sched(dev, 7, sampler)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    hist = torch.full((2, n), float("nan"), device=dev)          # a row with C == 0 must not read it
    x = _rand("b.xT", (n,)).to(dev)
    x0, xT = torch.empty_like(x), torch.empty_like(x)
    prev = None
    for i, r in enumerate(rows):
        pred = _rand(f"b.pred{i}", (n,), 0.9).to(dev)
        x_in = x.clone()
        K.solver_step(_args(x, pred, None, x, x0, xT, hist, table, 0, 0, 1.0, counter=counter))
        xi, e0, eT = x_in.double().cpu(), x0.double().cpu(), xT.double().cpu()
        if r.mode == L.SOLVER_FINAL:
            assert torch.equal(x, x0)
        else:
            want, bound, mag = back_half_bound(r, xi, e0, eT, prev)
            err = (x.double().cpu() - want).abs()
            assert bool((err <= bound).all()), (sampler, n, i, float((err / mag.clamp_min(1e-30)).max()))
        assert torch.equal(hist[i & 1], x0)                       # this step's slot; the other still holds the previous x_0 (or NaN before any)
        if prev is not None:
            assert torch.equal(hist[(i + 1) & 1].double().cpu(), prev)
        prev = e0
        assert counter.tolist() == [i + 1, 0]                     # the counter advanced inside the launch, the ticket word left zero
    assert [r.mode for r in rows] == ([1] * 6 + [0] if sampler == "ddim0" else [2, 3, 3, 3, 3, 3, 0])


def test_step_sources_agree_and_blend_selects(dev):
    """the three sources of the step index (host value, read-only device word, the counter) give the same bits; the blend variant equals the plain
    launch followed by the select on its own (mf_select_cells_f32 on a * z0 + c * eps0), vector and scalar paths"""
    for cells in (64, 63):
        B, Cc = 2, 8
        n = B * Cc * cells
        sch, ts, rows, table = _sched(dev, 6, "dpmpp2m")
        x_t, pred, pu, prevx0 = (_rand(f"s.{k}", (B, Cc, cells)).to(dev) for k in ("xt", "pred", "pu", "prev"))
        z0, eps0 = _rand("s.z0", (B, Cc, cells)).to(dev), _rand("s.eps", (B, Cc, cells)).to(dev)
        mask = (_rand("s.m", (B, 1, cells)) > 0).to(torch.uint8).to(dev)
        coef = sch.blend_records(ts).to(dev)
        bl = L.MfSchedBlend(z0.data_ptr(), eps0.data_ptr(), mask.data_ptr(), coef.data_ptr(), cells, Cc, 0)
        step = 3
        outs = []
        for src in ("host", "dev", "counter"):
            hist = torch.full((2, n), float("nan"), device=dev)
            hist[(step + 1) & 1] = prevx0.reshape(-1)
            out = torch.empty_like(x_t)
            word = torch.tensor([step, 0], dtype=torch.int32, device=dev)
            a = _args(x_t, pred, pu, out, None, None, hist, table, 0, 1, 2.5, step=step if src == "host" else 0, counter=word if src == "counter" else None,
                      step_dev=word[:1] if src == "dev" else None)
            K.solver_step(a)
            outs.append(out)
            assert word.tolist() == ([step + 1, 0] if src == "counter" else [step, 0])
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        hist = torch.full((2, n), float("nan"), device=dev)
        hist[(step + 1) & 1] = prevx0.reshape(-1)
        blended = torch.empty_like(x_t)
        K.solver_step(_args(x_t, pred, pu, blended, None, None, hist, table, 0, 1, 2.5, step=step), bl)
        a_, c_ = coef[step]
        known = K.rows_axpby(z0, a_.expand(B).contiguous(), eps0, c_.expand(B).contiguous())
        assert torch.equal(blended, K.select_cells(mask, outs[0], known))
        assert not torch.equal(blended, outs[0])


# ------------------------------------------------------------------------------------------------ 3. parity with the reference at eta = 0
@pytest.mark.parametrize("name", list(SC.DDIM0_CASES))
def test_ddim0_matches_the_reference_at_eta_zero(dev, name):
    case, g = SC.DDIM0_CASES[name], gold(name)
    pipe = product_pipe(case, dev)
    noise = oracle_noise(int(g["seed"]))
    img = pipe.sample(int(g["n"]), tuple(int(v) for v in g["size"]), steps=int(g["steps"]), sampler="ddim0", noise=noise, **SC.loop_kwargs(case, dev))
    assert noise.draw_index == 1                      # x_T only (the reference drew int(g["reference_draws"]) and multiplied the rest by zero)
    assert img.shape == tuple(g["image"].shape)
    e = relerr(img, T(g["image"]))
    print(f"[measured] ddim0 vs the reference at eta=0, {name}: {e:.1e} (tolerance {TOL:.0e})")
    assert e < TOL


# ------------------------------------------------------------------------------------------------ 4. dpmpp2m end to end
@pytest.mark.parametrize("name", list(SC.DPMPP2M_CASES))
def test_dpmpp2m_matches_the_cpu_composition(dev, name):
    """the oracle's CPU UNet (fp32, same synthetic weights) under a plain torch loop over the same (A, B, C) rows, 8 executed iterations.
    Bound: TOL; only if the case exceeds it, max(TOL, DRIFT_FACTOR x the composition's own fp32-vs-fp64 distance) -- the rule of
    tests/util.py::oracle_fp64_drift (2M extrapolates: 1 + 1/(2r) and -1/(2r) amplify a difference in x_0).
    Measured on an MI355X: see profiles/solver_parity_measured.txt."""
    case = SC.DPMPP2M_CASES[name]
    pipe = product_pipe(case, dev)
    n, size, seed = case["n"], SC.SIZE[case["dims"]], case["seed"]
    sch = pipe.noise_scheduler
    ts, executed = sch.loop_timesteps(case["steps"], True)
    assert executed == 8
    rows = sch.solver_records(ts, "dpmpp2m")
    g = None
    if case["dims"] == 3:
        # the restatement has no spatial_dims=3 UNet: the same composition ran on the reference's own 3-D pipeline (scripts/gen_solver_golden.py),
        # over the rows stored next to its result -- which must be the rows the product runs today
        g = gold(f"solver_dpmpp2m_{name}")
        assert np.array_equal(g["rows"], SC.rows_array(rows)) and int(g["seed"]) == seed and int(g["steps"]) == case["steps"]
        want = T(g["image"])
    else:
        ora = oracle_pipe(case)
        nz = S.PhiloxNoise(seed)
        x_T = nz(torch.empty((n, *size)))                 # draw #0
        ora.set_noise_fn(nz)
        want = SC.composed_solver_loop(ora, x_T, rows, **SC.loop_kwargs(case))
    noise = oracle_noise(seed)
    got = pipe.sample(n, size, steps=case["steps"], sampler="dpmpp2m", noise=noise, **SC.loop_kwargs(case, dev))
    assert noise.draw_index == 1
    e, bound = relerr(got, want), TOL
    line = f"[measured] dpmpp2m vs the CPU composition, {name}: {e:.1e}"
    if e >= TOL and g is not None:
        drift = float(g["fp64_drift"])
    elif e >= TOL:
        o64 = copy.deepcopy(ora).double()
        nz64 = S.PhiloxNoise(seed)
        o64.set_noise_fn(lambda like: nz64(like).double())
        torch.set_default_dtype(torch.float64)
        try:
            w64 = SC.composed_solver_loop(o64, x_T.double(), rows, **SC.loop_kwargs(case))
        finally:
            torch.set_default_dtype(torch.float32)
        drift = relerr(want, w64)
    if e >= TOL:
        bound = max(TOL, DRIFT_FACTOR * drift)
        line += f" (the fp32 composition vs its fp64 self: {drift:.1e})"
    print(f"{line}; bound {bound:.1e}")
    assert e < bound


# ------------------------------------------------------------------------------------------------ 5. loop forms, draws, nothing leaks
def _tiny_golden(pipe, dev):
    g = gold("sample_tiny_ddim5_uncond")
    return pipe.sample(int(g["n"]), tuple(int(v) for v in g["size"]), steps=5, use_ddim=True, noise=oracle_noise(int(g["seed"]))), T(g["image"])


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "cfg"])
@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("sampler,spacing", [("ddim0", None), ("dpmpp2m", None), ("dpmpp2m", "logsnr")])
def test_the_three_loop_forms_are_bit_identical(dev, sampler, spacing, dims, guided):
    case = dict(dims=dims, pipe=dict(tag="pipe_tiny", ncls=3) if dims == 2 else dict(tag="solver_ddim0_3d", ncls=2))
    pipe = product_pipe(case, dev)
    size = SC.SIZE[dims]
    extra = dict(condition=torch.tensor([1, 0], device=dev), guidance_scale=4.0, un_cond=None) if guided else {}
    kw = dict(steps=9, sampler=sampler, spacing=spacing, **extra)
    if dims == 2:
        before, want = _tiny_golden(pipe, dev)
        assert relerr(before, want) < TOL
    seen = []
    out = {}
    for loop in ("eager", "cmdlist", "graph", None):
        src = M.PhiloxDeviceNoise(7)
        pipe.last_cmdlist_launches, pipe.last_cmdlist_foreign_ops = 0, ["unset"]
        out[loop] = pipe.sample(2, size, noise=src, loop=loop, progress_cb=(lambda d, t: seen.append((d, t))) if loop == "eager" else None, **kw)
        assert src.draw_index == 1
        if loop in ("cmdlist", None):      # the default IS the command list; the solver step is a launch of the library
            assert pipe.last_cmdlist_foreign_ops == [] and pipe.last_cmdlist_launches > 0
    assert bool(out["eager"].isfinite().all())
    assert torch.equal(out["eager"], out["cmdlist"]) and torch.equal(out["eager"], out["graph"]) and torch.equal(out["eager"], out[None])
    executed = pipe.noise_scheduler.loop_timesteps(9, True, spacing)[1]
    assert seen == [(i + 1, executed) for i in range(executed)]
    if dims == 2:
        after, _ = _tiny_golden(pipe, dev)
        assert torch.equal(before, after)       # sampler=None: the default path, untouched by a solver run in between


def test_the_executed_count_is_what_the_caller_sees(dev):
    """a log-SNR grid that dropped duplicates: progress_cb reports the executed iterations; a host noise source does not stop the replay"""
    pipe = product_pipe(dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3)), dev, vae=False)
    executed = pipe.noise_scheduler.loop_timesteps(40, True, "logsnr")[1]
    assert executed < 40
    seen = []
    noise = oracle_noise(3)
    a = pipe.sample(2, (8, 8, 8), steps=40, sampler="dpmpp2m", spacing="logsnr", noise=noise, progress_cb=lambda d, t: seen.append((d, t)))
    assert pipe.last_cmdlist_launches > 0 and noise.draw_index == 1
    assert seen[-1] == (executed, executed) and all(t == executed for _, t in seen) and [d for d, _ in seen] == sorted(set(d for d, _ in seen))
    b = pipe.sample(2, (8, 8, 8), steps=40, sampler="dpmpp2m", spacing="logsnr", noise=oracle_noise(3), loop="eager")
    assert torch.equal(a, b)
    with pytest.raises(ValueError):      # 3 executed iterations are too few to record and replay
        pipe.sample(2, (8, 8, 8), steps=3, sampler="ddim0", noise=oracle_noise(3), loop="cmdlist")
    with pytest.raises(TypeError):
        pipe.sample(2, (8, 8, 8), steps=8, sampler="ddim0", eta=0.0)
    trace = []
    c = pipe.sample(2, (8, 8, 8), steps=40, sampler="dpmpp2m", spacing="logsnr", noise=oracle_noise(3), trace=trace)
    assert len(trace) == executed and torch.equal(c, a) and torch.equal(trace[-1][0], trace[-1][1])      # the last iteration returns its x_0


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_learned_variance_and_self_conditioning_pipelines(dev, sampler):
    """estimate_variance=True: the variance half of the estimator's output is dropped; use_self_conditioning=True: the first iteration runs with
    self_cond=None and takes the solver step too.  All loop forms give the same bits."""
    case = dict(dims=2, pipe=dict(tag="pipe_tiny_var", ncls=2))
    pipe = product_pipe(case, dev, estimate_variance=True, self_cond=True)
    kw = dict(steps=6, sampler=sampler, condition=torch.tensor([1, 0], device=dev), guidance_scale=1.0)
    outs = [pipe.sample(2, (8, 8, 8), noise=M.PhiloxDeviceNoise(5), loop=loop, **kw) for loop in ("eager", "cmdlist", "graph")]
    assert outs[0].shape == (2, 3, 64, 64) and bool(outs[0].isfinite().all())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------ 6. inpainting
@pytest.mark.parametrize("sampler,spacing", [("ddim0", None), ("dpmpp2m", None), ("dpmpp2m", "logsnr")])
def test_inpainting_keeps_its_contract(dev, sampler, spacing):
    pipe = product_pipe(dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3)), dev)
    z0 = _rand("i.z0", (2, 8, 8, 8)).to(dev)
    m = (_rand("i.m", (2, 1, 8, 8)) > 0).to(dev)
    kw = dict(is_latent=True, steps=12, mask=m, sampler=sampler, spacing=spacing, condition=torch.tensor([1, 2], device=dev), guidance_scale=4.0, un_cond=None,
              decode=False)
    lat = {}
    for loop in ("eager", "cmdlist", "graph"):
        src = M.PhiloxDeviceNoise(7)
        lat[loop] = pipe.sample_from(z0, 0.75, noise=src, loop=loop, **kw)
        assert src.draw_index == 1                    # eps0 only
    keep = ~m.expand_as(z0)
    assert torch.equal(lat["eager"][keep], z0[keep]) and not torch.equal(lat["eager"][~keep], z0[~keep])
    assert torch.equal(lat["eager"], lat["cmdlist"]) and torch.equal(lat["eager"], lat["graph"])
    assert bool(lat["eager"].isfinite().all())
    plain = pipe.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(7), **{**kw, "mask": None})
    ones = pipe.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(7), **{**kw, "mask": torch.ones((2, 1, 8, 8), device=dev)})
    assert torch.equal(plain, ones)                   # img2img == inpainting with nothing kept


# ------------------------------------------------------------------------------------------------ 7. sharding
@pytest.mark.parametrize("sampler,spacing", [("ddim0", None), ("dpmpp2m", "logsnr")])
def test_shards_concatenate_to_the_unsharded_batch(dev, sampler, spacing):
    pipe = product_pipe(dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3)), dev)
    cond = torch.tensor([2, 0, 1, 1], device=dev)
    kw = dict(steps=8, sampler=sampler, spacing=spacing, condition=cond, guidance_scale=4.0, un_cond=None)
    whole = pipe.sample(4, (8, 8, 8), noise=M.PhiloxDeviceNoise(9), **kw)
    parts = [pipe.sample(4, (8, 8, 8), noise=M.PhiloxDeviceNoise(9), shard=(r, 2), **kw) for r in range(2)]
    assert parts[0].shape[0] == 2 and torch.equal(torch.cat(parts), whole)
    z0 = _rand("sh.z0", (4, 8, 8, 8)).to(dev)
    m = (_rand("sh.m", (4, 1, 8, 8)) > 0).to(dev)
    kw = dict(is_latent=True, mask=m, **kw)
    whole = pipe.sample_from(z0, 0.5, noise=M.PhiloxDeviceNoise(9), **kw)
    parts = [pipe.sample_from(z0, 0.5, noise=M.PhiloxDeviceNoise(9), shard=(r, 2), **kw) for r in range(2)]
    assert torch.equal(torch.cat(parts), whole)
