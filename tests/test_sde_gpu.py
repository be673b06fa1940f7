"""The stochastic few-step samplers (sampler="ddim1" / "dpmpp2m_sde") on a real MI355X: the noise variant of the solver step (zero scales bit for
bit against mf_solver_step_f32, the DDIM row bit for bit against mf_sched_step_f32 on the same draw, the second-order row against fp64 under a
derived bound, the draw inside the launch bit for bit against mf_philox_normal_f32), parity with the reference's own DDIM loop and with the CPU
composition of SDE-DPM-Solver++(2M) (tests/golden/sde_*), and the properties of the contract (loop forms, draw count, sharding, inpainting,
nothing leaks into the default path)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from oracle import restate as R
from oracle import synth as S
from tests import sde_cases as SD
from tests.util import T, gold, oracle_noise, relerr, to_product_kwargs

TOL = 1e-4             # the tolerance of every model-level parity test here (tests/test_parity_gpu.py, tests/test_solver_gpu.py)
DRIFT_FACTOR = 2.0     # a case that exceeds it is held to max(TOL, 2 x the oracle's own fp32-vs-fp64 distance), the rule of tests/test_solver_gpu.py
STOCHASTIC = ("ddim1", "dpmpp2m_sde")
SHAPES = {"vector": (2, 8, 64), "element": (3, 5, 63)}     # n = 2*8*8*8 on 16-byte vectors; [3,5,7,9]: n = 945, 63 cells, odd everything


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rand(name, shape, scale=1.0):
    return S.synth_input("sde." + name, shape, scale)


def product_pipe(case, dev, vae=True):
    unet_kw, vae_kw, tag, flags = SD.pipe_args(case)
    pipe = M.DiffusionPipeline(noise_scheduler=M.GaussianNoiseScheduler, noise_estimator=M.UNet, latent_embedder=None,
                               noise_scheduler_kwargs=R.published_scheduler_kwargs(), noise_estimator_kwargs=to_product_kwargs(unet_kw),
                               estimator_objective=flags.get("objective", "x_T"), clip_x0=flags.get("clip_x0", False))
    S.synth_state_dict(pipe.noise_estimator, f"{tag}.unet.")
    if vae_kw and vae:
        pipe.latent_embedder = M.VAE(**vae_kw)
        S.synth_state_dict(pipe.latent_embedder, f"{tag}.vae.")
    return pipe.to(dev).eval()


@pytest.fixture(scope="module")
def tiny2d(dev):
    return product_pipe(dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3)), dev)


@pytest.fixture(scope="module")
def tiny3d(dev):
    return product_pipe(dict(dims=3, pipe=dict(tag="solver_ddim0_3d", ncls=2)), dev)


def _sched(dev, steps, sampler, spacing=None):
    sch = M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())
    ts, _ = sch.loop_timesteps(steps, True, spacing)
    if sampler in STOCHASTIC:
        rows, scales = sch.stochastic_records(ts, sampler)
    else:
        rows = sch.solver_records(ts, sampler)
        scales = [0.0] * len(rows)
    return sch, ts, rows, scales, sch.upload_solver_records(rows, dev)


def _p(t):
    return None if t is None else t.data_ptr()


def _args(x_t, pred, pu, out, x0, xT, hist, table, objective, clip, g, step=0, counter=None, step_dev=None):
    return L.MfSolverArgs(_p(x_t), _p(pred), _p(pu), _p(out), _p(x0), _p(xT), _p(hist), _p(table), _p(counter), None if counter is None else counter.data_ptr() + 4,
                          _p(step_dev), step, objective, clip, g, x_t.numel())


def _supplied(scale, eps, stride=0):
    return L.MfSolverNoise(scale.data_ptr(), eps.data_ptr(), stride, 0, 0, 0, 0, 0, 0)


def _philox(scale, seed, base, stride, offset, B):
    return L.MfSolverNoise(scale.data_ptr(), None, 0, seed, offset, base, stride, B, 0)


def _blend(sch, ts, shape, dev):
    B, Cc, cells = shape
    z0, eps0 = _rand("bl.z0", shape).to(dev), _rand("bl.eps", shape).to(dev)
    mask = (_rand("bl.m", (B, 1, cells)) > 0).to(torch.uint8).to(dev)
    coef = sch.blend_records(ts).to(dev)
    bl = L.MfSchedBlend(z0.data_ptr(), eps0.data_ptr(), mask.data_ptr(), coef.data_ptr(), cells, Cc, 0)
    bl._keep = (z0, eps0, mask, coef)
    return bl


# ------------------------------------------------------------------------------------------------ 1. all scales zero: the deterministic step
@pytest.mark.parametrize("shape", list(SHAPES))
def test_zero_scales_are_the_deterministic_step_bit_for_bit(dev, shape):
    """x_t_out, x0_out, xT_out and both history slots against mf_solver_step_f32 for all four modes, the blended form against
    mf_solver_step_blend_f32; the draw (caller-supplied here) is multiplied by zero"""
    shp = SHAPES[shape]
    n = int(np.prod(shp))
    x_t, pred, pu, prev, eps = (_rand(f"z.{k}", shp, 1.3).to(dev) for k in ("xt", "pred", "pu", "prev", "eps"))
    seen = set()
    for sampler in ("ddim0", "dpmpp2m"):
        sch, ts, rows, _, table = _sched(dev, 6, sampler)
        zero = torch.zeros(len(rows), device=dev)
        bl = _blend(sch, ts, shp, dev)
        for step in (0, 2, 5):
            seen.add(rows[step].mode)
            for blend in (None, bl):
                res = []
                for noisy in (False, True):
                    out, x0, xT = (torch.empty_like(x_t) for _ in range(3))
                    hist = torch.full((2, n), float("nan"), device=dev)
                    hist[(step + 1) & 1] = prev.reshape(-1)
                    a = _args(x_t, pred, pu, out, x0, xT, hist, table, 0, 1, 2.5, step=step)
                    if noisy:
                        K.solver_step_noise(a, _supplied(zero, eps), blend)
                    else:
                        K.solver_step(a, blend)
                    res.append((out, x0, xT, hist))
                for got, want in zip(res[1][:3], res[0][:3]):
                    assert torch.equal(got, want), (sampler, step, blend is not None)
                assert torch.equal(res[1][3][step & 1], res[0][3][step & 1]) and torch.equal(res[1][3][(step + 1) & 1], prev.reshape(-1))
    assert seen == {L.SOLVER_FINAL, L.SOLVER_DDIM0, L.SOLVER_ORDER1, L.SOLVER_ORDER2}


# ------------------------------------------------------------------------------------------------ 2. the ddim1 row is the reference's DDIM update
@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("objective", [0, 1])
def test_ddim1_row_plus_a_draw_is_the_scheduler_steps_ddim_update_bit_for_bit(dev, objective, cfg, clip):
    sch, ts, rows, scales, table = _sched(dev, 7, "ddim1")
    old = sch.upload_records(sch.step_records(ts, True), dev)
    scale = torch.tensor(scales, device=dev)
    for shape in SHAPES.values():
        n = int(np.prod(shape))
        x_t, pred, pu, eps, npost = (_rand(f"d.{k}", (n,), 1.3).to(dev) for k in ("xt", "pred", "pu", "eps", "post"))
        for step in (0, 3, 5):
            want = [torch.empty_like(x_t) for _ in range(3)]
            a = L.MfSchedArgs(x_t.data_ptr(), pred.data_ptr(), pu.data_ptr() if cfg else None, None, npost.data_ptr(), eps.data_ptr(), 0, want[0].data_ptr(),
                              want[1].data_ptr(), want[2].data_ptr(), old.data_ptr(), None, step, objective, clip, 3.5, n)
            K.sched_step(a)
            got = [torch.empty_like(x_t) for _ in range(3)]
            K.solver_step_noise(_args(x_t, pred, pu if cfg else None, got[0], got[1], got[2], None, table, objective, clip, 3.5, step=step), _supplied(scale, eps))
            assert rows[step].mode == L.SOLVER_DDIM0 and scales[step] > 0
            for g, w in zip(got, want):
                assert torch.equal(g, w), (n, step)


# ------------------------------------------------------------------------------------------------ 3. the second-order row against fp64
@pytest.mark.parametrize("shape", list(SHAPES))
def test_order2_row_plus_a_draw_against_fp64(dev, shape):
    """|got - want| <= 8 * 2^-24 * (|A x_t| + |B x_0| + |C x_0_prev| + |S eps|): four products and three sums, each rounded once (half an ulp of
    a magnitude the sum of the terms' magnitudes bounds; 8 half-ulps leave one to spare).  want: fp64 on the CPU from the kernel's own fp32 x_0.
    The element shape runs the blend too (the regenerated cells are held to the bound, the kept ones to the known latent, bit for bit); a bank of
    draws with a per-step stride feeds both."""
    shp = SHAPES[shape]
    B, Cc, cells = shp
    n = int(np.prod(shp))
    sch, ts, rows, scales, table = _sched(dev, 7, "dpmpp2m_sde", "logsnr")
    scale = torch.tensor(scales, device=dev)
    bank = _rand("o.bank", (len(rows), n)).to(dev)
    bl = _blend(sch, ts, shp, dev) if shape == "element" else None
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    hist = torch.full((2, n), float("nan"), device=dev)
    x = _rand("o.xT", shp).to(dev)
    x0 = torch.empty_like(x)
    prev = None
    for i, (r, s) in enumerate(zip(rows, scales)):
        pred = _rand(f"o.pred{i}", shp, 0.9).to(dev)
        x_in = x.clone()
        K.solver_step_noise(_args(x, pred, None, x, x0, None, hist, table, 0, 0, 1.0, counter=counter), _supplied(scale, bank, n), bl)
        xi, e0, ep = x_in.double().cpu().reshape(-1), x0.double().cpu().reshape(-1), bank[i].double().cpu()
        got = x.double().cpu().reshape(-1)
        regen = torch.ones(n, dtype=torch.bool)
        if bl is not None:
            z0, eps0, mask, coef = bl._keep
            regen = (mask != 0).expand(B, Cc, cells).reshape(-1).cpu()
            a_, c_ = coef[i]
            known = K.rows_axpby(z0, a_.expand(B).contiguous(), eps0, c_.expand(B).contiguous())
            assert torch.equal(x.reshape(-1)[~regen.to(dev)], known.reshape(-1)[~regen.to(dev)])
        if r.mode == L.SOLVER_FINAL:
            assert torch.equal(x.reshape(-1)[regen.to(dev)], x0.reshape(-1)[regen.to(dev)]) and s == 0.0
        else:
            terms = [r.A * xi, r.B * e0] + ([r.C * prev] if r.mode == L.SOLVER_ORDER2 else []) + [s * ep]
            want, mag = sum(terms), sum(t.abs() for t in terms)
            err = (got - want).abs()[regen]
            assert bool((err <= 8 * 2.0 ** -24 * mag[regen]).all()), (shape, i, float((err / mag[regen].clamp_min(1e-30)).max()))
            assert float((s * ep).abs().max()) > 0.01          # the draw is not a rounding-level term
        prev = e0
        assert counter.tolist() == [i + 1, 0]
    assert [r.mode for r in rows] == [2, 3, 3, 3, 3, 3, 0]


# ------------------------------------------------------------------------------------------------ 4. the draw inside the launch
def test_the_draw_inside_the_launch_is_philox_normal_bit_for_bit(dev):
    """against the caller-supplied form fed K.philox_normal of the same (seed, draw, offset), with and without the blend; the device counter walks
    the draw index over 3 consecutive launches; the three sources of the step index give the same bits; the shapes mf_philox_normal_f32
    refuses are refused"""
    shp = SHAPES["vector"]
    B = shp[0]
    n = int(np.prod(shp))
    seed, base, stride, offset = 0x1234567890ABCDEF, 5, 2, 3
    sch, ts, rows, scales, table = _sched(dev, 7, "dpmpp2m_sde", "logsnr")
    scale = torch.tensor(scales, device=dev)
    bl = _blend(sch, ts, shp, dev)
    x_t, pu, prev = (_rand(f"p.{k}", shp).to(dev) for k in ("xt", "pu", "prev"))
    preds = [_rand(f"p.pred{i}", shp, 0.9).to(dev) for i in range(3)]
    for blend in (None, bl):
        # the counter: three consecutive launches from step 2, draw = base + stride * step
        counter = torch.tensor([2, 0], dtype=torch.int32, device=dev)
        h_in, h_sup = (torch.full((2, n), float("nan"), device=dev) for _ in range(2))
        h_in[1], h_sup[1] = prev.reshape(-1), prev.reshape(-1)
        x_in, x_sup = x_t.clone(), x_t.clone()
        for k, step in enumerate((2, 3, 4)):
            K.solver_step_noise(_args(x_in, preds[k], pu, x_in, None, None, h_in, table, 0, 1, 2.5, counter=counter), _philox(scale, seed, base, stride, offset, B), blend)
            eps = K.philox_normal(torch.empty(shp, device=dev), seed, base + stride * step, offset)
            K.solver_step_noise(_args(x_sup, preds[k], pu, x_sup, None, None, h_sup, table, 0, 1, 2.5, step=step), _supplied(scale, eps), blend)
            assert torch.equal(x_in, x_sup), (blend is not None, step)
            assert counter.tolist() == [step + 1, 0]
        # the three sources of the step index
        outs = []
        for src in ("host", "dev", "counter"):
            hist = torch.full((2, n), float("nan"), device=dev)
            hist[0] = prev.reshape(-1)
            out = torch.empty_like(x_t)
            word = torch.tensor([3, 0], dtype=torch.int32, device=dev)
            a = _args(x_t, preds[0], pu, out, None, None, hist, table, 0, 1, 2.5, step=3 if src == "host" else 0, counter=word if src == "counter" else None,
                      step_dev=word[:1] if src == "dev" else None)
            K.solver_step_noise(a, _philox(scale, seed, base, stride, offset, B), blend)
            outs.append(out)
            assert word.tolist() == ([4, 0] if src == "counter" else [3, 0])
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], x_t)
    # another sample offset moves the rows: row b at offset 3 is row b - 1 at offset 4
    o3, o4 = (torch.empty_like(x_t) for _ in range(2))
    xx = x_t[:1].expand(B, -1, -1).contiguous()
    pp = preds[0][:1].expand(B, -1, -1).contiguous()
    for o, off in ((o3, 3), (o4, 4)):
        K.solver_step_noise(_args(xx, pp, None, o, None, None, None, table, 0, 0, 1.0, step=0), _philox(scale, seed, base, stride, off, B))
    assert torch.equal(o3[1], o4[0]) and not torch.equal(o3[0], o3[1])
    # refusals: where mf_philox_normal_f32 refuses, and a blend the vector path cannot take
    odd = SHAPES["element"]
    xo = _rand("p.odd", odd).to(dev)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        K.philox_normal(torch.empty(odd, device=dev), seed, 0, 0)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        K.solver_step_noise(_args(xo, xo, None, torch.empty_like(xo), None, None, None, table, 0, 0, 1.0), _philox(scale, seed, 0, 1, 0, odd[0]))
    shp63 = (2, 8, 63)
    x63 = _rand("p.63", shp63).to(dev)
    with pytest.raises(RuntimeError, match="aligned"):
        K.solver_step_noise(_args(x63, x63, None, torch.empty_like(x63), None, None, None, table, 0, 0, 1.0), _philox(scale, seed, 0, 1, 0, 2), _blend(sch, ts, shp63, dev))


# ------------------------------------------------------------------------------------------------ 5. parity
def _bound(e, drift):
    return TOL if e < TOL else max(TOL, DRIFT_FACTOR * drift)


@pytest.mark.parametrize("name", list(SD.DDIM1_CASES))
def test_ddim1_matches_the_references_ddim_loop(dev, name):
    """the reference's own denoise(use_ddim=True) with its DDIM draws injected (scripts/gen_sde_golden.py): per-iteration x_0 and latents, and the
    decoded image.  Bound: TOL; a figure that exceeds it is held to max(TOL, 2 x the reference's own fp32-vs-fp64 distance)."""
    case, g = SD.DDIM1_CASES[name], gold(name)
    pipe = product_pipe(case, dev)
    noise, trace = oracle_noise(int(g["seed"])), []
    img = pipe.sample(int(g["n"]), tuple(int(v) for v in g["size"]), steps=int(g["steps"]), sampler="ddim1", noise=noise, trace=trace, **SD.loop_kwargs(case, dev))
    assert noise.draw_index == int(g["steps"]) == len(trace)          # x_T and one draw per non-final iteration
    drift = float(g["fp64_drift"])
    figs = {"image": relerr(img, T(g["image"])), "x0": max(relerr(t[0], T(g["x0"][i])) for i, t in enumerate(trace)),
            "latents": max(relerr(t[1], T(g["latents"][i])) for i, t in enumerate(trace))}
    print(f"[measured] ddim1 vs the reference's DDIM loop, {name}: " + "  ".join(f"{k} {v:.1e}" for k, v in figs.items()) + f" (tolerance {TOL:.0e}, fp64 drift {drift:.1e})")
    for k, v in figs.items():
        assert v < _bound(v, drift), k


@pytest.mark.parametrize("name", list(SD.SDE2M_CASES))
def test_dpmpp2m_sde_matches_the_cpu_composition(dev, name):
    """the reference's forward() under a plain torch loop over the same rows, scales and draws (scripts/gen_sde_golden.py), 8 executed iterations;
    the rows stored next to the result must be the rows the product runs today"""
    case, g = SD.SDE2M_CASES[name], gold(name)
    pipe = product_pipe(case, dev)
    sch = pipe.noise_scheduler
    ts, executed = sch.loop_timesteps(case["steps"], True, case["spacing"])
    rows, scales = sch.stochastic_records(ts, "dpmpp2m_sde")
    assert executed == 8 and np.array_equal(g["rows"], SD.rows_array(rows, scales)) and int(g["seed"]) == case["seed"]
    noise, trace = oracle_noise(case["seed"]), []
    img = pipe.sample(case["n"], SD.SIZE[case["dims"]], steps=case["steps"], sampler="dpmpp2m_sde", spacing=case["spacing"], noise=noise, trace=trace,
                      **SD.loop_kwargs(case, dev))
    assert noise.draw_index == 8 == len(trace)
    drift = float(g["fp64_drift"])
    figs = {"image": relerr(img, T(g["image"])), "x0": max(relerr(t[0], T(g["x0"][i])) for i, t in enumerate(trace)),
            "latents": max(relerr(t[1], T(g["latents"][i])) for i, t in enumerate(trace))}
    print(f"[measured] dpmpp2m_sde vs the CPU composition, {name}: " + "  ".join(f"{k} {v:.1e}" for k, v in figs.items()) + f" (tolerance {TOL:.0e}, fp64 drift {drift:.1e})")
    for k, v in figs.items():
        assert v < _bound(v, drift), k


def test_ddim1_on_the_references_grid_is_the_default_loop_bit_for_bit(tiny2d, dev):
    """given the same draws: the default loop consumes (posterior, DDIM) pairs, "ddim1" the DDIM draws only -- a host source that hands the
    default loop's DDIM draws to "ddim1" in order makes the latents equal bit for bit (the posterior draw is multiplied by std[t == 0] = 0 on
    the one iteration that would use it)"""
    src = S.PhiloxNoise(17)
    like = torch.empty((2, 8, 8, 8))
    draws = [src(like) for _ in range(1 + 2 * 6)]
    feed = lambda seq: M.HostNoise(lambda shape, it=iter(seq): next(it))
    want = tiny2d.sample(2, (8, 8, 8), steps=6, noise=feed(draws), decode=False)
    got = tiny2d.sample(2, (8, 8, 8), steps=6, sampler="ddim1", noise=feed([draws[0]] + draws[2::2]), decode=False)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 6. loop forms, draws, nothing leaks
def _tiny_golden(pipe):
    g = gold("sample_tiny_ddim5_uncond")
    return pipe.sample(int(g["n"]), tuple(int(v) for v in g["size"]), steps=5, use_ddim=True, noise=oracle_noise(int(g["seed"]))), T(g["image"])


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "cfg"])
@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("sampler,spacing", [("ddim1", None), ("dpmpp2m_sde", "logsnr")])
def test_the_loop_forms_are_bit_identical(dev, tiny2d, tiny3d, sampler, spacing, dims, guided):
    pipe = tiny2d if dims == 2 else tiny3d
    size = SD.SIZE[dims]
    extra = dict(condition=torch.tensor([1, 0], device=dev), guidance_scale=4.0, un_cond=None) if guided else {}
    kw = dict(steps=9, sampler=sampler, spacing=spacing, **extra)
    executed = pipe.noise_scheduler.loop_timesteps(9, True, spacing)[1]
    if dims == 2:
        before, want = _tiny_golden(pipe)
        assert relerr(before, want) < TOL
    pipe.sample(2, size, noise=M.PhiloxDeviceNoise(7), loop="cmdlist", **{**kw, "sampler": "dpmpp2m"})
    launches_2m = pipe.last_cmdlist_launches
    seen, out = [], {}
    for loop in ("eager", "cmdlist", "graph", None):
        src = M.PhiloxDeviceNoise(7)
        pipe.last_cmdlist_launches, pipe.last_cmdlist_foreign_ops = 0, ["unset"]
        out[loop] = pipe.sample(2, size, noise=src, loop=loop, progress_cb=(lambda d, t: seen.append((d, t))) if loop == "eager" else None, **kw)
        assert src.draw_index == executed                  # x_T and one draw per non-final iteration
        if loop in ("cmdlist", None):      # the default IS the command list; still ONE step launch per iteration
            assert pipe.last_cmdlist_foreign_ops == [] and pipe.last_cmdlist_launches == launches_2m > 0
    assert bool(out["eager"].isfinite().all())
    assert torch.equal(out["eager"], out["cmdlist"]) and torch.equal(out["eager"], out["graph"]) and torch.equal(out["eager"], out[None])
    assert seen == [(i + 1, executed) for i in range(executed)]
    if dims == 2:
        after, _ = _tiny_golden(pipe)
        assert torch.equal(before, after)       # sampler=None: the default path, untouched by a stochastic run in between


@pytest.mark.parametrize("sampler", STOCHASTIC)
def test_draws(dev, tiny2d, sampler):
    """the same seed gives the same result, another seed another; the result differs from the deterministic sampler on the same x_T; a device
    source and a host source fed the same values agree bit for bit (the host source runs the eager loop and refuses the command list); `eta`
    stays a TypeError"""
    kw = dict(steps=8, sampler=sampler, spacing="logsnr", decode=False)
    a = tiny2d.sample(2, (8, 8, 8), noise=M.PhiloxDeviceNoise(11), **kw)
    b = tiny2d.sample(2, (8, 8, 8), noise=M.PhiloxDeviceNoise(11), **kw)
    c = tiny2d.sample(2, (8, 8, 8), noise=M.PhiloxDeviceNoise(12), **kw)
    d = tiny2d.sample(2, (8, 8, 8), noise=M.PhiloxDeviceNoise(11), **{**kw, "sampler": "dpmpp2m"})
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, d) and bool(a.isfinite().all())
    executed = tiny2d.noise_scheduler.loop_timesteps(8, True, "logsnr")[1]
    host = M.HostNoise(lambda shape, k=[0]: (K.philox_normal(torch.empty(tuple(shape), device=dev), 11, k[0]).cpu(), k.__setitem__(0, k[0] + 1))[0])
    tiny2d.last_cmdlist_launches = -1
    e = tiny2d.sample(2, (8, 8, 8), noise=host, **kw)
    assert torch.equal(a, e) and host.draw_index == executed
    with pytest.raises(ValueError, match="cmdlist"):
        tiny2d.sample(2, (8, 8, 8), noise=oracle_noise(3), loop="cmdlist", **kw)
    with pytest.raises(TypeError):
        tiny2d.sample(2, (8, 8, 8), eta=0.0, **kw)
    with pytest.raises(TypeError):
        tiny2d.denoise(torch.zeros((2, 8, 8, 8), device=dev), eta=0.0, **kw)
    x = _rand("dn.x", (2, 8, 8, 8)).to(dev)          # denoise(): nothing is draw #0, the loop's draws start at 0
    src = M.PhiloxDeviceNoise(11)
    src.begin(2, dev)
    tiny2d.denoise(x, noise=src, **kw)
    assert src.draw_index == executed - 1


@pytest.mark.parametrize("sampler,spacing", [("ddim1", None), ("dpmpp2m_sde", "logsnr")])
def test_shards_concatenate_to_the_unsharded_batch(dev, tiny2d, sampler, spacing):
    cond = torch.tensor([2, 0, 1, 1], device=dev)
    kw = dict(steps=8, sampler=sampler, spacing=spacing, condition=cond, guidance_scale=4.0, un_cond=None)
    whole = tiny2d.sample(4, (8, 8, 8), noise=M.PhiloxDeviceNoise(9), **kw)
    parts = [tiny2d.sample(4, (8, 8, 8), noise=M.PhiloxDeviceNoise(9), shard=(r, 2), **kw) for r in range(2)]
    assert parts[0].shape[0] == 2 and torch.equal(torch.cat(parts), whole)
    assert not torch.equal(parts[0], parts[1])
    z0 = _rand("sh.z0", (4, 8, 8, 8)).to(dev)
    m = (_rand("sh.m", (4, 1, 8, 8)) > 0).to(dev)
    kw = dict(is_latent=True, mask=m, **kw)
    whole = tiny2d.sample_from(z0, 0.5, noise=M.PhiloxDeviceNoise(9), **kw)
    parts = [tiny2d.sample_from(z0, 0.5, noise=M.PhiloxDeviceNoise(9), shard=(r, 2), **kw) for r in range(2)]
    assert torch.equal(torch.cat(parts), whole)


# ------------------------------------------------------------------------------------------------ 7. inpainting
@pytest.mark.parametrize("sampler,spacing", [("dpmpp2m_sde", "logsnr"), ("ddim1", None)])
def test_inpainting_keeps_its_contract(dev, tiny2d, sampler, spacing):
    z0 = _rand("i.z0", (2, 8, 8, 8)).to(dev)
    m = (_rand("i.m", (2, 1, 8, 8)) > 0).to(dev)
    kw = dict(is_latent=True, steps=12, mask=m, sampler=sampler, spacing=spacing, condition=torch.tensor([1, 2], device=dev), guidance_scale=4.0, un_cond=None,
              decode=False)
    k = M.DiffusionPipeline._strength_span(tiny2d.noise_scheduler.loop_timesteps(12, True, spacing)[1], 0.75)[1]
    lat = {}
    for loop in ("eager", "cmdlist", "graph", None):
        src = M.PhiloxDeviceNoise(7)
        lat[loop] = tiny2d.sample_from(z0, 0.75, noise=src, loop=loop, **kw)
        assert src.draw_index == k                    # eps0 and one draw per non-final iteration
    keep = ~m.expand_as(z0)
    assert torch.equal(lat["eager"][keep], z0[keep]) and not torch.equal(lat["eager"][~keep], z0[~keep])
    assert torch.equal(lat["eager"], lat["cmdlist"]) and torch.equal(lat["eager"], lat["graph"]) and torch.equal(lat["eager"], lat[None])
    assert bool(lat["eager"].isfinite().all())
    other = tiny2d.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(8), **kw)
    assert torch.equal(other[keep], z0[keep]) and not torch.equal(other[~keep], lat["eager"][~keep])      # the regenerated region is not a function of z0 alone
    plain = tiny2d.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(7), **{**kw, "mask": None})
    ones = tiny2d.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(7), **{**kw, "mask": torch.ones((2, 1, 8, 8), device=dev)})
    assert torch.equal(plain, ones)                   # img2img == inpainting with nothing kept
