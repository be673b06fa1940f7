"""Windowed denoising (window= / window_stride= / window_weight=) on a real MI355X: the two kernels (the crop bit for bit against torch slicing;
the merge against the fp64 plain-torch merge under the derived bound, exact where one window covers, the same bits on every launch), parity with the
reference's own loops run per window (tests/golden/md_*, scripts/gen_window_golden.py), and the properties of the contract (loop forms, launch
count, draws, sharding, inpainting, refusals, nothing leaks into the default path)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import kernels as K
from medfusion_amd.window import WindowPlan
from oracle import restate as R
from oracle import synth as S
from tests import window_cases as WC
from tests.util import T, gold, oracle_noise, relerr, to_product_kwargs

TOL = 1e-4             # the tolerance of every model-level parity test here (tests/test_parity_gpu.py, tests/test_solver_gpu.py)
DRIFT_FACTOR = 2.0     # a case that exceeds it is held to max(TOL, 2 x the oracle's own fp32-vs-fp64 distance), the rule of tests/test_solver_gpu.py
CANVAS, WINDOW = (8, 12, 12), (8, 8)      # the contract tests' canvas latent and window on pipe_tiny: stride 4, M = 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def product_pipe(case, dev, vae=True):
    unet_kw, vae_kw, tag, flags = WC.pipe_args(case)
    pipe = M.DiffusionPipeline(noise_scheduler=M.GaussianNoiseScheduler, noise_estimator=M.UNet, latent_embedder=None,
                               noise_scheduler_kwargs=R.published_scheduler_kwargs(), noise_estimator_kwargs=to_product_kwargs(unet_kw),
                               estimator_objective=flags.get("objective", "x_T"), clip_x0=flags.get("clip_x0", False), **flags.get("ctor", {}))
    S.synth_state_dict(pipe.noise_estimator, f"{tag}.unet.")
    if vae_kw and vae:
        pipe.latent_embedder = M.VAE(**vae_kw)
        S.synth_state_dict(pipe.latent_embedder, f"{tag}.vae.")
    return pipe.to(dev).eval()


@pytest.fixture(scope="module")
def tiny2d(dev):
    return product_pipe(dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3)), dev)


def _plans(v, weight, tiling=False):
    canvas, window, stride = (*v["tiling"], v["tiling"][1]) if tiling else (v["canvas"], v["window"], v["stride"])
    return WindowPlan(canvas, window, stride, weight), WC.RefPlan(canvas, window, stride, weight)


# ------------------------------------------------------------------------------------------------ 1. the crop
@pytest.mark.parametrize("name", list(WC.KERNEL_SHAPES))
def test_gather_is_torch_slicing_bit_for_bit(dev, name):
    v = WC.KERNEL_SHAPES[name]
    for tiling in (False, True):
        plan, ref = _plans(v, "tent", tiling)
        assert plan.windows == ref.windows
        canvas = S.synth_input(f"window.g.{name}.{tiling}", (v["B"], v["C"], *plan.canvas), 1.3)
        got = K.window_gather(canvas.to(dev), plan)
        want = WC.ref_gather(canvas, ref)                          # every (b, m): row b * M + m
        assert got.shape == want.shape == (v["B"] * plan.M, v["C"], *plan.window) and torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------------------------ 2. the merge
@pytest.mark.parametrize("weight", ["uniform", "tent"])
@pytest.mark.parametrize("name", list(WC.KERNEL_SHAPES))
def test_merge_against_fp64_and_exact_where_one_window_covers(dev, name, weight):
    v = WC.KERNEL_SHAPES[name]
    plan, ref = _plans(v, weight)
    wins = S.synth_input(f"window.m.{name}", (v["B"] * plan.M, v["C"], *plan.window), 1.7)
    d_wins = wins.to(dev)
    got = K.window_merge(d_wins, plan)
    again = K.window_merge(d_wins, plan)
    assert torch.equal(got, again)                                 # a fixed order: the same bits on a second launch
    got = got.cpu()
    want = WC.ref_merge(wins, ref, torch.float64)
    worst = float(((got.double() - want).abs() / WC.merge_bound(wins, ref)).max())
    print(f"[measured] window_merge vs fp64, {name} / {weight}: worst {worst:.2f} of (K + 2) 2^-24 max|p|")
    assert got.shape == want.shape and worst <= 1.0
    cover = ref.cover()
    assert int(cover.max()) > 1 and int(cover.min()) == 1
    single = (cover == 1).expand_as(got)
    for b in range(v["B"]):
        for m in range(plan.M):
            idx = (b, slice(None), *ref.slices(m))
            assert torch.equal(got[idx][single[idx]], wins[b * plan.M + m][single[idx]]), (b, m)     # no multiply, no divide


@pytest.mark.parametrize("weight", ["uniform", "tent"])
@pytest.mark.parametrize("name", list(WC.KERNEL_SHAPES))
def test_merge_without_overlap_is_the_concatenation(dev, name, weight):
    v = WC.KERNEL_SHAPES[name]
    plan, ref = _plans(v, weight, tiling=True)
    assert set(ref.cover().flatten().tolist()) == {1} and plan.M > 1
    wins = S.synth_input(f"window.t.{name}", (v["B"] * plan.M, v["C"], *plan.window), 1.7)
    got = K.window_merge(wins.to(dev), plan).cpu()
    want = torch.empty_like(got)
    for b in range(v["B"]):
        for m in range(plan.M):
            want[(b, slice(None), *ref.slices(m))] = wins[b * plan.M + m]
    assert torch.equal(got, want)
    assert torch.equal(K.window_merge(K.window_gather(got.to(dev), plan), plan).cpu(), got)           # crop, then merge: the canvas again


@pytest.mark.parametrize("name", list(WC.KERNEL_SHAPES))
def test_merge_of_the_guidance_pair_is_two_merges(dev, name):
    """2 B canvas rows in one launch (rows [0, B M) the un-guided windows, [B M, 2 B M) the guided ones) against one launch per half"""
    v = WC.KERNEL_SHAPES[name]
    plan, _ = _plans(v, "tent")
    rows = v["B"] * plan.M
    wins = S.synth_input(f"window.p.{name}", (2 * rows, v["C"], *plan.window), 1.7).to(dev)
    both = K.window_merge(wins, plan)
    assert both.shape[0] == 2 * v["B"]
    assert torch.equal(both[:v["B"]], K.window_merge(wins[:rows], plan)) and torch.equal(both[v["B"]:], K.window_merge(wins[rows:], plan))


def test_wrapper_refuses_shapes_that_do_not_fit_the_plan(dev):
    plan = WindowPlan((12, 12), (8, 8), 4)
    with pytest.raises(ValueError):
        K.window_gather(torch.zeros((2, 8, 12, 13), device=dev), plan)
    with pytest.raises(ValueError):
        K.window_merge(torch.zeros((7, 8, 8, 8), device=dev), plan)            # not a whole number of canvases
    with pytest.raises(ValueError):
        K.window_merge(torch.zeros((8, 8, 8, 7), device=dev), plan)
    with pytest.raises(RuntimeError):
        K.window_gather(torch.zeros((2, 8, 12, 12)), plan)                     # no CPU path


# ------------------------------------------------------------------------------------------------ 3. parity with the reference, run per window
def _bound(e, drift):
    return TOL if e < TOL else max(TOL, DRIFT_FACTOR * drift)


@pytest.mark.parametrize("name", list(WC.PARITY_CASES))
def test_windowed_sampling_matches_the_reference_run_per_window(dev, name):
    """scripts/gen_window_golden.py: the reference's own loop on the canvas, its estimator's forward() wrapped to crop, call the original per
    window and merge in plain torch, the draws injected in the product's order.  Bound: TOL; a figure that exceeds it is held to max(TOL, 2 x the
    reference's own fp32-vs-fp64 distance).  A fixture whose stored origins are not the product's plan is refused."""
    case, g = WC.PARITY_CASES[name], gold(name)
    pipe = product_pipe(case, dev)
    size = tuple(int(v) for v in g["size"])
    plan = WindowPlan(size[1:], case["window"], case["window_stride"], case["window_weight"])
    assert size == case["size"] and int(g["seed"]) == case["seed"] and int(g["M"]) == plan.M
    assert [list(o) for o in plan.origins] == [[int(x) for x in row[row >= 0]] for row in g["origins"]], "stale fixture: the plan changed"
    if "rows" in g:      # (the composition ran over the scheduler's rows as data: they must be the rows the product runs today)
        rows = pipe.noise_scheduler.solver_records(pipe.noise_scheduler.loop_timesteps(case["steps"], True)[0], case["sampler"])
        assert np.array_equal(g["rows"], np.asarray([[r.t, r.mode, r.A, r.B, r.C] for r in rows], dtype=np.float64)), "stale fixture: the solver rows changed"
    noise = oracle_noise(case["seed"])
    kw = dict(steps=case["steps"], sampler=case["sampler"], noise=noise, **WC.window_kwargs(case), **WC.loop_kwargs(case, dev))
    out = pipe.sample(case["n"], size, decode=case["decode"], **kw)
    assert noise.draw_index == int(g["draws"])
    drift = float(g["fp64_drift"])
    figs = {"result": relerr(out, T(g["image"]))}
    if case["decode"]:
        figs["latent"] = relerr(pipe.sample(case["n"], size, decode=False, **{**kw, "noise": oracle_noise(case["seed"])}), T(g["latent"]))
    print(f"[measured] windowed sampling vs the reference run per window, {name}: " + "  ".join(f"{k} {v:.1e}" for k, v in figs.items())
          + f" (tolerance {TOL:.0e}, fp64 drift {drift:.1e})")
    assert tuple(out.shape) == tuple(g["image"].shape)
    for k, v in figs.items():
        assert v < _bound(v, drift), k


# ------------------------------------------------------------------------------------------------ 4. the contract
def _guided(dev, n=2):
    return dict(condition=torch.tensor([2, 0, 1, 1][:n], device=dev), guidance_scale=4.0, un_cond=None)


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "cfg"])
def test_the_loop_forms_are_bit_identical_and_the_recorded_iteration_holds_two_more_launches(dev, tiny2d, guided):
    pipe, extra = tiny2d, (_guided(dev) if guided else {})
    plan = WindowPlan(CANVAS[1:], WINDOW)
    assert plan.M == 4 and plan.stride == (4, 4)
    rows = dict(extra, condition=extra["condition"].repeat_interleave(plan.M)) if guided else {}
    pipe.sample(2 * plan.M, (8, *WINDOW), steps=6, noise=M.PhiloxDeviceNoise(7), loop="cmdlist", decode=False, **rows)     # B M rows at the window size
    plain = pipe.last_cmdlist_launches
    assert plain > 0 and pipe.last_cmdlist_foreign_ops == []
    out = {}
    for loop in ("eager", "cmdlist", "graph", None):
        pipe.last_cmdlist_launches, pipe.last_cmdlist_foreign_ops = 0, ["unset"]
        out[loop] = pipe.sample(2, CANVAS, steps=6, noise=M.PhiloxDeviceNoise(7), loop=loop, window=WINDOW, **extra)
        if loop in ("cmdlist", None):
            assert pipe.last_cmdlist_foreign_ops == [] and pipe.last_cmdlist_launches == plain + 2
    assert tuple(out["eager"].shape) == (2, 3, 96, 96) and bool(out["eager"].isfinite().all())
    assert torch.equal(out["eager"], out["cmdlist"]) and torch.equal(out["eager"], out["graph"]) and torch.equal(out["eager"], out[None])
    other = pipe.sample(2, CANVAS, steps=6, noise=M.PhiloxDeviceNoise(7), window=WINDOW, window_weight="uniform", **extra)
    assert not torch.equal(other, out["eager"])                    # the weights reach the result


def test_a_window_equal_to_the_canvas_is_the_unwindowed_path(dev, tiny2d):
    g = gold("sample_tiny_ddim5_uncond")
    size = tuple(int(v) for v in g["size"])
    run = lambda **kw: tiny2d.sample(int(g["n"]), size, steps=5, use_ddim=True, noise=oracle_noise(int(g["seed"])), **kw)
    today = run()
    assert relerr(today, T(g["image"])) < TOL
    assert torch.equal(run(window=None), today) and torch.equal(run(window=size[1:]), today) and torch.equal(run(window=size[1:], window_stride=3), today)
    launches = {}
    for key, kw in (("none", {}), ("canvas", dict(window=size[1:]))):
        tiny2d.last_cmdlist_launches = 0
        launches[key] = (tiny2d.sample(2, size, steps=6, noise=M.PhiloxDeviceNoise(5), loop="cmdlist", **kw), tiny2d.last_cmdlist_launches)
    assert torch.equal(launches["none"][0], launches["canvas"][0]) and launches["none"][1] == launches["canvas"][1] > 0      # no new launch
    tiny2d.sample(2, CANVAS, steps=6, noise=M.PhiloxDeviceNoise(5), window=WINDOW)
    assert torch.equal(run(), today)                               # untouched by a windowed run in between


@pytest.mark.parametrize("kw", [dict(), dict(use_ddim=False), dict(sampler="ddim0"), dict(sampler="dpmpp2m_sde", spacing="logsnr")],
                         ids=["ddim", "ddpm", "ddim0", "dpmpp2m_sde"])
def test_draws_are_those_of_the_same_call_without_a_window(dev, tiny2d, kw):
    """canvas-shaped draws in the un-windowed order: the source ends where the un-windowed UNet run directly on the canvas leaves it.  Canvas
    (8, 16, 16) here, M = 9: the tiny UNet's three stride-2 levels cannot take a 12 x 12 latent without a window."""
    canvas = (8, 16, 16)
    left, first = [], []
    for window in (None, WINDOW):
        src = M.PhiloxDeviceNoise(21)
        out = tiny2d.sample(2, canvas, steps=6, noise=src, window=window, decode=False, **kw)
        left.append(src.draw_index)
        first.append(out)
    assert left[0] == left[1] > 0 and first[0].shape == first[1].shape == (2, *canvas) and not torch.equal(first[0], first[1])
    x = S.synth_input("window.dn", (2, *canvas)).to(dev)          # denoise(): the caller's x_t is the canvas
    ends = []
    for window in (None, WINDOW):
        src = M.PhiloxDeviceNoise(21)
        src.begin(2, dev)
        tiny2d.denoise(x, steps=6, noise=src, window=window, decode=False, **kw)
        ends.append(src.draw_index)
    assert ends[0] == ends[1] == left[0] - 1


def test_shards_concatenate_to_the_unsharded_batch(dev, tiny2d):
    kw = dict(steps=6, window=WINDOW, **_guided(dev, 4))
    whole = tiny2d.sample(4, CANVAS, noise=M.PhiloxDeviceNoise(9), **kw)
    parts = [tiny2d.sample(4, CANVAS, noise=M.PhiloxDeviceNoise(9), shard=(r, 2), **kw) for r in range(2)]
    assert parts[0].shape[0] == 2 and torch.equal(torch.cat(parts), whole) and not torch.equal(parts[0], parts[1])


@pytest.mark.parametrize("sampler,spacing", [(None, None), ("dpmpp2m", None)])
def test_inpainting_on_a_canvas_keeps_the_known_cells_exactly(dev, tiny2d, sampler, spacing):
    z0 = S.synth_input("window.i.z0", (2, *CANVAS)).to(dev)
    m = (S.synth_input("window.i.m", (2, 1, *CANVAS[1:])) > 0).to(dev)
    kw = dict(is_latent=True, steps=8, mask=m, sampler=sampler, spacing=spacing, window=WINDOW, decode=False, **_guided(dev))
    lat = {loop: tiny2d.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(7), loop=loop, **kw) for loop in ("eager", "cmdlist", "graph")}
    keep = ~m.expand_as(z0)
    assert bool(keep.any()) and bool((~keep).any())
    assert torch.equal(lat["eager"][keep], z0[keep]) and not torch.equal(lat["eager"][~keep], z0[~keep]) and bool(lat["eager"].isfinite().all())
    assert torch.equal(lat["eager"], lat["cmdlist"]) and torch.equal(lat["eager"], lat["graph"])
    other = tiny2d.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(8), **kw)
    assert torch.equal(other[keep], z0[keep]) and not torch.equal(other[~keep], lat["eager"][~keep])    # the regenerated region is not a function of z0 alone


def test_a_stochastic_sampler_runs_windowed_in_all_three_loop_forms(dev, tiny2d):
    kw = dict(steps=9, sampler="dpmpp2m_sde", spacing="logsnr", window=WINDOW, decode=False, **_guided(dev))
    executed = tiny2d.noise_scheduler.loop_timesteps(9, True, "logsnr")[1]
    out = {}
    for loop in ("eager", "cmdlist", "graph"):
        src = M.PhiloxDeviceNoise(7)
        out[loop] = tiny2d.sample(2, CANVAS, noise=src, loop=loop, **kw)
        assert src.draw_index == executed                          # x_T and one draw per non-final iteration
    assert bool(out["eager"].isfinite().all()) and torch.equal(out["eager"], out["cmdlist"]) and torch.equal(out["eager"], out["graph"])
    assert not torch.equal(out["eager"], tiny2d.sample(2, CANVAS, noise=M.PhiloxDeviceNoise(8), **kw))


def test_trace_and_progress_see_the_canvas(dev, tiny2d):
    trace, seen = [], []
    kw = dict(steps=6, window=WINDOW, decode=False)
    got = tiny2d.sample(2, CANVAS, noise=M.PhiloxDeviceNoise(3), trace=trace, progress_cb=lambda d, t: seen.append((d, t)), **kw)
    assert len(trace) == 6 and all(x0.shape == x.shape == (2, *CANVAS) for x0, x in trace) and torch.equal(trace[-1][1], got)
    assert seen == [(i + 1, 6) for i in range(6)]
    assert torch.equal(got, tiny2d.sample(2, CANVAS, noise=M.PhiloxDeviceNoise(3), **kw))          # the traced (eager) loop and the default one


def test_a_volume_runs_windowed_in_all_three_loop_forms(dev):
    """the 3-D architecture and canvas of the md_3d fixture: two windows along the depth too"""
    case = WC.PARITY_CASES["md_3d"]
    pipe = product_pipe(case, dev)
    kw = dict(steps=6, sampler="dpmpp2m", **WC.window_kwargs(case), **WC.loop_kwargs(case, dev))
    out = {loop: pipe.sample(1, case["size"], loop=loop, noise=M.PhiloxDeviceNoise(4), **kw) for loop in ("eager", "cmdlist", "graph")}
    assert pipe.last_cmdlist_foreign_ops == [] and tuple(out["eager"].shape) == (1, *case["size"]) and bool(out["eager"].isfinite().all())
    assert torch.equal(out["eager"], out["cmdlist"]) and torch.equal(out["eager"], out["graph"])


def test_refusals(dev, tiny2d):
    for flag in ("use_self_conditioning", "estimate_variance"):
        pipe = product_pipe(dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3, ctor={flag: True})), dev, vae=False)
        with pytest.raises(ValueError, match=flag):
            pipe.sample(2, CANVAS, steps=6, window=WINDOW)
    with pytest.raises(ValueError, match="cold_diffusion"):
        tiny2d.sample(2, CANVAS, steps=6, use_ddim=False, cold_diffusion=True, window=WINDOW)
    z = S.synth_input("window.r.z", (2, *CANVAS)).to(dev)
    with pytest.raises(ValueError, match="window= is not built for invert"):
        tiny2d.invert(z, steps=8, is_latent=True, window=WINDOW)
    with pytest.raises(ValueError, match="window= is not built for edit"):
        tiny2d.edit(z, None, steps=8, is_latent=True, window=WINDOW)
    with pytest.raises(ValueError, match="spatial axis"):
        tiny2d.sample(2, CANVAS, steps=6, window=(4, 8, 8))
    with pytest.raises(TypeError):
        tiny2d.sample(2, CANVAS, steps=6, window=WINDOW, eta=0.0)
    with pytest.raises(TypeError):
        tiny2d.denoise(z, steps=6, window=WINDOW, eta=0.0)
