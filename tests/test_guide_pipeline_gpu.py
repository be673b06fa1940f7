"""Guidance rescale, dynamic thresholding and guidance schedules through DiffusionPipeline on a real MI355X (the tiny configurations of the
existing goldens, 6 to 8 iterations): a constant schedule is the scalar scale bit for bit, the three loop forms agree with every option on and
record nothing foreign, the defaults issue the plain path's launches, shards / masks / windows / 3-D / inversion keep their contracts, and the
four tests/golden/guide_* fixtures (scripts/gen_guide_golden.py: the reference's own estimator and scheduler calls around the stage restated in
plain torch) are met at the project's path tolerance.  Measured: profiles/guide_parity_measured.txt."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import kernels as K
from oracle import synth as S
from tests import guide_cases as GC
from tests import solver_cases as SC
from tests.test_solver_gpu import product_pipe
from tests.util import T, gold, oracle_noise, relerr

TOL = 1e-4             # the tolerance of every model-level parity test here (the i2i_* and solver_* fixtures)
ALL = dict(guidance_rescale=0.7, dynamic_threshold=0.995, threshold_max=6.0)
TINY = dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tiny(dev):
    return product_pipe(TINY, dev)


def _cond(dev, n=2):
    return torch.tensor([1, 0, 2, 1][:n], device=dev)


# ------------------------------------------------------------------------------------------------ 1. a constant schedule is the scalar scale
@pytest.mark.parametrize("sampler,spacing,steps", [(None, None, 6), ("ddim0", None, 6), ("dpmpp2m", "logsnr", 8), ("ddim1", None, 6), ("ddim1", "logsnr", 8),
                                                   ("dpmpp2m_sde", "logsnr", 8), ("dpmpp2m_sde", None, 6)])
def test_a_constant_schedule_gives_the_bits_of_the_scalar_scale(dev, tiny, sampler, spacing, steps):
    """every sampler: the stochastic ones too, whose rows carry draw scales of their own next to the stage's guidance scales"""
    executed = tiny.noise_scheduler.loop_timesteps(steps, True, spacing if sampler else None)[1]
    kw = dict(steps=steps, sampler=sampler, spacing=spacing, condition=_cond(dev), un_cond=None)
    for loop in ("eager", "cmdlist"):
        a, b = M.PhiloxDeviceNoise(11), M.PhiloxDeviceNoise(11)
        want = tiny.sample(2, (8, 8, 8), noise=a, guidance_scale=4.0, loop=loop, **kw)
        assert tiny.last_guide_scale is None
        got = tiny.sample(2, (8, 8, 8), noise=b, guidance_scale=1.0, guidance_schedule=[4.0] * executed, loop=loop, **kw)
        assert torch.equal(got, want) and a.draw_index == b.draw_index            # same bits, same draws
        assert tiny.last_guide_scale.tolist() == [1.0, 1.0] and tiny.last_guide_limit.tolist() == [0.0, 0.0]
    ramp = tiny.sample(2, (8, 8, 8), noise=M.PhiloxDeviceNoise(11), guidance_scale=4.0, guidance_schedule=lambda t: 1.0 + 3.0 * t / 999.0, **kw)
    assert not torch.equal(ramp, want) and bool(ramp.isfinite().all())
    inside = tiny.sample(2, (8, 8, 8), noise=M.PhiloxDeviceNoise(11), guidance_scale=4.0, guidance_schedule=("interval", 0, 999), **kw)
    assert torch.equal(inside, want)                                               # an interval that covers the grid


# ------------------------------------------------------------------------------------------------ 2. the three loop forms, every option on
@pytest.mark.parametrize("case", ["tiny", "x0obj", "3d"])
@pytest.mark.parametrize("sampler,spacing", [(None, None), ("dpmpp2m", "logsnr"), ("dpmpp2m_sde", "logsnr")])
def test_the_three_loop_forms_are_bit_identical_with_every_option_on(dev, tiny, case, sampler, spacing):
    pipe = tiny if case == "tiny" else product_pipe(dict(dims=2, pipe=dict(GC.PIPE_CASES["guide_x0obj_all"]["pipe"])) if case == "x0obj" else
                                                    dict(dims=3, pipe=dict(tag="solver_ddim0_3d", ncls=2)), dev)
    size = SC.SIZE[3 if case == "3d" else 2]
    executed = pipe.noise_scheduler.loop_timesteps(8, True, spacing if sampler else None)[1]
    cond = torch.tensor([1, 0], device=dev)
    kw = dict(steps=8, sampler=sampler, spacing=spacing, condition=cond, guidance_scale=8.0, un_cond=None,
              guidance_schedule=[8.0 - 0.5 * i for i in range(executed)], **ALL)
    out, launches = {}, {}
    for loop in ("eager", "cmdlist", "graph"):
        src = M.PhiloxDeviceNoise(7)
        pipe.last_cmdlist_launches, pipe.last_cmdlist_foreign_ops = 0, ["unset"]
        out[loop] = pipe.sample(2, size, noise=src, loop=loop, **kw)
        if loop == "cmdlist":
            assert pipe.last_cmdlist_foreign_ops == [] and pipe.last_cmdlist_launches > 0
            launches["guided"] = pipe.last_cmdlist_launches
        k, s = pipe.last_guide_scale.cpu(), pipe.last_guide_limit.cpu()
        assert k.shape == (2,) and bool(k.isfinite().all()) and bool((k > 0).all()) and bool((s >= 1.0).all()) and bool((s <= 6.0).all())
    assert bool(out["eager"].isfinite().all())
    assert torch.equal(out["eager"], out["cmdlist"]) and torch.equal(out["eager"], out["graph"])
    plain_kw = {k: v for k, v in kw.items() if k not in ALL and k != "guidance_schedule"}
    plain = pipe.sample(2, size, noise=M.PhiloxDeviceNoise(7), loop="cmdlist", **plain_kw)
    assert not torch.equal(plain, out["eager"])
    assert launches["guided"] == pipe.last_cmdlist_launches + 1                    # one more launch per iteration: a row fits one workgroup
    # warm calls: the stage's table, workspace and outputs are tensors of its own made before the loop -- the per-stream scratch does not move
    grew = K.scratch_growth_count()
    for loop in ("cmdlist", "graph"):
        again = pipe.sample(2, size, noise=M.PhiloxDeviceNoise(7), loop=loop, **kw)
        assert torch.equal(again, out["eager"])
    assert K.scratch_growth_count() == grew and pipe.last_cmdlist_foreign_ops == []


def test_the_defaults_issue_the_plain_paths_launches(dev, tiny):
    kw = dict(steps=6, condition=_cond(dev), guidance_scale=4.0, un_cond=None, loop="cmdlist")
    for extra in (dict(), dict(sampler="dpmpp2m", spacing="logsnr"), dict(sampler="ddim1"), dict(sampler="dpmpp2m_sde", spacing="logsnr")):
        want = tiny.sample(2, (8, 8, 8), noise=M.PhiloxDeviceNoise(3), **kw, **extra)
        n_plain = tiny.last_cmdlist_launches
        got = tiny.sample(2, (8, 8, 8), noise=M.PhiloxDeviceNoise(3), guidance_rescale=0.0, dynamic_threshold=None, threshold_max=None, guidance_schedule=None,
                          **kw, **extra)
        assert n_plain > 0 and tiny.last_cmdlist_launches == n_plain and tiny.last_cmdlist_foreign_ops == []
        assert torch.equal(got, want) and tiny.last_guide_scale is None
    with pytest.raises(TypeError, match="eta"):
        tiny.sample(2, (8, 8, 8), steps=6, eta=0.0, dynamic_threshold=0.9)


# ------------------------------------------------------------------------------------------------ 3. shards, masks, windows, self-conditioning
def test_a_shards_rows_are_shard_invariant(dev, tiny):
    cond = torch.tensor([2, 0, 1, 1], device=dev)
    kw = dict(steps=6, sampler="dpmpp2m", condition=cond, guidance_scale=6.0, un_cond=None, guidance_schedule=("interval", 100, 900), **ALL)
    whole = tiny.sample(4, (8, 8, 8), noise=M.PhiloxDeviceNoise(9), **kw)
    parts = [tiny.sample(4, (8, 8, 8), noise=M.PhiloxDeviceNoise(9), shard=(r, 2), **kw) for r in range(2)]
    assert parts[0].shape[0] == 2 and torch.equal(torch.cat(parts), whole)
    one = tiny.sample(4, (8, 8, 8), noise=M.PhiloxDeviceNoise(9), shard=(3, 4), **kw)
    assert torch.equal(one, whole[3:4])                                            # a row alone: its bits do not depend on the batch


@pytest.mark.parametrize("sampler", [None, "dpmpp2m"])
def test_kept_cells_still_end_as_the_inputs_latent(dev, tiny, sampler):
    z0 = S.synth_input("guide.z0", (2, 8, 8, 8), 1.0).to(dev)
    m = (S.synth_input("guide.m", (2, 1, 8, 8), 1.0) > 0).to(dev)
    kw = dict(is_latent=True, steps=8, mask=m, sampler=sampler, condition=_cond(dev), guidance_scale=6.0, un_cond=None, decode=False,
              guidance_schedule=[6.0] * 6, **ALL)
    lat = {loop: tiny.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(7), loop=loop, **kw) for loop in ("eager", "cmdlist", "graph")}
    keep = ~m.expand_as(z0)
    assert torch.equal(lat["eager"][keep], z0[keep]) and not torch.equal(lat["eager"][~keep], z0[~keep])
    assert torch.equal(lat["eager"], lat["cmdlist"]) and torch.equal(lat["eager"], lat["graph"]) and bool(lat["eager"].isfinite().all())
    with pytest.raises(ValueError, match="8 entries for 6"):
        tiny.sample_from(z0, 0.75, noise=M.PhiloxDeviceNoise(7), **{**kw, "guidance_schedule": [6.0] * 8})


def test_windowed_canvases_on_both_row_paths(dev):
    pipe = product_pipe(TINY, dev, vae=False)
    kw = dict(steps=6, sampler="dpmpp2m", condition=torch.tensor([1], device=dev), guidance_scale=6.0, un_cond=None, **ALL)
    # a window equal to the canvas is the un-windowed path
    a = pipe.sample(1, (8, 8, 8), noise=M.PhiloxDeviceNoise(5), **kw)
    b = pipe.sample(1, (8, 8, 8), noise=M.PhiloxDeviceNoise(5), window=(8, 8), **kw)
    assert torch.equal(a, b)
    for canvas in ((8, 8, 12), (8, 36, 36)):      # 768 elements per row: one workgroup; 10368: the multi-workgroup sequence (six launches)
        assert (8 * canvas[1] * canvas[2] > GC.ONE_WG) == (canvas[1] == 36)
        out = {}
        for loop in ("eager", "cmdlist", "graph"):
            pipe.last_cmdlist_launches, pipe.last_cmdlist_foreign_ops = 0, ["unset"]
            out[loop] = pipe.sample(1, canvas, noise=M.PhiloxDeviceNoise(5), window=(8, 8), loop=loop, **kw)
            if loop == "cmdlist":
                assert pipe.last_cmdlist_foreign_ops == [] and pipe.last_cmdlist_launches > 0
                guided = pipe.last_cmdlist_launches
        assert out["eager"].shape == (1, *canvas) and bool(out["eager"].isfinite().all())
        assert torch.equal(out["eager"], out["cmdlist"]) and torch.equal(out["eager"], out["graph"])
        pipe.sample(1, canvas, noise=M.PhiloxDeviceNoise(5), window=(8, 8), loop="cmdlist", **{k: v for k, v in kw.items() if k not in ALL})
        assert guided == pipe.last_cmdlist_launches + (6 if canvas[1] == 36 else 1)


def test_self_conditioning_takes_the_unbatched_pair_path(dev):
    pipe = product_pipe(dict(dims=2, pipe=dict(tag="pipe_tiny_var", ncls=2)), dev, self_cond=True)
    kw = dict(steps=6, sampler="ddim0", condition=torch.tensor([1, 0], device=dev), guidance_scale=4.0, un_cond=None, guidance_schedule=[4.0, 4.0, 3.0, 3.0, 2.0, 2.0], **ALL)
    outs = [pipe.sample(2, (8, 8, 8), noise=M.PhiloxDeviceNoise(5), loop=loop, **kw) for loop in ("eager", "cmdlist", "graph")]
    assert bool(outs[0].isfinite().all()) and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_inversion_and_editing_take_the_options(dev, tiny):
    x = S.synth_input("guide.edit", (2, 8, 8, 8), 0.8).to(dev)
    src, tgt = torch.tensor([0, 1], device=dev), torch.tensor([2, 2], device=dev)
    kw = dict(is_latent=True, steps=8, sampler="ddim0", guidance_scale=4.0, un_cond=None, dynamic_threshold=0.995)
    tops = [tiny.invert(x, src, loop=loop, guidance_rescale=0.5, guidance_schedule=[4.0] * 7, **kw) for loop in ("eager", "cmdlist", "graph")]
    assert torch.equal(tops[0], tops[1]) and torch.equal(tops[0], tops[2]) and bool(tops[0].isfinite().all())
    assert not torch.equal(tops[0], tiny.invert(x, src, **{**kw, "dynamic_threshold": None}))
    keep_all = torch.zeros((2, 1, 8, 8), device=dev)
    ekw = dict(source_condition=src, source_guidance_scale=2.0, source_guidance_rescale=0.3, source_guidance_schedule=[2.0] * 7, guidance_rescale=0.7,
               guidance_schedule=("interval", 0, 700), decode=False, **kw)
    same = tiny.edit(x, tgt, mask=keep_all, **ekw)
    assert torch.equal(same, x)                                                    # nothing regenerated: the input's latent, bit for bit
    outs = [tiny.edit(x, tgt, loop=loop, **ekw) for loop in ("eager", "cmdlist")]
    assert torch.equal(outs[0], outs[1]) and bool(outs[0].isfinite().all()) and not torch.equal(outs[0], x)


# ------------------------------------------------------------------------------------------------ 4. the fixtures
@pytest.mark.parametrize("name", list(GC.PIPE_CASES))
def test_fixtures_composed_from_the_references_own_calls(dev, name):
    """tests/golden/guide_*: held to TOL, the 1e-4 max-norm relative error of the i2i_* and solver_* fixtures; `fp64_drift` is the composition's own
    fp32-vs-fp64 distance, stored for the record (no case needs it).  Measured on an MI355X: profiles/guide_parity_measured.txt."""
    case, g = GC.PIPE_CASES[name], gold(name)
    assert int(g["seed"]) == case["seed"] and int(g["steps"]) == case["steps"] and int(g["n"]) == case["n"]
    pipe = product_pipe(case, dev)
    noise = oracle_noise(case["seed"])
    got = pipe.sample(case["n"], SC.SIZE[case["dims"]], steps=case["steps"], sampler=case["sampler"], spacing=case["spacing"], noise=noise,
                      condition=torch.tensor(case["condition"], device=dev), guidance_scale=case["guidance_scale"], un_cond=None, **case["opts"])
    assert noise.draw_index == int(g["draws"])
    assert got.shape == tuple(g["image"].shape)
    e = relerr(got, T(g["image"]))
    print(f"[measured] guide fixture {name}: {e:.1e} (tolerance {TOL:.0e}; the fp32 composition vs its fp64 self {float(g['fp64_drift']):.1e}); "
          f"last k {[round(float(v), 5) for v in pipe.last_guide_scale]}, last s {[round(float(v), 5) for v in pipe.last_guide_limit]}")
    assert e < TOL
    if case["sampler"] is not None:      # the replayed loops land on the same bits as the eager loop a host noise source took
        again = pipe.sample(case["n"], SC.SIZE[case["dims"]], steps=case["steps"], sampler=case["sampler"], spacing=case["spacing"],
                            noise=oracle_noise(case["seed"]), loop="cmdlist", condition=torch.tensor(case["condition"], device=dev),
                            guidance_scale=case["guidance_scale"], un_cond=None, **case["opts"])
        assert torch.equal(again, got)
