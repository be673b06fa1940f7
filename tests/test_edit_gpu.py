"""DDIM inversion and counterfactual editing on a real MI355X: the solver step's trajectory forms (RECORD / KEEP) bit for bit against
mf_solver_step_f32, the change-map kernel, parity of invert() / edit() with the reference's own pieces composed the same way
(tests/golden/edit_*, scripts/gen_edit_golden.py), and the properties of the contract (three loop forms, kept cells, no draws)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from oracle import synth as S
from tests import edit_cases as E
from tests.test_solver_gpu import _args, _sched, product_pipe
from tests.util import T, gold, relerr
from tests.util import offset_view as _view

TOL = 1e-4             # as in tests/test_solver_gpu.py
DRIFT_FACTOR = 2.0     # a case over TOL is held to max(TOL, 2 x the fp32 composition's distance from its own fp64 evaluation): that file's rule
SAMPLERS = ("ddim0", "dpmpp2m")
# a 5-iteration loop's tables hold every mode: (sampler, row) per mode
MODE_ROWS = {"final": ("ddim0", 4), "ddim0": ("ddim0", 1), "order1": ("dpmpp2m", 0), "order2": ("dpmpp2m", 2)}
SLOTS = 7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pipes(dev):
    return {2: product_pipe(dict(dims=2, pipe=E._P2), dev), 3: product_pipe(dict(dims=3, pipe=E._P3), dev)}


def _rand(name, shape, scale=1.0):
    return S.synth_input("edit." + name, shape, scale)


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("stride", [1, -1])
@pytest.mark.parametrize("src", ["counter", "dev", "host"])
@pytest.mark.parametrize("mode", list(MODE_ROWS))
@pytest.mark.parametrize("shape,offset", [((2, 4, 16), False), ((2, 3, 10), True)], ids=["aligned", "offset_view"])
def test_record_and_keep_against_the_plain_step(dev, shape, offset, mode, src, stride):
    B, Cc, cells = shape
    n = B * Cc * cells
    sampler, step = MODE_ROWS[mode]
    sch, ts, rows, table = _sched(dev, 5, sampler)
    assert rows[step].mode == {"final": L.SOLVER_FINAL, "ddim0": L.SOLVER_DDIM0, "order1": L.SOLVER_ORDER1, "order2": L.SOLVER_ORDER2}[mode]
    x_t = _view(_rand("k.xt", shape, 1.3).to(dev), offset)
    pred, pu, prev = (_rand(f"k.{k}", shape).to(dev) for k in ("pred", "pu", "prev"))
    mask = (_rand("k.m", (B, 1, cells)) > 0).to(torch.uint8).to(dev)
    slot0 = 1 if stride == 1 else 5
    slot = slot0 + stride * step
    assert 0 < slot < SLOTS - 1

    def history():
        h = torch.full((2, n), float("nan"), device=dev)
        h[(step + 1) & 1] = prev.reshape(-1)
        return h

    def step_source():
        word = torch.tensor([step, 0], dtype=torch.int32, device=dev)
        return word, dict(step=step if src == "host" else 0, counter=word if src == "counter" else None, step_dev=word[:1] if src == "dev" else None)

    want = [torch.empty(shape, device=dev) for _ in range(3)]
    want_h = history()
    K.solver_step(_args(x_t, pred, pu, want[0], want[1], want[2], want_h, table, 0, 1, 2.5, step=step))

    # RECORD, in place on the latent as the loop runs it
    fill = _rand("k.traj", (SLOTS, *shape)).to(dev)
    traj = _view(fill, offset)
    x_io, x0, xT, h = _view(x_t.clone(), offset), torch.empty(shape, device=dev), torch.empty(shape, device=dev), history()
    word, kw = step_source()
    tr = L.MfSolverTraj(traj.data_ptr(), None, 0, 0, L.TRAJ_RECORD, slot0, stride, SLOTS, 0)
    K.solver_step_traj(_args(x_io, pred, pu, x_io, x0, xT, h, table, 0, 1, 2.5, **kw), tr)
    assert torch.equal(x_io, want[0]) and torch.equal(x0, want[1]) and torch.equal(xT, want[2])
    assert torch.equal(h[step & 1], want_h[step & 1]) and torch.equal(h[(step + 1) & 1], prev.reshape(-1))
    assert torch.equal(traj[slot], x_io)                                     # the recorded slot is x_t_out
    others = [s for s in range(SLOTS) if s != slot]
    assert torch.equal(traj[others], fill[others])                           # no other slot is written
    assert word.tolist() == ([step + 1, 0] if src == "counter" else [step, 0])      # the counter advanced, the ticket left zero

    # KEEP
    traj = _view(fill, offset)
    out, x0, xT, h = torch.empty(shape, device=dev), torch.empty(shape, device=dev), torch.empty(shape, device=dev), history()
    word, kw = step_source()
    tr = L.MfSolverTraj(traj.data_ptr(), mask.data_ptr(), cells, Cc, L.TRAJ_KEEP, slot0, stride, SLOTS, 0)
    K.solver_step_traj(_args(x_t, pred, pu, out, x0, xT, h, table, 0, 1, 2.5, **kw), tr)
    regen = mask.bool().expand(B, Cc, cells)
    assert torch.equal(out[regen], want[0][regen]) and torch.equal(out[~regen], fill[slot][~regen])     # kept cells: the slot, bit for bit
    assert bool((~regen).any()) and bool(regen.any())
    assert torch.equal(x0, want[1]) and torch.equal(xT, want[2]) and torch.equal(h[step & 1], want_h[step & 1])      # the estimates stay the estimates
    assert torch.equal(traj, fill)                                           # nothing is written to the trajectory
    assert word.tolist() == ([step + 1, 0] if src == "counter" else [step, 0])


def test_a_slot_outside_the_buffer(dev):
    """known on the host: refused (MF_EINVAL).  Resolved on the device: no slot is touched -- RECORD records nothing, KEEP's kept cells are NaN."""
    shape, n = (2, 4, 16), 128
    sch, ts, rows, table = _sched(dev, 5, "ddim0")
    x_t, pred = _rand("o.xt", shape).to(dev), _rand("o.pred", shape).to(dev)
    fill = _rand("o.traj", (3, *shape)).to(dev)
    mask = (_rand("o.m", (2, 1, 16)) > 0).to(torch.uint8).to(dev)
    for slot0, stride in ((2, 1), (0, -1)):        # step 1 -> slot 3 of 3, slot -1
        traj, out = fill.clone(), torch.empty(shape, device=dev)
        rec = L.MfSolverTraj(traj.data_ptr(), None, 0, 0, L.TRAJ_RECORD, slot0, stride, 3, 0)
        with pytest.raises(RuntimeError, match="slot"):
            K.solver_step_traj(_args(x_t, pred, None, out, None, None, None, table, 0, 0, 1.0, step=1), rec)
        want = torch.empty(shape, device=dev)
        K.solver_step(_args(x_t, pred, None, want, None, None, None, table, 0, 0, 1.0, step=1))
        word = torch.tensor([1, 0], dtype=torch.int32, device=dev)
        K.solver_step_traj(_args(x_t, pred, None, out, None, None, None, table, 0, 0, 1.0, counter=word), rec)
        assert torch.equal(out, want) and torch.equal(traj, fill) and word.tolist() == [2, 0]
        keep = L.MfSolverTraj(traj.data_ptr(), mask.data_ptr(), 16, 4, L.TRAJ_KEEP, slot0, stride, 3, 0)
        one = torch.tensor([1], dtype=torch.int32, device=dev)
        K.solver_step_traj(_args(x_t, pred, None, out, None, None, None, table, 0, 0, 1.0, step_dev=one), keep)
        regen = mask.bool().expand(2, 4, 16)
        assert torch.equal(out[regen], want[regen]) and bool(out[~regen].isnan().all()) and torch.equal(traj, fill)
    with pytest.raises(RuntimeError, match="overlaps"):     # the trajectory may not be one of the launch's other tensors
        K.solver_step_traj(_args(x_t, pred, None, fill[1], None, None, None, table, 0, 0, 1.0, step=0),
                           L.MfSolverTraj(fill.data_ptr(), None, 0, 0, L.TRAJ_RECORD, 0, 1, 3, 0))


@pytest.mark.parametrize("shape", [(2, 3, 10), (2, 4, 4, 4, 4)])
def test_absdiff_mean_over_channels(dev, shape):
    a, b = _rand("d.a", shape).to(dev), _rand("d.b", shape, 0.7).to(dev)
    got = K.absdiff_mean_c(a, b)
    assert got.shape == (shape[0], 1, *shape[2:])
    want = (a.double() - b.double()).abs().sum(1, keepdim=True) / shape[1]
    e = float(((got.double() - want).abs() / want).max())
    print(f"[measured] absdiff_mean_c {shape}: relative {e:.1e}")
    assert e < 1e-6
    assert float(K.absdiff_mean_c(a, a).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 2. parity with the reference's pieces
def run_product(pipe, name, dev, **kw):
    c = E.CASES[name]
    z0, m = E.case_inputs(name)
    z0 = z0.to(dev)
    if c["kind"] == "invert":
        return pipe.invert(z0, is_latent=True, steps=E.STEPS, sampler=c["sampler"], **E.source_kwargs(c, dev), **kw)
    tk = E.target_kwargs(c, dev)
    return pipe.edit(z0, tk["condition"], source_condition=E.source_kwargs(c, dev)["condition"], strength=c.get("strength", 1.0), steps=E.STEPS,
                     sampler=c["sampler"], guidance_scale=tk["guidance_scale"], un_cond=None, mask=None if m is None else m.to(dev), is_latent=True,
                     decode=False, **kw)


@pytest.mark.parametrize("name", list(E.CASES))
def test_matches_the_reference_composition(dev, pipes, name):
    """8 asked steps on the uniform grid.  Bound: TOL; only where a case exceeds it, max(TOL, DRIFT_FACTOR x the distance of the fp32 composition
    from its own fp64 evaluation, both stored in the fixture)."""
    c, g = E.CASES[name], gold(name)
    assert int(g["steps"]) == E.STEPS and int(g["k"]) == E.span(c)
    got = run_product(pipes[c["dims"]], name, dev)
    want = T(g["result"])
    assert got.shape == want.shape
    e, bound = relerr(got, want), TOL
    line = f"[measured] {name} vs the reference's composition: {e:.1e}"
    if e >= TOL:
        drift = relerr(want, T(g["result64"]))
        bound = max(TOL, DRIFT_FACTOR * drift)
        line += f" (the fp32 composition vs its fp64 self: {drift:.1e})"
    print(f"{line}; bound {bound:.1e}")
    assert e < bound


# ------------------------------------------------------------------------------------------------ 3. the contract
@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("sampler,spacing", [("ddim0", None), ("dpmpp2m", None), ("dpmpp2m", "logsnr")])
def test_the_three_loop_forms_are_bit_identical(dev, pipes, sampler, spacing, dims):
    pipe, size = pipes[dims], E.SIZE[dims]
    z0 = _rand("l.z0", (2, *size)).to(dev)
    m = (_rand("l.m", (2, 1, *size[1:])) > 0).to(dev)
    src_c, tgt_c = torch.tensor([1, 0], device=dev), torch.tensor([0, 1], device=dev)
    kw = dict(steps=12, sampler=sampler, spacing=spacing, strength=0.75, is_latent=True)
    k = M.DiffusionPipeline._strength_span(pipe.noise_scheduler.loop_timesteps(12, True, spacing)[1], 0.75)[1]
    assert k - 1 >= 4
    inv, traj, ed, seen = {}, {}, {}, []
    for loop in ("eager", "cmdlist", "graph", None):
        pipe.last_cmdlist_launches, pipe.last_cmdlist_foreign_ops = 0, ["unset"]
        inv[loop], traj[loop] = pipe.invert(z0, src_c, guidance_scale=4.0, loop=loop, return_trajectory=True, **kw)
        if loop in ("cmdlist", None):      # the default IS the command list; the trajectory step is a launch of the library
            assert pipe.last_cmdlist_foreign_ops == [] and pipe.last_cmdlist_launches > 0
        pipe.last_cmdlist_launches = 0
        ed[loop] = pipe.edit(z0, tgt_c, source_condition=src_c, guidance_scale=4.0, mask=m, decode=False, loop=loop,
                             progress_cb=(lambda d, t: seen.append((d, t))) if loop == "eager" else None, **kw)
        if loop in ("cmdlist", None):
            assert pipe.last_cmdlist_launches > 0
    assert traj["eager"].shape == (k, *z0.shape) and torch.equal(traj["eager"][0], z0) and torch.equal(traj["eager"][-1], inv["eager"])
    assert bool(traj["eager"].isfinite().all()) and bool(ed["eager"].isfinite().all())
    for loop in ("cmdlist", "graph", None):
        assert torch.equal(inv["eager"], inv[loop]) and torch.equal(traj["eager"], traj[loop]) and torch.equal(ed["eager"], ed[loop]), loop
    keep = ~m.expand_as(z0)
    assert torch.equal(ed["eager"][keep], z0[keep]) and not torch.equal(ed["eager"][~keep], z0[~keep])
    assert seen == [(i + 1, 2 * k - 1) for i in range(2 * k - 1)]       # both passes, strictly increasing
    with pytest.raises(ValueError):      # 3 upward iterations are too few to record and replay
        pipe.invert(z0, src_c, steps=4, sampler=sampler, is_latent=True, loop="cmdlist")


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_invert_then_denoise_is_edit_with_the_source_as_target(dev, pipes, sampler):
    pipe = pipes[2]
    z0 = _rand("r.z0", (2, 8, 8, 8)).to(dev)
    cond = torch.tensor([2, 1], device=dev)
    kw = dict(steps=8, sampler=sampler, guidance_scale=4.0, un_cond=None)
    trace = []
    top = pipe.invert(z0, cond, is_latent=True, trace=trace, **kw)
    assert len(trace) == 7 and torch.equal(trace[-1][1], top)           # a trace runs the eager loop: (x_0 estimate, next latent) per iteration
    assert torch.equal(top, pipe.invert(z0, cond, is_latent=True, **kw))
    back = pipe.denoise(top, condition=cond, decode=False, **kw)
    same = pipe.edit(z0, cond, source_condition=cond, source_guidance_scale=4.0, is_latent=True, decode=False, **kw)
    assert torch.equal(back, same)
    assert not torch.equal(same, pipe.edit(z0, torch.tensor([0, 0], device=dev), source_condition=cond, source_guidance_scale=4.0, is_latent=True, decode=False, **kw))


def test_nothing_is_drawn(dev, pipes):
    pipe = pipes[2]
    z0 = _rand("n.z0", (2, 8, 8, 8)).to(dev)
    cond = torch.tensor([0, 2], device=dev)
    src = M.PhiloxDeviceNoise(7)
    src.begin(2, dev)
    src.draw((2, 8, 8, 8))
    state = torch.random.get_rng_state()
    for sampler in SAMPLERS:
        a = pipe.invert(z0, cond, is_latent=True, steps=8, sampler=sampler, noise=src)
        b = pipe.edit(z0, cond, is_latent=True, steps=8, sampler=sampler, noise=src, decode=False)
        assert src.draw_index == 1                                      # the caller's source is carried, never drawn from
        assert torch.equal(a, pipe.invert(z0, cond, is_latent=True, steps=8, sampler=sampler))
        assert torch.equal(b, pipe.edit(z0, cond, is_latent=True, steps=8, sampler=sampler, decode=False))
    assert torch.equal(state, torch.random.get_rng_state())             # without a source no key is taken from torch's generator either


def test_image_input_kept_cells_composite_and_change_map(dev, pipes):
    """through the tiny VAE: the kept cells of edit(decode=False, mask=m) are the encoded input bit for bit; composite=True pastes the input's
    pixels; return_map is [B, 1, H, W], the mean over channels of |result - x|, zero where the composite kept pixels"""
    pipe = pipes[2]
    x = _rand("v.img", (2, 3, 64, 64), 0.5).to(dev)
    m = torch.zeros((2, 1, 64, 64), dtype=torch.bool, device=dev)
    m[0, :, 10:37, 20:49] = True     # (edges inside cells: the max-reduction decides those cells)
    m[1, :, 40:64, 0:13] = True
    cond, enc = torch.tensor([2, 0], device=dev), (lambda: M.PhiloxDeviceNoise(58))
    kw = dict(steps=8, sampler="dpmpp2m", strength=0.75, guidance_scale=4.0, mask=m)
    enc_z = pipe.latent_embedder.encode(x, noise=enc())
    z0 = 2 * enc_z - 1 if pipe.do_input_centering else enc_z
    _, traj = pipe.invert(x, None, steps=8, sampler="dpmpp2m", strength=0.75, encode_noise=enc(), return_trajectory=True)
    assert torch.equal(traj[0], z0)                                     # slot 0 is the input's latent
    lat = pipe.edit(x, cond, decode=False, encode_noise=enc(), **kw)
    cells = K.mask_maxpool(m, [8, 8]).bool().expand_as(z0)
    assert torch.equal(lat[~cells], z0[~cells]) and not torch.equal(lat[cells], z0[cells])
    img, cmap = pipe.edit(x, cond, composite=True, return_map=True, encode_noise=enc(), **kw)
    assert img.shape == x.shape and cmap.shape == (2, 1, 64, 64)
    pix = m.expand_as(x)
    assert torch.equal(img[~pix], x[~pix])
    assert float(cmap[~m].abs().max()) == 0.0 and float(cmap[m].max()) > 0.0
    assert relerr(cmap, (img.double() - x.double()).abs().mean(1, keepdim=True)) < 1e-6
    plain = pipe.edit(x, cond, encode_noise=enc(), **kw)
    assert torch.equal(img[pix], plain[pix])                            # the composite changes nothing inside the mask
