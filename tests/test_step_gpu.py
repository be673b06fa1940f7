"""The step and noise kernels (csrc/sched_noise.hip, csrc/philox.h) on a real MI355X at the edges no other test runs, the library entries directly
(medfusion_amd.kernels / lib), on the shapes of tests/step_cases.py.  Exact expectations are the fp32 ATen chain on the CPU (oracle.restate's
scheduler, step_cases.chain32) or another launch of the library; Philox is held to the numpy spec (oracle.synth.philox_normal).  Every output lives
in a buffer with sentinel floats around it that must survive the launch; every comparison prints a [measured] line
(profiles/step_edges_measured.txt holds one run's).

Which gap each test closes:
  1. the grid cap (a second trip of the grid-stride loop, the ticket taken by all 1024 workgroups)
       test_sched_step_bit_for_bit_at_the_cap                sched_step_kernel, five trips
       test_one_launch_tail_at_the_cap                       sched_step_philox_kernel plain and blended, two trips, 1024 tickets per launch
       test_solver_step_at_the_cap_both_paths                solver_step_kernel, vector (two trips) and scalar (five), the counter and its ticket
       test_solver_step_blend_at_the_cap / _traj_at_the_cap  the blend and RECORD / KEEP forms
       test_solver_step_noise_at_the_cap                     solver_step_noise_kernel, all four variants
       test_philox_at_the_cap / test_absdiff_mean_c          the 2048-workgroup caps
  2. vector body plus scalar tail in one launch of solver_step_kernel
       test_solver_step_body_plus_tail_without_history
  3. a solver step without a history buffer
       test_solver_step_body_plus_tail_without_history       DDIM0, ORDER1 and FINAL rows
       test_order2_without_a_history_is_nan_and_nothing_else the second-order row
  4. sched_step_kernel at sizes that are no whole number of workgroups
       test_sched_step_bit_for_bit_at_the_tails, test_sched_step_nonfinite_in_the_last_partial_group
  5. learned variance element by element
       test_learned_variance_element_by_element
  6. Philox's counters and the ends of its uniforms
       test_philox_one_quad_per_sample, test_philox_sample_counter_wraps_mod_2_32, test_philox_draw_index_reaches_int32_max,
       test_philox_at_the_ends_of_its_uniforms, test_saturated_uniform_inside_the_fused_launches
  7. the host's refusals
       test_refusals_*"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from oracle import restate as R
from oracle import synth as S
from tests import step_cases as SC
from tests.test_solver_gpu import back_half_bound
from tests.util import offset_view

SENT = -7.25          # the sentinel: no seeded input and no result of a step equals it bit for bit over a whole guard
GUARD = 8
N_CAP = SC.numel(SC.CAP)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Out:
    """an [n] output with one sentinel float before it (when `offset`: the tensor then starts 4 bytes off a 16-byte boundary) and GUARD behind it"""

    def __init__(self, n, dev, offset=False, init=None):
        self.off, self.n = (1 if offset else 0), n
        self.buf = torch.full((self.off + n + GUARD,), SENT, device=dev)
        self.t = self.buf[self.off: self.off + n]
        assert self.t.data_ptr() % 16 == 4 * self.off and self.t.is_contiguous()
        if init is not None:
            self.t.copy_(init.reshape(-1))

    def intact(self):
        guard = torch.cat([self.buf[: self.off], self.buf[self.off + self.n:]])
        return guard.numel() >= GUARD and bool((guard == SENT).all())

    def reset(self):
        self.buf.fill_(SENT)

    def virgin(self):
        return bool((self.buf == SENT).all())


def _p(t):
    return None if t is None else t.data_ptr()


def _sched_args(x_t, pred, pu, pv, npost, nddim, out, x0, xT, table, step, objective, clip, g, step_dev=None, n=None):
    return L.MfSchedArgs(_p(x_t), _p(pred), _p(pu), _p(pv), _p(npost), _p(nddim), 0, _p(out), _p(x0), _p(xT), _p(table), _p(step_dev), step, objective, clip, g,
                         x_t.numel() if n is None else n)


def _solver_args(x_t, pred, pu, out, x0, xT, hist, table, objective, clip, g, step=0, counter=None, step_dev=None, n=None):
    return L.MfSolverArgs(_p(x_t), _p(pred), _p(pu), _p(out), _p(x0), _p(xT), _p(hist), _p(table), _p(counter), None if counter is None else counter.data_ptr() + 4,
                          _p(step_dev), step, objective, clip, g, x_t.numel() if n is None else n)


def _supplied(scale, eps, stride=0):
    return L.MfSolverNoise(_p(scale), _p(eps), stride, 0, 0, 0, 0, 0, 0)


def _philox(scale, seed, base, stride, offset, B):
    return L.MfSolverNoise(_p(scale), None, 0, seed, offset, base, stride, B, 0)


def _no_diff(got, want, what):
    bad = SC.same_bits(got, want)
    assert bad == [], (what, "first differing elements", [(i, float(got.reshape(-1)[i]), float(want.reshape(-1)[i])) for i in bad])


@pytest.fixture(scope="module")
def tables(dev):
    """one scheduler, its 7-iteration grid, and every table the tests index, uploaded once"""
    sch = M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())
    ts, _ = sch.loop_timesteps(SC.STEPS, True)
    assert ts == SC.timesteps()
    t = dict(sch=sch, ts=ts, osch=SC.oracle_scheduler())
    t["step"] = sch.upload_records(sch.step_records(ts, True), dev)
    for sampler in ("ddim0", "dpmpp2m"):
        rows = sch.solver_records(ts, sampler)
        t[sampler] = (rows, sch.upload_solver_records(rows, dev))
    lts, _ = sch.loop_timesteps(SC.STEPS, True, "logsnr")
    rows, scales = sch.stochastic_records(lts, "dpmpp2m_sde")
    t["sde"] = (rows, sch.upload_solver_records(rows, dev), torch.tensor(scales, device=dev), lts)
    t["coef"] = sch.blend_records(ts).to(dev)
    t["coef_sde"] = sch.blend_records(lts).to(dev)
    assert [r.mode for r in t["ddim0"][0]] == [1] * 6 + [0] and [r.mode for r in t["dpmpp2m"][0]] == [2, 3, 3, 3, 3, 3, 0]
    assert [r.mode for r in rows] == [2, 3, 3, 3, 3, 3, 0] and len(rows) == SC.STEPS
    return t


@pytest.fixture(scope="module")
def cap(dev):
    """the CAP inputs, made once: host copies for the CPU chain, device copies for the launches, and the blend state; nothing writes to them"""
    host = SC.step_inputs(N_CAP)
    host["prev"] = SC.rand("cap.prev", (N_CAP,))
    d = {k: v.to(dev) for k, v in host.items()}
    B, Cc, cells = SC.CAP
    z0, eps0 = SC.rand("cap.z0", SC.CAP).to(dev), SC.rand("cap.eps0", SC.CAP).to(dev)
    mask = (SC.rand("cap.mask", (B, 1, cells)) > 0).to(torch.uint8).to(dev)
    assert 0 < int(mask.sum()) < mask.numel()
    return dict(host=host, dev=d, z0=z0, eps0=eps0, mask=mask)


def _blend(cap, coef):
    B, Cc, cells = SC.CAP
    return L.MfSchedBlend(cap["z0"].data_ptr(), cap["eps0"].data_ptr(), cap["mask"].data_ptr(), coef.data_ptr(), cells, Cc, 0)


# ------------------------------------------------------------------------------------------------ a. sched_step bit for bit
def _sched_step_case(dev, tables, host, d, n, offset, objective, clip, cfg, i, what):
    c = SC.chain32(tables["osch"], tables["ts"], i, True, host["x_t"], host["pred"], host["pu"] if cfg else None, SC.G, objective, bool(clip), host["npost"], host["nddim"])
    v = {k: offset_view(d[k], offset) for k in ("x_t", "pred", "pu", "npost", "nddim")}
    outs = [Out(n, dev, offset) for _ in range(3)]
    K.sched_step(_sched_args(v["x_t"], v["pred"], v["pu"] if cfg else None, None, v["npost"], v["nddim"], outs[0].t, outs[1].t, outs[2].t, tables["step"], i,
                             objective, clip, SC.G))
    for o, k in zip(outs, ("x_t", "x0", "xT")):
        _no_diff(o.t, c[k], (what, n, offset, i, k))
        assert o.intact(), (what, n, offset, i, k, "a store outside the tensor")
    return c


@pytest.mark.parametrize("objective,clip,cfg", SC.STEP_CONFIGS)
def test_sched_step_bit_for_bit_at_the_tails(dev, tables, objective, clip, cfg):
    runs = 0
    for n in SC.TAILS:
        host = SC.step_inputs(n)
        d = {k: v.to(dev) for k, v in host.items()}
        for offset in (False, True):
            for i in SC.STEP_ROWS.values():
                _sched_step_case(dev, tables, host, d, n, offset, objective, clip, cfg, i, "tails")
                runs += 1
    print(f"[measured] sched_step objective {objective} clip {clip} pair {cfg}: {runs} launches over n in {SC.TAILS}, aligned and 4 bytes off, x_t / x_0 / x_T: "
          f"0 elements differ from the fp32 chain, every guard intact")


@pytest.mark.parametrize("objective,clip,cfg", SC.STEP_CONFIGS)
def test_sched_step_bit_for_bit_at_the_cap(dev, tables, cap, objective, clip, cfg):
    blocks, trips = SC.launch(N_CAP, SC.STEP_CAP)
    assert (blocks, trips) == (1024, 5)
    for row, i in SC.STEP_ROWS.items():
        _sched_step_case(dev, tables, cap["host"], cap["dev"], N_CAP, False, objective, clip, cfg, i, "cap")
    print(f"[measured] sched_step at n = {N_CAP} ({blocks} workgroups, {trips} trips) objective {objective} clip {clip} pair {cfg}: 0 elements differ from the fp32 chain")


@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("cfg", [False, True])
def test_sched_step_nonfinite_in_the_last_partial_group(dev, tables, objective, cfg):
    """n = 1023, clip_x0 on: a NaN, a +Inf and a -Inf in elements 1020..1022, the three scalars behind the last whole vector"""
    n = 1023
    host = SC.step_inputs(n)
    host["pred"] = SC.plant_nonfinite(host["pred"])
    d = {k: v.to(dev) for k, v in host.items()}
    for offset in (False, True):
        for row, i in SC.STEP_ROWS.items():
            c = _sched_step_case(dev, tables, host, d, n, offset, objective, 1, cfg, i, "nonfinite")
            assert {k: SC.nonfinite_counts(c[k]) for k in ("x_t", "x0", "xT")} == SC.planted_counts(objective, row)
    print(f"[measured] sched_step n = 1023, NaN / +Inf / -Inf in the last partial group, objective {objective} pair {cfg}: NaN masks and all other bits equal the chain's")


# ------------------------------------------------------------------------------------------------ b. the one-launch tail at the cap
@pytest.mark.parametrize("blend", [False, True], ids=["plain", "blend"])
def test_one_launch_tail_at_the_cap(dev, tables, cap, blend):
    """three consecutive iterations driven by the device counter: mf_sched_step_philox[_blend]_f32 against mf_philox_normal_f32 x 2 +
    mf_sched_step[_blend]_f32 + mf_counter_add_i32, rows 3.. of a larger batch"""
    B = SC.CAP[0]
    seed, off, base, stride = 0x1234567890ABCDEF, 3, 1, 2
    assert SC.launch(N_CAP // 4, SC.STEP_CAP) == (1024, 2)
    d = cap["dev"]
    bl = _blend(cap, tables["coef"]) if blend else None
    xa, xb, x0a, x0b = Out(N_CAP, dev, init=d["x_t"]), Out(N_CAP, dev, init=d["x_t"]), Out(N_CAP, dev), Out(N_CAP, dev)
    n_post, n_ddim = torch.empty(SC.CAP, device=dev), torch.empty(SC.CAP, device=dev)
    ca = torch.zeros(1, dtype=torch.int32, device=dev)
    cb = torch.zeros(2, dtype=torch.int32, device=dev)
    for i in range(3):
        pred, pu = SC.rand(f"cap.tail.pred{i}", (N_CAP,)).to(dev), d["pu"]
        K.philox_normal(n_post, seed, base, off, step_dev=ca, draw_stride=stride)
        K.philox_normal(n_ddim, seed, base + 1, off, step_dev=ca, draw_stride=stride)
        a = _sched_args(xa.t, pred, pu, None, n_post, n_ddim, xa.t, x0a.t, None, tables["step"], 0, 0, 0, 3.0, step_dev=ca)
        b = _sched_args(xb.t, pred, pu, None, None, None, xb.t, x0b.t, None, tables["step"], 0, 0, 0, 3.0, step_dev=cb)
        if blend:
            K.sched_step_blend(a, bl)
            K.sched_step_philox_blend(b, bl, seed, base, stride, off, B, cb)
        else:
            K.sched_step(a)
            K.sched_step_philox(b, seed, base, stride, off, B, cb)
        K.counter_add(ca, 1)
        _no_diff(xb.t, xa.t, ("x_t", i, blend))
        _no_diff(x0b.t, x0a.t, ("x_0", i, blend))
        assert cb.tolist() == [i + 1, 0] and int(ca.item()) == i + 1, (i, cb.tolist())      # 1024 tickets taken, the word back at zero
        assert all(o.intact() for o in (xa, xb, x0a, x0b))
    assert bool(xa.t.isfinite().all())
    if blend:
        keep = (cap["mask"] == 0).expand(*SC.CAP).reshape(-1)
        a_, c_ = tables["coef"][2]
        known = K.rows_axpby(cap["z0"], a_.expand(B).contiguous(), cap["eps0"], c_.expand(B).contiguous()).reshape(-1)
        assert torch.equal(xb.t[keep], known[keep]) and not torch.equal(xb.t[~keep], known[~keep])
    print(f"[measured] one-launch tail at n = {N_CAP} ({'blend' if blend else 'plain'}): 3 iterations, x_t and x_0 bit-identical to the four launches, "
          f"counter [1, 0] [2, 0] [3, 0]")


# ------------------------------------------------------------------------------------------------ c. solver_step
SOLVER_ROWS = {"ddim0": ("ddim0", 1), "order1": ("dpmpp2m", 0), "final": ("ddim0", 6)}


@pytest.mark.parametrize("objective,cfg", [(0, False), (0, True), (1, False), (1, True)])
def test_solver_step_body_plus_tail_without_history(dev, tables, objective, cfg):
    """no history buffer: aligned, the launch runs n // 4 vectors and then 1..3 scalars; on views 4 bytes off, scalars only.  Same bits; the front
    half is mf_sched_step_f32's; the back half within the bound of tests/test_solver_gpu.py"""
    worst, runs = 0.0, 0
    for n in SC.TAILS:
        host = SC.step_inputs(n, "c")
        d = {k: v.to(dev) for k, v in host.items()}
        for name, (sampler, step) in SOLVER_ROWS.items():
            rows, table = tables[sampler]
            r = rows[step]
            assert r.mode == {"ddim0": L.SOLVER_DDIM0, "order1": L.SOLVER_ORDER1, "final": L.SOLVER_FINAL}[name]
            res = []
            for offset in (False, True):
                v = {k: offset_view(d[k], offset) for k in ("x_t", "pred", "pu")}
                outs = [Out(n, dev, offset) for _ in range(3)]
                K.solver_step(_solver_args(v["x_t"], v["pred"], v["pu"] if cfg else None, outs[0].t, outs[1].t, outs[2].t, None, table, objective, 1, SC.G, step=step))
                assert all(o.intact() for o in outs), (n, name, offset, "a store outside the tensor")
                res.append(outs)
            for a, b, k in zip(res[0], res[1], ("x_t", "x0", "xT")):
                _no_diff(a.t, b.t, (n, name, k, "aligned against 4 bytes off"))
            want = [Out(n, dev) for _ in range(3)]
            K.sched_step(_sched_args(d["x_t"], d["pred"], d["pu"] if cfg else None, None, d["npost"], d["nddim"], want[0].t, want[1].t, want[2].t, tables["step"], step,
                                     objective, 1, SC.G))
            _no_diff(res[0][1].t, want[1].t, (n, name, "x_0 against sched_step"))
            _no_diff(res[0][2].t, want[2].t, (n, name, "x_T against sched_step"))
            got = res[0][0].t
            if r.mode == L.SOLVER_FINAL:
                _no_diff(got, res[0][1].t, (n, name, "the final row returns its x_0"))
            else:
                w64, bound, mag = back_half_bound(r, d["x_t"].double().cpu(), res[0][1].t.double().cpu(), res[0][2].t.double().cpu(), None)
                err = (got.double().cpu() - w64).abs()
                bad = (err > bound).nonzero().reshape(-1)
                assert bad.numel() == 0, (n, name, [(int(i), float(got[i]), float(w64[i])) for i in bad[:8]])
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            runs += 1
    print(f"[measured] solver_step without a history, objective {objective} pair {cfg}: {runs} (n, row) pairs, vector body + scalar tail bit-identical to the "
          f"scalar path, x_0 / x_T to sched_step; back half largest |x_t - fp64| / bound {worst:.3f}")
    assert worst <= 1.0


def test_order2_without_a_history_is_nan_and_nothing_else(dev, tables):
    rows, table = tables["dpmpp2m"]
    step = 2
    assert rows[step].mode == L.SOLVER_ORDER2
    for n in SC.TAILS + (4096,):
        host = SC.step_inputs(n, "c")
        d = {k: v.to(dev) for k, v in host.items()}
        prev = SC.rand(f"c.{n}.prev", (n,)).to(dev)
        bare = [Out(n, dev) for _ in range(3)]
        K.solver_step(_solver_args(d["x_t"], d["pred"], d["pu"], bare[0].t, bare[1].t, bare[2].t, None, table, 0, 1, SC.G, step=step))
        full = [Out(n, dev) for _ in range(3)]
        hist = Out(2 * n, dev)
        h = hist.t.view(2, n)
        h[(step + 1) & 1] = prev
        K.solver_step(_solver_args(d["x_t"], d["pred"], d["pu"], full[0].t, full[1].t, full[2].t, hist.t, table, 0, 1, SC.G, step=step))
        assert bool(bare[0].t.isnan().all()), (n, (~bare[0].t.isnan()).nonzero()[:8].tolist())
        _no_diff(bare[1].t, full[1].t, (n, "x_0"))
        _no_diff(bare[2].t, full[2].t, (n, "x_T"))
        assert bool(full[0].t.isfinite().all()) and torch.equal(h[(step + 1) & 1], prev) and torch.equal(h[step & 1], full[1].t)
        assert all(o.intact() for o in bare + full + [hist]), n
    print(f"[measured] solver_step, second-order row without a history, n in {SC.TAILS + (4096,)}: x_t NaN everywhere, x_0 / x_T bit-equal to the run with one")


def test_solver_step_at_the_cap_both_paths(dev, tables, cap):
    """three iterations of dpmpp2m (first-order, then two second-order rows) driven by the counter: aligned with a history (16-byte vectors, two
    trips) against everything 4 bytes off (scalars, five trips); the front half against mf_sched_step_f32"""
    rows, table = tables["dpmpp2m"]
    d = cap["dev"]
    assert SC.launch(N_CAP // 4, SC.STEP_CAP) == (1024, 2) and SC.launch(N_CAP, SC.STEP_CAP) == (1024, 5)
    runs = []
    for offset in (False, True):
        runs.append(dict(x=Out(N_CAP, dev, offset, init=d["x_t"]), x0=Out(N_CAP, dev, offset), xT=Out(N_CAP, dev, offset), hist=Out(2 * N_CAP, dev, offset),
                         counter=torch.zeros(2, dtype=torch.int32, device=dev), pu=offset_view(d["pu"], offset)))
    w0, wT, junk = Out(N_CAP, dev), Out(N_CAP, dev), torch.empty(N_CAP, device=dev)
    for i in range(3):
        pred = SC.rand(f"cap.solver.pred{i}", (N_CAP,), 0.9).to(dev)
        x_in = runs[0]["x"].t.clone()
        prev = None if i == 0 else runs[0]["hist"].t.view(2, N_CAP)[(i + 1) & 1].clone()
        for offset, r in zip((False, True), runs):
            K.solver_step(_solver_args(r["x"].t, offset_view(pred, offset), r["pu"], r["x"].t, r["x0"].t, r["xT"].t, r["hist"].t, table, 0, 1, SC.G, counter=r["counter"]))
            assert r["counter"].tolist() == [i + 1, 0], (i, offset, r["counter"].tolist())
            assert all(r[k].intact() for k in ("x", "x0", "xT", "hist")), (i, offset)
        a, b = runs
        for k in ("x", "x0", "xT"):
            _no_diff(a[k].t, b[k].t, (i, k, "vector against scalar"))
        ha, hb = a["hist"].t.view(2, N_CAP), b["hist"].t.view(2, N_CAP)
        _no_diff(ha[i & 1], a["x0"].t, (i, "this step's slot"))
        _no_diff(hb[i & 1], ha[i & 1], (i, "this step's slot, scalar"))
        if prev is None:
            assert bool((ha[1] == SENT).all()) and bool((hb[1] == SENT).all())          # the slot the first step must not write
        else:
            _no_diff(ha[(i + 1) & 1], prev, (i, "the other slot"))
            _no_diff(hb[(i + 1) & 1], prev, (i, "the other slot, scalar"))
        K.sched_step(_sched_args(x_in, pred, d["pu"], None, d["npost"], d["nddim"], junk, w0.t, wT.t, tables["step"], i, 0, 1, SC.G))
        _no_diff(a["x0"].t, w0.t, (i, "x_0 against sched_step"))
        _no_diff(a["xT"].t, wT.t, (i, "x_T against sched_step"))
    assert bool(runs[0]["x"].t.isfinite().all())
    print(f"[measured] solver_step at n = {N_CAP}: 3 counter-driven iterations, vector path (2 trips) and scalar path (5 trips) bit-identical, x_0 / x_T equal "
          f"sched_step's, counter [1, 0] [2, 0] [3, 0] on both")


def test_solver_step_blend_at_the_cap(dev, tables, cap):
    rows, table = tables["dpmpp2m"]
    B = SC.CAP[0]
    d, step = cap["dev"], 3
    hist = Out(2 * N_CAP, dev)
    hist.t.view(2, N_CAP)[(step + 1) & 1] = d["prev"]
    plain, blended = Out(N_CAP, dev), Out(N_CAP, dev)
    K.solver_step(_solver_args(d["x_t"], d["pred"], d["pu"], plain.t, None, None, hist.t, table, 0, 1, 2.5, step=step))
    x0 = hist.t.view(2, N_CAP)[step & 1].clone()
    K.solver_step(_solver_args(d["x_t"], d["pred"], d["pu"], blended.t, None, None, hist.t, table, 0, 1, 2.5, step=step), _blend(cap, tables["coef"]))
    a_, c_ = tables["coef"][step]
    known = K.rows_axpby(cap["z0"], a_.expand(B).contiguous(), cap["eps0"], c_.expand(B).contiguous())
    want = K.select_cells(cap["mask"], plain.t.view(SC.CAP), known)
    _no_diff(blended.t, want, "blend against rows_axpby + select_cells")
    _no_diff(hist.t.view(2, N_CAP)[step & 1], x0, "the history slot stays the estimate")
    assert not torch.equal(blended.t, plain.t) and plain.intact() and blended.intact() and hist.intact()
    print(f"[measured] solver_step_blend at n = {N_CAP}: 0 elements differ from the plain step + rows_axpby + select_cells")


def test_solver_step_traj_at_the_cap(dev, tables, cap):
    """RECORD and KEEP on a [2][n] trajectory, slot 1 = slot0 + step: the slot is bit-equal, slot 0 is untouched"""
    rows, table = tables["ddim0"]
    B, Cc, cells = SC.CAP
    d, step, slots = cap["dev"], 1, 2
    want = [Out(N_CAP, dev) for _ in range(3)]
    K.solver_step(_solver_args(d["x_t"], d["pred"], d["pu"], want[0].t, want[1].t, want[2].t, None, table, 0, 1, 2.5, step=step))
    fill = torch.stack([d["prev"], d["nddim"]])
    # RECORD
    traj, got = Out(slots * N_CAP, dev, init=fill), [Out(N_CAP, dev) for _ in range(3)]
    word = torch.tensor([step, 0], dtype=torch.int32, device=dev)
    tr = L.MfSolverTraj(traj.t.data_ptr(), None, 0, 0, L.TRAJ_RECORD, 0, 1, slots, 0)
    K.solver_step_traj(_solver_args(d["x_t"], d["pred"], d["pu"], got[0].t, got[1].t, got[2].t, None, table, 0, 1, 2.5, counter=word), tr)
    for g, w, k in zip(got, want, ("x_t", "x0", "xT")):
        _no_diff(g.t, w.t, ("RECORD", k))
    tv = traj.t.view(slots, N_CAP)
    _no_diff(tv[1], want[0].t, "the recorded slot")
    _no_diff(tv[0], fill[0], "the other slot")
    assert word.tolist() == [step + 1, 0] and traj.intact() and all(o.intact() for o in got)
    # KEEP
    traj, got = Out(slots * N_CAP, dev, init=fill), [Out(N_CAP, dev) for _ in range(3)]
    tr = L.MfSolverTraj(traj.t.data_ptr(), cap["mask"].data_ptr(), cells, Cc, L.TRAJ_KEEP, 0, 1, slots, 0)
    K.solver_step_traj(_solver_args(d["x_t"], d["pred"], d["pu"], got[0].t, got[1].t, got[2].t, None, table, 0, 1, 2.5, step=step), tr)
    regen = cap["mask"].bool().expand(B, Cc, cells).reshape(-1)
    _no_diff(got[0].t[regen], want[0].t[regen], "KEEP, regenerated cells")
    _no_diff(got[0].t[~regen], fill[1][~regen], "KEEP, kept cells")
    _no_diff(got[1].t, want[1].t, "KEEP x0")
    _no_diff(got[2].t, want[2].t, "KEEP xT")
    _no_diff(traj.t, fill, "KEEP writes nothing to the trajectory")
    assert traj.intact() and all(o.intact() for o in got)
    print(f"[measured] solver_step_traj at n = {N_CAP}: RECORD's slot and KEEP's kept cells bit-equal, the other slot untouched")


# ------------------------------------------------------------------------------------------------ d. solver_step_noise at the cap
def test_solver_step_noise_at_the_cap(dev, tables, cap):
    rows, table, scale, lts = tables["sde"]
    B = SC.CAP[0]
    d, step = cap["dev"], 2
    seed, base, stride, off = 0x1234567890ABCDEF, 5, 2, 3
    assert rows[step].mode == L.SOLVER_ORDER2 and float(scale[step]) > 0 and rows[6].mode == L.SOLVER_FINAL
    zero = torch.zeros(len(rows), device=dev)
    eps = K.philox_normal(torch.empty(SC.CAP, device=dev), seed, base + stride * step, off)
    nan_bank = torch.full((N_CAP,), float("nan"), device=dev)

    def run(fn, st):
        outs, hist = [Out(N_CAP, dev) for _ in range(3)], Out(2 * N_CAP, dev)
        hist.t.view(2, N_CAP)[(st + 1) & 1] = d["prev"]
        word = torch.tensor([st, 0], dtype=torch.int32, device=dev)
        fn(_solver_args(d["x_t"], d["pred"], d["pu"], outs[0].t, outs[1].t, outs[2].t, hist.t, table, 0, 1, 2.5, counter=word))
        assert word.tolist() == [st + 1, 0] and all(o.intact() for o in outs + [hist])
        assert torch.equal(hist.t.view(2, N_CAP)[(st + 1) & 1], d["prev"])
        return [o.t for o in outs] + [hist.t.view(2, N_CAP)[st & 1]]

    def same(a, b, what):
        for x, y, k in zip(a, b, ("x_t", "x0", "xT", "history slot")):
            _no_diff(x, y, (what, k))

    for bl in (None, _blend(cap, tables["coef_sde"])):
        tag = "blend" if bl is not None else "plain"
        sup = run(lambda a: K.solver_step_noise(a, _supplied(scale, eps), bl), step)
        phx = run(lambda a: K.solver_step_noise(a, _philox(scale, seed, base, stride, off, B), bl), step)
        same(phx, sup, (tag, "Philox in the launch against the supplied draw"))
        det = run(lambda a: K.solver_step(a, bl), step)
        same(run(lambda a: K.solver_step_noise(a, _supplied(zero, eps), bl), step), det, (tag, "zero scales against solver_step"))
        assert not torch.equal(sup[0], det[0])
        # the final row draws nothing, whatever the bank holds
        fin = run(lambda a: K.solver_step(a, bl), 6)
        same(run(lambda a: K.solver_step_noise(a, _supplied(scale, nan_bank), bl), 6), fin, (tag, "final row, supplied NaN bank"))
        same(run(lambda a: K.solver_step_noise(a, _philox(scale, seed, base, stride, off, B), bl), 6), fin, (tag, "final row, Philox form"))
        assert bool(fin[0].isfinite().all())
        print(f"[measured] solver_step_noise at n = {N_CAP} ({tag}): Philox form = supplied form, zero scales = solver_step, final row = solver_step with a NaN "
              f"bank: 0 elements differ")


# ------------------------------------------------------------------------------------------------ e. learned variance
@pytest.mark.parametrize("t", SC.VAR_T)
def test_learned_variance_element_by_element(dev, tables, t):
    """x_0 bit for bit; |x_t - want64| <= E per element, want64 and E from the fp32 chain's own mean and exponent (step_cases.variance_bound);
    t = 0: sd = 0 and x_t is the mean bit for bit"""
    sch, osch = tables["sch"], tables["osch"]
    table = sch.upload_records(sch.step_records([t], False), dev)
    worst, n_cases = 0.0, 0
    for case in [c for c in SC.variance_cases() if c["t"] == t]:
        n = case["n"]
        x_t, pred, pv, npost = SC.variance_inputs(case)
        c = SC.chain32(osch, [t], 0, False, x_t, pred, None, 1.0, 0, False, npost, pv=pv)
        want, E = SC.variance_bound(c["mean"], c["hl"], npost, t)
        out, x0 = Out(n, dev), Out(n, dev)
        dv = [v.to(dev) for v in (x_t, pred, pv, npost)]
        K.sched_step(_sched_args(dv[0], dv[1], None, dv[2], dv[3], None, out.t, x0.t, None, table, 0, 0, 0, 1.0))
        assert out.intact() and x0.intact()
        _no_diff(x0.t, c["x0"], (case["name"], "x_0"))
        if t == 0:
            _no_diff(out.t, c["mean"], (case["name"], "x_t is the mean"))
        else:
            got = out.t.double().cpu()
            err = (got - want).abs()
            bad = (err > E).nonzero().reshape(-1)
            worst = max(worst, float((err / E).max()))
            assert bad.numel() == 0, (case["name"], [(int(i), float(got[i]), float(want[i]), float(E[i])) for i in bad[:8]])
        n_cases += 1
    print(f"[measured] learned variance t = {t}, the kernel: {n_cases} cases, x_0 bit for bit, largest |x_t - fp64| / E {worst:.3f} (k = {SC.EXP_ULPS})")


# ------------------------------------------------------------------------------------------------ f. Philox
def _philox_out(B, per, dev):
    o = Out(B * per, dev)
    return o, o.t.view(B, per)


def _against_spec(got, want, what, skip=None):
    """per element: |got - want| <= PHILOX_TOL, no NaN -> the largest difference"""
    g = got.detach().cpu().double().reshape(-1)
    w = torch.from_numpy(np.ascontiguousarray(want)).double().reshape(-1)
    err = (g - w).abs()
    if skip is not None:
        err[skip] = 0.0
    assert not bool(torch.isnan(g).any()), (what, torch.isnan(g).nonzero()[:8].tolist())
    bad = (~(err <= SC.PHILOX_TOL)).nonzero().reshape(-1)
    assert bad.numel() == 0, (what, [(int(i), float(g[i]), float(w[i])) for i in bad[:8]])
    return float(err.max())


def test_philox_at_the_cap(dev):
    B, per = SC.CAP_PHILOX[0], SC.CAP_PHILOX[1] * SC.CAP_PHILOX[2]
    assert SC.launch(B * per // 4, SC.WIDE_CAP) == (2048, 2)
    o, v = _philox_out(B, per, dev)
    K.philox_normal(v, SC.SEED, 5, 10)
    e = _against_spec(v, S.philox_normal(SC.SEED, 5, np.arange(10, 10 + B), per), "cap")
    assert o.intact()
    print(f"[measured] philox_normal at {B * per} elements (2048 workgroups, 2 trips): largest |philox - spec| {e:.2e} (tolerance {SC.PHILOX_TOL:.0e})")


def test_philox_one_quad_per_sample(dev):
    o, v = _philox_out(1000, 4, dev)
    K.philox_normal(v, SC.SEED, 5, 10)
    e = _against_spec(v, S.philox_normal(SC.SEED, 5, np.arange(10, 1010), 4), "one quad per sample")
    assert o.intact()
    print(f"[measured] philox_normal B = 1000, per_sample = 4: largest |philox - spec| {e:.2e}")


@pytest.mark.parametrize("offset", [2 ** 31 - 2, 2 ** 32 - 2])
def test_philox_sample_counter_wraps_mod_2_32(dev, offset):
    """the sample index is one 32-bit word of the counter: rows past 2^31 keep their bits, rows past 2^32 draw what rows 0, 1 draw"""
    B, per = 4, 1024
    o, v = _philox_out(B, per, dev)
    K.philox_normal(v, SC.SEED, 7, offset)
    e = _against_spec(v, SC.spec_rows(SC.SEED, 7, offset, B, per), ("offset", offset))
    assert o.intact()
    if offset == 2 ** 32 - 2:
        low = torch.empty((2, per), device=dev)
        K.philox_normal(low, SC.SEED, 7, 0)
        _no_diff(v[2:], low, "rows 2^32 and 2^32 + 1 against rows 0 and 1")
    print(f"[measured] philox_normal sample_offset = {offset}, B = 4: largest |philox - spec(index mod 2^32)| {e:.2e}")


def test_philox_draw_index_reaches_int32_max(dev):
    B, per = 3, 512
    base, stride, step = 1, 715827882, 3
    assert base + stride * step == 2 ** 31 - 1
    o, v = _philox_out(B, per, dev)
    K.philox_normal(v, SC.SEED, base, 2, step_dev=torch.tensor([step], dtype=torch.int32, device=dev), draw_stride=stride)
    e = _against_spec(v, S.philox_normal(SC.SEED, 2 ** 31 - 1, np.arange(2, 2 + B), per), "draw 2^31 - 1")
    host = torch.empty((B, per), device=dev)
    K.philox_normal(host, SC.SEED, 2 ** 31 - 1, 2)
    _no_diff(v, host, "the device step against the host's draw index")
    assert o.intact()
    print(f"[measured] philox_normal draw = 1 + 715827882 * 3 = 2^31 - 1 from a device step: largest |philox - spec| {e:.2e}")


def _pair_at(sample, quad, word):
    i = sample * SC.EXTREME_PER_SAMPLE + 4 * quad + 2 * (word // 2)
    return [i, i + 1]


@pytest.mark.parametrize("entry", SC.EXTREMES, ids=[f"s{e[0]}q{e[1]}d{e[2]}w{e[3]}{'ones' if e[4] else 'zero'}" for e in SC.EXTREMES])
def test_philox_at_the_ends_of_its_uniforms(dev, entry):
    sample, quad, draw, word, top = entry
    o, v = _philox_out(SC.EXTREME_SAMPLES, SC.EXTREME_PER_SAMPLE, dev)
    K.philox_normal(v, SC.SEED, draw, 0)
    want = SC.spec_block(draw)
    pair = _pair_at(sample, quad, word)
    got = v.reshape(-1)[pair].cpu()
    if word in (0, 2) and top == SC.ONES:
        # u = 1.0 exactly: the radius is sqrt(-2 log 1) = -0, both normals +-0 -- finite, never NaN
        assert bool(torch.isfinite(got).all()) and bool((got == 0.0).all()), (entry, got.tolist())
    e = _against_spec(v, want, entry)
    assert o.intact()
    print(f"[measured] philox_normal at sample {sample} quad {quad} draw {draw} word {word} ({'ones' if top else 'zero'}): the pair {got.tolist()}, spec "
          f"{want.reshape(-1)[pair].tolist()}; largest |philox - spec| over the [8, 4096] block {e:.2e}")


@pytest.mark.parametrize("entry", SC.EXTREMES[:2], ids=["word0", "word2"])
def test_saturated_uniform_inside_the_fused_launches(dev, tables, entry):
    """the two counters whose radius uniform is exactly 1.0, through mf_sched_step_philox_f32 (the posterior draw) and mf_solver_step_noise_f32 (the
    Philox form): the element there is finite and equals the deterministic part, and the launch agrees with its unfused form everywhere"""
    sample, quad, draw, word, top = entry
    shape = (SC.EXTREME_SAMPLES, 4, 1024)
    B, n = shape[0], SC.numel(shape)
    assert top == SC.ONES and word in (0, 2) and n // B == SC.EXTREME_PER_SAMPLE
    pair = _pair_at(sample, quad, word)
    host = SC.step_inputs(n, "sat")
    d = {k: v.to(dev) for k, v in host.items()}
    eps = K.philox_normal(torch.empty(shape, device=dev), SC.SEED, draw, 0)
    assert bool((eps.reshape(-1)[pair] == 0.0).all())
    zeros = torch.zeros(n, device=dev)
    # the posterior rows of a loop without DDIM: x_t = mean + sd * draw
    sch = tables["sch"]
    ts, _ = sch.loop_timesteps(SC.STEPS, False)
    recs = sch.step_records(ts, False)
    table = sch.upload_records(recs, dev)
    assert recs[0].mode == 0 and recs[0].std_fixed > 0
    fused, f0, unf, u0, det = (Out(n, dev) for _ in range(5))
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    K.sched_step_philox(_sched_args(d["x_t"], d["pred"], d["pu"], None, None, None, fused.t, f0.t, None, table, 0, 0, 1, SC.G), SC.SEED, draw, 1, 0, B, counter)
    K.sched_step(_sched_args(d["x_t"], d["pred"], d["pu"], None, eps, None, unf.t, u0.t, None, table, 0, 0, 1, SC.G))
    K.sched_step(_sched_args(d["x_t"], d["pred"], d["pu"], None, zeros, None, det.t, None, None, table, 0, 0, 1, SC.G))
    _no_diff(fused.t, unf.t, "sched_step_philox against philox_normal + sched_step")
    _no_diff(f0.t, u0.t, "x_0")
    assert bool(fused.t.isfinite().all()) and counter.tolist() == [1, 0]
    _no_diff(fused.t[pair], det.t[pair], "the element at the saturated uniform is the posterior mean")
    assert not torch.equal(fused.t, det.t) and all(o.intact() for o in (fused, f0, unf, u0, det))
    # the stochastic solver step
    rows, stable, scale, lts = tables["sde"]
    assert rows[0].mode == L.SOLVER_ORDER1 and float(scale[0]) > 0
    fused, unf, det = (Out(n, dev) for _ in range(3))
    K.solver_step_noise(_solver_args(d["x_t"], d["pred"], d["pu"], fused.t, None, None, None, stable, 0, 1, SC.G, step=0), _philox(scale, SC.SEED, draw, 0, 0, B))
    K.solver_step_noise(_solver_args(d["x_t"], d["pred"], d["pu"], unf.t, None, None, None, stable, 0, 1, SC.G, step=0), _supplied(scale, eps))
    K.solver_step(_solver_args(d["x_t"], d["pred"], d["pu"], det.t, None, None, None, stable, 0, 1, SC.G, step=0))
    _no_diff(fused.t, unf.t, "solver_step_noise, Philox form against the supplied draw")
    assert bool(fused.t.isfinite().all())
    _no_diff(fused.t[pair], det.t[pair], "the element at the saturated uniform is the deterministic step")
    assert not torch.equal(fused.t, det.t) and all(o.intact() for o in (fused, unf, det))
    print(f"[measured] saturated radius uniform (sample {sample} quad {quad} draw {draw} word {word}) inside sched_step_philox and solver_step_noise: finite, "
          f"equal to the deterministic part; fused = unfused, 0 elements differ")


# ------------------------------------------------------------------------------------------------ g. absdiff_mean_c
@pytest.mark.parametrize("shape", [SC.CAP_ABSDIFF, (3, 1, 257), (2, 3, 255), (1, 5, 1)], ids=["cap", "C1", "odd_cells", "one_cell"])
def test_absdiff_mean_c(dev, shape):
    """against the fp32 chain in channel order on the CPU: s = s + |a - b| for c = 0 .. C - 1, then (1 / C) * s"""
    N, Cc, cells = shape
    a, b = SC.rand(f"abs.a.{shape}", shape), SC.rand(f"abs.b.{shape}", shape, 0.7)
    s = torch.zeros((N, cells))
    for c in range(Cc):
        s = s + (a[:, c] - b[:, c]).abs()
    want = (torch.tensor(1.0) / torch.tensor(float(Cc))) * s
    out = Out(N * cells, dev)
    ad, bd = a.to(dev), b.to(dev)
    L.check(L.load().mf_absdiff_mean_c_f32(ad.data_ptr(), bd.data_ptr(), out.t.data_ptr(), N, Cc, cells, K.stream()), "mf_absdiff_mean_c_f32")
    _no_diff(out.t, want, shape)
    assert out.intact()
    _no_diff(K.absdiff_mean_c(ad, bd), want, (shape, "the wrapper"))
    blocks, trips = SC.launch(N * cells, SC.WIDE_CAP)
    print(f"[measured] absdiff_mean_c {shape} ({blocks} workgroups, {trips} trips): 0 elements differ from the fp32 chain")


# ------------------------------------------------------------------------------------------------ h. what the entries refuse
class Refusals:
    """a valid call, then one rule broken at a time: the code and the message, nothing written, the counter words unchanged, the valid call unchanged"""

    def __init__(self, outs, words, valid):
        self.outs, self.words, self.valid = outs, words, valid
        self.words0 = [w.clone() for w in words]
        self.first = self._run_valid()
        self.count = 0

    def _run_valid(self):
        for o in self.outs:
            o.reset()
        for w, w0 in zip(self.words, self.words0):
            w.copy_(w0)
        rc = self.valid()
        assert rc == 0, (rc, L.last_error())
        assert all(o.intact() for o in self.outs)
        res = [o.t.clone() for o in self.outs]
        for w, w0 in zip(self.words, self.words0):
            w.copy_(w0)
        return res

    def refused(self, rule, call):
        line, text, code, fragment = SC.REFUSALS[rule]
        for o in self.outs:
            o.reset()
        rc = call()
        msg = L.last_error()
        assert rc == code and fragment in msg, (rule, rc, msg)
        assert all(o.virgin() for o in self.outs), (rule, "an output was written")
        assert all(torch.equal(w, w0) for w, w0 in zip(self.words, self.words0)), (rule, [w.tolist() for w in self.words])
        self.count += 1

    def done(self, what):
        again = self._run_valid()
        for a, b in zip(again, self.first):
            _no_diff(a, b, (what, "the valid call after the refusals"))
        print(f"[measured] {what}: {self.count} broken rules refused with their code and message, nothing written, the valid call unchanged")


def _small(dev, tables, n=64):
    host = SC.step_inputs(n, "h")
    d = {k: v.to(dev) for k, v in host.items()}
    d["pv"] = SC.uniform("h.pv", n, 1.0).to(dev)
    return d


def _small_blend(dev, tables, B, Cc, cells):
    z0, eps0 = SC.rand("h.z0", (B, Cc, cells)).to(dev), SC.rand("h.eps0", (B, Cc, cells)).to(dev)
    mask = (SC.rand("h.mask", (B, 1, cells)) > 0).to(torch.uint8).to(dev)
    make = lambda z=z0, e=eps0, m=mask, cells_=cells, ch=Cc: L.MfSchedBlend(_p(z), _p(e), _p(m), tables["coef"].data_ptr(), cells_, ch, 0)
    return make, (z0, eps0, mask)


def _sched_step_setup(dev, tables):
    lib, n = L.load(), 64
    d = _small(dev, tables)
    outs = [Out(n, dev) for _ in range(3)]
    args = lambda **kw: _sched_args(d["x_t"], d["pred"], kw.get("pu"), kw.get("pv"), d["npost"], d["nddim"], outs[0].t, outs[1].t, outs[2].t, tables["step"], 2,
                                    kw.get("objective", 0), 1, SC.G, n=kw.get("n"))
    return lib, d, outs, args


def test_refusals_sched_step(dev, tables):
    lib, d, outs, args = _sched_step_setup(dev, tables)
    call = lambda a: lib.mf_sched_step_f32(C.byref(a), K.stream())
    r = Refusals(outs, [], lambda: call(args(pu=d["pu"])))
    r.refused("sched_step.objective", lambda: call(args(objective=2)))
    r.refused("sched_step.objective", lambda: call(args(objective=-1)))
    r.refused("sched_step.var_with_pair", lambda: call(args(pu=d["pu"], pv=d["pv"])))
    r.done("mf_sched_step_f32")


def test_refusals_sched_step_blend(dev, tables):
    lib, d, outs, args = _sched_step_setup(dev, tables)
    make, keep = _small_blend(dev, tables, 2, 4, 8)
    callb = lambda a, bl: lib.mf_sched_step_blend_f32(C.byref(a), None if bl is None else C.byref(bl), K.stream())
    r = Refusals(outs, [], lambda: callb(args(pu=d["pu"]), make()))
    r.refused("blend.state", lambda: callb(args(), None))
    r.refused("blend.state", lambda: callb(args(), make(z=None)))
    r.refused("blend.state", lambda: callb(args(), make(cells_=0)))
    r.refused("blend.samples", lambda: callb(args(), make(cells_=7)))
    r.refused("sched_step.var_with_pair", lambda: callb(args(pu=d["pu"], pv=d["pv"]), make()))
    r.done("mf_sched_step_blend_f32")


def _philox_setup(dev, tables):
    lib, n, B = L.load(), 64, 2
    d = _small(dev, tables)
    outs = [Out(n, dev) for _ in range(3)]
    counter = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    off_x = offset_view(d["x_t"], True)

    def args(**kw):
        return _sched_args(kw.get("x_t", d["x_t"]), d["pred"], kw.get("pu"), kw.get("pv"), kw.get("npost"), kw.get("nddim"), kw.get("out", outs[0].t), outs[1].t, outs[2].t,
                           tables["step"], 0, kw.get("objective", 0), 1, SC.G, n=kw.get("n"))

    return lib, n, B, d, outs, counter, off_x, args


def test_refusals_sched_step_philox(dev, tables):
    lib, n, B, d, outs, counter, off_x, args = _philox_setup(dev, tables)
    call = lambda a, B_=B: lib.mf_sched_step_philox_f32(C.byref(a), SC.SEED, 3, 2, 0, B_, counter.data_ptr(), counter.data_ptr() + 4, K.stream())
    r = Refusals(outs, [counter], lambda: call(args(pu=d["pu"])))
    r.refused("philox.objective", lambda: call(args(objective=2)))
    r.refused("philox.var_with_pair", lambda: call(args(pu=d["pu"], pv=d["pv"])))
    r.refused("philox.noise_pointers", lambda: call(args(npost=d["npost"])))
    r.refused("philox.noise_pointers", lambda: call(args(nddim=d["nddim"])))
    r.refused("philox.quads", lambda: call(args(), 3))                 # 64 elements are not 3 samples of whole quads
    r.refused("philox.quads", lambda: call(args(n=62)))
    r.refused("philox.aligned", lambda: call(args(x_t=off_x)))
    off_out = Out(n, dev, offset=True)
    r.refused("philox.aligned", lambda: call(args(out=off_out.t)))
    assert off_out.virgin()
    r.done("mf_sched_step_philox_f32")


def test_refusals_sched_step_philox_blend(dev, tables):
    lib, n, B, d, outs, counter, off_x, args = _philox_setup(dev, tables)
    make, (z0, eps0, mask) = _small_blend(dev, tables, B, 4, 8)
    callb = lambda a, bl, B_=B: lib.mf_sched_step_philox_blend_f32(C.byref(a), SC.SEED, 3, 2, 0, B_, counter.data_ptr(), counter.data_ptr() + 4,
                                                                  None if bl is None else C.byref(bl), K.stream())
    r = Refusals(outs, [counter], lambda: callb(args(pu=d["pu"]), make()))
    r.refused("blend.state", lambda: callb(args(), None))
    r.refused("blend.state", lambda: callb(args(), make(cells_=0)))
    r.refused("blend.samples", lambda: callb(args(), make(cells_=7)))
    r.refused("philox_blend.cells", lambda: callb(args(n=48), make(cells_=6)))        # 48 = 2 x 4 x 6: whole samples, whole quads per sample, cells % 4 != 0
    r.refused("philox_blend.n", lambda: callb(args(), make(), 1))                     # 64 = 2 samples of 4 x 8, B = 1 given
    r.refused("philox_blend.z0", lambda: callb(args(), make(z=offset_view(z0, True))))
    r.refused("philox_blend.z0", lambda: callb(args(), make(e=offset_view(eps0, True))))
    r.refused("philox.noise_pointers", lambda: callb(args(npost=d["npost"]), make()))
    r.done("mf_sched_step_philox_blend_f32")


def _solver_setup(dev, tables):
    lib, n = L.load(), 64
    rows, table = tables["dpmpp2m"]
    d = _small(dev, tables)
    outs = [Out(n, dev) for _ in range(3)]
    counter = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    # one buffer of 4 n floats: the history is its middle half, [n, 3 n)
    big = torch.empty(4 * n, device=dev)
    hist = big[n: 3 * n]

    def fill():
        big.fill_(SENT)
        hist.view(2, n)[1] = d["prev"]

    d["prev"] = SC.rand("h.prev", (n,)).to(dev)

    def args(**kw):
        a = _solver_args(kw.get("x_t", d["x_t"]), kw.get("pred", d["pred"]), d["pu"], kw.get("out", outs[0].t), kw.get("x0", outs[1].t), kw.get("xT", outs[2].t),
                         kw.get("hist", hist), table, kw.get("objective", 0), 1, SC.G, step=kw.get("step", 2), counter=kw.get("counter"), n=n)
        if "ticket" in kw:
            a.ticket = kw["ticket"]
        return a

    return lib, n, d, outs, counter, big, hist, fill, args


def test_refusals_solver_step(dev, tables):
    """one buffer of 4 n floats whose middle half is the history: every other tensor of the launch is laid inside it, one element short of clearing
    it on either side (refused), and exactly clear of it (p + n == h0, p == h1: accepted, same bits)"""
    lib, n, d, outs, counter, big, hist, fill, args = _solver_setup(dev, tables)
    call = lambda a: lib.mf_solver_step_f32(C.byref(a), K.stream())

    def valid():
        fill()
        return call(args())

    r = Refusals(outs, [counter], valid)
    h_first = hist.clone()

    def refused(rule, make_args):
        fill()
        r.refused(rule, lambda: call(make_args()))
        assert torch.equal(hist.view(2, n)[1], d["prev"]) and bool((hist.view(2, n)[0] == SENT).all()) and bool((big[:n] == SENT).all()) and bool((big[3 * n:] == SENT).all()), rule

    refused("solver.objective", lambda: args(objective=2))
    refused("solver.counter_ticket", lambda: args(counter=counter, ticket=None))
    refused("solver.counter_ticket", lambda: args(ticket=counter.data_ptr() + 4))
    refused("solver.step", lambda: args(step=-1))
    # the history against each other tensor: inside it, one element short of clearing it below, one element short above
    for role in ("x_t", "pred", "out", "x0", "xT"):
        for lo in (n, 2 * n, 1, 3 * n - 1):
            refused("solver.hist_overlap", lambda: args(**{role: big[lo: lo + n]}))
    r.done("mf_solver_step_f32")
    assert torch.equal(hist, h_first)
    # the boundary: a tensor that ends where the history begins (p + n == h0), or begins where it ends, is accepted -- same bits as the valid call
    for role, k in (("out", 0), ("x0", 1), ("xT", 2)):
        for lo in (0, 3 * n):
            fill()
            rc = call(args(**{role: big[lo: lo + n]}))
            assert rc == 0, (role, lo, L.last_error())
            _no_diff(big[lo: lo + n], r.first[k], (role, lo, "the boundary case"))
            other = big[3 * n:] if lo == 0 else big[:n]
            assert bool((other == SENT).all()) and torch.equal(hist, h_first)
    for role in ("x_t", "pred"):
        for lo in (0, 3 * n):
            fill()
            big[lo: lo + n] = d[role]
            assert call(args(**{role: big[lo: lo + n]})) == 0, (role, lo, L.last_error())
            _no_diff(outs[0].t, r.first[0], (role, lo, "the boundary case"))
    print("[measured] mf_solver_step_f32: tensors that touch the history's ends (p + n == h0, p == h1) accepted, same bits")


def test_refusals_solver_step_blend(dev, tables):
    lib, n, d, outs, counter, big, hist, fill, args = _solver_setup(dev, tables)
    make, keep = _small_blend(dev, tables, 2, 4, 8)
    callb = lambda a, bl: lib.mf_solver_step_blend_f32(C.byref(a), None if bl is None else C.byref(bl), K.stream())

    def valid_b():
        fill()
        return callb(args(), make())

    r = Refusals(outs, [counter], valid_b)
    for rule, bl in (("solver_blend.state", None), ("solver_blend.state", make(m=None)), ("solver_blend.state", make(cells_=0)), ("solver_blend.samples", make(cells_=7))):
        fill()
        r.refused(rule, lambda: callb(args(), bl))
        assert bool((hist.view(2, n)[0] == SENT).all())
    r.done("mf_solver_step_blend_f32")


def test_refusals_solver_step_noise(dev, tables):
    lib, n, B = L.load(), 64, 2
    rows, table, scale, lts = tables["sde"]
    d = _small(dev, tables)
    outs = [Out(n, dev) for _ in range(3)]
    counter = torch.tensor([0, 0], dtype=torch.int32, device=dev)          # a first-order row: it needs no history
    assert rows[0].mode == L.SOLVER_ORDER1
    args = lambda **kw: _solver_args(kw.get("x_t", d["x_t"]), d["pred"], d["pu"], outs[0].t, outs[1].t, outs[2].t, None, table, kw.get("objective", 0), 1, SC.G,
                                     counter=counter, n=kw.get("n"))
    call = lambda a, nz, bl=None: lib.mf_solver_step_noise_f32(C.byref(a), C.byref(nz), None if bl is None else C.byref(bl), K.stream())
    r = Refusals(outs, [counter], lambda: call(args(), _philox(scale, SC.SEED, 3, 2, 0, B)))
    r.refused("noise.scale", lambda: call(args(), _philox(None, SC.SEED, 3, 2, 0, B)))
    r.refused("noise.scale", lambda: call(args(), _supplied(None, d["npost"])))
    r.refused("noise.samples", lambda: call(args(), _philox(scale, SC.SEED, 3, 2, 0, 3)))
    r.refused("noise.samples", lambda: call(args(), _philox(scale, SC.SEED, 3, 2, 0, 0)))
    r.refused("noise.stride", lambda: call(args(), _supplied(scale, d["npost"], -4)))
    r.refused("solver.objective", lambda: call(args(objective=2), _supplied(scale, d["npost"])))
    r.done("mf_solver_step_noise_f32")


def test_refusals_philox_normal(dev):
    lib = L.load()
    out = Out(64, dev)
    off = Out(64, dev, offset=True)
    call = lambda o, per, B=4: lib.mf_philox_normal_f32(o.data_ptr(), SC.SEED, 3, 0, None, 0, 0, B, per, K.stream())
    r = Refusals([out, off], [], lambda: call(out.t, 16))
    r.refused("normal.per_sample", lambda: call(out.t, 6))
    r.refused("normal.per_sample", lambda: call(out.t, 15))
    r.refused("normal.aligned", lambda: call(off.t, 16))
    r.done("mf_philox_normal_f32")
