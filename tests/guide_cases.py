"""The guidance stage (mf_guide_f32: guidance schedule, guidance rescale, dynamic thresholding) without a device: the seeded cases of
tests/test_guide_gpu.py, the stage restated in fp64 in plain torch on the CPU (`restate`), the same stage as the chain of fp32 torch operators each
rounded on its own (`chain32`, with the EXACT order statistics of its x_0 estimate), and the bounds derived from the number formats."""
from __future__ import annotations

import math

import numpy as np
import torch

ONE_WG = 8192            # MF_GUIDE_ROW_ONE_WG (tests/test_guide_cpu.py holds the header and medfusion_amd.lib to it)
U = 2.0 ** -24           # unit roundoff of fp32


def f32(v: float) -> float:
    """a Python float as the table's fp32 field holds it"""
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------ the fp64 restatement
def restate(pc, pu, xt, g, phi, q, s_max, a, b, objective):
    """One row in fp64 on the fp32 inputs: torch.std, torch.quantile, clamp -- the papers' formulas.  pc / pu / xt: fp32 1-D tensors (pu None: no
    pair); g, phi, q, s_max, a, b: the table row's fp32 values as Python floats (phi None / 0: no rescale; q None: no threshold; s_max None: no
    cap).  The two standard deviations are those of the fp32 VALUES the stage holds, as its definition says -- pc, and p32 = fl(pu + fl(g fl(pc -
    pu))) -- taken in fp64: where a row's spread is a few fp32 spacings of its mean, the standard deviation of the rounded values is another number
    than that of the unrounded ones, and k is defined on the former.  Everything else is fp64 throughout.
    -> dict of fp64 tensors / floats: p (combined), p32 (the fp32 combine), k, pk (rescaled), x0, s, x0n, out."""
    pc64 = pc.double()
    p = pc64 if pu is None else pu.double() + g * (pc64 - pu.double())
    p32 = pc if pu is None else pu + torch.tensor(g, dtype=torch.float32) * (pc - pu)
    n = p.numel()
    k = 1.0
    if phi:
        s_cfg = float(torch.std(p32.double())) if n > 1 else 0.0
        if n > 1 and s_cfg != 0.0:
            # phi * (p * sigma_pos / sigma_cfg) + (1 - phi) * p = k p
            k = phi * float(torch.std(pc64)) / s_cfg + (1.0 - phi)
    pk = k * p
    r = dict(p=p, p32=p32, k=k, pk=pk, x0=None, s=None, x0n=None, out=pk)
    if q is None:
        return r
    x0 = a * xt.double() - b * pk if objective == 0 else pk
    s = float(torch.quantile(x0.abs(), q, interpolation="linear"))
    s = max(s, 1.0)
    if s_max is not None:
        s = min(s, s_max)
    x0n = x0.clamp(-s, s) / s
    out = (a * xt.double() - x0n) / b if objective == 0 else x0n
    r.update(x0=x0, s=s, x0n=x0n, out=out)
    return r


# ------------------------------------------------------------------------------------------------ the fp32 chain
def order_statistic_limit(x0: torch.Tensor, q: float, s_max):
    """the limit of include/medfusion_hip.h from an fp32 x_0 row: EXACT order statistics of |x0| (torch.sort; no NaN in the row), the fp64
    interpolation at pos = q (n - 1), rounded to fp32 once, then max(., 1) and the cap -> (fp32 0-dim tensor, lo, hi)"""
    v = torch.sort(x0.abs()).values
    n = v.numel()
    pos = q * (n - 1)
    lo, hi = int(math.floor(pos)), int(math.ceil(pos))
    vlo, vhi = float(v[lo]), float(v[hi])
    sd = vlo if hi == lo else vlo + (vhi - vlo) * (pos - lo)
    s = torch.tensor(sd, dtype=torch.float64).to(torch.float32)
    s = torch.maximum(s, torch.tensor(1.0))
    if s_max is not None:
        s = torch.minimum(s, torch.tensor(s_max, dtype=torch.float32))
    return s, lo, hi


def chain32(pc, pu, xt, g, k, q, s_max, a, b, objective):
    """The stage as fp32 torch operators on the CPU, each rounded on its own (ATen's elementwise chain): the combine, fl(k p) with the GIVEN fp32 k
    (the kernel's scale_out, or 1), the x_0 estimate, the exact limit, the clamp, the division, the way back.  -> (out, s or None, x0 or None)"""
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    p = pc if pu is None else pu + t(g) * (pc - pu)
    if k is not None:
        p = t(k) * p
    if q is None:
        return p, None, None
    x0 = t(a) * xt - t(b) * p if objective == 0 else p
    s, _, _ = order_statistic_limit(x0, q, s_max)
    x0n = x0.clamp(-float(s), float(s)) / s
    out = (t(a) * xt - x0n) / t(b) if objective == 0 else x0n
    return out, s, x0


# ------------------------------------------------------------------------------------------------ bounds
def ulp32(v: float) -> float:
    return float(np.spacing(np.float32(abs(v))))


def scale_bound(k: float) -> float:
    """|scale_out - k| <= one fp32 ulp of k: the kernel evaluates k in fp64 from fp64 sums about a pivot (relative error ~ n 2^-53, far below
    2^-24) and rounds once, so it lands on one of the two fp32 neighbours of the restatement's k"""
    return ulp32(k)


def element_bound(r, pc, pu, xt, g, a, b, objective, rescale, threshold):
    """|pred_out - restate()['out']| per element, from the fp32 roundings of the chain (u = 2^-24, first order, times 1 + 2^-10 for the rest):
      combine   three roundings, every intermediate at most M = |pu| + max(1, |g|) |pc - pu|:        E_p  = 3 u M                  (0 without a pair)
      rescale   k within one ulp (2 u |k|) of the restatement's, one product:                        E_pk = |k| E_p + 3 u |k p|
      x_0       two products, one difference ('x_T'; nothing for 'x_0'):                             E_x0 = 2 u (|a x_t| + |b pk|) + |b| E_pk
      limit     an order statistic and a convex combination of two are 1-Lipschitz in the max norm,
                one rounding to fp32, max(., 1) and the cap are 1-Lipschitz:                         E_s  = max_row E_x0 + u s
      clamp / s clamp is 1-Lipschitz in x and in s, |x0'| <= 1, one division:                        E_n  = (E_x0 + 2 E_s) / s + u
      way back  one product, one difference, one division ('x_T'):                                   E    = (2 u |a x_t| + u + E_n) / |b| + u |out|
    -> fp64 tensor"""
    pc64 = pc.double()
    if pu is None:
        e_p = torch.zeros_like(pc64)
    else:
        e_p = 3 * U * (pu.double().abs() + max(1.0, abs(g)) * (pc64 - pu.double()).abs())
    k = abs(r["k"])
    e_pk = k * e_p + 3 * U * (k * r["p"].abs()) if rescale else e_p
    if not threshold:
        return e_pk * (1 + 2.0 ** -10) + 1e-300
    if objective == 0:
        axt = (a * xt.double()).abs()
        e_x0 = 2 * U * (axt + (b * r["pk"]).abs()) + abs(b) * e_pk
    else:
        axt = None
        e_x0 = e_pk
    e_s = float(e_x0.max()) + U * r["s"]
    e_n = (e_x0 + 2 * e_s) / r["s"] + U
    if objective == 0:
        e = (2 * U * axt + U + e_n) / abs(b) + U * r["out"].abs()
    else:
        e = e_n
    return e * (1 + 2.0 ** -10) + 1e-300


# ------------------------------------------------------------------------------------------------ the seeded cases
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def contents(kind: str, n: int, seed: int, q=None):
    """-> (pc, pu or None, xt): fp32 [n] rows of one content kind"""
    g = _gen(seed)
    rnd = lambda s=1.0: torch.randn(n, generator=g) * s
    if kind == "normal":
        return rnd(1.3), rnd(1.3), rnd(1.1)
    if kind == "ties3":        # three distinct magnitudes, the quantile position between the first and the second
        pos = q * (n - 1)
        lo = int(math.floor(pos))
        mags = torch.full((n,), 3.5)
        mags[: lo + 1] = 1.5
        if lo + 1 < n:
            mags[lo + 1: lo + 1 + max(1, (n - lo - 1) // 2)] = 2.5
        sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        return (mags * sign)[torch.randperm(n, generator=g)], None, rnd()
    if kind == "all_equal":    # sigma_cfg = 0
        c = torch.full((n,), 0.75)
        return c, c.clone(), rnd()
    if kind == "low_byte":     # magnitudes that differ only in their lowest byte
        low = torch.randint(0, 256, (n,), generator=g, dtype=torch.int32)
        mags = (low + 0x40000000).view(torch.float32)
        sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        return mags * sign, None, rnd()
    if kind == "zeros_denormals":   # +-0, denormals, a few ordinary values
        pick = torch.randint(0, 4, (n,), generator=g)
        den = torch.randint(1, 1 << 20, (n,), generator=g, dtype=torch.int32).view(torch.float32)
        v = torch.where(pick == 0, torch.zeros(n), torch.where(pick == 1, -torch.zeros(n), torch.where(pick == 2, den, -den)))
        v = v.clone()
        v[torch.randint(0, n, (max(1, n // 16),), generator=g)] = 2.75
        return v, None, rnd()
    if kind == "offset":       # a large common offset: mean 64, spread 1e-3 (the variance pivot)
        return 64.0 + rnd(1e-3), 64.0 + rnd(1e-3), rnd()
    raise KeyError(kind)


SHAPES = [(4, 1), (4, 3), (36, 2), (33, 2), (ONE_WG, 2), (ONE_WG + 4, 2), (2 * ONE_WG + 12, 2), (2 * ONE_WG + 13, 1)]   # (n, B)
# n = 36 and 33 are read at a 4-byte offset (the element-wise path); n = 33 and 2 ONE_WG + 13: q (n - 1) is an integer for q = 0.5 and 0.25
SCHED = dict(a=f32(1.0206207), b=f32(0.2041241))          # sqrt_recip_ac, sqrt_recipm1_ac of a mid-range timestep (ac = 0.96)


def all_cases():
    """-> list of dicts: name, n, B, kind, objective, pair, g, phi (0: off), q (None: off), s_max, offset (elements the tensors are shifted by)"""
    out = []

    def add(n, B, kind, objective, g, phi, q, s_max=None):
        name = f"n{n}-B{B}-{kind}-{'xT' if objective == 0 else 'x0'}-g{g}-phi{phi}-q{q}" + (f"-cap{s_max}" if s_max else "")
        out.append(dict(name=name, n=n, B=B, kind=kind, objective=objective, g=f32(g), phi=f32(phi), q=None if q is None else f32(q),
                        s_max=None if s_max is None else f32(s_max), offset=1 if n in (36, 33) else 0, **SCHED))

    for n, B in SHAPES:
        integer_q = [0.25] if (n - 1) % 4 == 0 else []
        for q in [0.5, 0.995, 1.0] + integer_q:
            add(n, B, "normal", 0, 8.0, 0.7, q)
        add(n, B, "normal", 1, 3.0, 1.0, 0.995, 2.5)
        add(n, B, "normal", 0, 8.0, 0.7, None)
        add(n, B, "normal", 1, 1.5, 0.0, 0.5)
        for q in [0.5] + integer_q:
            add(n, B, "ties3", 1, 1.0, 0.0, q)
        add(n, B, "all_equal", 1, 4.0, 0.7, 0.5)
        add(n, B, "low_byte", 1, 1.0, 0.0, 0.5)
        add(n, B, "low_byte", 1, 1.0, 0.0, 0.995)
        add(n, B, "zeros_denormals", 1, 1.0, 0.0, 0.5)
        add(n, B, "zeros_denormals", 1, 1.0, 0.0, 1.0)
        add(n, B, "offset", 0, 1.5, 0.7, None)
        add(n, B, "offset", 1, 1.5, 1.0, 0.5)
    return out


def case_rows(case):
    """the B rows of a case -> list of (pc, pu or None, xt)"""
    return [contents(case["kind"], case["n"], 1000 * case["n"] + 17 * b + len(case["kind"]), case["q"]) for b in range(case["B"])]


# ------------------------------------------------------------------------------------------------ the pipeline-level fixtures
# fixture name -> the case in tests/solver_cases.py's form (pipe_args / SIZE apply), the sampler, and the three options.  scripts/gen_guide_golden.py
# runs each through the reference's own estimator and scheduler calls with the stage restated in plain torch; tests/test_guide_pipeline_gpu.py holds
# the product to the result at the project's path tolerance.
PIPE_CASES = {
    "guide_default_g8_phi07": dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3), steps=6, n=2, seed=81, condition=[2, 0], guidance_scale=8.0, sampler=None,
                                   spacing=None, opts=dict(guidance_rescale=0.7)),
    "guide_dpmpp2m_logsnr_q995": dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3), steps=8, n=2, seed=82, condition=[1, 2], guidance_scale=4.0,
                                      sampler="dpmpp2m", spacing="logsnr", opts=dict(dynamic_threshold=0.995)),
    "guide_x0obj_all": dict(dims=2, pipe=dict(tag="guide_tiny_x0", ncls=3, objective="x_0", clip_x0=True), steps=7, n=2, seed=83, condition=[0, 2],
                            guidance_scale=5.0, sampler="ddim0", spacing=None,
                            opts=dict(guidance_rescale=0.5, dynamic_threshold=0.9, threshold_max=3.0, guidance_schedule=("interval", 100, 900))),
    "guide_3d": dict(dims=3, pipe=dict(tag="solver_ddim0_3d", ncls=2), steps=6, n=2, seed=84, condition=[1, 0], guidance_scale=4.0, sampler="ddim0",
                     spacing=None, opts=dict(guidance_rescale=0.7, dynamic_threshold=0.995)),
}


def stage_torch(x, pc, pu, t, sch, g, phi, q, s_max, objective):
    """The stage as a user of the reference would write it from the papers, batched, in the dtype of its inputs: torch.std, torch.quantile, clamp,
    and `sch`'s own estimate_x_0 / estimate_x_T (the reference's scheduler, or the restatement's).  -> the prediction handed to the step"""
    dims = tuple(range(1, pc.dim()))
    p = pu + g * (pc - pu)
    if phi:
        rescaled = p * (pc.std(dim=dims, keepdim=True) / p.std(dim=dims, keepdim=True))
        p = phi * rescaled + (1 - phi) * p
    if q is None:
        return p
    x0 = sch.estimate_x_0(x, p, t, clip_x0=False) if objective == "x_T" else p
    s = torch.quantile(x0.abs().flatten(1), q, dim=1).clamp(min=1.0, max=s_max)
    s = s.reshape(-1, *([1] * (x0.dim() - 1)))
    x0 = torch.maximum(torch.minimum(x0, s), -s) / s
    return sch.estimate_x_T(x, x_0=x0, t=t, clip_x0=False) if objective == "x_T" else x0
