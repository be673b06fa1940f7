"""The windowed-denoising cases (window= / window_stride= / window_weight=) shared by scripts/gen_window_golden.py and the tests: the window plan
restated in plain Python (`RefPlan`, independent of medfusion_amd.window), `ref_merge`, the plain-torch weighted merge in a chosen dtype,
`windowed`, the wrapper that makes any estimator's forward() run per window, the geometries with their expected counts, the kernel-level shapes
and the table of the tests/golden/md_* fixtures."""
from __future__ import annotations

import itertools
import math

import torch

from tests.solver_cases import pipe_args  # noqa: F401  (re-exported: one import for the users of the cases)

MAX_PER_AXIS = 32

# canvas, window, stride -> M, the set of cover counts, the origins per axis
GEOMETRIES = {
    "overlap2d": dict(canvas=(12, 12), window=(8, 8), stride=4, M=4, cover={1, 2, 4}, origins=((0, 4), (0, 4))),
    "clamped2d": dict(canvas=(8, 13), window=(8, 8), stride=4, M=3, cover={1, 2, 3}, origins=((0,), (0, 4, 5))),     # the irregular last window
    "overlap3d": dict(canvas=(6, 12, 12), window=(4, 8, 8), stride=(2, 4, 4), M=8, cover={1, 2, 4, 8}, origins=((0, 2), (0, 4), (0, 4))),
    "tiling2d": dict(canvas=(8, 12), window=(4, 6), stride=(4, 6), M=4, cover={1}, origins=((0, 4), (0, 6))),         # stride == window: no overlap
}

# kernel-level shapes: B, C, canvas, window, stride, and the stride-equals-window twin (canvas, window) of the same path
KERNEL_SHAPES = {
    "vector": dict(B=2, C=8, canvas=(12, 12), window=(8, 8), stride=4, tiling=((16, 24), (8, 8))),                  # 16-byte vectors
    "element": dict(B=3, C=5, canvas=(9, 13), window=(7, 6), stride=(3, 5), tiling=((14, 18), (7, 6))),             # odd everything, clamped last windows, cover up to 2 x 2
    "3d": dict(B=2, C=4, canvas=(6, 12, 12), window=(4, 8, 8), stride=(2, 4, 4), tiling=((8, 8, 16), (4, 8, 8))),
}

# fixture -> pipeline (tests/solver_cases.pipe_args), batch, canvas latent, window arguments, loop arguments, noise seed
PARITY_CASES = {
    "md_ddim_cfg_2d": dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3), n=2, size=(8, 12, 12), window=(8, 8), window_stride=4, window_weight="tent",
                           steps=5, sampler=None, condition=[2, 0], guidance_scale=4.0, decode=True, seed=101),
    "md_uniform_odd_2d": dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3), n=2, size=(8, 8, 13), window=(8, 8), window_stride=4, window_weight="uniform",
                              steps=8, sampler="dpmpp2m", decode=False, seed=102),
    "md_3d": dict(dims=3, pipe=dict(tag="solver_ddim0_3d", ncls=2), n=1, size=(4, 6, 12, 12), window=(4, 8, 8), window_stride=None, window_weight="tent",
                  steps=5, sampler="ddim0", condition=[1], guidance_scale=1.0, decode=False, seed=103),
}


def window_kwargs(case: dict) -> dict:
    return dict(window=case["window"], window_stride=case["window_stride"], window_weight=case["window_weight"])


def loop_kwargs(case: dict, device=None) -> dict:
    if "condition" not in case:
        return {}
    return dict(condition=torch.tensor(case["condition"], device=device), guidance_scale=case["guidance_scale"], un_cond=None)


class RefPlan:
    """The plan as DESIGN.md states it: per axis o_k = min(k s, L - h), k = 0 .. ceil((L - h) / s), duplicates dropped; windows row-major, last
    axis fastest; stride h // 2 (at least 1) by default; weights the separable product of 1 ("uniform") or min(i + 1, h - i) ("tent")."""

    def __init__(self, canvas, window, stride=None, weight="tent"):
        canvas, window = tuple(canvas), tuple(window)
        if stride is None:
            stride = tuple(max(1, h // 2) for h in window)
        elif isinstance(stride, int):
            stride = (stride,) * len(canvas)
        self.canvas, self.window, self.stride, self.weight = canvas, window, tuple(stride), weight
        self.origins = []
        for L, h, s in zip(canvas, window, self.stride):
            o = sorted({min(k * s, L - h) for k in range(math.ceil((L - h) / s) + 1)})
            self.origins.append(tuple(o))
        self.origins = tuple(self.origins)
        self.windows = tuple(itertools.product(*self.origins))
        self.M = len(self.windows)

    def weights(self, dtype=torch.float32) -> torch.Tensor:
        """the weight of a window at each of its cells, shape `window`"""
        w = torch.ones(self.window, dtype=dtype)
        for a, h in enumerate(self.window):
            prof = torch.tensor([1 if self.weight == "uniform" else min(i + 1, h - i) for i in range(h)], dtype=dtype)
            w = w * prof.reshape([-1 if b == a else 1 for b in range(len(self.window))])
        return w

    def cover(self) -> torch.Tensor:
        c = torch.zeros(self.canvas, dtype=torch.int64)
        for org in self.windows:
            c[tuple(slice(o, o + h) for o, h in zip(org, self.window))] += 1
        return c

    def slices(self, m: int):
        return tuple(slice(o, o + h) for o, h in zip(self.windows[m], self.window))


def ref_gather(canvas: torch.Tensor, plan: RefPlan) -> torch.Tensor:
    """[B, C, *canvas] -> [B * M, C, *window] by slicing: row b * M + m = window m of sample b"""
    return torch.stack([canvas[(b, slice(None), *plan.slices(m))] for b in range(canvas.shape[0]) for m in range(plan.M)])


def ref_merge(windows: torch.Tensor, plan: RefPlan, dtype=torch.float32) -> torch.Tensor:
    """[B * M, C, *window] -> [B, C, *canvas] in `dtype`: per cell sum_m w_m p_m / sum_m w_m over the covering windows in ascending m; a cell that
    one window covers takes that window's value as it is"""
    B, C = windows.shape[0] // plan.M, windows.shape[1]
    p = windows.to(dtype)
    w = plan.weights(dtype)
    acc = torch.zeros((B, C, *plan.canvas), dtype=dtype)
    only = torch.zeros_like(acc)
    den = torch.zeros(plan.canvas, dtype=dtype)
    for m in range(plan.M):
        sl = plan.slices(m)
        rows = p[m::plan.M]                          # window m of every sample
        acc[(slice(None), slice(None), *sl)] += w * rows
        only[(slice(None), slice(None), *sl)] = rows
        den[sl] += w
    return torch.where(plan.cover() == 1, only, acc / den)


def merge_bound(windows: torch.Tensor, plan: RefPlan) -> torch.Tensor:
    """[B, C, *canvas]: (K + 2) * 2^-24 * max|p| per cell, K the cell's cover count and max|p| the largest covering value.  The weights are
    normalised, so the K products' roundings sum to at most one half-ulp of max|p|, the K - 1 additions to at most one each (a partial sum is at
    most the total), the division adds one: K + 1, and one to spare.  Cover-1 cells are exact."""
    B, C = windows.shape[0] // plan.M, windows.shape[1]
    big = torch.zeros((B, C, *plan.canvas), dtype=torch.float64)
    for m in range(plan.M):
        idx = (slice(None), slice(None), *plan.slices(m))
        big[idx] = torch.maximum(big[idx], windows[m::plan.M].abs().double())
    return (plan.cover().double() + 2.0) * 2.0 ** -24 * big


def windowed(forward, plan: RefPlan, dtype=None):
    """an estimator forward(self, x_t, t, condition=None, self_cond=None) -> (pred, ...) that crops its canvas input into the plan's windows, calls
    the original on the B * M rows (t and the condition repeated per window) and merges the prediction back with ref_merge: what
    unittest.mock.patch.object(type(estimator), "forward", ...) installs around a reference estimator"""

    def wrapped(self, x_t, t=None, condition=None, self_cond=None):
        assert self_cond is None
        rep = lambda v: None if v is None else v.repeat_interleave(plan.M, dim=0)
        pred = forward(self, ref_gather(x_t, plan), rep(t), condition=rep(condition), self_cond=None)[0]
        return ref_merge(pred, plan, dtype or pred.dtype), []

    return wrapped
