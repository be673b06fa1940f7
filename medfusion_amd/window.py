"""The window plan of windowed denoising (MultiDiffusion, Bar-Tal et al. 2023): a canvas larger than the size the estimator was trained at is
covered by overlapping windows of the trained size; every iteration the estimator runs on the windows, the per-cell predictions are averaged with
fixed weights and the scheduler / solver step runs once on the whole canvas (DiffusionPipeline._predict).  Pure host code: nothing here touches
the device.

Per axis of canvas length L, window h and stride s the origins are o_k = min(k s, L - h) for k = 0 .. ceil((L - h) / s), duplicates dropped: the
last window is clamped to the edge, so the coverage is total without padding and the last overlap may be larger than the others.  Windows are
ordered row-major over the axes, the last axis fastest.  The weight of a window at a cell is the product over the axes of a profile at the cell's
offset i inside the window: "uniform" 1 (MultiDiffusion's plain average), "tent" min(i + 1, h - i) (strictly positive small integers, exact in
fp32, softer seams).
"""
from __future__ import annotations

import itertools

MF_WINDOW_MAX_PER_AXIS = 32
WEIGHTS = ("uniform", "tent")


def _axis_origins(L: int, h: int, s: int):
    last = -(-(L - h) // s)
    out = []
    for k in range(last + 1):
        o = min(k * s, L - h)
        if not out or o != out[-1]:
            out.append(o)
    return out


class WindowPlan:
    """WindowPlan(canvas, window, stride=None, weight="tent", dims=None): canvas / window / stride in latent cells, 2 or 3 axes (a stride may be one
    int for all axes; default h // 2 per axis, at least 1).  dims: the model's spatial dims, checked against the number of axes when given.
    .origins (per axis), .M, .windows (the origin tuple of every window, in order), .cover (nested lists: the number of windows over each cell),
    .none (canvas == window on every axis: one window, the caller takes the un-windowed path)."""

    def __init__(self, canvas, window, stride=None, weight="tent", dims=None):
        try:
            canvas, window = tuple(int(v) for v in canvas), tuple(int(v) for v in window)
        except TypeError:
            raise ValueError(f"window={window!r} on canvas {canvas!r}: one extent per spatial axis") from None
        n = len(canvas)
        if n not in (2, 3) or len(window) != n or (dims is not None and n != int(dims)):
            raise ValueError(f"window={window} on a canvas {canvas}: windowed sampling takes one extent per spatial axis"
                             + (f" of the model ({dims})" if dims is not None else " (2 or 3)"))
        if stride is None:
            stride = tuple(max(1, h // 2) for h in window)
        elif isinstance(stride, int):
            stride = (stride,) * n
        else:
            stride = tuple(int(v) for v in stride)
        if len(stride) != n:
            raise ValueError(f"window_stride={stride}: one stride per spatial axis ({n})")
        if weight not in WEIGHTS:
            raise ValueError(f"window_weight={weight!r}: one of {WEIGHTS}")
        for L, h, s in zip(canvas, window, stride):
            if h < 1 or L < h:
                raise ValueError(f"window={window} does not fit the canvas {canvas}: every window extent must be 1 .. the canvas extent")
            if not 1 <= s <= h:
                raise ValueError(f"window_stride={stride} for window={window}: a stride is 1 .. the window extent (a larger one would leave gaps)")
        self.canvas, self.window, self.stride, self.weight = canvas, window, stride, weight
        self.origins = tuple(tuple(_axis_origins(L, h, s)) for L, h, s in zip(canvas, window, stride))
        for a, o in enumerate(self.origins):
            if len(o) > MF_WINDOW_MAX_PER_AXIS:
                raise ValueError(f"window={window} with window_stride={stride} on canvas {canvas}: {len(o)} windows on axis {a}, at most "
                                 f"MF_WINDOW_MAX_PER_AXIS = {MF_WINDOW_MAX_PER_AXIS}")
        self.windows = tuple(itertools.product(*self.origins))
        self.M = len(self.windows)
        self.none = canvas == window

    @property
    def dims(self) -> int:
        return len(self.canvas)

    def profile(self, axis: int):
        """the per-axis weight profile, a list of ints"""
        h = self.window[axis]
        return [1] * h if self.weight == "uniform" else [min(i + 1, h - i) for i in range(h)]

    @property
    def cover(self):
        """the number of covering windows per canvas cell (nested lists of the canvas shape)"""
        per_axis = [[sum(1 for o in org if o <= p < o + h) for p in range(L)] for org, L, h in zip(self.origins, self.canvas, self.window)]

        def scaled(t, c):
            return [scaled(u, c) for u in t] if isinstance(t, list) else t * c

        def outer(axes):   # the separable product of the per-axis counts
            if len(axes) == 1:
                return list(axes[0])
            rest = outer(axes[1:])
            return [scaled(rest, c) for c in axes[0]]

        return outer(per_axis)

    def desc(self, B: int, C: int):
        """the MfWindowDesc of a launch over B canvas rows of C channels"""
        from . import lib as L

        d = L.MfWindowDesc()
        d.dims = self.dims
        pad = 3 - self.dims
        for a in range(3):
            if a < pad:
                d.canvas[a], d.window[a], d.count[a] = 1, 1, 1
                d.origin[a][0] = 0
            else:
                org = self.origins[a - pad]
                d.canvas[a], d.window[a], d.count[a] = self.canvas[a - pad], self.window[a - pad], len(org)
                for k, o in enumerate(org):
                    d.origin[a][k] = o
        d.weight = L.WINDOW_TENT if self.weight == "tent" else L.WINDOW_UNIFORM
        d.B, d.C, d.reserved = int(B), int(C), 0
        return d

    def describe(self) -> str:
        return (f"canvas {self.canvas}, window {self.window}, stride {self.stride}, weight {self.weight}: M = {self.M} windows, origins per axis "
                f"{[list(o) for o in self.origins]}")
