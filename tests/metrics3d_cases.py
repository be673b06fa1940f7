"""Shared by tests/test_metrics3d_cpu.py and tests/test_metrics3d_gpu.py: the plain-torch restatement of the VOLUME metric's definition (README
"Metrics, volumes"; F.conv3d on the full k^3 window, groups = C; F.avg_pool3d) -- the ORACLE when run in fp64 on the CPU, the YARDSTICK when run in
fp32 -- the seeded input generators (the 2-D ones of tests/metrics_cases.py lifted to three axes), and the project's comparison rule: the kernel's
distance from fp64 is at most MARGIN x the fp32 restatement's own distance (d32), computed at run time for every case and never written down."""
import math
from functools import lru_cache

import torch
import torch.nn.functional as F

from tests.metrics_cases import BETAS, MARGIN, MIN_TERM, _normal, all_pairs, ms_terms, ref_ms_ssim, rel_distance, taps, term_distance  # noqa: F401

# `flat` (x = 0.7 + 1e-3 noise, y = x + 1e-3 noise) has a second, absolute bound, because there d32 is useless: with data_range=None c2 is of the
# order of 1e-7 and the fp32 restatement is off by 0.5 .. 2.  The bound is derived as metrics_cases.FLAT_CAP is, with one more filter pass: the
# kernel takes second moments about a voxel p of the workgroup, E'[u^2] = var + (mean - p)^2, at most var + (5 sigma)^2 = 26 var = 26 * 2e-6.
# 3 k = 33 fused steps and three more roundings leave at most 36 * 2^-24 = 2.1e-6 of that on each of s_x^2, s_y^2 and s_xy: 2.1e-6 * 26 * 2e-6 =
# 1.1e-10.  cs = (2 s_xy + c2) / (s_x^2 + s_y^2 + c2) has a denominator of at least s_x^2 + s_y^2 = 3e-6, so its error in the WORST window is
# (2 + 2) * 1.1e-10 / 3e-6 = 1.5e-4; the per-scale means are at most that, and a larger c2 (data_range=1) only shrinks it.
FLAT_CAP_3D = 1.5e-4

# The kernel's tile is 16 x 16 window origins in-plane and 16 origins in depth (csrc/metrics3d.hip TILE, DCHUNK): within the 32 / 16 these shapes
# were chosen for, so every axis of the edge cases has at least two tiles and a partial last one.
TILE, DCHUNK = 16, 16
# the squares one thread adds in fp32 before its sum goes to fp64: the four voxels it stages per plane (csrc/metrics3d.hip: one group of four per
# thread and plane, flushed to fp64 after every plane)
MSE_FP32_SQUARES = 4

# (P, C, D, H, W) of the single-scale kernel tests
KERNEL_SHAPES = {"one_window": (1, 1, 11, 11, 11), "small": (2, 3, 12, 13, 45), "edges_scalar": (1, 2, 24, 43, 75), "deep": (1, 1, 40, 23, 40),
                 "vec4": (2, 1, 28, 32, 64)}
WINDOWS = {"k11": (11, 1.5), "k7": (7, 1.0), "k3": (3, 0.5)}
# every shape at every window that fits (`deep` at k7 and k3 has several depth chunks with a partial last one: 34 and 38 origins)
KERNEL_CASES = [(name, win) for name in KERNEL_SHAPES for win in WINDOWS if min(KERNEL_SHAPES[name][2:]) >= WINDOWS[win][0]]
# name -> ((B, C, D, H, W), k, sigma, S) of the MS-SSIM tests, with betas_for(S)
MS_CASES = {"one_window_last": ((3, 2, 20, 20, 20), 5, 1.0, 3), "odd": ((2, 1, 23, 27, 45), 5, 1.0, 3), "k11s2": ((1, 1, 22, 22, 24), 11, 1.5, 2),
            "k7s3": ((2, 1, 28, 30, 37), 7, 1.0, 3)}


def betas_for(scales):
    total = sum(BETAS[:scales])
    return tuple(b / total for b in BETAS[:scales])


def ref_scale3d(x, y, k, sigma, L, k1=0.01, k2=0.03):
    """one scale, in the dtype of x: (sim [B], cs [B]); L: a number or a [B] tensor"""
    g = taps(k, sigma).to(x)
    C = x.shape[1]
    w = (g[:, None, None] * g[None, :, None] * g[None, None, :])[None, None].expand(C, 1, k, k, k).contiguous()
    f = lambda t: F.conv3d(t, w, groups=C)
    mux, muy, exx, eyy, exy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    vx, vy, vxy = exx - mux * mux, eyy - muy * muy, exy - mux * muy
    L = torch.as_tensor(L).to(x).reshape(-1, 1, 1, 1, 1)
    c1, c2 = (k1 * L) ** 2, (k2 * L) ** 2
    cs = (2 * vxy + c2) / (vx + vy + c2)
    ssim = (2 * mux * muy + c1) / (mux * mux + muy * muy + c1) * cs
    return ssim.flatten(1).mean(1), cs.flatten(1).mean(1)


def ref_terms3d(x, y, dtype, data_range=1.0, k=11, sigma=1.5, scales=1, k1=0.01, k2=0.03, device="cpu"):
    """-> dict(sim [B, S], cs [B, S], mse [B], L [B]) in `dtype` on the CPU (the tests; scripts/metrics3d_bench.py times it on the GPU)"""
    x, y = x.to(device, dtype), y.to(device, dtype)
    if data_range is None:
        L = torch.maximum(x.flatten(1).amax(1) - x.flatten(1).amin(1), y.flatten(1).amax(1) - y.flatten(1).amin(1))
    else:
        L = torch.full((x.shape[0],), data_range, dtype=dtype, device=x.device)
    mse = ((x - y) ** 2).flatten(1).mean(1)
    sims, css = [], []
    for s in range(scales):
        sim, cs = ref_scale3d(x, y, k, sigma, L, k1, k2)
        sims.append(sim)
        css.append(cs)
        if s + 1 < scales:
            x, y = F.avg_pool3d(x, 2, 2), F.avg_pool3d(y, 2, 2)          # floor: an odd trailing plane / row / column is dropped
    return dict(sim=torch.stack(sims, 1), cs=torch.stack(css, 1), mse=mse, L=L)


def ref_ms_ssim3d(t, normalize="relu"):
    return ref_ms_ssim(t, betas_for(t["sim"].shape[1]), normalize)


# ------------------------------------------------------------------------------------------------ inputs
def _smooth3d(B, D, H, W, shared: bool):
    """0.5 + 0.3 sin cos cos: one field for the whole batch (shared) or one per volume; i, j, k the normalised H, W, D coordinates"""
    i = torch.arange(H, dtype=torch.float64)[None, None, :, None] / H
    j = torch.arange(W, dtype=torch.float64)[None, None, None, :] / W
    k = torch.arange(D, dtype=torch.float64)[None, :, None, None] / D
    b = torch.zeros(B, 1, 1, 1, dtype=torch.float64) if shared else torch.arange(B, dtype=torch.float64)[:, None, None, None]
    f = 0.5 + 0.3 * torch.sin(2 * math.pi * ((1.5 + b) * i + 0.13 + 0.37 * b)) * torch.cos(2 * math.pi * ((2.5 + 0.5 * b) * j + 0.29 * b)) \
        * torch.cos(2 * math.pi * ((1 + 0.5 * b) * k + 0.11 + 0.23 * b))
    return f.to(torch.float32)[:, None]                                    # [B, 1, D, H, W]


def _texture3d(seed, draw, shape):
    return 0.15 * F.avg_pool3d(_normal(seed, draw, shape), 3, 1, 1)      # 3 x 3 x 3 box


@lru_cache(maxsize=None)
def make_inputs(kind: str, shape, seed: int = 0):
    """-> (x, y) fp32 CPU tensors in [0, 1] of `shape` = (B, C, D, H, W); cached and shared: do not write to them"""
    B, C, D, H, W = shape
    if kind == "recon":
        x = (_smooth3d(B, D, H, W, False) + _texture3d(1000 + seed, 0, shape)).clamp(0, 1)
        y = (x + 0.03 * _normal(1000 + seed, 1, shape)).clamp(0, 1)
    elif kind == "flat":
        x = 0.7 + 1e-3 * _normal(2000 + seed, 0, shape)
        y = x + 1e-3 * _normal(2000 + seed, 1, shape)
    elif kind == "inverted":
        x = make_inputs("recon", shape, seed)[0]
        y = 1 - x
    else:
        raise ValueError(kind)
    return x.contiguous(), y.contiguous()


@lru_cache(maxsize=None)
def make_bank(shape, seed: int = 0):
    """N volumes over ONE smooth field, an independent texture each"""
    N, C, D, H, W = shape
    return (_smooth3d(N, D, H, W, True) + _texture3d(4000 + seed, 0, shape)).clamp(0, 1).contiguous()


@lru_cache(maxsize=None)
def references(kind: str, shape, data_range, k=11, sigma=1.5, scales=1, seed: int = 0):
    """(fp64 terms, fp32 terms) of a case, computed once and shared"""
    x, y = make_inputs(kind, shape, seed)
    kw = dict(data_range=data_range, k=k, sigma=sigma, scales=scales)
    return ref_terms3d(x, y, torch.float64, **kw), ref_terms3d(x, y, torch.float32, **kw)
