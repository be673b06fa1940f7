"""Shared by tests/test_metrics_cpu.py and tests/test_metrics_gpu.py: the plain-torch restatement of the metric's definition (README "Metrics";
F.conv2d on the full 2-D window, F.avg_pool2d) -- the ORACLE when run in fp64 on the CPU, the YARDSTICK when run in fp32 -- the seeded input
generators, and the comparison rule: the kernel's distance from fp64 is at most MARGIN x the fp32 restatement's own distance (d32), which is
computed at run time for every case and never written down."""
import math
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

from oracle import synth as S

BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MARGIN = 4.0          # the kernel filters separably and sums in another order than conv2d, and d32 is ONE sample of rounding noise
# `flat` (x = 0.7 + 1e-3 noise, y = x + 1e-3 noise) has a second, absolute bound, because there d32 can be useless: with data_range=None c2 is 1.3e-7
# and the fp32 restatement is off by more than 1.  The kernel takes second moments about a pixel p of the tile: E'[u^2] = var + (mean - p)^2, at
# most var + (5 sigma)^2 = 26 var.  2 k = 22 fused steps and three more roundings leave at most 25 * 2^-24 = 1.5e-6 of that on each of s_x^2
# (var 1e-6), s_y^2 (var 2e-6) and s_xy: 1.5e-6 * 26 * 2e-6 = 7.8e-11.  cs = (2 s_xy + c2) / (s_x^2 + s_y^2 + c2) has a denominator of at least
# s_x^2 + s_y^2 = 3e-6, so its error in the WORST window is (2 + 2) * 7.8e-11 / 3e-6 = 1e-4, the per-scale means are at most that, and a larger c2
# (data_range=1) only shrinks it.  ms_ssim, a product of powers whose exponents sum to 1, moves by at most that over its smallest term, relatively.
FLAT_CAP = 1e-4
MIN_TERM = 0.1        # a relative comparison of ms_ssim first asserts every fp64 term >= this: a clamp cannot hide a wrong kernel

# (P, C, H, W) of the single-scale kernel tests: one window; a tile edge on neither axis; tile edges on both axes on the element-wise path;
# the 16-byte path over several tiles
KERNEL_SHAPES = {"one_window": (1, 1, 11, 11), "small": (2, 3, 12, 45), "edges_scalar": (1, 2, 43, 75), "vec4": (2, 1, 64, 96)}
WINDOWS = {"k11": (11, 1.5), "k7": (7, 1.0)}
# (B, C, H, W) of the MS-SSIM tests: the last scale is ONE window; odd extents at three scales (183 -> 91 -> 45 -> 22 -> 11, 201 -> 100 -> 50 -> 25 -> 12)
MS_SHAPES = {"min176": (3, 2, 176, 176), "odd183x201": (2, 1, 183, 201)}


def taps(k=11, sigma=1.5):
    """normalised in fp64, rounded to fp32"""
    r = (k - 1) / 2.0
    g = np.exp(-((np.arange(k, dtype=np.float64) - r) ** 2) / (2.0 * sigma ** 2))
    return torch.from_numpy((g / g.sum()).astype(np.float32))


def ref_scale(x, y, k, sigma, L, k1=0.01, k2=0.03):
    """one scale, in the dtype of x: (sim [B], cs [B]); L: a number or a [B] tensor"""
    g = taps(k, sigma).to(x)
    C = x.shape[1]
    w = torch.outer(g, g)[None, None].expand(C, 1, k, k).contiguous()
    f = lambda t: F.conv2d(t, w, groups=C)
    mux, muy, exx, eyy, exy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    vx, vy, vxy = exx - mux * mux, eyy - muy * muy, exy - mux * muy
    L = torch.as_tensor(L).to(x).reshape(-1, 1, 1, 1)
    c1, c2 = (k1 * L) ** 2, (k2 * L) ** 2
    cs = (2 * vxy + c2) / (vx + vy + c2)
    ssim = (2 * mux * muy + c1) / (mux * mux + muy * muy + c1) * cs
    return ssim.flatten(1).mean(1), cs.flatten(1).mean(1)


def ref_terms(x, y, dtype, data_range=1.0, k=11, sigma=1.5, scales=5, k1=0.01, k2=0.03, device="cpu"):
    """-> dict(sim [B, S], cs [B, S], mse [B], L [B]) in `dtype` on the CPU (the tests; scripts/metrics_bench.py times it on the GPU)"""
    x, y = x.to(device, dtype), y.to(device, dtype)
    if data_range is None:
        L = torch.maximum(x.flatten(1).amax(1) - x.flatten(1).amin(1), y.flatten(1).amax(1) - y.flatten(1).amin(1))
    else:
        L = torch.full((x.shape[0],), data_range, dtype=dtype, device=x.device)
    mse = ((x - y) ** 2).flatten(1).mean(1)
    sims, css = [], []
    for s in range(scales):
        sim, cs = ref_scale(x, y, k, sigma, L, k1, k2)
        sims.append(sim)
        css.append(cs)
        if s + 1 < scales:
            x, y = F.avg_pool2d(x, 2, 2), F.avg_pool2d(y, 2, 2)          # floor: an odd trailing row / column is dropped
    return dict(sim=torch.stack(sims, 1), cs=torch.stack(css, 1), mse=mse, L=L)


def ms_terms(t):
    """the S terms before normalisation: cs_0 .. cs_{S-2}, sim_{S-1}"""
    return torch.cat([t["cs"][:, :-1], t["sim"][:, -1:]], dim=1)


def ref_ms_ssim(t, betas=BETAS, normalize="relu"):
    terms = ms_terms(t)
    n = torch.relu(terms) if normalize == "relu" else terms
    return torch.prod(n ** torch.tensor(betas, dtype=terms.dtype, device=terms.device), dim=1)


def term_distance(a, b):
    """the largest absolute distance over every per-scale sim_s, cs_s and the mse (a, b: ref_terms dicts or the same keys from the kernel)"""
    return max(float((a[key].double().cpu() - b[key].double().cpu()).abs().max()) for key in ("sim", "cs", "mse") if key in a and key in b)


def rel_distance(a, b):
    return float(((a.double().cpu() - b.double().cpu()).abs() / b.double().cpu().abs()).max())


# ------------------------------------------------------------------------------------------------ inputs
def _normal(name_seed: int, draw: int, shape):
    per = int(np.prod(shape[1:]))
    padded = (per + 3) // 4 * 4                                            # the generator draws four values at a time
    z = S.philox_normal(name_seed, draw, np.arange(shape[0]), padded).reshape(shape[0], padded)[:, :per]
    return torch.from_numpy(np.ascontiguousarray(z).reshape(shape).astype(np.float32))


def _smooth(B, H, W, shared: bool):
    """0.5 + 0.3 sin cos: one field for the whole batch (shared) or one per image (frequencies and phases move with b)"""
    i = torch.arange(H, dtype=torch.float64)[None, :, None] / H
    j = torch.arange(W, dtype=torch.float64)[None, None, :] / W
    b = torch.zeros(B, 1, 1, dtype=torch.float64) if shared else torch.arange(B, dtype=torch.float64)[:, None, None]
    f = 0.5 + 0.3 * torch.sin(2 * math.pi * ((1.5 + b) * i + 0.13 + 0.37 * b)) * torch.cos(2 * math.pi * ((2.5 + 0.5 * b) * j + 0.29 * b))
    return f.to(torch.float32)[:, None]                                    # [B, 1, H, W]


def _texture(seed, draw, shape):
    return 0.15 * F.avg_pool2d(_normal(seed, draw, shape), 3, 1, 1)      # 3 x 3 box


@lru_cache(maxsize=None)
def make_inputs(kind: str, shape, seed: int = 0):
    """-> (x, y) fp32 CPU tensors in [0, 1] of `shape` = (B, C, H, W); cached and shared: do not write to them"""
    B, C, H, W = shape
    if kind == "recon":
        x = (_smooth(B, H, W, False) + _texture(1000 + seed, 0, shape)).clamp(0, 1)
        y = (x + 0.03 * _normal(1000 + seed, 1, shape)).clamp(0, 1)
    elif kind == "flat":
        x = 0.7 + 1e-3 * _normal(2000 + seed, 0, shape)
        y = x + 1e-3 * _normal(2000 + seed, 1, shape)
    elif kind == "unrelated":
        x = (_smooth(B, H, W, False) + _texture(3000 + seed, 0, shape)).clamp(0, 1)
        y = x.roll(1, 0)
    else:
        raise ValueError(kind)
    return x.contiguous(), y.contiguous()


@lru_cache(maxsize=None)
def make_bank(shape, seed: int = 0):
    """N images over ONE smooth field, an independent texture each"""
    N, C, H, W = shape
    return (_smooth(N, H, W, True) + _texture(4000 + seed, 0, shape)).clamp(0, 1).contiguous()


@lru_cache(maxsize=None)
def references(kind: str, shape, data_range, k=11, sigma=1.5, scales=5, seed: int = 0):
    """(fp64 terms, fp32 terms) of a case, computed once and shared"""
    x, y = make_inputs(kind, shape, seed)
    kw = dict(data_range=data_range, k=k, sigma=sigma, scales=scales)
    return ref_terms(x, y, torch.float64, **kw), ref_terms(x, y, torch.float32, **kw)


def all_pairs(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]
