"""Image-quality metrics of VOLUMES on the device: SSIM, MS-SSIM and MSE of volume pairs, the pairwise MS-SSIM of a set and the reconstruction
meter of a 3-D latent embedder (csrc/metrics3d.hip, include/medfusion_hip.h MfSsim3dDesc).

The definition is the 2-D one (metrics.py, README "Metrics") with one more axis, and it is ours (README "Metrics, volumes"): a k-tap Gaussian
window g (x) g (x) g (the same g: normalised in fp64, rounded to fp32), VALID windows only -- (D - k + 1)(H - k + 1)(W - k + 1) per channel --, the
same cs and ssim per window, sim_s / cs_s the means over all channels and positions of a pair at scale s; the next scale is the mean of
2 x 2 x 2 blocks (an odd trailing plane, row or column dropped: F.avg_pool3d(x, 2, 2)); the same product over the scales.  It is NOT the 2-D metric
slice by slice: that has no window and no pooling along depth.

Every function returns device tensors and never synchronises.  Inputs are fp32 [B, C, D, H, W] tensors on the GPU; anything else is a ValueError
that names the argument.  The size rule min(D, H, W) // 2^(S - 1) >= k leaves the 2-D defaults (5 scales of 11 taps: sides >= 176) to very few
volumes, so betas_for(S) gives the weights of a shorter pyramid: the published 64 x 128 x 128 volume takes betas_for(3) at k = 11."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import kernels as K
from . import lib as L
from .metrics import BETAS, _check_lpips_net, _check_ms, _check_range, _check_window, _combine, _summary, gaussian_taps, plan_pairs

# the partial sums of one launch: P C tiles 24 bytes, a tile being 16 x 16 x 16 window origins (mf_ssim3d_workspace_bytes).  A pair of 1 x 64 x 128 x 128
# volumes is 256 tiles = 6 KiB at scale 0 (an image pair of the 2-D metric: 64 tiles of 32 x 32 at 256 x 256), a pair of 1 x 256^3 4096 tiles =
# 96 KiB: the pairs per launch of pairwise_ms_ssim3d are as many as keep the workspace within this bound, at least one, at most 65535
WORKSPACE_BOUND = 64 << 20


def betas_for(scales: int):
    """the first `scales` of the five published weights, divided by their sum: the weights of a pyramid of 1 .. 5 levels"""
    if isinstance(scales, bool) or not isinstance(scales, int) or not 1 <= scales <= len(BETAS):
        raise ValueError(f"scales: 1 .. {len(BETAS)}, got {scales!r}")
    total = sum(BETAS[:scales])
    return tuple(b / total for b in BETAS[:scales])


def min_side3d(scales: int = len(BETAS), kernel_size: int = 11) -> int:
    """the smallest side MS-SSIM of volumes takes: min(D, H, W) // 2^(S - 1) >= k  (176 for the 2-D defaults; 44 for betas_for(3))"""
    return kernel_size << (scales - 1)


def max_scales3d(side: int, kernel_size: int = 11) -> int:
    """the largest number of scales a volume whose smallest side is `side` admits at this kernel_size (0: not even one)"""
    s = 0
    while side // (1 << s) >= kernel_size:
        s += 1
    return s


def _pair_chunk(C_: int, D: int, H: int, W: int, kernel_size: int) -> int:
    """pairs per launch that keep the scale-0 partial sums within WORKSPACE_BOUND (the library says what one pair takes; host-only)"""
    one = K.make_ssim3d_desc(1, C_, D, H, W, 1, 1, [0.0] * kernel_size, 0.01, 0.03, 1.0)
    per_pair = L.load().mf_ssim3d_workspace_bytes(C.byref(one))
    if per_pair == 0:
        raise ValueError(f"x: a volume of {C_} x {D} x {H} x {W} is refused: {L.last_error()}")
    return max(1, min(65535, WORKSPACE_BOUND // per_pair))


def _check_volumes(scales: int, kernel_size: int, **named) -> None:
    """the rules of the inputs in the order of metrics._check_images: rank, dtype, one shape, size rule -- all on the host -- and only then the device"""
    first = None
    for name, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: a tensor, got {type(t).__name__}")
        if t.dim() == 4:
            raise ValueError(f"{name}: volumes only ([B, C, D, H, W]); for a 4-D batch of images of shape {tuple(t.shape)} use the 2-D function "
                             f"(medfusion_amd.ssim / ms_ssim / mse / pairwise_ms_ssim)")
        if t.dim() != 5 or t.shape[0] == 0 or t.shape[1] == 0:
            raise ValueError(f"{name}: a non-empty [B, C, D, H, W] tensor, got shape {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: fp32, got {t.dtype}")
        if first is None:
            first = (name, t)
        elif t.shape != first[1].shape:
            raise ValueError(f"{name}: of the shape of {first[0]} {tuple(first[1].shape)}, got {tuple(t.shape)}")
    name, t = first
    side = min(t.shape[2:])
    if side // (1 << (scales - 1)) < kernel_size:
        most = max_scales3d(side, kernel_size)
        admits = f"at most {most} scale(s) (betas=betas_for({most}))" if most else "not even one scale"
        raise ValueError(f"{name}: {scales} scale(s) of a {kernel_size}-tap window need sides of at least {min_side3d(scales, kernel_size)}, "
                         f"got {t.shape[2]} x {t.shape[3]} x {t.shape[4]}, which admits {admits} at kernel_size={kernel_size}")
    for name, t in named.items():
        if not t.is_cuda:
            raise ValueError(f"{name}: on a ROCm device -- the metrics have no CPU path, got a {t.device.type} tensor")
        if t.device != first[1].device:
            raise ValueError(f"{name}: on the device of {first[0]}")


def pyramid3d(x: torch.Tensor, scales: int):
    """[x, pool(x), pool(pool(x)), ...]: the `scales` levels of a bank of volumes, built once per bank"""
    levels = [x.contiguous()]
    for _ in range(scales - 1):
        levels.append(K.avgpool2_volumes(levels[-1]))
    return levels


def pair_range3d(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """L of data_range=None for the pairs (x[b], y[b]): max(max x - min x, max y - min y) over the whole volume, as the kernel forms it"""
    _check_volumes(1, 3, x=x, y=y)
    mx, my = K.rows_minmax(x), K.rows_minmax(y)
    return torch.maximum(mx[:, 1] - mx[:, 0], my[:, 1] - my[:, 0])


def _terms3d(xpyr, ypyr, ix, iy, P: int, minmax, data_range, taps, k1: float, k2: float, want_mse: bool):
    """-> sim [P, S], cs [P, S], mse [P] or None: one launch pair per scale over all P pairs of the two pyramids"""
    S = len(xpyr)
    dev = xpyr[0].device
    sim, cs = torch.empty((P, S), dtype=torch.float32, device=dev), torch.empty((P, S), dtype=torch.float32, device=dev)
    mse = torch.empty((P,), dtype=torch.float32, device=dev) if want_mse else None
    indexed = (1 if ix is not None else 0) | (2 if iy is not None else 0)
    for s in range(S):
        xs, ys = xpyr[s], ypyr[s]
        d = K.make_ssim3d_desc(P, xs.shape[1], xs.shape[2], xs.shape[3], xs.shape[4], xs.shape[0], ys.shape[0], taps, k1, k2, data_range, indexed,
                               want_mse and s == 0)
        K.ssim3d_pairs(xs, ys, d, sim[:, s], cs[:, s], mse if s == 0 else None, ix, iy, *(minmax if data_range is None else (None, None)))
    return sim, cs, mse


def ssim3d(x: torch.Tensor, y: torch.Tensor, *, data_range: Optional[float] = 1.0, kernel_size: int = 11, sigma: float = 1.5, k1: float = 0.01,
           k2: float = 0.03) -> torch.Tensor:
    """single-scale SSIM of the volumes (x[b], y[b]) -> [B]"""
    _check_window(kernel_size, sigma)
    _check_range(data_range)
    _check_volumes(1, kernel_size, x=x, y=y)
    x, y = x.contiguous(), y.contiguous()
    minmax = (K.rows_minmax(x), K.rows_minmax(y)) if data_range is None else None
    sim, _, _ = _terms3d([x], [y], None, None, x.shape[0], minmax, data_range, gaussian_taps(kernel_size, sigma), k1, k2, False)
    return sim[:, 0]


def ms_ssim3d(x: torch.Tensor, y: torch.Tensor, *, data_range: Optional[float] = 1.0, betas: Sequence[float] = BETAS, normalize: Optional[str] = "relu",
              return_terms: bool = False, kernel_size: int = 11, sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03):
    """MS-SSIM of the volumes (x[b], y[b]) -> [B]; return_terms: also the [B, S] terms before normalisation (cs_0 .. cs_{S-2}, sim_{S-1}).
    The default betas are the five of the 2-D metric (sides >= 176): pass betas=betas_for(S) for a shorter pyramid."""
    _check_window(kernel_size, sigma)
    _check_range(data_range)
    betas = _check_ms(betas, normalize)
    _check_volumes(len(betas), kernel_size, x=x, y=y)
    x, y = x.contiguous(), y.contiguous()
    minmax = (K.rows_minmax(x), K.rows_minmax(y)) if data_range is None else None
    sim, cs, _ = _terms3d(pyramid3d(x, len(betas)), pyramid3d(y, len(betas)), None, None, x.shape[0], minmax, data_range,
                          gaussian_taps(kernel_size, sigma), k1, k2, False)
    value, terms = _combine(sim, cs, betas, normalize)
    return (value, terms) if return_terms else value


def mse3d(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The mean of (x[b] - y[b])^2 over C D H W -> [B], summed by the SSIM kernel's staging pass: in fp32 over the four voxels a thread stages per
    plane, in fp64 from there on.  The launch is that of an 11-tap SSIM (of the largest odd window that fits, for sides under 11; at least 3), so
    the bits are those of the MSE that comes with ms_ssim3d_and_mse at the default window; a bare call pays for that launch and drops its sim / cs."""
    _check_volumes(1, 3, x=x, y=y)
    x, y = x.contiguous(), y.contiguous()
    k = min(L.SSIM_MAX_K, (min(x.shape[2:]) - 1) // 2 * 2 + 1)
    return _terms3d([x], [y], None, None, x.shape[0], None, 1.0, gaussian_taps(k, 1.5), 0.01, 0.03, True)[2]


def ms_ssim3d_and_mse(x: torch.Tensor, y: torch.Tensor, *, data_range: Optional[float] = 1.0, betas: Sequence[float] = BETAS,
                      normalize: Optional[str] = "relu", kernel_size: int = 11, sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03):
    """(ms_ssim3d(x, y), mse3d(x, y)) from one pass over scale 0 -- at kernel_size=11 the same bits as the two calls"""
    _check_window(kernel_size, sigma)
    _check_range(data_range)
    betas = _check_ms(betas, normalize)
    _check_volumes(len(betas), kernel_size, x=x, y=y)
    x, y = x.contiguous(), y.contiguous()
    minmax = (K.rows_minmax(x), K.rows_minmax(y)) if data_range is None else None
    sim, cs, err = _terms3d(pyramid3d(x, len(betas)), pyramid3d(y, len(betas)), None, None, x.shape[0], minmax, data_range,
                            gaussian_taps(kernel_size, sigma), k1, k2, True)
    return _combine(sim, cs, betas, normalize)[0], err


def pairwise_ms_ssim3d(x: torch.Tensor, pairs=None, *, seed: int = 0, data_range: Optional[float] = 1.0, betas: Sequence[float] = BETAS,
                       normalize: Optional[str] = "relu", kernel_size: int = 11, sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03,
                       chunk: Optional[int] = None):
    """MS-SSIM between volumes of ONE set -> (values [P], index [P, 2]); `pairs` as in metrics.plan_pairs.  One pyramid per volume, the pairs in
    chunks of `chunk` per launch; nothing is gathered.  chunk=None: as many pairs as keep the partial sums of scale 0 within WORKSPACE_BOUND
    (64 MiB: 10,922 pairs of 1 x 64 x 128 x 128 at k = 11, 682 pairs of 1 x 256^3), at least 1, at most 65535.  The values do not depend on it."""
    _check_window(kernel_size, sigma)
    _check_range(data_range)
    betas = _check_ms(betas, normalize)
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or not 1 <= chunk <= 65535):
        raise ValueError(f"chunk: None or 1 .. 65535 pairs per launch, got {chunk!r}")
    _check_volumes(len(betas), kernel_size, x=x)
    if chunk is None:
        chunk = _pair_chunk(*x.shape[1:], kernel_size)
    index = plan_pairs(int(x.shape[0]), pairs, seed)
    pyr = pyramid3d(x.contiguous(), len(betas))
    mm = K.rows_minmax(pyr[0]) if data_range is None else None
    dev_index = index.to(torch.int32).to(x.device)
    taps, values = gaussian_taps(kernel_size, sigma), []
    for lo in range(0, index.shape[0], chunk):
        part = dev_index[lo:lo + chunk]
        ix, iy = part[:, 0].contiguous(), part[:, 1].contiguous()
        sim, cs, _ = _terms3d(pyr, pyr, ix, iy, part.shape[0], (mm, mm), data_range, taps, k1, k2, False)
        values.append(_combine(sim, cs, betas, normalize)[0])
    return (values[0] if len(values) == 1 else torch.cat(values)), dev_index.to(torch.int64)


class VolumeReconstructionMeter:
    """MS-SSIM and MSE of a 3-D embedder's reconstructions, accumulated on the device: the protocol of metrics.ReconstructionMeter.  update(x)
    takes x [B, C, D, H, W] in [-1, 1], runs embedder(x)[0].clamp(-1, 1), maps both to [0, 1] and keeps the per-volume MS-SSIM (data_range=None:
    the range of each pair) and MSE, both from one pass; compute() is the only host sync: the mean and torch.std of each over all volumes seen.
    `noise`: the NoiseSource handed to the embedder; None leaves the embedder its default, exactly as a bare embedder(x) -- the meter draws nothing.
    The default pyramid is betas_for(3) at 11 taps (sides >= 44): what the published 64 x 128 x 128 volume admits.
    `lpips`: an LPIPSNet; update() then also keeps LPIPS of (x, reconstruction) -- per slice, the mean over depth -- and compute() adds "lpips_mean",
    "lpips_std" and "lpips_score" = 1 - mean.  None: exactly the figures above."""

    def __init__(self, embedder, noise=None, *, betas: Sequence[float] = betas_for(3), kernel_size: int = 11, sigma: float = 1.5, lpips=None):
        _check_window(kernel_size, sigma)
        self.embedder, self.noise, self.lpips = embedder, noise, _check_lpips_net(lpips)
        self.betas, self.kernel_size, self.sigma = _check_ms(betas, "relu"), kernel_size, sigma
        self.reset()

    def reset(self) -> None:
        self._ms, self._mse, self._lp = [], [], []

    @torch.no_grad()
    def update(self, x: torch.Tensor) -> None:
        _check_volumes(len(self.betas), self.kernel_size, x=x)
        pred = (self.embedder(x) if self.noise is None else self.embedder(x, noise=self.noise))[0].clamp(-1, 1)
        a, b = (x + 1) / 2, (pred + 1) / 2
        v, e = ms_ssim3d_and_mse(a, b, data_range=None, betas=self.betas, kernel_size=self.kernel_size, sigma=self.sigma)
        self._ms.append(v)
        self._mse.append(e)
        if self.lpips is not None:
            from .lpips import lpips
            self._lp.append(lpips(x, pred, self.lpips))

    def values(self):
        """the per-volume MS-SSIM and MSE so far, as two device tensors"""
        if not self._ms:
            raise ValueError("VolumeReconstructionMeter: no update() yet")
        return torch.cat(self._ms), torch.cat(self._mse)

    def lpips_values(self) -> torch.Tensor:
        """the per-volume LPIPS so far, as a device tensor (a meter built with lpips=net)"""
        if not self._lp:
            raise ValueError("VolumeReconstructionMeter: no update() with an LPIPS net yet")
        return torch.cat(self._lp)

    def compute(self) -> dict:
        ms, err = self.values()
        return _summary(ms, err, self.lpips_values() if self.lpips is not None else None)
