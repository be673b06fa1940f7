"""Image-quality metrics on the device: SSIM, MS-SSIM and MSE of image pairs, the pairwise MS-SSIM of a set (the paper's diversity figure) and
the reconstruction meter of a latent embedder (csrc/metrics.hip, include/medfusion_hip.h MfSsimDesc).

The metric is defined HERE (README "Metrics"), not by a library: a k-tap Gaussian window g (x) g (g normalised in fp64, rounded to fp32), VALID
windows only, per window and channel cs = (2 s_xy + c2) / (s_x^2 + s_y^2 + c2) and ssim = (2 mu_x mu_y + c1) / (mu_x^2 + mu_y^2 + c1) * cs with
c1 = (k1 L)^2, c2 = (k2 L)^2; sim_s / cs_s are the means over all channels and positions of a pair at scale s; the next scale is a 2 x 2 mean (an
odd trailing row or column dropped); ms_ssim = prod_{s < S-1} n(cs_s)^beta_s * n(sim_{S-1})^beta_{S-1}, n = relu or the identity.

Every function returns device tensors and never synchronises.  Inputs are fp32 [B, C, H, W] tensors on the GPU; anything else is a ValueError
that names the argument.  One launch per scale covers all pairs; the pyramid of a bank is built once, whatever the number of pairs."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import kernels as K
from . import lib as L

BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
PAIR_CHUNK = 8192      # pairs per launch of pairwise_ms_ssim: bounds the partial-sum workspace (a 256 x 256 RGB pair: 4.6 KB at scale 0)


def gaussian_taps(kernel_size: int = 11, sigma: float = 1.5):
    """g[i] = exp(-(i - r)^2 / 2 sigma^2), r = (k - 1) / 2, normalised to sum 1 in fp64, then rounded to fp32 (returned as Python floats)"""
    r = (kernel_size - 1) / 2.0
    g = np.exp(-((np.arange(kernel_size, dtype=np.float64) - r) ** 2) / (2.0 * float(sigma) ** 2))
    return [float(v) for v in (g / g.sum()).astype(np.float32)]


def min_side(scales: int = len(BETAS), kernel_size: int = 11) -> int:
    """the smallest side MS-SSIM takes: min(H, W) // 2^(S - 1) >= k  (176 for the defaults)"""
    return kernel_size << (scales - 1)


def _check_window(kernel_size, sigma) -> None:
    if not isinstance(kernel_size, int) or kernel_size < 3 or kernel_size > L.SSIM_MAX_K or kernel_size % 2 == 0:
        raise ValueError(f"kernel_size: an odd integer in 3 .. {L.SSIM_MAX_K}, got {kernel_size!r}")
    if not (isinstance(sigma, (int, float)) and sigma > 0 and math.isfinite(sigma)):
        raise ValueError(f"sigma: a positive number, got {sigma!r}")


def _check_range(data_range) -> None:
    if data_range is not None and not (isinstance(data_range, (int, float)) and data_range > 0 and math.isfinite(data_range)):
        raise ValueError(f"data_range: a positive number or None, got {data_range!r}")


def _check_images(scales: int, kernel_size: int, **named) -> None:
    """the rules of the inputs in the order: rank, dtype, one shape, size rule -- all on the host -- and only then the device"""
    first = None
    for name, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: a tensor, got {type(t).__name__}")
        if t.dim() == 5:
            raise ValueError(f"{name}: 2-D images only ([B, C, H, W]); a 5-D volume of shape {tuple(t.shape)} is not built")
        if t.dim() != 4 or t.shape[0] == 0 or t.shape[1] == 0:
            raise ValueError(f"{name}: a non-empty [B, C, H, W] tensor, got shape {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: fp32, got {t.dtype}")
        if first is None:
            first = (name, t)
        elif t.shape != first[1].shape:
            raise ValueError(f"{name}: of the shape of {first[0]} {tuple(first[1].shape)}, got {tuple(t.shape)}")
    name, t = first
    if min(t.shape[2], t.shape[3]) // (1 << (scales - 1)) < kernel_size:
        raise ValueError(f"{name}: {scales} scale(s) of a {kernel_size}-tap window need sides of at least {min_side(scales, kernel_size)}, "
                         f"got {t.shape[2]} x {t.shape[3]}")
    for name, t in named.items():
        if not t.is_cuda:
            raise ValueError(f"{name}: on a ROCm device -- the metrics have no CPU path, got a {t.device.type} tensor")
        if t.device != first[1].device:
            raise ValueError(f"{name}: on the device of {first[0]}")


def pyramid(x: torch.Tensor, scales: int):
    """[x, pool(x), pool(pool(x)), ...]: the `scales` levels of a bank, built once per bank"""
    levels = [x.contiguous()]
    for _ in range(scales - 1):
        levels.append(K.avgpool2_planes(levels[-1]))
    return levels


def pair_range(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """L of data_range=None for the pairs (x[b], y[b]): max(max x - min x, max y - min y) from mf_rows_minmax_f32, as the SSIM kernel forms it"""
    _check_images(1, 3, x=x, y=y)
    mx, my = K.rows_minmax(x), K.rows_minmax(y)
    return torch.maximum(mx[:, 1] - mx[:, 0], my[:, 1] - my[:, 0])


def _terms(xpyr, ypyr, ix, iy, P: int, minmax, data_range, taps, k1: float, k2: float, want_mse: bool):
    """-> sim [P, S], cs [P, S], mse [P] or None: one launch pair per scale over all P pairs of the two pyramids"""
    S = len(xpyr)
    dev = xpyr[0].device
    sim, cs = torch.empty((P, S), dtype=torch.float32, device=dev), torch.empty((P, S), dtype=torch.float32, device=dev)
    mse = torch.empty((P,), dtype=torch.float32, device=dev) if want_mse else None
    indexed = (1 if ix is not None else 0) | (2 if iy is not None else 0)
    for s in range(S):
        xs, ys = xpyr[s], ypyr[s]
        d = K.make_ssim_desc(P, xs.shape[1], xs.shape[2], xs.shape[3], xs.shape[0], ys.shape[0], taps, k1, k2, data_range, indexed, want_mse and s == 0)
        K.ssim_pairs(xs, ys, d, sim[:, s], cs[:, s], mse if s == 0 else None, ix, iy, *(minmax if data_range is None else (None, None)))
    return sim, cs, mse


def _combine(sim: torch.Tensor, cs: torch.Tensor, betas, normalize):
    """the S terms before normalisation (cs_s for s < S - 1, sim_{S-1}) and their weighted product"""
    terms = torch.cat([cs[:, :-1], sim[:, -1:]], dim=1)
    n = torch.relu(terms) if normalize == "relu" else terms
    return torch.prod(n ** torch.tensor(betas, dtype=torch.float32, device=terms.device), dim=1), terms


def _check_ms(betas, normalize):
    betas = tuple(float(b) for b in betas)
    if len(betas) < 1 or not all(b > 0 and math.isfinite(b) for b in betas):
        raise ValueError(f"betas: positive weights, one per scale, got {betas!r}")
    if normalize not in ("relu", None):
        raise ValueError(f"normalize: 'relu' or None, got {normalize!r}")
    return betas


def ssim(x: torch.Tensor, y: torch.Tensor, *, data_range: Optional[float] = 1.0, kernel_size: int = 11, sigma: float = 1.5, k1: float = 0.01,
         k2: float = 0.03) -> torch.Tensor:
    """single-scale SSIM of (x[b], y[b]) -> [B]"""
    _check_window(kernel_size, sigma)
    _check_range(data_range)
    _check_images(1, kernel_size, x=x, y=y)
    x, y = x.contiguous(), y.contiguous()
    minmax = (K.rows_minmax(x), K.rows_minmax(y)) if data_range is None else None
    sim, _, _ = _terms([x], [y], None, None, x.shape[0], minmax, data_range, gaussian_taps(kernel_size, sigma), k1, k2, False)
    return sim[:, 0]


def ms_ssim(x: torch.Tensor, y: torch.Tensor, *, data_range: Optional[float] = 1.0, betas: Sequence[float] = BETAS, normalize: Optional[str] = "relu",
            return_terms: bool = False, kernel_size: int = 11, sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03):
    """MS-SSIM of (x[b], y[b]) -> [B]; return_terms: also the [B, S] terms before normalisation (cs_0 .. cs_{S-2}, sim_{S-1})"""
    _check_window(kernel_size, sigma)
    _check_range(data_range)
    betas = _check_ms(betas, normalize)
    _check_images(len(betas), kernel_size, x=x, y=y)
    x, y = x.contiguous(), y.contiguous()
    minmax = (K.rows_minmax(x), K.rows_minmax(y)) if data_range is None else None
    sim, cs, _ = _terms(pyramid(x, len(betas)), pyramid(y, len(betas)), None, None, x.shape[0], minmax, data_range, gaussian_taps(kernel_size, sigma),
                        k1, k2, False)
    value, terms = _combine(sim, cs, betas, normalize)
    return (value, terms) if return_terms else value


def mse(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The mean of (x[b] - y[b])^2 over C H W -> [B], summed by the SSIM kernel's staging pass: in fp32 over the (at most eight) pixels of a
    thread, in fp64 from there on.  The launch is that of an 11-tap SSIM (of the largest odd window that fits, for sides under 11; at least 3), so
    the bits are those of the MSE that comes with ms_ssim_and_mse at the default window.  There is no reduction kernel of its own: a bare call
    pays for that SSIM launch and drops its sim / cs (ms_ssim_and_mse returns both from one pass), and sides under 3 are refused."""
    _check_images(1, 3, x=x, y=y)
    x, y = x.contiguous(), y.contiguous()
    k = min(L.SSIM_MAX_K, (min(x.shape[2], x.shape[3]) - 1) // 2 * 2 + 1)
    return _terms([x], [y], None, None, x.shape[0], None, 1.0, gaussian_taps(k, 1.5), 0.01, 0.03, True)[2]


def ms_ssim_and_mse(x: torch.Tensor, y: torch.Tensor, *, data_range: Optional[float] = 1.0, betas: Sequence[float] = BETAS,
                    normalize: Optional[str] = "relu", kernel_size: int = 11, sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03):
    """(ms_ssim(x, y), mse(x, y)) from one pass over scale 0 -- at the default kernel_size the same bits as the two calls"""
    _check_window(kernel_size, sigma)
    _check_range(data_range)
    betas = _check_ms(betas, normalize)
    _check_images(len(betas), kernel_size, x=x, y=y)
    x, y = x.contiguous(), y.contiguous()
    minmax = (K.rows_minmax(x), K.rows_minmax(y)) if data_range is None else None
    sim, cs, err = _terms(pyramid(x, len(betas)), pyramid(y, len(betas)), None, None, x.shape[0], minmax, data_range, gaussian_taps(kernel_size, sigma),
                          k1, k2, True)
    return _combine(sim, cs, betas, normalize)[0], err


def plan_pairs(n: int, pairs=None, seed: int = 0) -> torch.Tensor:
    """The pairs of pairwise_ms_ssim as an int64 [P, 2] host tensor, i < j in every row.  pairs=None: all n (n - 1) / 2 unordered pairs in
    lexicographic order; an int: that many DISTINCT unordered pairs drawn without replacement by numpy's default_rng(seed), in draw order; a
    [P, 2] integer tensor: those pairs as given (i != j, both in 0 .. n - 1; a pair may repeat)."""
    if not isinstance(n, int) or n < 2:
        raise ValueError(f"x: at least two images to pair, got {n!r}")
    total = n * (n - 1) // 2
    if pairs is None:
        return torch.triu_indices(n, n, 1).t().contiguous()
    if isinstance(pairs, bool) or not isinstance(pairs, (int, torch.Tensor)):
        raise ValueError(f"pairs: None, an int or a [P, 2] integer tensor, got {type(pairs).__name__}")
    if isinstance(pairs, int):
        if not 1 <= pairs <= total:
            raise ValueError(f"pairs: 1 .. {total} distinct pairs of {n} images, got {pairs}")
        lin = np.random.default_rng(seed).choice(total, size=pairs, replace=False).astype(np.int64)
        starts = np.array([i * n - i * (i + 1) // 2 for i in range(n)], dtype=np.int64)     # the linear index of pair (i, i + 1)
        i = np.searchsorted(starts, lin, side="right") - 1
        j = lin - starts[i] + i + 1
        return torch.from_numpy(np.stack([i, j], axis=1))
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] == 0 or pairs.is_floating_point() or pairs.is_complex() or pairs.dtype == torch.bool:
        raise ValueError(f"pairs: a non-empty [P, 2] integer tensor, got {tuple(pairs.shape)} {pairs.dtype}")
    idx = pairs.detach().to("cpu", torch.int64)
    if bool((idx < 0).any()) or bool((idx >= n).any()) or bool((idx[:, 0] == idx[:, 1]).any()):
        raise ValueError(f"pairs: rows (i, j) with i != j in 0 .. {n - 1}")
    return idx


def pairwise_ms_ssim(x: torch.Tensor, pairs=None, *, seed: int = 0, data_range: Optional[float] = 1.0, betas: Sequence[float] = BETAS,
                     normalize: Optional[str] = "relu", kernel_size: int = 11, sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03,
                     chunk: int = PAIR_CHUNK):
    """MS-SSIM between images of ONE set -> (values [P], index [P, 2]); `pairs` as in plan_pairs (a tensor of pairs that lives on the device is
    copied to the host once, to be checked).  One pyramid per image, the pairs in chunks of `chunk` per launch; nothing is gathered."""
    _check_window(kernel_size, sigma)
    _check_range(data_range)
    betas = _check_ms(betas, normalize)
    if not isinstance(chunk, int) or not 1 <= chunk <= 65535:
        raise ValueError(f"chunk: 1 .. 65535 pairs per launch, got {chunk!r}")
    _check_images(len(betas), kernel_size, x=x)
    index = plan_pairs(int(x.shape[0]), pairs, seed)
    pyr = pyramid(x.contiguous(), len(betas))
    mm = K.rows_minmax(pyr[0]) if data_range is None else None
    dev_index = index.to(torch.int32).to(x.device)
    taps, values = gaussian_taps(kernel_size, sigma), []
    for lo in range(0, index.shape[0], chunk):
        part = dev_index[lo:lo + chunk]
        ix, iy = part[:, 0].contiguous(), part[:, 1].contiguous()
        sim, cs, _ = _terms(pyr, pyr, ix, iy, part.shape[0], (mm, mm), data_range, taps, k1, k2, False)
        values.append(_combine(sim, cs, betas, normalize)[0])
    return (values[0] if len(values) == 1 else torch.cat(values)), dev_index.to(torch.int64)


class ReconstructionMeter:
    """MS-SSIM and MSE of an embedder's reconstructions, accumulated on the device.  update(x) takes x in [-1, 1], runs
    embedder(x)[0].clamp(-1, 1), maps both to [0, 1] and keeps the per-image MS-SSIM (data_range=None: the range of each pair) and MSE;
    compute() is the only host sync: the mean and torch.std of each over all images seen.  `noise`: the NoiseSource handed to the embedder
    (a VAE draws its latent); None leaves the embedder its default, exactly as a bare embedder(x) -- the meter itself draws nothing.
    `lpips`: an LPIPSNet (medfusion_amd.lpips); update() then also keeps LPIPS of (x, reconstruction) in [-1, 1], and compute() adds
    "lpips_mean", "lpips_std" and "lpips_score" = 1 - mean (the reference script's figure).  None: exactly the figures above."""

    def __init__(self, embedder, noise=None, lpips=None):
        self.embedder, self.noise, self.lpips = embedder, noise, _check_lpips_net(lpips)
        self.reset()

    def reset(self) -> None:
        self._ms, self._mse, self._lp = [], [], []

    @torch.no_grad()
    def update(self, x: torch.Tensor) -> None:
        _check_images(len(BETAS), 11, x=x)
        pred = (self.embedder(x) if self.noise is None else self.embedder(x, noise=self.noise))[0].clamp(-1, 1)
        a, b = (x + 1) / 2, (pred + 1) / 2
        v, e = ms_ssim_and_mse(a, b, data_range=None)
        self._ms.append(v)
        self._mse.append(e)
        if self.lpips is not None:
            from .lpips import lpips
            self._lp.append(lpips(x, pred, self.lpips))

    def values(self):
        """the per-image MS-SSIM and MSE so far, as two device tensors"""
        if not self._ms:
            raise ValueError("ReconstructionMeter: no update() yet")
        return torch.cat(self._ms), torch.cat(self._mse)

    def lpips_values(self) -> torch.Tensor:
        """the per-image LPIPS so far, as a device tensor (a meter built with lpips=net)"""
        if not self._lp:
            raise ValueError("ReconstructionMeter: no update() with an LPIPS net yet")
        return torch.cat(self._lp)

    def compute(self) -> dict:
        ms, err = self.values()
        return _summary(ms, err, self.lpips_values() if self.lpips is not None else None)


def _check_lpips_net(net):
    if net is not None:
        from .lpips import LPIPSNet
        if not isinstance(net, LPIPSNet):
            raise ValueError(f"lpips: None or an LPIPSNet, got {type(net).__name__}")
    return net


def _summary(ms: torch.Tensor, err: torch.Tensor, lp: Optional[torch.Tensor]) -> dict:
    """the meters' compute(): one copy to the host"""
    rows = [ms.mean(), torch.std(ms), err.mean(), torch.std(err)] + ([lp.mean(), torch.std(lp)] if lp is not None else [])
    stats = torch.stack(rows).tolist()
    res = {"ms_ssim_mean": stats[0], "ms_ssim_std": stats[1], "mse_mean": stats[2], "mse_std": stats[3], "count": int(ms.numel())}
    if lp is not None:
        res.update(lpips_mean=stats[4], lpips_std=stats[5], lpips_score=1.0 - stats[4])
    return res
