"""ValidationMeter -- the held-out denoising loss of DiffusionPipeline.validation_step accumulated over a data set: what the reference's
Lightning loop logs as val/loss, val/L1, val/L2 and val/variance_loss (`on_epoch=True`: the mean over the rows seen), plus the same figures by
timestep bin -- at which noise levels the model is weak.  Per-row results and their timesteps stay on the device until compute(), the only
host synchronisation.
"""
from __future__ import annotations

from typing import Optional

import torch

from .noise import NoiseSource


class ValidationMeter:
    KEYS = (("loss", "loss_rows"), ("L1", "l1_rows"), ("L2", "l2_rows"), ("variance_loss", "variance_rows"))

    def __init__(self, pipe, bins: int = 10, loss: str = "l1"):
        if not (isinstance(bins, int) and bins >= 1):
            raise ValueError(f"bins={bins!r}: a positive integer")
        if loss not in pipe.LOSSES:
            raise ValueError(f"loss={loss!r}: one of {pipe.LOSSES}")
        self.pipe, self.bins, self.loss = pipe, bins, loss
        self.reset()

    def reset(self) -> None:
        self._rows, self._t = [], []

    def update(self, x, condition=None, *, t=None, noise: Optional[NoiseSource] = None, is_latent=False, encode_noise: Optional[NoiseSource] = None) -> None:
        """one validation_step over the batch; its per-row figures and timesteps are kept on the device (no synchronisation)"""
        r = self.pipe.validation_step(x, condition, t=t, noise=noise, loss=self.loss, is_latent=is_latent, encode_noise=encode_noise, per_sample=True)
        self._rows.append(torch.stack([r[rows] for _, rows in self.KEYS if rows in r]))
        self._t.append(r["t"])

    def compute(self) -> dict:
        """-> {"n", "loss", "L1", "L2" (, "variance_loss"): the means over every row seen (python floats), "bins": {"edges": [bins + 1] timesteps,
        "count": [bins], "loss" / "L1" / "L2" (/ "variance_loss"): [bins] means of the rows whose t falls in [edge_i, edge_i+1), NaN where
        empty}} -- one device-to-host copy"""
        if not self._rows:
            raise RuntimeError("ValidationMeter.compute() before any update()")
        rows, t = torch.cat(self._rows, dim=1), torch.cat(self._t)
        host = torch.cat((rows, t.to(torch.float64)[None]), dim=0).cpu()   # the one host sync (timesteps are exact in fp64)
        rows, t = host[:-1], host[-1].to(torch.long)
        names = [name for name, _ in self.KEYS][: rows.shape[0]]
        T = self.pipe.noise_scheduler.T
        which = (t * self.bins) // T
        count = torch.bincount(which, minlength=self.bins)[: self.bins]
        out = {"n": int(t.numel())}
        table = {"edges": [(i * T + self.bins - 1) // self.bins for i in range(self.bins + 1)], "count": count.tolist()}
        for name, v in zip(names, rows):
            out[name] = float(v.mean())
            sums = torch.zeros(self.bins, dtype=torch.float64).index_add_(0, which, v)
            table[name] = [float(s / c) if c else float("nan") for s, c in zip(sums.tolist(), count.tolist())]
        out["bins"] = table
        return out
