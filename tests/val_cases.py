"""The held-out denoising loss (DiffusionPipeline.validation_step, csrc/loss.hip): the cases of the tests/golden/val_* fixtures shared by
scripts/gen_val_golden.py (which runs the reference's own `_step`) and the tests; `restated_step`, the plain-torch restatement of `_step` at
state != 'train' in any dtype; the definitions the kernels are held to (`loss_sums`, `variance_sums`), and the bounds DERIVED for them -- from
the precision of the formats, never from what the kernels give."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import synth as S

U = 2.0 ** -24        # unit roundoff of fp32
U64 = 2.0 ** -53
MARGIN = 4.0          # an expf / logf chain is held to MARGIN x the distance of its own restatement in fp32 (tests/metrics_cases.py)
SCALARS = ("loss", "L1", "L2", "variance_loss", "variance_scale")

# fixture name -> spatial dims, pipeline (tag of the synthetic weights, label classes, constructor flags), extra UNet arguments, loss, the injected
# timesteps (one per row), the Philox seed of x_T (draw #0), and for an image input: the encoder's seed, labels.
# 2-D: latent (8, 8, 8) -- through the tiny VAE's encoder from (3, 64, 64) images where `image` -- heads at 4 x 4 and 2 x 2;
# 3-D: the tests/d3_cases.unet_kwargs architecture on a (4, 4, 8, 8) latent, heads at 2 x 4 x 4 and 1 x 2 x 2.
CASES = {
    "val_2d_xT_ds_l1": dict(dims=2, pipe=dict(tag="val_ds", ncls=None), unet=dict(deep_supervision=True), loss="l1", t=[0, 417, 999], seed=81),
    "val_2d_x0_l2": dict(dims=2, pipe=dict(tag="pipe_tiny_x0", ncls=None, clip_x0=True, objective="x_0"), loss="l2", t=[1, 650], seed=82),
    "val_2d_var_xT": dict(dims=2, pipe=dict(tag="val_var", ncls=None, clip_x0=True, estimate_variance=True), unet=dict(deep_supervision=True), loss="l1",
                          t=[0, 500, 998], seed=83),
    "val_2d_var_x0": dict(dims=2, pipe=dict(tag="val_var_x0", ncls=None, objective="x_0", estimate_variance=True), loss="l1", t=[0, 300], seed=84),
    "val_2d_vae_labels": dict(dims=2, pipe=dict(tag="pipe_tiny", ncls=3), loss="l1", t=[120, 870], seed=85, image=True, enc_seed=86, condition=[2, 0]),
    "val_3d_xT": dict(dims=3, pipe=dict(tag="solver_ddim0_3d", ncls=2), unet=dict(deep_supervision=True), loss="l1", t=[3, 700], seed=87, condition=[1, 0]),
}
LATENT = {2: (8, 8, 8), 3: (4, 4, 8, 8)}
IMAGE = (3, 64, 64)


def pipe_args(case: dict):
    """-> (unet kwargs in the oracle's form, vae kwargs or None, tag, constructor flags): tests/solver_cases.pipe_args plus the case's UNet extras"""
    from tests.solver_cases import pipe_args as base

    unet_kw, vae_kw, tag, flags = base(case)
    return {**unet_kw, **case.get("unet", {})}, (vae_kw if case.get("image") else None), tag, flags


def case_input(name: str) -> torch.Tensor:
    """the case's input: images in [0, 1] (centred by the pipeline) or the latent itself"""
    c = CASES[name]
    n = len(c["t"])
    if c.get("image"):
        return S.synth_input(f"val.{name}.x", (n, *IMAGE), 0.5).abs().clamp(0, 1)
    return S.synth_input(f"val.{name}.x", (n, *LATENT[c["dims"]]), 0.6)


def case_condition(name: str, device=None):
    c = CASES[name].get("condition")
    return None if c is None else torch.tensor(c, device=device)


def ds_weights(heads: int):
    """diffusion_pipeline.py:144-146"""
    w = [1 / 2 ** i for i in range(1 + heads)]
    return [v / sum(w) for v in w]


def pool_factor(pred_shape, target_shape):
    """the integer factor of the area pooling, or None where F.interpolate(mode='area') is not a block mean (a side that does not divide)"""
    f = None
    for p, t in zip(pred_shape[2:], target_shape[2:]):
        if p < 1 or t % p or (f is not None and t // p != f):
            return None
        f = t // p
    return f


# ------------------------------------------------------------------------------------------------ `_step`, restated
def gather(table, t, ndim, dtype):
    return table.to(dtype).gather(0, t).reshape(-1, *((1,) * (ndim - 1)))


F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))   # a python constant as the fp32 chain holds it


def variance_terms(tb, x_0, x_t, x_T, pred, pred_var, t, objective, clip_x0, var_floor=1e-20, nll_floor=1e-6):
    """diffusion_pipeline.py:152-173 per element -> (kl, nll, var_scale); tb: the scheduler's fp32 tables, every operation in x_0's dtype.
    var_floor, nll_floor: the two clamps' constants (estimate_variance_t's eps, F.gaussian_nll_loss's eps) as the reference writes them; torch rounds
    them to the tensors' dtype, so the fp32 run holds F32(1e-20) and F32(1e-6)."""
    dt, nd = x_0.dtype, x_0.ndim
    var_scale = (pred_var + 1) / 2
    lmin = torch.log(gather(tb["posterior_variance"], t, nd, dt).clamp(min=var_floor))
    lmax = torch.log(gather(tb["betas"], t, nd, dt).clamp(min=var_floor))
    pred_logvar = var_scale * lmax + (1 - var_scale) * lmin
    true_logvar = 0 * lmax + (1 - 0) * lmin
    if objective == "x_T":
        pred_x_0 = gather(tb["sqrt_recip_alphas_cumprod"], t, nd, dt) * x_t - gather(tb["sqrt_recipm1_alphas_cumprod"], t, nd, dt) * x_T
        pred_x_0 = pred_x_0.clamp(-1, 1) if clip_x0 else pred_x_0
    else:
        pred_x_0 = pred
    c1, c2 = gather(tb["posterior_mean_coef1"], t, nd, dt), gather(tb["posterior_mean_coef2"], t, nd, dt)
    pred_mean, true_mean = c1 * pred_x_0 + c2 * x_t, c1 * x_0 + c2 * x_t
    kl = 0.5 * (pred_logvar - true_logvar + torch.exp(true_logvar - pred_logvar) + torch.pow(true_mean - pred_mean, 2) * torch.exp(-pred_logvar) - 1.0)
    nll = F.gaussian_nll_loss(pred_x_0, x_0, torch.exp(pred_logvar), reduction="none", eps=nll_floor)
    return kl, nll, var_scale


def variance_sums(tb, x_0, x_t, x_T, pred, pred_var, t, objective, clip_x0, dtype):
    """[B, 3] per-row sums (kl, nll, var_scale) of the restatement run in `dtype` on the fp32 DATA: what K.variance_loss is held to.  The two clamp
    constants are data of the fp32 definition like the tables -- the fp64 run takes the values the fp32 chain holds, F32(1e-20) and F32(1e-6), not
    the decimal ones 2.5e-8 away: at t = 0 nearly every variance sits ON the 1e-6 floor and (x - mu)^2 / floor would carry that 2.5e-8 into the sum,
    a difference of definition, not of arithmetic (the fp32 run is unchanged by this: torch rounds the constants to fp32 itself)."""
    c = lambda v: v.to(dtype)
    terms = variance_terms(tb, c(x_0), c(x_t), c(x_T), c(pred), c(pred_var), t, objective, clip_x0, F32(1e-20), F32(1e-6))
    return torch.stack([v.reshape(v.shape[0], -1).sum(1) for v in terms], dim=1)


def diffuse(tb, x_0, x_T, t, dtype):
    nd = x_0.ndim
    return gather(tb["sqrt_alphas_cumprod"], t, nd, dtype) * x_0 + gather(tb["sqrt_one_minus_alphas_cumprod"], t, nd, dtype) * x_T


@torch.no_grad()
def restated_step(est, tb, x_0, x_T, t, condition, *, objective="x_T", estimate_variance=False, clip_x0=False, loss="l1", self_cond=False):
    """`_step` at state != 'train' (diffusion_pipeline.py:96-190) in plain torch, in x_0's dtype, with t and x_T injected and the condition kept
    -> the result scalars.  est: the restatement's UNet (forward(x_t, t, condition, self_cond) -> (y, y_ver))."""
    x_t = diffuse(tb, x_0, x_T, t, x_0.dtype)
    pred, pred_vertical = est(x_t, t, condition, x_t if self_cond else None)
    if estimate_variance:
        pred, pred_var = pred.chunk(2, dim=1)
    target = x_T if objective == "x_T" else x_0
    fct = F.l1_loss if loss == "l1" else F.mse_loss
    w = ds_weights(len(pred_vertical))
    out = {}
    total = fct(pred, target) * w[0]
    if estimate_variance:
        kl, nll, var_scale = variance_terms(tb, x_0, x_t, x_T, pred, pred_var, t, objective, clip_x0)
        dims = list(range(1, x_0.ndim))
        var_loss = torch.mean(torch.where(t == 0, nll.mean(dims), kl.mean(dims)))
        total = total + var_loss
        out["variance_scale"], out["variance_loss"] = torch.mean(var_scale), var_loss
    for i, p in enumerate(pred_vertical):
        total = total + fct(p, F.interpolate(target, size=p.shape[2:], mode="area")) * w[i + 1]
    out.update(loss=total, L2=F.mse_loss(pred, target), L1=F.l1_loss(pred, target))
    return out


# ------------------------------------------------------------------------------------------------ the error sums and their bound
def loss_sums(pred, target):
    """the definition K.denoise_loss is held to, in fp64 on the fp32 inputs: per row (sum |d|, sum d^2), d = pred - the exact block mean of the
    target -> ([B, 2] sums, the fields the bound needs)"""
    p, t = pred.double(), target.double()
    f = pool_factor(pred.shape, target.shape)
    assert f is not None
    nd = pred.ndim - 2
    pool = (F.avg_pool2d if nd == 2 else F.avg_pool3d)
    tm = t if f == 1 else pool(t, f)
    ta = t.abs() if f == 1 else pool(t.abs(), f)                      # the mean of |v| over the block
    d = p - tm
    rows = lambda v: v.reshape(v.shape[0], -1).sum(1)
    return torch.stack((rows(d.abs()), rows(d * d)), dim=1), dict(d=d, tm=tm, ta=ta, n=f ** nd)


def loss_bound(fields):
    """[B, 2]: how far the kernel's row sums may lie from loss_sums.  Per element the kernel forms
      tgt = fl32(the f^dims block summed one by one in fp32, divided by f^dims): n - 1 additions, each within U of its partial sum (all at most
            the sum of |v| = n ta), and a division that is exact for a power of two and within U otherwise:  e_t <= (n - 1) U ta + [n not 2^k] U |tm|;
      d   = fl32(pred - tgt): within U |pred - tgt| of it, so delta = |d_kernel - d| <= U |d| + e_t (second order: the factor 1 + 2^-10 below);
    |d| then enters an fp64 sum exactly and d d as an exact fp64 product, so  |S1 - S1*| <= sum delta  and  |S2 - S2*| <= sum delta (2 |d| + delta),
    plus the fp64 additions of N terms: N 2^-53 of the sum.  Of order 2^-24 sum |d| plus the pooled mean's (f^dims - 1) 2^-24 term."""
    d, tm, ta, n = fields["d"].abs(), fields["tm"].abs(), fields["ta"], fields["n"]
    e_t = (n - 1) * U * ta + (0.0 if n & (n - 1) == 0 else U) * tm
    delta = (U * d + e_t) * (1 + 2.0 ** -10)
    rows = lambda v: v.reshape(v.shape[0], -1).sum(1)
    count = d[0].numel()
    b1 = rows(delta) + count * U64 * rows(d + delta)
    b2 = rows(delta * (2 * d + delta)) + count * U64 * rows((d + delta) ** 2)
    return torch.stack((b1, b2), dim=1)


def emulate_kernel_sums(pred, target):
    """an fp32 emulation of the kernel's arithmetic on the CPU: the block summed in (depth, row, column) order in fp32, divided, d = fl32(pred - tgt),
    then fp64 sums (the CPU tests hold loss_bound against it)"""
    f = pool_factor(pred.shape, target.shape)
    nd = pred.ndim - 2
    if f == 1:
        tg = target
    else:
        B, C = target.shape[:2]
        sp = pred.shape[2:]
        if nd == 2:
            blocks = target.reshape(B, C, sp[0], f, sp[1], f).permute(0, 1, 2, 4, 3, 5).reshape(B, C, *sp, f * f)
        else:
            blocks = target.reshape(B, C, sp[0], f, sp[1], f, sp[2], f).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(B, C, *sp, f ** 3)
        s = torch.zeros_like(blocks[..., 0])
        for j in range(blocks.shape[-1]):
            s = s + blocks[..., j]
        tg = s / float(f ** nd)
    d = (pred - tg).double()
    rows = lambda v: v.reshape(v.shape[0], -1).sum(1)
    return torch.stack((rows(d.abs()), rows(d * d)), dim=1)


def hash_rows(name: str, shape, scale: float = 1.0) -> torch.Tensor:
    return S.synth_input("val." + name, shape, scale)
