"""The image-conditioned sampling cases (img2img and masked inpainting) shared by scripts/gen_i2i_golden.py (which runs them through the reference)
and the tests (which run them through the oracle restatement and through medfusion_amd): pipeline arguments, inputs, masks, noise seeds of the
tests/golden/i2i_* fixtures, and the loop they all drive -- `composed_loop`, a composition of the pipeline's own `forward` and the scheduler's own
`estimate_x_t` that works on the reference pipeline and on its restatement alike (they share the interface)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import restate as R
from oracle import synth as S

B, LATENT = 2, (8, 8, 8)

# fixture name -> pipeline (tag of the synthetic weights, UNet classes, constructor flags), loop arguments, mask kind.
# k = min(steps, int(strength * steps + 0.5)) iterations run.  mask: None | "cells" (latent resolution, hash-random) | "pixels" (image
# resolution, a rectangle per sample: through VAE.encode, composite=True)
CASES = {
    "i2i_ddim6of10_cfg4": dict(pipe=dict(tag="pipe_tiny", ncls=3), steps=10, strength=0.6, use_ddim=True, guidance_scale=4.0, condition=[2, 0],
                               mask=None, seed=51),
    "i2i_inpaint_ddim8of8": dict(pipe=dict(tag="pipe_tiny", ncls=3), steps=8, strength=1.0, use_ddim=True, mask="cells", seed=52),
    "i2i_inpaint_ddim5of12_cfg4": dict(pipe=dict(tag="pipe_tiny", ncls=3), steps=12, strength=0.42, use_ddim=True, guidance_scale=4.0,
                                       condition=[1, 2], mask="cells", seed=53),
    "i2i_inpaint_ddpm7of20": dict(pipe=dict(tag="pipe_tiny", ncls=3), steps=20, strength=0.35, use_ddim=False, mask="cells", seed=54),
    "i2i_inpaint_x0obj_clip": dict(pipe=dict(tag="pipe_tiny_x0", ncls=None, clip_x0=True, objective="x_0"), steps=6, strength=0.67, use_ddim=True,
                                   mask="cells", seed=55),
    "i2i_inpaint_learned_var": dict(pipe=dict(tag="pipe_i2i_var", ncls=2, estimate_variance=True), steps=6, strength=1.0, use_ddim=False,
                                    guidance_scale=1.0, condition=[1, 0], mask="cells", seed=56),
    "i2i_vae_composite": dict(pipe=dict(tag="pipe_tiny", ncls=3), steps=6, strength=0.5, use_ddim=True, mask="pixels", seed=57, enc_seed=58,
                              centering=True),
}
EXECUTED = {"i2i_ddim6of10_cfg4": 6, "i2i_inpaint_ddim8of8": 8, "i2i_inpaint_ddim5of12_cfg4": 5, "i2i_inpaint_ddpm7of20": 7, "i2i_inpaint_x0obj_clip": 4,
            "i2i_inpaint_learned_var": 6, "i2i_vae_composite": 3}


def span(steps: int, strength: float):
    """-> (s, k): iterations s .. steps-1 of the full loop run"""
    k = min(steps, int(strength * steps + 0.5))
    return steps - k, k


def pipe_args(name: str):
    """-> (unet kwargs, vae kwargs, tag, constructor flags) in the form build_oracle_pipe / build_product_pipe take"""
    p = dict(CASES[name]["pipe"])
    tag, ncls = p.pop("tag"), p.pop("ncls")
    return R.tiny_unet_kwargs(ncls, "none"), R.tiny_vae_kwargs(), tag, p


def case_inputs(name: str):
    """-> (x, mask, is_latent): the latent (or the image in [-1, 1]) and the boolean mask (True = regenerate) or None"""
    c = CASES[name]
    if c["mask"] == "pixels":
        x = S.synth_input(f"{name}.img", (B, 3, 64, 64), 0.5)
        m = torch.zeros((B, 1, 64, 64), dtype=torch.bool)
        m[0, :, 10:37, 20:49] = True     # (edges inside cells: the max-reduction decides those cells)
        m[1, :, 40:64, 0:13] = True
        return x, m, False
    x = S.synth_input(f"{name}.z0", (B, *LATENT))
    m = None if c["mask"] is None else (S.synth_input(f"{name}.mask", (B, 1, *LATENT[1:])) > 0.2)
    return x, m, True


def cell_mask(mask: torch.Tensor, latent_shape) -> torch.Tensor:
    """a mask at image resolution reduced to the latent's cells: a cell is regenerated if any of its pixels is (max over the block)"""
    sp = tuple(latent_shape[2:])
    if tuple(mask.shape[2:]) == sp:
        return mask.bool()
    f = [a // b for a, b in zip(mask.shape[2:], sp)]
    pool = F.max_pool2d if len(sp) == 2 else F.max_pool3d
    return pool(mask.float(), f) > 0.5


def loop_kwargs(name: str) -> dict:
    c = CASES[name]
    kw = {}
    if "condition" in c:
        kw.update(condition=torch.tensor(c["condition"]), guidance_scale=c["guidance_scale"], un_cond=None)
    return kw


@torch.no_grad()
def composed_loop(pipe, randn, x, strength, steps, use_ddim, mask=None, is_latent=True, centering=False, composite=False, decode=True, trace=None,
                  condition=None, guidance_scale=1.0, un_cond=None):
    """Image-conditioned sampling out of the pipeline's own pieces.  `pipe`: the reference DiffusionPipeline or its restatement; `randn(like)`: the
    source of every N(0,1) draw of the loop, in draw order (eps0 first).  -> (result, z0)."""
    sch = pipe.noise_scheduler
    if is_latent:
        z0 = x
    else:
        z0 = pipe.latent_embedder.encode(x) if pipe.latent_embedder is not None else x
        if centering:
            z0 = 2 * z0 - 1
    n = z0.shape[0]
    ts = torch.linspace(0, sch.T - 1, steps, dtype=torch.long) if use_ddim else sch.timesteps_array[slice(0, steps)]
    steps = len(ts)
    s, _ = span(steps, strength)
    rev = list(reversed(ts))
    cells = None if mask is None else cell_mask(mask, z0.shape)
    eps0 = randn(z0)                                                        # draw #0
    x_t = sch.estimate_x_t(z0, rev[s].expand(n), eps0)
    self_cond = None
    for i in range(s, steps):
        t = rev[i]
        x_t, x_0, x_T, self_cond = pipe(x_t, t.expand(n), condition, self_cond=self_cond, guidance_scale=guidance_scale, un_cond=un_cond)
        self_cond = self_cond if pipe.use_self_conditioning else None
        if use_ddim and steps - i - 1 > 0:                                  # the DDIM update of the sampling loop
            alpha, alpha_next = sch.alphas_cumprod[t], sch.alphas_cumprod[ts[steps - i - 2]]
            sigma = ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
            c = (1 - alpha_next - sigma ** 2).sqrt()
            x_t = x_0 * alpha_next.sqrt() + c * x_T + sigma * randn(x_t)
        if cells is not None:                                               # the kept cells: the known latent at the same time, same eps0
            t_next = rev[i + 1] if i + 1 < steps else torch.tensor(-1)
            x_t = torch.where(cells, x_t, sch.estimate_x_t(z0, t_next.expand(n), eps0))
        if trace is not None:
            trace.append((x_0.clone(), x_t.clone()))
    out = x_t
    if decode and pipe.latent_embedder is not None:
        out = pipe.latent_embedder.decode(out)
    if composite:
        out = torch.where(mask.bool(), out, x)
    return out, z0
