"""The spatial_dims=3 cases shared by scripts/gen_3d_golden.py (which runs them through the reference) and the tests (which run them through
medfusion_amd): constructor arguments, input shapes and noise seeds of the tests/golden/d3_* fixtures."""
from __future__ import annotations

from oracle import restate as R

GN8 = ("GROUP", {"num_groups": 8, "affine": True})
ACT = ("SWISH", {})

# name -> (class name in conv_blocks.py / blocks3d.py, constructor kwargs, input shapes (two: a torch.cat([h, skip], 1) input), emb width)
BLOCK_CASES = {
    "res_emb": ("UnetResBlock", dict(in_channels=32, out_channels=64, kernel_size=3, stride=1, norm_name=GN8, act_name=ACT, emb_channels=16),
                [(2, 32, 3, 5, 6)], 16),
    "res_cat": ("UnetResBlock", dict(in_channels=96, out_channels=32, kernel_size=3, stride=1, norm_name=GN8, act_name=ACT, emb_channels=16),
                [(2, 64, 3, 5, 6), (2, 32, 3, 5, 6)], 16),
    "basic_emb": ("UnetBasicBlock", dict(in_channels=32, out_channels=32, kernel_size=3, stride=1, norm_name=GN8, act_name=ACT, emb_channels=16),
                  [(2, 32, 4, 4, 4)], 16),
    "down2": ("BasicDown", dict(in_channels=32, out_channels=64, kernel_size=3, stride=2), [(2, 32, 5, 7, 9)], 0),
    "down122": ("BasicDown", dict(in_channels=32, out_channels=32, kernel_size=3, stride=(1, 2, 2)), [(2, 32, 5, 7, 9)], 0),
    "up2": ("BasicUp", dict(in_channels=64, out_channels=32, kernel_size=2, stride=2), [(2, 64, 3, 4, 5)], 0),
    "up122": ("BasicUp", dict(in_channels=32, out_channels=32, kernel_size=(1, 2, 2), stride=(1, 2, 2)), [(2, 32, 3, 4, 5)], 0),
}

# name -> (strides, input shape NCDHW)
UNET_CASES = {
    "unet_s2": ([1, 2, 2, 2], (2, 8, 4, 8, 8)),
    "unet_s122": ([1, (1, 2, 2), (1, 2, 2), (1, 2, 2)], (2, 8, 3, 8, 8)),
}

VAE_CASE = dict(R.tiny_vae_kwargs(), in_channels=1, out_channels=1, spatial_dims=3)

# fixture name -> (noise seed, steps, use_ddim, guidance scale, condition, estimator objective); B = 2, latent (4, 4, 8, 8)
SAMPLE_CASES = {
    "d3_sample_ddim5_cfg8": (41, 5, True, 8.0, [1, 0], "x_T"),
    "d3_sample_ddpm4": (42, 4, False, 1.0, None, "x_T"),
    "d3_sample_ddim4_x0": (43, 4, True, 1.0, [0, 1], "x_0"),
}


def block_kwargs(cls: str, kw: dict) -> dict:
    return dict(kw, spatial_dims=3)


def unet_kwargs(strides, in_ch: int = 8) -> dict:
    """a tiny 3-D UNet (oracle kwargs: restate classes for the embedders; tests.util.to_product_kwargs swaps them)"""
    return R.tiny_unet_kwargs(2, "none", hid=(32, 32, 64, 64), spatial_dims=3, strides=list(strides), in_ch=in_ch, out_ch=in_ch)
