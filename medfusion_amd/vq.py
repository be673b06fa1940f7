"""The other three latent embedders of medical_diffusion/models/embedders/latent_embedders.py on the HIP kernels: `VectorQuantizer` (:40-71),
`VQVAE` (:191-340), `VQGAN` (:408-490) and `VAEGAN` (:860-940).

VQVAE has VAE's layout (vae.VAE: same encoder, decoder and deep-supervision heads) with a single 1x1 `out_enc` block and a codebook in place of
the Gaussian: `encode` returns the encoder's output unquantized, `decode` quantizes first (the nearest-codebook kernel of csrc/vq.hip), then runs
VAE's decoder pass.  VQGAN and VAEGAN hold a VQVAE, respectively a VAE, under the name `vqvae` and delegate to it; their discriminators are
training-only and not built (their tensors in a checkpoint are unexpected keys).  Training losses / perceiver / optimiser arguments are accepted
and ignored, as VAE does.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import kernels as K
from . import lib as L
from .blocks import BasicBlock
from .vae import VAE, _require_device


class VectorQuantizer(nn.Module):
    """latent_embedders.py:40-71.  forward(z [B,C,H,W]) -> (z + (e_idx - z), beta * mse + mse) on the device."""

    def __init__(self, num_embeddings, emb_channels, beta=0.25):
        super().__init__()
        self.num_embeddings = num_embeddings
        self.emb_channels = emb_channels
        self.beta = beta
        self.embedder = nn.Embedding(num_embeddings, emb_channels)
        self.embedder.weight.data.uniform_(-1.0 / self.num_embeddings, 1.0 / self.num_embeddings)

    def quantize(self, z: torch.Tensor, want_loss: bool = False):
        """(z_q, loss or None); the loss (:62) is (1 + beta) * sum((e_idx - z)^2) / numel, the sum in fp64"""
        if z.shape[1] != self.emb_channels:
            raise RuntimeError(f"VectorQuantizer: z has {z.shape[1]} channels, the codebook {self.emb_channels}")
        z_q, _, sq = K.vector_quantize(z, self.embedder.weight, want_sqerr=want_loss)
        if not want_loss:
            return z_q, None
        return z_q, ((1.0 + self.beta) * sq / max(z.numel(), 1)).to(torch.float32)

    def forward(self, z: torch.Tensor):
        return self.quantize(z, want_loss=True)


def _only_2d(who: str, spatial_dims) -> None:
    if spatial_dims != 2:
        raise NotImplementedError(f"{who}(spatial_dims={spatial_dims}): the codebook / GAN embedders are built in 2-D only")


class VQVAE(VAE):
    def __init__(self, in_channels=3, out_channels=3, spatial_dims=2, emb_channels=4, num_embeddings=8192, hid_chs=[32, 64, 128, 256],
                 kernel_sizes=[3, 3, 3, 3], strides=[1, 2, 2, 2], norm_name=("GROUP", {"num_groups": 32, "affine": True}), act_name=("Swish", {}),
                 dropout=0.0, use_res_block=True, deep_supervision=False, learnable_interpolation=True, use_attention="none", beta=0.25,
                 **_training_only):
        _only_2d(type(self).__name__, spatial_dims)
        super().__init__(in_channels, out_channels, spatial_dims, emb_channels, hid_chs, kernel_sizes, strides, norm_name, act_name, dropout,
                         use_res_block, deep_supervision, learnable_interpolation, use_attention)
        # (re-assigning a registered child keeps its place: the state-dict order is the reference's, :241-296)
        self.out_enc = BasicBlock(spatial_dims, hid_chs[-1], emb_channels, 1)
        self.quantizer = VectorQuantizer(num_embeddings, emb_channels, beta)

    def _encode_z(self, x):
        h = self.inc(x.contiguous(), None, in_layout=L.LAYOUT_NCHW)
        for enc in self.encoders:
            h = enc(h)
        return self.out_enc(h, out_layout=L.LAYOUT_NCHW)

    @torch.no_grad()
    def encode(self, x: torch.Tensor, noise=None) -> torch.Tensor:
        """:304-309 -- the encoder's output, NOT quantized (`noise` is accepted for VAE's signature and unused: nothing is drawn)"""
        _require_device(x, type(self).__name__)
        K.SyncWords.reset(x.device)
        return K.with_fused_fallback(x.device, lambda: self._encode_z(x))

    def _decode_input(self, z):
        """:312 -- decode quantizes first"""
        return self.quantizer.quantize(z)[0]

    @torch.no_grad()
    def forward(self, x_in: torch.Tensor, noise=None):
        """:319-338 -> (out, deep-supervision outputs finest first, emb_loss)"""
        _require_device(x_in, type(self).__name__)
        K.SyncWords.reset(x_in.device)

        def run():
            z_q, emb_loss = self.quantizer(self._encode_z(x_in))
            out_hor = []
            out = self._decode_pass(z_q, out_hor)
            return out, out_hor[::-1], emb_loss

        return K.with_fused_fallback(x_in.device, run)


class _GanWrapper(nn.Module):
    """VQGAN / VAEGAN at inference: the autoencoder under `vqvae`, everything delegated to it"""

    @property
    def scale(self):
        return self.vqvae.scale

    @property
    def emb_channels(self):
        return self.vqvae.emb_channels

    @property
    def out_channels(self):
        return self.vqvae.out_channels

    def encode(self, x, noise=None):
        return self.vqvae.encode(x, noise=noise)

    def decode(self, z):
        return self.vqvae.decode(z)

    def forward(self, x, noise=None):
        return self.vqvae(x, noise=noise)


class VQGAN(_GanWrapper):
    """latent_embedders.py:408-490"""

    def __init__(self, in_channels=3, out_channels=3, spatial_dims=2, emb_channels=4, num_embeddings=8192, hid_chs=[64, 128, 256, 512],
                 kernel_sizes=[3, 3, 3, 3], strides=[1, 2, 2, 2], norm_name=("GROUP", {"num_groups": 32, "affine": True}), act_name=("Swish", {}),
                 dropout=0.0, use_res_block=True, deep_supervision=False, learnable_interpolation=True, use_attention="none", beta=0.25,
                 **_training_only):
        _only_2d(type(self).__name__, spatial_dims)
        super().__init__()
        self.vqvae = VQVAE(in_channels, out_channels, spatial_dims, emb_channels, num_embeddings, hid_chs, kernel_sizes, strides, norm_name,
                           act_name, dropout, use_res_block, deep_supervision, learnable_interpolation, use_attention, beta)


class VAEGAN(_GanWrapper):
    """latent_embedders.py:860-940 (its `vqvae` is a VAE)"""

    def __init__(self, in_channels=3, out_channels=3, spatial_dims=2, emb_channels=4, hid_chs=[64, 128, 256, 512], kernel_sizes=[3, 3, 3, 3],
                 strides=[1, 2, 2, 2], norm_name=("GROUP", {"num_groups": 8, "affine": True}), act_name=("Swish", {}), dropout=0.0,
                 use_res_block=True, deep_supervision=False, learnable_interpolation=True, use_attention="none", **_training_only):
        _only_2d(type(self).__name__, spatial_dims)
        super().__init__()
        self.vqvae = VAE(in_channels, out_channels, spatial_dims, emb_channels, hid_chs, kernel_sizes, strides, norm_name, act_name, dropout,
                         use_res_block, deep_supervision, learnable_interpolation, use_attention)
