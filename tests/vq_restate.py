"""Test infrastructure: an independent CPU restatement of the reference's codebook embedders (medical_diffusion/models/embedders/
latent_embedders.py), built on the blocks of oracle/restate.py (imported, not edited).  scripts/gen_vq_golden.py checks it against the real
reference bit for bit before it writes tests/golden/vq_*.npz; the tests use it where the reference itself cannot go (the GPU box).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from oracle import restate as R

GN32 = ("GROUP", {"num_groups": 32, "affine": True})


class VectorQuantizer(nn.Module):
    """latent_embedders.py:40-71"""

    def __init__(self, num_embeddings, emb_channels, beta=0.25):
        super().__init__()
        self.num_embeddings, self.emb_channels, self.beta = num_embeddings, emb_channels, beta
        self.embedder = nn.Embedding(num_embeddings, emb_channels)

    def distances(self, z):
        """:49-54: [pixels, K] in fp32 by the reference's cancelling formula; pixels in (n, h, w) order"""
        zf = torch.moveaxis(z, 1, -1).reshape(-1, self.emb_channels)
        w = self.embedder.weight
        return torch.sum(zf ** 2, dim=1, keepdim=True) + torch.sum(w ** 2, dim=1) - 2 * torch.einsum("bd,dn->bn", zf, w.t())

    def indices(self, z):
        """:56 -- first minimum"""
        return torch.argmin(self.distances(z), dim=1)

    def forward(self, z):
        """:58-71 -> (z + (z_q - z), beta * mse + mse)"""
        z_ch = torch.moveaxis(z, 1, -1)
        z_q = self.embedder(self.indices(z)).view(z_ch.shape)
        z_q = torch.moveaxis(z_q, -1, 1)
        loss = self.beta * torch.mean((z_q - z) ** 2) + torch.mean((z_q - z) ** 2)
        return z + (z_q - z), loss


class VQVAE(R.VAE):
    """latent_embedders.py:191-340: VAE's layout (R.VAE) with a single 1x1 out_enc block and the codebook; encode does not quantize (:304-309),
    decode quantizes first (:311-317), forward returns (out, out_hor[::-1], emb_loss) (:319-338)"""

    def __init__(self, in_channels=3, out_channels=3, spatial_dims=2, emb_channels=4, num_embeddings=8192, hid_chs=(32, 64, 128, 256),
                 kernel_sizes=(3, 3, 3, 3), strides=(1, 2, 2, 2), norm_name=GN32, use_res_block=True, deep_supervision=False,
                 learnable_interpolation=True, use_attention="none", beta=0.25, **_ignored):
        super().__init__(in_channels, out_channels, spatial_dims, emb_channels, hid_chs, kernel_sizes, strides, norm_name, use_res_block,
                         deep_supervision, learnable_interpolation, use_attention)
        self.out_enc = R.BasicBlock(list(hid_chs)[-1], emb_channels, 1)
        self.quantizer = VectorQuantizer(num_embeddings, emb_channels, beta)

    def encode(self, x):
        h = self.inc(x)
        for enc in self.encoders:
            h = enc(h)
        return self.out_enc(h)

    def decode(self, z):
        z, _ = self.quantizer(z)
        return super().decode(z)

    def decode_quantized(self, z_q):
        """the decoder after the quantizer: what decode does to a z_q it was handed"""
        return super().decode(z_q)


class VQGAN(nn.Module):
    """latent_embedders.py:408-490 (inference: the discriminator is not built)"""

    def __init__(self, in_channels=3, out_channels=3, spatial_dims=2, emb_channels=4, num_embeddings=8192, hid_chs=(64, 128, 256, 512),
                 kernel_sizes=(3, 3, 3, 3), strides=(1, 2, 2, 2), norm_name=GN32, use_res_block=True, deep_supervision=False,
                 learnable_interpolation=True, use_attention="none", beta=0.25, **_ignored):
        super().__init__()
        self.vqvae = VQVAE(in_channels, out_channels, spatial_dims, emb_channels, num_embeddings, hid_chs, kernel_sizes, strides, norm_name,
                           use_res_block, deep_supervision, learnable_interpolation, use_attention, beta)

    def encode(self, x):
        return self.vqvae.encode(x)

    def decode(self, z):
        return self.vqvae.decode(z)

    def forward(self, x):
        return self.vqvae(x)


class VAEGAN(nn.Module):
    """latent_embedders.py:860-940 (its `vqvae` is a VAE; inference: no discriminator)"""

    def __init__(self, in_channels=3, out_channels=3, spatial_dims=2, emb_channels=4, hid_chs=(64, 128, 256, 512), kernel_sizes=(3, 3, 3, 3),
                 strides=(1, 2, 2, 2), norm_name=("GROUP", {"num_groups": 8, "affine": True}), use_res_block=True, deep_supervision=False,
                 learnable_interpolation=True, use_attention="none", **_ignored):
        super().__init__()
        self.vqvae = R.VAE(in_channels, out_channels, spatial_dims, emb_channels, hid_chs, kernel_sizes, strides, norm_name, use_res_block,
                           deep_supervision, learnable_interpolation, use_attention)

    def encode(self, x):
        return self.vqvae.encode(x)

    def decode(self, z):
        return self.vqvae.decode(z)

    def forward(self, x):
        return self.vqvae(x)


# ----------------------------------------------------------------------------- fixture configs
def tiny_vq_kwargs(hid=(32, 32, 64, 64), num_embeddings=300, emb_channels=4, **extra) -> dict:
    """K = 300: not a multiple of any slice of the kernel; hid 32: one channel per group at 32 groups"""
    kw = dict(in_channels=3, out_channels=3, emb_channels=emb_channels, num_embeddings=num_embeddings, spatial_dims=2, hid_chs=list(hid),
              kernel_sizes=[3, 3, 3, 3], strides=[1, 2, 2, 2], deep_supervision=2, use_attention="none")
    kw.update(extra)
    return kw


def tiny_vaegan_kwargs(hid=(32, 32, 64, 64), emb_channels=4) -> dict:
    return dict(in_channels=3, out_channels=3, emb_channels=emb_channels, spatial_dims=2, hid_chs=list(hid), kernel_sizes=[3, 3, 3, 3],
                strides=[1, 2, 2, 2], deep_supervision=2, use_attention="none")


def margins(dist64: torch.Tensor, zz: torch.Tensor, ee_max: float) -> torch.Tensor:
    """(second-best - best) fp64 distance of every pixel relative to |z|^2 + max |e|^2"""
    two = torch.topk(dist64, 2, dim=1, largest=False).values if dist64.shape[1] > 1 else torch.cat([dist64, dist64 + 1e30], 1)
    return (two[:, 1] - two[:, 0]) / (zz + ee_max)


def exact_margins(z: torch.Tensor, codebook: torch.Tensor) -> torch.Tensor:
    zf = torch.moveaxis(z, 1, -1).reshape(-1, codebook.shape[1]).double()
    e = codebook.double()
    d = ((zf[:, None, :] - e[None, :, :]) ** 2).sum(-1)
    return margins(d, (zf ** 2).sum(1), float((e ** 2).sum(1).max()))
