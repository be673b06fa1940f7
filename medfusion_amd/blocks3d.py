"""The 3-D building blocks (spatial_dims=3) of the UNet and the VAE on the HIP kernels: host-side mirror of the reference's
medical_diffusion/models/utils/conv_blocks.py at spatial_dims=3 (MONAI Conv[CONV, 3], get_padding per axis).  Same class names, constructor
meaning and state-dict keys as the 2-D classes of blocks.py, with 5-D (OIDHW) convolution weights.

An activation is an NDHWC fp32 tensor held as its [N, D*H, W, C] view, tagged with its spatial size (`_mf_dhw`): every per-voxel kernel of the
2-D path -- GroupNorm statistics and apply, Swish, residual and embedding adds, the fp16-pair split, layout changes -- runs on that view
unchanged.  The convolutions (3x3x3 and 1x1x1, strided, nearest-x2 upsampled, with the fused two-source concat of the UNet out-blocks) go
to mf_conv3d_f16x2 (csrc/conv3d.hip).  Only the default arithmetic MF_CONV_FP32_F16X2 is built in 3-D; a forward on any other
blocks.CONV_PRECISION raises.  A forward makes no torch device op: every launch goes through the library (the command-list and hipGraph
loops of pipeline.py record them).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import blocks as BLK
from . import kernels as K
from .blocks import Attention, GroupNorm, _norm, _split, zero_module  # noqa: F401  (GroupNorm: re-exported for the model modules)


def _triple(v) -> Tuple[int, int, int]:
    if isinstance(v, (tuple, list)):
        if len(v) != 3:
            raise ValueError(f"expected 3 values per axis, got {v!r}")
        return tuple(int(a) for a in v)
    return (int(v),) * 3


def monai_padding3(kernel_size, stride) -> Tuple[int, int, int]:
    """MONAI get_padding per axis: int((k - s + 1) / 2)"""
    out = []
    for k, s in zip(_triple(kernel_size), _triple(stride)):
        p = (k - s + 1) / 2
        if p < 0:
            raise AssertionError("padding value should not be negative")
        out.append(int(p))
    return tuple(out)


def dims(x) -> Tuple[int, int, int]:
    """(D, H, W) of an activation of the 3-D path"""
    d = getattr(_split(x)[0], "_mf_dhw", None)
    if d is None:
        raise RuntimeError("medfusion_amd.blocks3d: the input is not an activation of the 3-D path (no spatial size attached)")
    return d


def tag(t: torch.Tensor, dhw) -> torch.Tensor:
    t._mf_dhw = tuple(int(a) for a in dhw)
    return t


def from_ncdhw(x: torch.Tensor, cp: int = 32) -> torch.Tensor:
    """NCDHW network input -> its operand: [N, D*H, W, cp] fp16 pairs (channels C.. zero), no fp32 form (mf_pack_nchw_pairs_f32)"""
    n, c, d, h, w = x.shape
    return tag(K.pack_nchw_pairs(x.contiguous().view(n, c, d * h, w), cp), (d, h, w))


def to_ncdhw(y: torch.Tensor) -> torch.Tensor:
    d, h, w = dims(y)
    n, c = y.shape[0], y.shape[-1]
    return K.nhwc_to_nchw(y.view(n, d * h, w, c)).view(n, c, d, h, w)


def _require_f16x2():
    if BLK.CONV_PRECISION != 5:
        raise NotImplementedError(f"blocks.CONV_PRECISION = {BLK.CONV_PRECISION}: the 3-D path is built on the fp16-pair arithmetic "
                                  "MF_CONV_FP32_F16X2 (5) only")


class Conv3d(nn.Module):
    """Parameter holder + launcher of one 3-D convolution (nn.Conv3d replacement, keys weight / bias, OIDHW).  k in {1, 3} on every axis."""

    def __init__(self, in_ch, out_ch, kernel_size, stride=1, padding=0, upsample=0):
        super().__init__()
        ks = _triple(kernel_size)
        if len(set(ks)) != 1 or ks[0] not in (1, 3):
            raise NotImplementedError(f"kernel_size={kernel_size}: the 3-D convolution is built for 1 or 3 on every axis")
        holder = nn.Conv3d(in_ch, out_ch, ks, _triple(stride), _triple(padding), bias=True)
        self.weight, self.bias = holder.weight, holder.bias
        self.in_ch, self.out_ch, self.k = in_ch, out_ch, ks[0]
        self.stride, self.pad, self.upsample = _triple(stride), _triple(padding), _triple(upsample)
        self._wkey, self._wh = None, None
        self._descs = {}

    def _weights(self, cin_pad: int):
        key = (self.weight.data_ptr(), self.weight._version, self.weight.device, cin_pad)
        if key != self._wkey:   # load-time packing + split (one host sync), redone when the parameter changes
            self._wh = K.split_weight_f16x2(K.pack_conv3d_weight(self.weight.detach(), cin_pad))
            self._wkey = key
        return self._wh

    def out_dims(self, dhw):
        return tuple((d * (2 if u else 1) + 2 * p - self.k) // s + 1 for d, u, p, s in zip(dhw, self.upsample, self.pad, self.stride))

    def forward(self, x) -> torch.Tensor:
        """x: an activation [N, D*H, W, C] (or a pair (h, skip): the channel concat fused into the gather) -> y fp32 [N, Do*Ho, Wo, Cout]"""
        _require_f16x2()
        x1, x2 = _split(x)
        dhw = dims(x1)
        n, c1 = x1.shape[0], x1.shape[-1]
        c2 = 0 if x2 is None else x2.shape[-1]
        if x2 is not None and dims(x2) != dhw:
            raise RuntimeError(f"conv3d: the two sources differ in size: {dhw} vs {dims(x2)}")
        cin = self.in_ch
        if c1 + c2 != cin:
            # the padded pair operand of a network input (from_ncdhw) carries zero channels up to a whole chunk
            if not (x2 is None and c1 % 32 == 0 and K.pairs_only(x1) and cin < c1):
                raise RuntimeError(f"conv3d expects {cin} input channels, got {c1}+{c2}")
        elif c1 % 32 or c2 % 32:
            if x2 is not None:
                raise NotImplementedError(f"conv3d: a fused concat of {c1} + {c2} channels (each source must be whole 32-channel chunks)")
            x1 = from_ncdhw(to_ncdhw(x1), -(-c1 // 32) * 32)   # (a narrow tensor inside the network: the padded operand, two small passes)
            c1 = x1.shape[-1]
        key = (n, dhw, c1, c2)
        d = self._descs.get(key)
        if d is None:
            d = K.make_conv3d_desc(n, *dhw, c1, c2, self.out_ch, self.k, self.stride, self.pad, self.upsample)
            if not K.conv3d_ok(d):
                raise RuntimeError(f"conv3d: shape not supported by mf_conv3d_f16x2: N={n} DHW={dhw} C={c1}+{c2} Cout={self.out_ch}")
            d.tile_hint, d.splitk_hint = K.conv3d_plan(d)    # pinned: per-launch planning is a field read
            self._descs[key] = d
        do, ho, wo = self.out_dims(dhw)
        out = torch.empty((n, do * ho, wo, self.out_ch), dtype=torch.float32, device=x1.device)
        K.conv3d_f16x2(x1, self._weights(c1 + c2), self.bias, d, x2=x2, out=out)
        return tag(out, (do, ho, wo))


def _apply(y, norm, act: bool, residual=None, emb=None, emb_stride=0):
    """GroupNorm (statistics on the flattened view) -> Swish -> + residual -> + embedding, one apply pass writing fp32 and the pair mirror"""
    dhw = dims(y)
    if norm is not None:
        G = norm.num_groups
        partial, parts = K.gn_stats_partial(y, G)
        bc = norm.bound_const(dhw[0] * dhw[1] * dhw[2] * (y.shape[-1] // G))
        out = K.gn_apply(y, K.GnPartials(partial, parts, norm.eps), norm.weight, norm.bias, G, int(act), residual, emb, emb_stride, out=y,
                         split=True, bconst=bc)
    elif act or residual is not None or emb is not None:
        out = K.gn_apply(y, None, None, None, 1, int(act), residual, emb, emb_stride, out=y)
    else:
        return y
    return tag(out, dhw)


class BasicBlock(nn.Module):
    """conv -> GroupNorm -> (Dropout: identity at inference) -> Swish.  conv_blocks.py:134-192 at spatial_dims=3."""

    def __init__(self, spatial_dims, in_channels, out_channels, kernel_size, stride=1, norm_name=None, act_name=None, dropout=None,
                 zero_conv=False):
        super().__init__()
        assert spatial_dims == 3
        conv = Conv3d(in_channels, out_channels, kernel_size, stride, monai_padding3(kernel_size, stride))
        self.conv = zero_module(conv) if zero_conv else conv
        if norm_name is not None:
            self.norm = _norm(norm_name, out_channels)
        self.has_act = act_name is not None

    def forward(self, x, residual=None, emb=None, emb_stride=0):
        return _apply(self.conv(x), getattr(self, "norm", None), self.has_act, residual, emb, emb_stride)


class BasicResBlock(nn.Module):
    """BasicBlock(x) + (conv1x1x1(x) if Cin != Cout else x).  conv_blocks.py:194-240 at spatial_dims=3."""

    def __init__(self, spatial_dims, in_channels, out_channels, kernel_size, stride=1, norm_name=None, act_name=None, dropout=None,
                 zero_conv=False):
        super().__init__()
        self.basic_block = BasicBlock(spatial_dims, in_channels, out_channels, kernel_size, stride, norm_name, act_name, dropout, zero_conv)
        self.conv_res = Conv3d(in_channels, out_channels, 1, stride, monai_padding3(1, stride)) if in_channels != out_channels else nn.Identity()

    def forward(self, x, emb=None, emb_stride=0):
        if isinstance(self.conv_res, nn.Identity):
            if isinstance(x, (tuple, list)):
                raise RuntimeError("identity residual needs a single input")
            return self.basic_block(x, residual=x, emb=emb, emb_stride=emb_stride)
        return self.basic_block(x, residual=self.conv_res(x), emb=emb, emb_stride=emb_stride)


class _EmbBlock(nn.Module):
    BlockCls = None
    emb_after_last = False

    def __init__(self, spatial_dims, in_channels, out_channels, kernel_size, stride=1, norm_name=None, act_name=None, dropout=None,
                 emb_channels=None, blocks=2):
        super().__init__()
        self.out_channels = out_channels
        self.block_seq = nn.ModuleList([
            self.BlockCls(spatial_dims, in_channels if i == 0 else out_channels, out_channels, kernel_size, stride, norm_name, act_name,
                          dropout, i == blocks - 1)
            for i in range(blocks)])
        if emb_channels is not None:
            self.local_embedder = nn.Sequential(nn.Identity(), nn.Linear(emb_channels, out_channels))

    def forward(self, x, emb: Optional[torch.Tensor] = None, out_fp32: bool = True):
        """`emb`: the block's local embedding [B, Cout] (already through Swish -> Linear), possibly a strided view into a wider matrix"""
        n = len(self.block_seq)
        last = n if self.emb_after_last else n - 1
        for i, blk in enumerate(self.block_seq):
            e = emb if (emb is not None and i < last) else None
            x = blk(x, emb=e, emb_stride=e.stride(0) if e is not None else 0)
        return x

    def local_embed(self, emb: torch.Tensor) -> torch.Tensor:
        lin = self.local_embedder[1]
        return K.linear(emb, lin.weight, lin.bias, act_in=True)


class UnetResBlock(_EmbBlock):
    """conv_blocks.py:305-364"""
    BlockCls = BasicResBlock
    emb_after_last = False


class UnetBasicBlock(_EmbBlock):
    """conv_blocks.py:244-302"""
    BlockCls = BasicBlock
    emb_after_last = True


class BasicDown(nn.Module):
    """conv_blocks.py:28-70: the strided 3x3x3 convolution (key `down_op.*`); stride 2 or per axis, e.g. (1, 2, 2)"""

    def __init__(self, spatial_dims, in_channels, out_channels, kernel_size=3, stride=2, learnable_interpolation=True, use_res=False):
        super().__init__()
        if not learnable_interpolation:
            raise NotImplementedError("BasicDown(learnable_interpolation=False) is not built in 3-D")
        if use_res:
            raise NotImplementedError("BasicDown(use_res=True): PixelUnshuffle is 2-D only")
        self.learnable, self.use_res = True, False
        self.down_op = Conv3d(in_channels, out_channels, kernel_size, stride, monai_padding3(kernel_size, stride))

    def forward(self, x, emb=None):
        return self.down_op(x)


class BasicUp(nn.Module):
    """conv_blocks.py:72-131: nearest x2 per axis where the stride is 2 (F.interpolate to (x - 1) s + k - 2 get_padding(k, s) = x s for k = s),
    then the 3x3x3 convolution (key `up_op.*`) -- the resize folded into the convolution's gather"""

    def __init__(self, spatial_dims, in_channels, out_channels, kernel_size=2, stride=2, learnable_interpolation=True, use_res=False):
        super().__init__()
        ks, st = _triple(kernel_size), _triple(stride)
        if ks != st or any(s not in (1, 2) for s in st):
            raise NotImplementedError(f"BasicUp(kernel_size={kernel_size}, stride={stride}): only x1 / x2 per axis with kernel_size == stride")
        if not learnable_interpolation:
            raise NotImplementedError("BasicUp(learnable_interpolation=False) is not built in 3-D")
        if use_res:
            raise NotImplementedError("BasicUp(use_res=True): PixelShuffle is 2-D only (in the reference too)")
        self.learnable, self.use_res = True, False
        self.up_op = Conv3d(in_channels, out_channels, 3, 1, 1, upsample=tuple(1 if s == 2 else 0 for s in st))

    def forward(self, x, emb=None):
        return self.up_op(x)


class UnetOutBlock(nn.Module):
    """MONAI UnetOutBlock: 1x1x1 conv, keys `.conv.conv.{weight,bias}`; returns the fp32 activation (to_ncdhw for the network output)"""

    def __init__(self, spatial_dims, in_channels, out_channels, dropout=None):
        super().__init__()
        inner = nn.Sequential()
        inner.add_module("conv", Conv3d(in_channels, out_channels, 1, 1, 0))
        self.conv = inner

    def forward(self, x):
        return self.conv.conv(x)


def _no_attention(use_attention):
    if use_attention != "none":
        raise NotImplementedError(f"use_attention={use_attention!r}: attention is not built in 3-D")


class DownBlock(nn.Module):
    """VAE encoder stage (conv_blocks.py:368-441) at spatial_dims=3"""

    def __init__(self, spatial_dims, in_channels, out_channels, kernel_size, stride, downsample_kernel_size, norm_name, act_name, dropout=None,
                 use_res_block=False, learnable_interpolation=True, use_attention="none", emb_channels=None):
        super().__init__()
        _no_attention(use_attention)
        enable_down = _triple(stride) != (1, 1, 1)
        down_out = out_channels if learnable_interpolation and enable_down else in_channels
        self.down_op = BasicDown(spatial_dims, in_channels, out_channels, downsample_kernel_size, stride, learnable_interpolation) if enable_down else nn.Identity()
        self.attention = Attention(spatial_dims, down_out, down_out, 8, down_out // 8, norm_name, dropout, emb_channels, 1, "none")
        Blk = UnetResBlock if use_res_block else UnetBasicBlock
        self.conv_block = Blk(spatial_dims, down_out, out_channels, kernel_size, 1, norm_name, act_name, dropout, emb_channels)

    def forward(self, x, emb=None):
        return self.conv_block(self.down_op(x), None)


class UpBlock(nn.Module):
    """VAE decoder stage (conv_blocks.py:444-528) at spatial_dims=3, without a skip input (the VAE passes none)"""

    def __init__(self, spatial_dims, in_channels, out_channels, kernel_size, stride, upsample_kernel_size, norm_name, act_name, dropout=None,
                 use_res_block=False, learnable_interpolation=True, use_attention="none", emb_channels=None, skip_channels=0):
        super().__init__()
        _no_attention(use_attention)
        if skip_channels:
            raise NotImplementedError("UpBlock(skip_channels > 0) is not built in 3-D")
        enable_up = _triple(stride) != (1, 1, 1)
        skip_out = out_channels if learnable_interpolation and enable_up else in_channels + skip_channels
        self.learnable_interpolation = bool(learnable_interpolation)
        self.up_op = BasicUp(spatial_dims, in_channels, out_channels, upsample_kernel_size, stride, learnable_interpolation) if enable_up else nn.Identity()
        self.attention = Attention(spatial_dims, skip_out, skip_out, 8, skip_out // 8, norm_name, dropout, emb_channels, 1, "none")
        Blk = UnetResBlock if use_res_block else UnetBasicBlock
        self.conv_block = Blk(spatial_dims, skip_out, out_channels, kernel_size, 1, norm_name, act_name, dropout, emb_channels)

    def forward(self, x_enc, x_skip=None, emb=None):
        if x_skip is not None:
            raise NotImplementedError("UpBlock with a skip input is not built in 3-D")
        return self.conv_block(self.up_op(x_enc), None)
