"""The Inception network of medfusion_amd.inception restated in plain torch (include/medfusion_hip.h "Inception" is the definition), and the shape
lists of its tests.  Everything here runs on the CPU; the resize and the pools are restated operation by operation in fp32, so their results are the
kernels' bits; the convolution with one chain has an exact oracle (fma_chain_conv); the network is restated in a chosen dtype (fp64: the reference;
fp32: the yardstick of the tolerance)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from medfusion_amd import inception as I
from medfusion_amd import lib as L

# (Cin, Cout, (kh, kw), stride, padded, (H, W), N): the convolution alone
CONV_SHAPES = [
    (3, 32, (3, 3), 2, False, (19, 23), 2),
    (80, 192, (3, 3), 1, False, (9, 9), 2),
    (48, 64, (5, 5), 1, True, (7, 7), 2),
    (160, 160, (1, 7), 1, True, (5, 6), 2),
    (160, 160, (7, 1), 1, True, (5, 6), 2),
    (448, 384, (3, 3), 1, True, (1, 1), 2),
    (448, 384, (3, 3), 1, True, (2, 3), 2),
    (384, 384, (1, 3), 1, True, (3, 3), 2),
    (384, 384, (3, 1), 1, True, (3, 3), 2),
    (2048, 1008, (1, 1), 1, False, (1, 1), 2),
    (33, 129, (3, 3), 1, False, (11, 13), 3),
    (64, 192, (3, 3), 1, True, (35, 35), 2),
]
CONV_IDS = [f"{c[0]}to{c[1]}_k{c[2][0]}x{c[2][1]}_s{c[3]}_{'p' if c[4] else 'np'}_{c[5][0]}x{c[5][1]}_n{c[6]}" for c in CONV_SHAPES]

SIDES = {75: (37, 35, 35, 17, 17, 15, 7, 3, 1), 107: (53, 51, 51, 25, 25, 23, 11, 5, 2), 299: (149, 147, 147, 73, 73, 71, 35, 17, 8)}
SIDE_BUFFERS = ("c1a", "c2a", "c2b", "p64", "c3b", "c4a", "p192", "Mixed_6a", "Mixed_7a")
BLOCK_CHANNELS = (256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048)


def conv_case(case, seed=0):
    """seeded normal-range operands of a convolution case: x NHWC, w [KH][KW][Cin][Cout], bias, the padding per axis"""
    cin, cout, (kh, kw), stride, padded, (h, w), n = case
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn((n, h, w, cin), generator=g)
    wt = torch.randn((kh, kw, cin, cout), generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    return x, wt, b, ((kh - 1) // 2 if padded else 0, (kw - 1) // 2 if padded else 0)


def fma32(a, b, c):
    """fp32 fma(a, b, c) of fp32 numpy arrays, exactly (finite data): the product of two fp32 values is exact in fp64; c is added in fp64 with the TwoSum
    error term; where the error is non-zero and the sum's last mantissa bit is even the sum moves one fp64 step toward the error (round to odd: 53 bits
    rounded to odd, then to 24, is one rounding to 24); then round to fp32.  Plain (double) a b + c rounded to fp32 rounds twice and is NOT this."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    odd = (e != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(odd, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def fma_chain_conv(x: torch.Tensor, w: torch.Tensor, pads, stride: int) -> torch.Tensor:
    """The exact oracle of the convolution with one chain: x NHWC, w [KH][KW][Cin][Cout] -> fp32 NHWC, every output ONE fused multiply-add chain from +0
    over k = (kh KW + kw) Cin + cin ascending, padding taps as zeros.  On the CPU, vectorised over the outputs and sequential over K.  The bias is one
    fp32 add on top and ReLU is v < 0 ? 0 : v: derive those from this result."""
    n, h, w_, cin = x.shape
    kh_, kw_, _, cout = w.shape
    ho, wo = (h + 2 * pads[0] - kh_) // stride + 1, (w_ + 2 * pads[1] - kw_) // stride + 1
    xp = np.zeros((n, h + 2 * pads[0], w_ + 2 * pads[1], cin), dtype=np.float32)
    xp[:, pads[0]:pads[0] + h, pads[1]:pads[1] + w_] = x.numpy()
    wn = w.numpy()
    acc = np.zeros((n, ho, wo, cout), dtype=np.float32)
    for kh in range(kh_):
        for kw in range(kw_):
            tap = xp[:, kh:kh + (ho - 1) * stride + 1:stride, kw:kw + (wo - 1) * stride + 1:stride]
            for ci in range(cin):
                acc = fma32(tap[..., ci:ci + 1], wn[kh, kw, ci], acc)
    return torch.from_numpy(acc)


@functools.lru_cache(maxsize=None)
def conv_oracle(case) -> torch.Tensor:
    """fma_chain_conv of conv_case(case) without the bias, computed once per case and never modified"""
    x, w, _, pads = conv_case(case)
    return fma_chain_conv(x, w, pads, case[3])


def prepare_ref(x: torch.Tensor, size: int) -> torch.Tensor:
    """uint8 [B, 1|3, H, W] -> fp32 NHWC [B, size, size, 3]: the TF1-style resize and the value map, every operation rounded to fp32 as written"""
    B, C, H, W = x.shape

    def axis(n_in):
        s = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(size), dtype=torch.float32)
        g = torch.arange(size, dtype=torch.float32) * s
        lo = g.to(torch.int64)
        return lo, torch.clamp(lo + 1, max=n_in - 1), g - lo.to(torch.float32)

    y0, y1, dy = axis(H)
    x0, x1, dx = axis(W)
    v = x.to(torch.float32)
    if C == 1:
        v = v.expand(B, 3, H, W)
    a00, a01 = v[:, :, y0][:, :, :, x0], v[:, :, y0][:, :, :, x1]
    a10, a11 = v[:, :, y1][:, :, :, x0], v[:, :, y1][:, :, :, x1]
    dxr, dyr = dx.view(1, 1, 1, -1), dy.view(1, 1, -1, 1)
    top = a00 + (a01 - a00) * dxr
    bottom = a10 + (a11 - a10) * dxr
    out = top + (bottom - top) * dyr
    return ((out - 128.0) / 128.0).permute(0, 2, 3, 1).contiguous()


def pool_ref(x: torch.Tensor, stride: int, pad: int, mode: int) -> torch.Tensor:
    """the 3 x 3 pool of an NCHW tensor in its own dtype: max = the largest valid tap (a NaN wins); avg = the sum of the valid taps in ascending
    (kh, kw) order divided once by their number (an invalid tap adds an exact zero)"""
    _, _, H, W = x.shape
    Ho, Wo = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
    xp = F.pad(x, (pad, pad, pad, pad), value=float("-inf") if mode == L.POOL_MAX else 0.0)
    ones = F.pad(torch.ones((1, 1, H, W), dtype=x.dtype), (pad, pad, pad, pad))
    acc = cnt = None
    for kh in range(3):
        for kw in range(3):
            sl = (slice(None), slice(None), slice(kh, kh + (Ho - 1) * stride + 1, stride), slice(kw, kw + (Wo - 1) * stride + 1, stride))
            tap = xp[sl]
            if mode == L.POOL_MAX:
                acc = tap if acc is None else torch.maximum(acc, tap)
            else:
                acc = tap if acc is None else acc + tap
                cnt = ones[sl] if cnt is None else cnt + ones[sl]
    return acc if mode == L.POOL_MAX else acc / cnt


def forward_ref(net: I.InceptionNet, x: torch.Tensor, size: int, dtype=torch.float64) -> dict:
    """the six taps of the network on the CPU in `dtype`: the fp32 resize, then the folded convolutions (F.conv2d), the pools above, the pixel means and
    the fc -- {"64", "192", "768", "2048", "logits_unbiased", "logits"} -> [B, D] in `dtype`"""
    shape = I.trace(size)
    B = x.shape[0]
    bufs = {"in": prepare_ref(x, size).permute(0, 3, 1, 2).to(dtype)}
    out = {}
    for op in I.OPS:
        if op[0] == "tap":
            out[op[1]] = bufs[op[2]].mean(dim=(2, 3))
            continue
        dst = op[3] if op[0] == "conv" else op[2]
        if dst not in bufs:
            h, w, c = shape[dst]
            bufs[dst] = torch.empty((B, c, h, w), dtype=dtype)
        if op[0] == "conv":
            _, _, cout, _, _, s, ph, pw = I.LAYERS[op[1]]
            wf, bf = net.folded(op[1])
            bufs[dst][:, op[4]:op[4] + cout] = torch.relu(F.conv2d(bufs[op[2]], wf.to(dtype), bf.to(dtype), stride=s, padding=(ph, pw)))
        else:
            src = bufs[op[1]]
            bufs[dst][:, op[6]:op[6] + src.shape[1]] = pool_ref(src, op[3], op[4], op[5])
    out["logits_unbiased"] = out["2048"] @ net.state["fc.weight"].to(dtype).t()
    out["logits"] = out["logits_unbiased"] + net.state["fc.bias"].to(dtype)
    return out


def images(B: int, C: int, H: int, W: int, seed: int) -> torch.Tensor:
    """uint8 noise, the last image a smooth one"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (B, C, H, W), generator=g, dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    smooth = (127.5 + 127.5 * torch.sin(6.0 * xx + 2.0) * torch.cos(4.0 * yy)).round().clamp(0, 255).to(torch.uint8)
    x[-1] = smooth.expand(C, H, W)
    return x
