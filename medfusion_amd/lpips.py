"""LPIPS v0.1 on the device: the VGG16 / AlexNet trunks from user-supplied weights and the learned distance on top (csrc/lpips.hip, the plain layers
of csrc/cnn_layers.hip, include/medfusion_hip.h "LPIPS"; README "LPIPS" has the definition).

Nothing pretrained is shipped or fetched.  LPIPSNet.from_files takes the two files anyone who trained with the reference has on disk -- the
torchvision trunk state dict and the lpips package's linear-layer file --, LPIPSNet.seeded draws weights for tests and the benchmark.

The first convolution of both trunks (Cin = 3) and AlexNet's 5 x 5 run on mf_conv2d_direct_f32 (the general fp32 matrix-core convolution
of cnn_layers.hip with one fma chain per output, the one the Inception trunk runs; bias and ReLU fused; no bit depends on the tile it plans); every
other 3 x 3 layer runs on the implicit-GEMM convolution mf_conv2d_f32 in one of its fp32-class arithmetics -- chosen HERE, per net, never through
blocks.CONV_PRECISION -- followed by mf_relu_f32.  The tile and the split of the K loop of those layers are pinned by rules that look at the layer
only, never at the batch, so a pair's bits do not depend on how many pairs travel with it: chunk=1 gives the bits of chunk=None.

lpips() returns device tensors, never waits for the device and draws nothing.  Inputs are fp32 [B, C, H, W] or [B, C, D, H, W] tensors on the GPU
with C in {1, 3}; anything else is a ValueError that names the argument, raised before anything touches the device."""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import kernels as K
from . import lib as L

MIN_SIDE = {"vgg": 16, "alex": 31}
NET_ID = {"vgg": L.LPIPS_VGG, "alex": L.LPIPS_ALEX}
ARITHMETICS = {"split3": 3, "fp32": 0}      # MF_CONV_FP32_SPLIT3_W3 (default), MF_CONV_FP32
PIXEL_BUDGET = 1 << 20                       # full-resolution pixels of x per trunk pass when chunk is None: 16 pairs of 256 x 256


def _vgg_ops():
    ops, cin, idx = [], 3, 0
    for block, (width, n) in enumerate(((64, 2), (128, 2), (256, 3), (512, 3), (512, 3))):
        if block:
            ops.append(("pool", 2, 2))
            idx += 1
        for _ in range(n):
            ops.append(("conv", idx, cin, width, 3, 1, 1))
            cin = width
            idx += 2
        ops.append(("tap",))
    return ops


# ("conv", state-dict index, Cin, Cout, k, stride, pad) -- always with bias and ReLU --, ("pool", k, stride), ("tap",)
OPS = {
    "vgg": _vgg_ops(),
    "alex": [("conv", 0, 3, 64, 11, 4, 2), ("tap",), ("pool", 3, 2), ("conv", 3, 64, 192, 5, 1, 2), ("tap",), ("pool", 3, 2),
             ("conv", 6, 192, 384, 3, 1, 1), ("tap",), ("conv", 8, 384, 256, 3, 1, 1), ("tap",), ("conv", 10, 256, 256, 3, 1, 1), ("tap",)],
}
TAP_CHANNELS = {"vgg": (64, 128, 256, 512, 512), "alex": (64, 192, 384, 256, 256)}


def _check_net_name(net) -> str:
    if not isinstance(net, str) or net not in OPS:
        raise ValueError(f"net: 'vgg' or 'alex', got {net!r}")
    return net


# Chunks of 32 products one accumulation chain of a 3 x 3 layer holds at most; the chains of a layer are added by the convolution's split-K reduction.
# The planner's own rule (csrc/conv.hip) lets a chain grow to 96 chunks; LPIPS compares features through up to thirteen layers, and measured against
# the fp64 restatement the terms of the deep VGG taps then sit at 0.9 (bf16 triplets) and 1.6 (fp32 MFMA) of the tests' bound.  The fp32-MFMA figure
# falls with the chain length (0.8 at 32 chunks, 0.4 at 16, 0.3 at 4); the bf16-triplet one scatters between 0.3 and 1.0 and was lowest at 16
# (README "LPIPS" has the table).  At 16 the layers of 64 / 128 / 256 / 512 input channels run 2 / 3 / 5 / 9 chains.
CHAIN_CHUNKS = 16


def _splitk(cin: int) -> int:
    """in how many chains the K loop of a 3 x 3 layer of `cin` channels runs: a rule of the layer alone"""
    return -(-9 * (cin // 32) // CHAIN_CHUNKS)


def _igemm_desc(N: int, H: int, W: int, cin: int, cout: int, precision: int) -> L.MfConvDesc:
    """the 3 x 3 pad-1 layer on mf_conv2d_f32 with its plan pinned by the layer alone: the 128 x 128 tile where Cout allows, else 64 x 64; the K loop
    split so that one accumulation chain holds at most CHAIN_CHUNKS chunks"""
    return K.make_conv_desc(N, H, W, cin, 0, cout, 3, 1, 1, tile_hint=8 if cout % 128 == 0 else 4, splitk_hint=_splitk(cin), precision=precision)


def _on_igemm(cin: int, cout: int, k: int, stride: int, pad: int, precision: int) -> bool:
    """does mf_conv2d_f32 take this layer on its implicit-GEMM kernel (asked of the library: host logic, no device)?  Everything else is the direct kernel's"""
    if (k, stride, pad) != (3, 1, 1) or cin % 32 or cout % 64:
        return False
    return K.conv_is_igemm(_igemm_desc(2, 8, 8, cin, cout, precision))


def plan(net: str, H: int, W: int, arithmetic: str = "split3") -> dict:
    """Host only: what one pair of H x W images costs on `net` -- the layers with the kernel that takes each, the tap sizes, the launches and the bytes
    of the distance workspace.  {"layers": [...], "taps": [(h, w, c), ...], "launches": n, "workspace_bytes": n, "activation_bytes": n (the largest
    layer output of the 2-image batch)}"""
    net = _check_net_name(net)
    if arithmetic not in ARITHMETICS:
        raise ValueError(f"arithmetic: one of {sorted(ARITHMETICS)}, got {arithmetic!r}")
    for name, v in (("H", H), ("W", W)):
        if not isinstance(v, int) or v < MIN_SIDE[net]:
            raise ValueError(f"{name}: sides of at least {MIN_SIDE[net]} for net {net!r}, got {v!r}")
    lib = L.load()
    prec = ARITHMETICS[arithmetic]
    h, w, c = H, W, 3
    layers, taps, launches, ws, act = [{"op": "prepare", "kernel": "mf_lpips_prepare_f32", "out": (h, w, c)}], [], 1, 0, 2 * h * w * 3 * 4
    for op in OPS[net]:
        if op[0] == "conv":
            _, idx, cin, cout, k, s, p = op
            ig = _on_igemm(cin, cout, k, s, p, prec)
            h, w, c = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1, cout
            split = _splitk(cin) if ig else 1
            layers.append({"op": "conv", "key": f"features.{idx}", "kernel": "mf_conv2d_f32" if ig else "mf_conv2d_direct_f32", "k": k, "stride": s, "pad": p,
                           "cin": cin, "cout": cout, "out": (h, w, c), "splitk": split})
            launches += (2 + (split > 1)) if ig else 1       # implicit GEMM (+ its split-K reduction) + ReLU; the direct kernel fuses bias and ReLU
        elif op[0] == "pool":
            h, w = (h - op[1]) // op[2] + 1, (w - op[1]) // op[2] + 1
            layers.append({"op": "pool", "kernel": "mf_maxpool_nhwc_f32", "k": op[1], "stride": op[2], "out": (h, w, c)})
            launches += 1
        else:
            taps.append((h, w, c))
            ws = max(ws, int(lib.mf_lpips_workspace_bytes(1, h * w)))
            launches += 2
        act = max(act, 2 * h * w * c * 4)
    return {"net": net, "arithmetic": arithmetic, "layers": layers, "taps": taps, "launches": launches, "workspace_bytes": ws, "activation_bytes": act}


class LPIPSNet:
    """The weights of one LPIPS net: the trunk's convolutions (OIHW fp32 + bias) and the five linear-layer vectors, on the host until .to(device);
    the packed / split device copies are derived once per device and arithmetic (the way blocks._Packed does it for a module's weights)."""

    def __init__(self, net: str, convs, lins, arithmetic: str = "split3"):
        self.net = _check_net_name(net)
        if arithmetic not in ARITHMETICS:
            raise ValueError(f"arithmetic: one of {sorted(ARITHMETICS)}, got {arithmetic!r}")
        self.arithmetic = arithmetic
        self.convs, self.lins = list(convs), list(lins)
        self._dev = {}

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_state(cls, trunk_state, lin_state, net: str, arithmetic: str = "split3") -> "LPIPSNet":
        """trunk_state: the torchvision state dict (features.N.weight / .bias; classifier.* ignored); lin_state: the lpips package's
        (lin{l}.model.1.weight, [1, C_l, 1, 1]).  A missing or mis-shaped tensor is a ValueError naming the key."""
        net = _check_net_name(net)

        def take(state, key, shape, what):
            if not hasattr(state, "keys") or key not in state:
                raise ValueError(f"{what}: key {key!r} is missing")
            t = state[key]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
                raise ValueError(f"{what}: key {key!r} must be a tensor of shape {tuple(shape)}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            return t.detach().to("cpu", torch.float32).contiguous().clone()

        convs = []
        for op in OPS[net]:
            if op[0] == "conv":
                _, idx, cin, cout, k, _, _ = op
                convs.append((take(trunk_state, f"features.{idx}.weight", (cout, cin, k, k), "trunk_state"), take(trunk_state, f"features.{idx}.bias", (cout,), "trunk_state")))
        lins = [take(lin_state, f"lin{l}.model.1.weight", (1, c, 1, 1), "lin_state").reshape(c) for l, c in enumerate(TAP_CHANNELS[net])]
        return cls(net, convs, lins, arithmetic)

    @classmethod
    def from_files(cls, trunk_path, lin_path, net: str = "vgg", arithmetic: str = "split3") -> "LPIPSNet":
        trunk = torch.load(str(trunk_path), map_location="cpu", weights_only=True)
        lin = torch.load(str(lin_path), map_location="cpu", weights_only=True)
        return cls.from_state(trunk, lin, net, arithmetic)

    @classmethod
    def seeded(cls, net: str, seed: int, bias_std: float = 0.0, arithmetic: str = "split3") -> "LPIPSNet":
        """Weights for tests and the benchmark from ONE torch.Generator on the CPU, in fp64, rounded to fp32, in trunk order: per convolution the weight
        N(0, 2 / fan_in), then the bias N(0, bias_std^2); then the five linear vectors, uniform in [0, 8 / C_l)."""
        net = _check_net_name(net)
        g = torch.Generator(device="cpu").manual_seed(int(seed))
        convs = []
        for op in OPS[net]:
            if op[0] == "conv":
                _, _, cin, cout, k, _, _ = op
                w = torch.randn((cout, cin, k, k), generator=g, dtype=torch.float64) * math.sqrt(2.0 / (cin * k * k))
                b = torch.randn((cout,), generator=g, dtype=torch.float64) * float(bias_std)
                convs.append((w.float(), b.float()))
        lins = [(torch.rand((c,), generator=g, dtype=torch.float64) * (8.0 / c)).float() for c in TAP_CHANNELS[net]]
        return cls(net, convs, lins, arithmetic)

    # ------------------------------------------------------------------ state
    def state_dicts(self):
        """(trunk_state, lin_state) under the torchvision / lpips key names: what from_state and from_files read"""
        trunk, i = {}, 0
        for op in OPS[self.net]:
            if op[0] == "conv":
                trunk[f"features.{op[1]}.weight"], trunk[f"features.{op[1]}.bias"] = self.convs[i]
                i += 1
        lin = {f"lin{l}.model.1.weight": v.reshape(1, -1, 1, 1) for l, v in enumerate(self.lins)}
        return trunk, lin

    def with_arithmetic(self, arithmetic: str) -> "LPIPSNet":
        """the same weights on the other arithmetic of the 3 x 3 layers"""
        return LPIPSNet(self.net, self.convs, self.lins, arithmetic)

    def to(self, device) -> "LPIPSNet":
        self._on(torch.device(device))
        return self

    def _on(self, device: torch.device):
        """the device copies: per convolution (kind, weights, bias, op) with kind "direct" ([KH][KW][Cin][Cout]) or "igemm" (packed; split for split3)"""
        if device.type != "cuda":
            raise RuntimeError("medfusion_amd: LPIPS runs on a ROCm device -- there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        ent = self._dev.get(device)
        if ent is None:
            prec = ARITHMETICS[self.arithmetic]
            convs, i = [], 0
            for op in OPS[self.net]:
                if op[0] != "conv":
                    continue
                _, _, cin, cout, k, s, p = op
                w, b = (t.to(device) for t in self.convs[i])
                i += 1
                if _on_igemm(cin, cout, k, s, p, prec):
                    wp = K.pack_conv_weight(w)
                    convs.append(("igemm", K.split_conv_weight(wp) if prec == 3 else wp, b))
                else:
                    convs.append(("direct", K.pack_direct_conv_weight(w), b))
            ent = self._dev[device] = (convs, [v.to(device) for v in self.lins])
        return ent


def _check_inputs(x, y, net, chunk):
    if not isinstance(net, LPIPSNet):
        raise ValueError(f"net: an LPIPSNet (LPIPSNet.from_files / from_state / seeded), got {type(net).__name__}")
    for name, t in (("x", x), ("y", y)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: a tensor, got {type(t).__name__}")
        if t.dim() not in (4, 5) or any(s == 0 for s in t.shape):
            raise ValueError(f"{name}: a non-empty [B, C, H, W] or [B, C, D, H, W] tensor, got shape {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: fp32, got {t.dtype}")
    if y.shape != x.shape:
        raise ValueError(f"y: of the shape of x {tuple(x.shape)}, got {tuple(y.shape)}")
    if x.shape[1] not in (1, 3):
        raise ValueError(f"x: 1 or 3 channels, got {x.shape[1]} (shape {tuple(x.shape)})")
    if min(x.shape[-2:]) < MIN_SIDE[net.net]:
        raise ValueError(f"x: net {net.net!r} needs sides of at least {MIN_SIDE[net.net]}, got {x.shape[-2]} x {x.shape[-1]}")
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1):
        raise ValueError(f"chunk: None or a positive number of pairs per trunk pass, got {chunk!r}")
    for name, t in (("x", x), ("y", y)):
        if not t.is_cuda:
            raise ValueError(f"{name}: on a ROCm device -- LPIPS has no CPU path, got a {t.device.type} tensor")
    if y.device != x.device:
        raise ValueError("y: on the device of x")


def _trunk_pass(x, y, net: LPIPSNet, normalize: bool, terms, total) -> None:
    """one pass of b pairs: scaling layer, trunk over the 2b rows, the five distances into terms [b, 5] / total [b]"""
    convs, lins = net._on(x.device)
    prec = ARITHMETICS[net.arithmetic]
    b = x.shape[0]
    h = K.lpips_prepare(x, y, normalize, NET_ID[net.net])
    ci = tap = 0
    for op in OPS[net.net]:
        if op[0] == "conv":
            _, _, cin, cout, k, s, p = op
            kind, w, bias = convs[ci]
            ci += 1
            n, hh, ww, _ = h.shape
            if kind == "direct":
                h = K.conv2d_direct(h, w, bias, K.make_direct_conv_desc(n, hh, ww, cin, cout, k, k, s, p, relu=True))
            else:
                h = K.relu_(K.conv2d(h, w, bias, _igemm_desc(n, hh, ww, cin, cout, prec)))
        elif op[0] == "pool":
            h = K.maxpool_nhwc(h, op[1], op[2])
        else:
            K.lpips_layer(h[:b], h[b:], lins[tap], terms, tap, total if tap == len(lins) - 1 else None)
            tap += 1


@torch.no_grad()
def lpips(x: torch.Tensor, y: torch.Tensor, net: LPIPSNet, *, normalize: bool = False, return_terms: bool = False, chunk: Optional[int] = None):
    """LPIPS of the pairs (x[b], y[b]) -> [B] fp32 (and the per-layer terms [B, 5] fp32 with return_terms).  x, y in [-1, 1], or in [0, 1] with
    normalize.  5-D input [B, C, D, H, W]: the mean over d of the 2-D value of slice d.  `chunk`: pairs per trunk pass (None: as many as keep the
    full-resolution activations of a pass at PIXEL_BUDGET pixels of x); the bits do not depend on it."""
    _check_inputs(x, y, net, chunk)
    depth = None
    if x.dim() == 5:
        B, Cc, depth, H, W = x.shape
        x, y = (t.permute(0, 2, 1, 3, 4).reshape(B * depth, Cc, H, W) for t in (x, y))
    x, y = x.contiguous(), y.contiguous()
    n, _, H, W = x.shape
    step = chunk if chunk is not None else max(1, PIXEL_BUDGET // (H * W))
    terms = torch.empty((n, 5), dtype=torch.float64, device=x.device)
    total = torch.empty((n,), dtype=torch.float32, device=x.device)
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        _trunk_pass(x[lo:hi], y[lo:hi], net, normalize, terms[lo:hi], total[lo:hi])
    if depth is not None:        # the reference's wrapper: the mean over the slices (D values per volume: host-side plumbing in fp64)
        terms = terms.view(-1, depth, 5).mean(dim=1)
        total = total.view(-1, depth).double().mean(dim=1).float()
    return (total, terms.float()) if return_terms else total


def add_lpips_arguments(ap) -> None:
    """--lpips-net / --lpips-trunk / --lpips-lin of the evaluation scripts: all three or none"""
    ap.add_argument("--lpips-net", default=None, choices=sorted(OPS), help="also LPIPS of the reconstructions on this trunk (torchmetrics' default, the reference script's: alex)")
    ap.add_argument("--lpips-trunk", default=None, help="the torchvision state dict of the trunk (vgg16 / alexnet), a file on disk")
    ap.add_argument("--lpips-lin", default=None, help="the lpips package's linear-layer file of that trunk (weights/v0.1/vgg.pth / alex.pth)")


def net_from_args(args, error) -> Optional[LPIPSNet]:
    """the LPIPSNet the three flags name, or None without them; `error`: the parser's error function (given some of the three only)"""
    given = [v is not None for v in (args.lpips_net, args.lpips_trunk, args.lpips_lin)]
    if not any(given):
        return None
    if not all(given):
        error("--lpips-net, --lpips-trunk and --lpips-lin go together")
    return LPIPSNet.from_files(args.lpips_trunk, args.lpips_lin, args.lpips_net)
