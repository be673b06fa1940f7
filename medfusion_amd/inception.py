"""The FID variant of Inception-v3 on the device: the 2048-wide pool features behind FID, precision / recall and the Inception Score, from
user-supplied weights (csrc/inception.hip, the general layers of csrc/cnn_layers.hip, include/medfusion_hip.h "Inception"; README "Inception features" has the definition).

Nothing pretrained is shipped or fetched.  InceptionNet.from_file takes the file a reference run already has on disk -- torch-fidelity's
pt_inception-2015-12-05-6726825d.pth, which torchmetrics' FID puts into the torch hub cache --, InceptionNet.seeded draws weights for tests and the
benchmark.  The BatchNorm of every BasicConv is folded into its convolution once, on the host, in fp64; all 94 convolutions and the fc run on the tiled
implicit-GEMM convolution of the fp32 matrix cores (mf_conv2d_gemm_f32, bias and ReLU fused), every branch writing straight into its block's
concatenated tensor.  The chain length of those launches is a rule of the layer alone (CHAIN), the tile is the library's choice and changes no bit, so
an image's features do not depend on the batch it travels in: chunk=1 gives the bits of chunk=None.

features() returns device tensors, never waits for the device and draws nothing.  Inputs are uint8 [B, C, H, W] tensors on the GPU with C in {1, 3};
anything else is a ValueError that names the argument, raised before anything touches the device."""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import kernels as K
from . import lib as L

MIN_SIZE = L.INCEPTION_MIN_SIZE
BN_EPS = 0.001
LAYER_NAMES = ("64", "192", "768", "2048", "logits_unbiased", "logits")
ACTIVATION_BUDGET = 512 << 20                # bytes of the largest activation of a trunk pass when chunk is None (LPIPS's figure)
# Products one fp32-MFMA accumulation chain holds at most (MfGemmConvDesc.chain): LPIPS measured a single chain of 3072 products outside "4 x the fp32
# restatement" and chains of 16 chunks of 32 inside it with margin (lpips.CHAIN_CHUNKS); the longest K here is 448 * 9 = 4032.
CHAIN = 512
FC_IN = 2048


def _build():
    """-> (layers, ops): layers = [(name, cin, cout, kh, kw, stride, pad_h, pad_w)] in state-dict order (94 BasicConvs);
    ops = ("conv", layer index, src, dst, y_offset) | ("pool", src, dst, stride, pad, mode, y_offset) | ("tap", name, buffer); `width` of a buffer: its channels"""
    layers, ops, width = [], [], {"in": 3}

    def buf(name, channels):
        width.setdefault(name, channels)
        return name

    def conv(name, src, dst, cout, k=(1, 1), s=1, p=False, off=0):
        kh, kw = k
        layers.append((name, width[src], cout, kh, kw, s, (kh - 1) // 2 if p else 0, (kw - 1) // 2 if p else 0))
        ops.append(("conv", len(layers) - 1, src, buf(dst, cout), off))

    def pool(src, dst, s, p, mode, off=0):
        ops.append(("pool", src, buf(dst, width[src]), s, p, mode, off))

    conv("Conv2d_1a_3x3", "in", "c1a", 32, (3, 3), 2)
    conv("Conv2d_2a_3x3", "c1a", "c2a", 32, (3, 3))
    conv("Conv2d_2b_3x3", "c2a", "c2b", 64, (3, 3), p=True)
    pool("c2b", "p64", 2, 0, L.POOL_MAX)
    ops.append(("tap", "64", "p64"))
    conv("Conv2d_3b_1x1", "p64", "c3b", 80)
    conv("Conv2d_4a_3x3", "c3b", "c4a", 192, (3, 3))
    pool("c4a", "p192", 2, 0, L.POOL_MAX)
    ops.append(("tap", "192", "p192"))
    cur = "p192"

    def block_a(name, src, pool_ch):
        dst = buf(name, 224 + pool_ch)
        conv(f"{name}.branch1x1", src, dst, 64)
        conv(f"{name}.branch5x5_1", src, f"{name}.t0", 48)
        conv(f"{name}.branch5x5_2", f"{name}.t0", dst, 64, (5, 5), p=True, off=64)
        conv(f"{name}.branch3x3dbl_1", src, f"{name}.t1", 64)
        conv(f"{name}.branch3x3dbl_2", f"{name}.t1", f"{name}.t2", 96, (3, 3), p=True)
        conv(f"{name}.branch3x3dbl_3", f"{name}.t2", dst, 96, (3, 3), p=True, off=128)
        pool(src, f"{name}.t3", 1, 1, L.POOL_AVG_VALID)
        conv(f"{name}.branch_pool", f"{name}.t3", dst, pool_ch, off=224)
        return dst

    def block_b(name, src):
        dst = buf(name, 384 + 96 + width[src])
        conv(f"{name}.branch3x3", src, dst, 384, (3, 3), 2)
        conv(f"{name}.branch3x3dbl_1", src, f"{name}.t0", 64)
        conv(f"{name}.branch3x3dbl_2", f"{name}.t0", f"{name}.t1", 96, (3, 3), p=True)
        conv(f"{name}.branch3x3dbl_3", f"{name}.t1", dst, 96, (3, 3), 2, off=384)
        ops.append(("pool", src, dst, 2, 0, L.POOL_MAX, 480))
        return dst

    def block_c(name, src, c7):
        dst = buf(name, 768)
        conv(f"{name}.branch1x1", src, dst, 192)
        conv(f"{name}.branch7x7_1", src, f"{name}.t0", c7)
        conv(f"{name}.branch7x7_2", f"{name}.t0", f"{name}.t1", c7, (1, 7), p=True)
        conv(f"{name}.branch7x7_3", f"{name}.t1", dst, 192, (7, 1), p=True, off=192)
        conv(f"{name}.branch7x7dbl_1", src, f"{name}.t2", c7)
        conv(f"{name}.branch7x7dbl_2", f"{name}.t2", f"{name}.t3", c7, (7, 1), p=True)
        conv(f"{name}.branch7x7dbl_3", f"{name}.t3", f"{name}.t4", c7, (1, 7), p=True)
        conv(f"{name}.branch7x7dbl_4", f"{name}.t4", f"{name}.t5", c7, (7, 1), p=True)
        conv(f"{name}.branch7x7dbl_5", f"{name}.t5", dst, 192, (1, 7), p=True, off=384)
        pool(src, f"{name}.t6", 1, 1, L.POOL_AVG_VALID)
        conv(f"{name}.branch_pool", f"{name}.t6", dst, 192, off=576)
        return dst

    def block_d(name, src):
        dst = buf(name, 320 + 192 + width[src])
        conv(f"{name}.branch3x3_1", src, f"{name}.t0", 192)
        conv(f"{name}.branch3x3_2", f"{name}.t0", dst, 320, (3, 3), 2)
        conv(f"{name}.branch7x7x3_1", src, f"{name}.t1", 192)
        conv(f"{name}.branch7x7x3_2", f"{name}.t1", f"{name}.t2", 192, (1, 7), p=True)
        conv(f"{name}.branch7x7x3_3", f"{name}.t2", f"{name}.t3", 192, (7, 1), p=True)
        conv(f"{name}.branch7x7x3_4", f"{name}.t3", dst, 192, (3, 3), 2, off=320)
        ops.append(("pool", src, dst, 2, 0, L.POOL_MAX, 512))
        return dst

    def block_e(name, src, mode):
        dst = buf(name, 2048)
        conv(f"{name}.branch1x1", src, dst, 320)
        conv(f"{name}.branch3x3_1", src, f"{name}.t0", 384)
        conv(f"{name}.branch3x3_2a", f"{name}.t0", dst, 384, (1, 3), p=True, off=320)
        conv(f"{name}.branch3x3_2b", f"{name}.t0", dst, 384, (3, 1), p=True, off=704)
        conv(f"{name}.branch3x3dbl_1", src, f"{name}.t1", 448)
        conv(f"{name}.branch3x3dbl_2", f"{name}.t1", f"{name}.t2", 384, (3, 3), p=True)
        conv(f"{name}.branch3x3dbl_3a", f"{name}.t2", dst, 384, (1, 3), p=True, off=1088)
        conv(f"{name}.branch3x3dbl_3b", f"{name}.t2", dst, 384, (3, 1), p=True, off=1472)
        pool(src, f"{name}.t3", 1, 1, mode)
        conv(f"{name}.branch_pool", f"{name}.t3", dst, 192, off=1856)
        return dst

    for name, pool_ch in (("Mixed_5b", 32), ("Mixed_5c", 64), ("Mixed_5d", 64)):
        cur = block_a(name, cur, pool_ch)
    cur = block_b("Mixed_6a", cur)
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        cur = block_c(name, cur, c7)
    ops.append(("tap", "768", cur))
    cur = block_d("Mixed_7a", cur)
    cur = block_e("Mixed_7b", cur, L.POOL_AVG_VALID)
    cur = block_e("Mixed_7c", cur, L.POOL_MAX)
    ops.append(("tap", "2048", cur))
    return layers, ops, width


LAYERS, OPS, WIDTH = _build()
BLOCKS = ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b", "Mixed_7c")
BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def state_keys(fc: bool = True):
    """the keys from_state reads, in trunk order"""
    keys = []
    for name, *_ in LAYERS:
        keys.append(f"{name}.conv.weight")
        keys += [f"{name}.bn.{k}" for k in BN_KEYS]
    return keys + (["fc.weight", "fc.bias"] if fc else [])


def trace(size: int) -> dict:
    """Host only: buffer name -> (H, W, C) of a pass at `size`"""
    size = _check_size(size)
    shape = {"in": (size, size, 3)}
    for op in OPS:
        if op[0] == "conv":
            _, cin, _, kh, kw, s, ph, pw = LAYERS[op[1]]
            h, w, _ = shape[op[2]]
            out = ((h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1, WIDTH[op[3]])
        elif op[0] == "pool":
            h, w, _ = shape[op[1]]
            out = ((h + 2 * op[4] - 3) // op[3] + 1, (w + 2 * op[4] - 3) // op[3] + 1, WIDTH[op[2]])
        else:
            continue
        dst = op[3] if op[0] == "conv" else op[2]
        if shape.setdefault(dst, out) != out:
            raise AssertionError(f"{dst}: {shape[dst]} and {out}")
    return shape


def _check_size(size) -> int:
    if isinstance(size, bool) or not isinstance(size, int) or size < MIN_SIZE or size > 4096:
        raise ValueError(f"size: an integer of at least {MIN_SIZE} (299 is the metric; at most 4096), got {size!r}")
    return size


def _check_layers(layer):
    names = (layer,) if isinstance(layer, str) else tuple(layer) if isinstance(layer, (tuple, list)) else None
    if not names or any(not isinstance(n, str) or n not in LAYER_NAMES for n in names):
        raise ValueError(f"layer: one of {LAYER_NAMES} or a tuple of them, got {layer!r}")
    return names


def _check_chunk(chunk):
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1):
        raise ValueError(f"chunk: None or a positive number of images per trunk pass, got {chunk!r}")


def default_chunk(size: int = 299) -> int:
    """images per trunk pass that keep the pass's largest activation at ACTIVATION_BUDGET bytes"""
    largest = max(h * w * c for h, w, c in trace(size).values()) * 4
    return max(1, ACTIVATION_BUDGET // largest)


def conv_desc(index: int, N: int, H: int, W: int, ldy: int = 0, y_offset: int = 0, tile: int = 0) -> L.MfGemmConvDesc:
    """the launch of BasicConv `index` on an [N, H, W, Cin] input: ReLU fused, the chain rule of the net"""
    _, cin, cout, kh, kw, s, ph, pw = LAYERS[index]
    return K.make_gemm_conv_desc(N, H, W, cin, cout, kh, kw, s, ph, pw, relu=True, ldy=ldy, y_offset=y_offset, chain=CHAIN, tile=tile)


def fc_desc(N: int, rows: int) -> L.MfGemmConvDesc:
    """the fc as a 1 x 1 convolution of the [N, 1, 1, 2048] pool features"""
    return K.make_gemm_conv_desc(N, 1, 1, FC_IN, rows, 1, 1, chain=CHAIN)


def plan(B: int, size: int = 299, rows: int = 1008) -> dict:
    """Host only: what one pass of B images costs -- {"launches", "conv_launches", "workgroups" (of the convolutions), "flops" (of the convolutions and
    the fc), "activation_bytes" (all buffers of the pass), "largest_activation_bytes", "weight_bytes", "layers": [...]}"""
    if isinstance(B, bool) or not isinstance(B, int) or B < 1:
        raise ValueError(f"B: a positive number of images, got {B!r}")
    shape = trace(size)
    rows_out, launches, wgs, flops = [{"op": "prepare", "kernel": "mf_inception_prepare_u8", "out": shape["in"]}], 1, 0, 0
    for op in OPS:
        if op[0] == "conv":
            name, cin, cout, kh, kw, s, ph, pw = LAYERS[op[1]]
            h, w, _ = shape[op[2]]
            ho, wo, ldy = shape[op[3]]
            tile, wg = K.gemm_conv_plan(conv_desc(op[1], B, h, w, ldy=ldy, y_offset=op[4]))
            f = 2 * B * ho * wo * cout * kh * kw * cin
            rows_out.append({"op": "conv", "key": name, "kernel": "mf_conv2d_gemm_f32", "k": (kh, kw), "stride": s, "pad": (ph, pw), "cin": cin, "cout": cout,
                             "out": (ho, wo, cout), "into": (op[3], op[4]), "tile": tile, "workgroups": wg, "flops": f})
            launches, wgs, flops = launches + 1, wgs + wg, flops + f
        elif op[0] == "pool":
            rows_out.append({"op": "pool", "kernel": "mf_pool2d_nhwc_f32", "stride": op[3], "pad": op[4], "mode": "max" if op[5] == L.POOL_MAX else "avg",
                             "out": shape[op[2]], "into": (op[2], op[6])})
            launches += 1
    convs = launches - 1 - sum(1 for op in OPS if op[0] == "pool")
    tile, wg = K.gemm_conv_plan(fc_desc(B, rows))
    rows_out.append({"op": "mean", "kernel": "mf_mean_pixels_f32", "out": (FC_IN,)})
    rows_out.append({"op": "fc", "kernel": "mf_conv2d_gemm_f32", "cin": FC_IN, "cout": rows, "tile": tile, "workgroups": wg, "flops": 2 * B * FC_IN * rows})
    elems = [h * w * c for h, w, c in shape.values()]
    weights = sum(cin * cout * kh * kw + cout for _, cin, cout, kh, kw, *_ in LAYERS) + FC_IN * rows + rows
    return {"B": B, "size": size, "launches": launches + 2, "conv_launches": convs + 1, "workgroups": wgs + wg, "flops": flops + 2 * B * FC_IN * rows,
            "activation_bytes": 4 * B * sum(elems), "largest_activation_bytes": 4 * B * max(elems), "weight_bytes": 4 * weights, "layers": rows_out}


def fold_batchnorm(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor, var: torch.Tensor):
    """the eval-mode BatchNorm (eps = 0.001) folded into its convolution, in fp64, rounded once: (w' OIHW fp32, b' fp32)"""
    s = gamma.double() / torch.sqrt(var.double() + BN_EPS)
    return (w.double() * s.view(-1, 1, 1, 1)).float(), (beta.double() - mean.double() * s).float()


class InceptionNet:
    """The weights of the network under the reference file's key names (fp32, on the host until .to(device)); the folded [KH][KW][Cin][Cout] device
    copies are derived once per device."""

    def __init__(self, state: dict):
        self.state = dict(state)
        self.rows = int(self.state["fc.weight"].shape[0])
        self._dev, self._bufs = {}, {}

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_state(cls, sd) -> "InceptionNet":
        """sd: the state dict of torch-fidelity's FeatureExtractorInceptionV3 ({layer}.conv.weight, {layer}.bn.*, fc.weight, fc.bias; AuxLogits.* and
        *.num_batches_tracked are ignored).  A missing or mis-shaped tensor is a ValueError naming the key."""
        def take(key, shape):
            if not hasattr(sd, "keys") or key not in sd:
                raise ValueError(f"sd: key {key!r} is missing")
            t = sd[key]
            ok = isinstance(t, torch.Tensor) and t.dim() == len(shape) and all(want is None or got == want for got, want in zip(t.shape, shape))
            if not ok:
                raise ValueError(f"sd: key {key!r} must be a tensor of shape {tuple('F' if s is None else s for s in shape)}, got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            return t.detach().to("cpu", torch.float32).contiguous().clone()

        state = {}
        for name, cin, cout, kh, kw, *_ in LAYERS:
            state[f"{name}.conv.weight"] = take(f"{name}.conv.weight", (cout, cin, kh, kw))
            for k in BN_KEYS:
                state[f"{name}.bn.{k}"] = take(f"{name}.bn.{k}", (cout,))
        state["fc.weight"] = take("fc.weight", (None, FC_IN))
        if state["fc.weight"].shape[0] < 1:
            raise ValueError("sd: key 'fc.weight' must have at least one row")
        state["fc.bias"] = take("fc.bias", (state["fc.weight"].shape[0],))
        return cls(state)

    @classmethod
    def from_file(cls, path) -> "InceptionNet":
        return cls.from_state(torch.load(str(path), map_location="cpu", weights_only=True))

    @classmethod
    def seeded(cls, seed: int, bias_std: float = 0.0, rows: int = 1008) -> "InceptionNet":
        """Weights for tests and the benchmark from ONE torch.Generator on the CPU, in fp64, rounded to fp32, in trunk order: per BasicConv the weight
        N(0, 2 / fan_in), then gamma U[0.5, 1.5), beta N(0, 0.05^2), the running mean N(0, 0.05^2), the running variance U[0.5, 2); then fc.weight
        N(0, 0.01^2) and fc.bias N(0, bias_std^2)."""
        g = torch.Generator(device="cpu").manual_seed(int(seed))

        def normal(shape, std):
            return (torch.randn(shape, generator=g, dtype=torch.float64) * std).float()

        def uniform(shape, lo, hi):
            return (lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)).float()

        state = {}
        for name, cin, cout, kh, kw, *_ in LAYERS:
            state[f"{name}.conv.weight"] = normal((cout, cin, kh, kw), math.sqrt(2.0 / (cin * kh * kw)))
            state[f"{name}.bn.weight"] = uniform((cout,), 0.5, 1.5)
            state[f"{name}.bn.bias"] = normal((cout,), 0.05)
            state[f"{name}.bn.running_mean"] = normal((cout,), 0.05)
            state[f"{name}.bn.running_var"] = uniform((cout,), 0.5, 2.0)
        state["fc.weight"] = normal((rows, FC_IN), 0.01)
        state["fc.bias"] = normal((rows,), float(bias_std))
        return cls(state)

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        """the weights under the reference file's key names: what from_state reads"""
        return dict(self.state)

    def folded(self, index: int):
        """(w' OIHW, b') of BasicConv `index` on the host"""
        name = LAYERS[index][0]
        return fold_batchnorm(self.state[f"{name}.conv.weight"], *(self.state[f"{name}.bn.{k}"] for k in BN_KEYS))

    def to(self, device) -> "InceptionNet":
        self._on(torch.device(device))
        return self

    def _on(self, device: torch.device):
        """the device copies: ([(w' [KH][KW][Cin][Cout], b')] per BasicConv, fc weight [1][1][2048][F], fc bias)"""
        if device.type != "cuda":
            raise RuntimeError("medfusion_amd: the Inception network runs on a ROCm device -- there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        ent = self._dev.get(device)
        if ent is None:
            convs = []
            for i in range(len(LAYERS)):
                w, b = self.folded(i)
                convs.append((K.pack_direct_conv_weight(w).to(device), b.to(device)))
            fcw = self.state["fc.weight"].t().contiguous().view(1, 1, FC_IN, self.rows).to(device)
            ent = self._dev[device] = (convs, fcw, self.state["fc.bias"].to(device))
        return ent

    def _buffers(self, device: torch.device, B: int, size: int) -> dict:
        """the activations of a pass of B images at `size`: allocated once per (device, B, size) and reused"""
        key = (device, B, size)
        bufs = self._bufs.get(key)
        if bufs is None:
            bufs = self._bufs[key] = {name: torch.empty((B, h, w, c), dtype=torch.float32, device=device) for name, (h, w, c) in trace(size).items()}
            bufs["pool"] = torch.empty((B, 1, 1, FC_IN), dtype=torch.float32, device=device)
        return bufs

    # ------------------------------------------------------------------ the forward pass
    def _pass(self, x: torch.Tensor, size: int, names, outs, lo: int) -> None:
        """one pass of b images: resize, trunk as far as the deepest wanted tap, the wanted rows into outs[name][lo : lo + b]"""
        convs, fcw, fcb = self._on(x.device)
        b = x.shape[0]
        bufs = self._buffers(x.device, b, size)
        K.inception_prepare(x, size, out=bufs["in"])
        want = {"2048" if n.startswith("logits") else n for n in names}
        for op in OPS:
            if not want:
                break
            if op[0] == "conv":
                src, dst = bufs[op[2]], bufs[op[3]]
                w, bias = convs[op[1]]
                K.conv2d_gemm(src, w, bias, conv_desc(op[1], b, src.shape[1], src.shape[2], ldy=dst.shape[3], y_offset=op[4]), out=dst)
            elif op[0] == "pool":
                dst = bufs[op[2]]
                K.pool2d_nhwc(bufs[op[1]], op[3], op[4], op[5], out=dst, ldy=dst.shape[3], y_offset=op[6])
            elif op[1] in want:
                want.discard(op[1])
                if op[1] in names:
                    K.mean_pixels(bufs[op[2]], out=outs[op[1]][lo:lo + b])
                if op[1] == "2048" and any(n.startswith("logits") for n in names):
                    pooled = K.mean_pixels(bufs[op[2]], out=bufs["pool"].view(b, FC_IN)).view(b, 1, 1, FC_IN)
                    for n, bias in (("logits_unbiased", None), ("logits", fcb)):
                        if n in names:
                            K.conv2d_gemm(pooled, fcw, bias, fc_desc(b, self.rows), out=outs[n][lo:lo + b].view(b, 1, 1, self.rows))

    def width(self, name: str) -> int:
        return self.rows if name.startswith("logits") else int(name)

    @torch.no_grad()
    def features(self, x: torch.Tensor, layer="2048", *, size: int = 299, chunk: Optional[int] = None):
        """x uint8 [B, 1|3, H, W] on the device -> [B, D] fp32 on the device (a tuple of them for a tuple of layers): "64", "192", "768" the pixel means
        of the spatial taps (as torch-fidelity returns them), "2048" the pool features of FID, "logits_unbiased" / "logits" the fc.  `chunk`: images per
        trunk pass (None: default_chunk(size)); the bits do not depend on it."""
        names = _check_layers(layer)
        size = _check_size(size)
        _check_chunk(chunk)
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"x: a tensor, got {type(x).__name__}")
        if x.dtype != torch.uint8:
            raise ValueError(f"x: uint8 (the bytes of the image files), got {x.dtype}")
        if x.dim() != 4 or any(s == 0 for s in x.shape):
            raise ValueError(f"x: a non-empty [B, C, H, W] tensor, got shape {tuple(x.shape)}")
        if x.shape[1] not in (1, 3):
            raise ValueError(f"x: 1 or 3 channels, got {x.shape[1]} (shape {tuple(x.shape)})")
        if max(x.shape[2:]) > 16384:
            raise ValueError(f"x: sides of at most 16384, got {x.shape[2]} x {x.shape[3]}")
        if not x.is_cuda:
            raise ValueError(f"x: on a ROCm device -- the Inception network has no CPU path, got a {x.device.type} tensor")
        x = x.contiguous()
        n = x.shape[0]
        step = chunk
        if step is None:                      # as few passes as the budget allows, of equal size: 100 images at 299 run as 50 + 50, not 97 + 3
            step = default_chunk(size)
            step = -(-n // -(-n // step))
        outs = {name: torch.empty((n, self.width(name)), dtype=torch.float32, device=x.device) for name in set(names)}
        for lo in range(0, n, step):
            self._pass(x[lo:min(n, lo + step)], size, names, outs, lo)
        return outs[names[0]] if isinstance(layer, str) else tuple(outs[name] for name in names)


class InceptionFeatures:
    """A callable for FidelityMeter(features=...): fp32 images [B, 1|3, H, W] in value_range (-1, 1) or (0, 1) are turned into bytes by the rounding
    scripts/sample_dataset.py uses before it writes PNG files (kernels.image_to_uint8), so the features of device tensors equal the features of the
    files written from them; uint8 images pass as they are."""

    def __init__(self, net: InceptionNet, layer: str = "2048", *, size: int = 299, value_range=(-1, 1), chunk: Optional[int] = None):
        if not isinstance(net, InceptionNet):
            raise ValueError(f"net: an InceptionNet (InceptionNet.from_file / from_state / seeded), got {type(net).__name__}")
        if not isinstance(layer, str) or layer not in LAYER_NAMES:
            raise ValueError(f"layer: one of {LAYER_NAMES}, got {layer!r}")
        if tuple(value_range) not in ((-1, 1), (0, 1)):
            raise ValueError(f"value_range: (-1, 1) or (0, 1), got {value_range!r}")
        _check_chunk(chunk)
        self.net, self.layer, self.size, self.value_range, self.chunk = net, layer, _check_size(size), tuple(value_range), chunk

    @torch.no_grad()
    def __call__(self, imgs: torch.Tensor) -> torch.Tensor:
        if not isinstance(imgs, torch.Tensor) or imgs.dim() != 4:
            raise ValueError(f"imgs: 2-D images [B, C, H, W], got {tuple(imgs.shape) if isinstance(imgs, torch.Tensor) else type(imgs).__name__}")
        if imgs.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"imgs: fp32 or uint8, got {imgs.dtype}")
        if not imgs.is_cuda:
            raise ValueError(f"imgs: on a ROCm device, got a {imgs.device.type} tensor")
        if imgs.dtype == torch.float32:
            if self.value_range == (0, 1):
                imgs = imgs * 2.0 - 1.0
            imgs = K.image_to_uint8(imgs).permute(0, 3, 1, 2).contiguous()
        return self.net.features(imgs, self.layer, size=self.size, chunk=self.chunk)


def inception_score(logits: torch.Tensor, splits: int = 1) -> dict:
    """The Inception Score of [N, F] logits in fp64 torch: p = softmax(logits); per split s (rows [s N // splits, (s + 1) N // splits)):
    exp(mean_x sum_k p (log p - log mean_x p)); -> {"inception_score_mean", "inception_score_std"} over the splits (the population deviation)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"logits: a non-empty [N, F] tensor, got {tuple(logits.shape) if isinstance(logits, torch.Tensor) else type(logits).__name__}")
    if isinstance(splits, bool) or not isinstance(splits, int) or not 1 <= splits <= logits.shape[0]:
        raise ValueError(f"splits: an integer in 1 .. N = {logits.shape[0]}, got {splits!r}")
    logp = torch.log_softmax(logits.double(), dim=1)
    p = logp.exp()
    n = logits.shape[0]
    scores = []
    for s in range(splits):
        ps, lps = p[s * n // splits:(s + 1) * n // splits], logp[s * n // splits:(s + 1) * n // splits]
        kl = (ps * (lps - ps.mean(dim=0, keepdim=True).log())).sum(dim=1).mean()
        scores.append(kl.exp())
    scores = torch.stack(scores)
    return {"inception_score_mean": float(scores.mean()), "inception_score_std": float(scores.std(unbiased=False))}


def parse_features_spec(spec: str):
    """'inception:FILE[:layer]' -> (FILE, layer); None when `spec` does not start with 'inception:'"""
    if not isinstance(spec, str) or not spec.startswith("inception:"):
        return None
    parts = spec.split(":")
    if len(parts) not in (2, 3) or not parts[1] or (len(parts) == 3 and parts[2] not in LAYER_NAMES):
        raise ValueError(f"--features: inception:FILE[:layer] with layer one of {', '.join(LAYER_NAMES)}, got {spec!r}")
    return parts[1], parts[2] if len(parts) == 3 else "2048"
