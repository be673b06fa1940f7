"""LPIPS v0.1 restated in plain torch on the CPU (F.conv2d, F.max_pool2d; fp64 and fp32), the seeded nets, the case lists and the bounds of
tests/test_lpips_cpu.py and tests/test_lpips_gpu.py.  References are computed once (functools caches) and never modified."""
import functools

import torch
import torch.nn.functional as F

from medfusion_amd.lpips import OPS, LPIPSNet

SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
NETS = ("vgg", "alex")
SEEDED = ((1, 0.0), (2, 0.05))                                  # (seed, bias_std) of the whole-metric nets
SHAPES = ((2, 3, 32, 32), (3, 1, 48, 40), (1, 3, 35, 31))      # one pool chain each: even sides, one channel, odd sides (floor mode at every pool)
MARGIN = 4.0                                                    # what tests/test_metrics_gpu.py gives its kernels over the same kind of restatement

# (N, H, W, Cin, Cout, k, stride, pad) of the direct convolution
DIRECT_CASES = ((2, 9, 7, 3, 5, 3, 1, 1), (1, 35, 31, 3, 64, 11, 4, 2), (2, 7, 7, 33, 40, 5, 1, 2), (1, 11, 11, 3, 4, 11, 4, 2), (1, 5, 6, 8, 3, 3, 2, 0))
POOL_CASES = ((2, 5), (2, 8), (3, 7), (3, 15), (3, 3))         # (k, side), stride 2: 5 -> 2, 8 -> 4, 7 -> 3, 15 -> 7, 3 -> 1
POOL_CHANNELS = (1, 65)
LAYER_CHANNELS = (5, 64, 192, 512)
LAYER_PIXELS = (1, 49, 33 * 31)


@functools.lru_cache(maxsize=None)
def seeded(net, seed, bias_std=0.0):
    return LPIPSNet.seeded(net, seed, bias_std)


def make_pair(shape, seed):
    """x uniform in [-1, 1], y = clamp(x + 0.3 N(0, 1))"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1
    y = (x + 0.3 * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(-1, 1)
    return x.float(), y.float()


def ref_scale(x, dtype, normalize=False):
    x = x.to(dtype)
    if normalize:
        x = 2 * x - 1
    if x.shape[1] == 1:
        x = x.expand(-1, 3, -1, -1)
    return (x - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)


def ref_taps(net: LPIPSNet, x, dtype, normalize=False):
    """the five tapped feature maps (NCHW) of the trunk on the scaled input"""
    h, taps, i = ref_scale(x, dtype, normalize), [], 0
    for op in OPS[net.net]:
        if op[0] == "conv":
            w, b = net.convs[i]
            i += 1
            h = F.relu(F.conv2d(h, w.to(dtype), b.to(dtype), stride=op[5], padding=op[6]))
        elif op[0] == "pool":
            h = F.max_pool2d(h, op[1], op[2])
        else:
            taps.append(h)
    return taps


def ref_layer_term(a, b, w, dtype=torch.float64):
    """term_l of the feature maps a, b [B, C, ...] under w [C] -> [B]"""
    a, b, w = a.to(dtype).flatten(2), b.to(dtype).flatten(2), w.to(dtype)
    an = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    bn = b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return ((an - bn).pow(2) * w.view(1, -1, 1)).sum(1).mean(1)


def ref_terms(net: LPIPSNet, x, y, dtype, normalize=False):
    """[B, 5]: the per-layer terms of the pairs (x[b], y[b]); lpips = their sum over the layers"""
    fa, fb = ref_taps(net, x, dtype, normalize), ref_taps(net, y, dtype, normalize)
    return torch.stack([ref_layer_term(a, b, w, dtype) for a, b, w in zip(fa, fb, net.lins)], dim=1)


@functools.lru_cache(maxsize=None)
def whole_case(net_name, seed, bias_std, shape):
    """(x, y, terms64 [B, 5], terms32 [B, 5]) of one whole-metric case"""
    net = seeded(net_name, seed, bias_std)
    x, y = make_pair(shape, 1000 * seed + shape[-1])
    return x, y, ref_terms(net, x, y, torch.float64), ref_terms(net, x, y, torch.float32)


def whole_cases(net_name):
    return [(seed, std, shape) + whole_case(net_name, seed, std, shape) for seed, std in SEEDED for shape in SHAPES]


@functools.lru_cache(maxsize=None)
def whole_bounds(net_name):
    """the relative bound of every layer's term: MARGIN x the largest relative distance of the fp32 restatement from the fp64 one over all pairs of
    all cases of the net -- computed from the reference alone"""
    d = torch.zeros(5, dtype=torch.float64)
    for *_, t64, t32 in whole_cases(net_name):
        d = torch.maximum(d, ((t32.double() - t64).abs() / t64).max(dim=0).values)
    return MARGIN * d


# ------------------------------------------------------------------------------------------------ the direct convolution
def direct_case(case, seed=0):
    """x NHWC, w OIHW, bias; y64 NHWC and the element-wise bound (K + 2) 2^-24 (sum |w| |x| + |b|), K = KH KW Cin: K fma roundings, the bias add, and
    the fp64 reference's own share"""
    n, h, w_, cin, cout, k, s, p = case
    g = torch.Generator().manual_seed(100 + seed + cin * k)
    x = torch.randn((n, h, w_, cin), generator=g)
    w = torch.randn((cout, cin, k, k), generator=g) / (cin * k * k) ** 0.5
    b = torch.randn((cout,), generator=g)
    xn = x.permute(0, 3, 1, 2).double()
    y64 = F.conv2d(xn, w.double(), b.double(), stride=s, padding=p)
    mag = F.conv2d(xn.abs(), w.double().abs(), b.double().abs(), stride=s, padding=p)
    bound = (cin * k * k + 2) * 2.0 ** -24 * mag
    return x, w, b, y64.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ the layer distance
def layer_case(C, P, B=2, seed=0):
    """feature maps [B, P, C] as a ReLU leaves them (half the values 0), the second near the first, and linear weights in [0, 8 / C)"""
    g = torch.Generator().manual_seed(7 * C + P + seed)
    fx = torch.randn((B, P, C), generator=g).clamp_min(0)
    fy = (fx + 0.3 * torch.randn((B, P, C), generator=g)).clamp_min(0)
    w = torch.rand((C,), generator=g) * (8.0 / C)
    return fx, fy, w


def layer_reference(fx, fy, w):
    """(term64 [B], bound [B]) of NHWC maps [B, P, C].  The kernel evaluates the chain in fp64 (u = 2^-53) on the fp32 values: per channel
    a^ = a r with r = 1 / (sqrt(S) + 1e-10): S carries C + 1 roundings, sqrt, +, 1 /, the product one each -> |delta a^| <= (C/2 + 5) u |a^| (first order; the
    sqrt halves S's); e = a^ - b^ adds u |e| and inherits (C/2 + 5) u (|a^| + |b^|) WITHOUT cancellation; w e^2 two more; the sum over C channels and the P
    pixels (a 16-lane butterfly, the lane loops, the 16 groups, the partials, / P) at most C + P + 8 roundings of non-negative terms.  So
    |delta term| <= u mean_p sum_c w_c [2 |e_c| (C/2 + 6) (|a^_c| + |b^_c|) + (C + P + 12) e_c^2]; the fp64 restatement takes the same chain: twice that."""
    a, b, w = fx.double(), fy.double(), w.double()
    C, P = a.shape[-1], a.shape[1]
    an = a / (a.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    bn = b / (b.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    e = an - bn
    term = (e.pow(2) * w).sum(-1).mean(-1)
    slack = (w * (2 * e.abs() * (C / 2 + 6) * (an.abs() + bn.abs()) + (C + P + 12) * e.pow(2))).sum(-1).mean(-1)
    return term, 2 * 2.0 ** -53 * slack
