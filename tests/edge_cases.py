"""Cases, input generators, restatements, derived bounds and the restated host dispatch ("census") of tests/test_edge_cpu.py and
tests/test_edge_gpu.py: the layout kernels that almost every GPU test converts its operands with, the resampling and skip kernels of
csrc/edge_ops.hip, the embedding / table kernels, the VAE edge of csrc/small_ops.hip, the image egress and the network input's pair operand.
Importable without a GPU.

INPUTS are functions of the case alone.
  copy kernels (layout, upsample, gather, broadcast): `tagged` -- element i holds the int32 pattern 0x3F800000 + i viewed as fp32: distinct
      normal numbers, compared as int32 (`bits`), so a misplaced element, a -0 or a NaN payload cannot pass.
  arithmetic kernels: `scaled` -- N(0, 1) times 2^(12 (n mod 3)) per sample and 2^(6 (c mod 2)) per channel: a value taken from the wrong sample or
      channel is off by orders of magnitude, not by rounding.

YARDSTICKS.  Everything in sections A to C and the egress is bit-equal: torch's own permute / repeat_interleave / pixel_(un)shuffle / indexing and
one fp32 addition on the CPU, the numpy / torchvision chains of the egress, and for AvgPool `avgpool_restated` (the clipped window summed row by
row in fp32 from 0, the divisor from the window clipped to the PADDED extent, one division), which tests/test_edge_cpu.py holds bit-equal to
F.avg_pool2d (NCHW and channels-last) on every case.  Bounds that are not zero:

  learned_sinusoidal  the angle ((t w) 2) pi is restated in fp32 step by step (the library is built with -ffp-contract=off: same bits); sin / cos
      of that fp32 angle in fp64 is the reference.  The accuracy figure of the device sinf / cosf is not in this tree, so the kernel's largest
      absolute error per case is held to 4 x that of torch.sin / torch.cos (fp32, CPU) on the same angles, floored at 2^-24: the host's
      functions are within 1 ulp, the device's are specified to a few.
  diag_gaussian_sample  fp64 mean + exp(0.5 clamp(logvar, -30, 20)) noise; E = u |z| + (2u + 2u) |sd noise|, u = 2^-24: expf at its 1 ulp (2u, as
      tests/transformer_cases.py takes it), the product, one u spare; the final addition.  (0.5 logvar is exact.)
  diag_gaussian_kl  fp64 0.5 Sum(mean^2 + exp(lv) - 1 - lv) / N; E = (0.5 / N) Sum(u mean^2 + 2u exp(lv)) + u |kl|
      + 2^-50 (0.5 / N) Sum(mean^2 + exp(lv) + 1 + |lv|): the fp32 square and expf, the rounding of the result to fp32, the fp64 accumulation
      over the terms' magnitudes.
  pack_nchw_pairs  (hi + lo / 2048) 2^s, s = floor(log2 bound) - 14, within 2^-23 |x| + 2^-50 bound (the claim of test_split_f16x2_format);
      the padded channels exactly +0; the bound bit-equal to max |x|.

No constant here comes from a run of the kernels.  CENSUS: `blocks_of` restates the block count and the grid-stride cap of every launch
(4096 x 256 threads in csrc/edge_ops.hip, 2048 x 256 for add and the gathers, none for the one-thread-per-element kernels), `layout_grid` the
32 x 32 tiling of transpose_planes_kernel, so that the CPU suite can assert which case -- and only which -- crosses a cap or a tile edge."""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
SENTINEL = -7777.0
PAD = 64                      # floats behind every output of the sentinel checks
CAP_EDGE = 4096               # blocks of 256 threads: the grid-stride cap of csrc/edge_ops.hip
CAP_SMALL = 2048              # ... of add_kernel and the gathers
NONFINITE = (float("nan"), float("inf"), float("-inf"))


def case_id(case) -> str:
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in case) if isinstance(case, (tuple, list)) else str(case)


# ---------------------------------------------------------------- inputs
def tagged(*shape, start: int = 0) -> torch.Tensor:
    """fp32 tensor whose element i is the bit pattern 0x3F800000 + start + i: distinct normal numbers in [1, 2^127)"""
    n = math.prod(shape)
    assert 0 < n and start + n < 0x3F000000
    return (torch.arange(n, dtype=torch.int64) + (0x3F800000 + start)).to(torch.int32).view(torch.float32).reshape(shape)


def bits(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.float32
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> int:
    """how many elements of a differ from b in their bits (shape and dtype must agree)"""
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, (a.shape, b.shape, a.dtype, b.dtype)
    return int((bits(a) != bits(b)).sum())


def _gen(name: str, case) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32((name + repr(tuple(case))).encode()))


def scaled(name: str, case, shape, sample_axis: int = 0, channel_axis: int = -1) -> torch.Tensor:
    """N(0, 1) x 2^(12 (n mod 3)) x 2^(6 (c mod 2)) x 2^-12"""
    x = torch.randn(shape, generator=_gen(name, case))
    sh = [1] * len(shape)
    sh[sample_axis] = shape[sample_axis]
    x = x * torch.exp2(12.0 * (torch.arange(shape[sample_axis]) % 3) - 12.0).reshape(sh)
    if channel_axis is not None:
        sh = [1] * len(shape)
        sh[channel_axis] = shape[channel_axis]
        x = x * torch.exp2(6.0 * (torch.arange(shape[channel_axis]) % 2)).reshape(sh)
    return x.contiguous()


# ---------------------------------------------------------------- A. layout
# (N, C, H, W)
LAYOUT_CASES = [
    (1, 1, 1, 1),           # one element in one tile
    (2, 31, 1, 33),         # one column past a tile in HW, one row short in C
    (3, 32, 4, 8),          # exactly one tile
    (2, 33, 5, 13),         # one row and one column past a tile in both dimensions (HW = 65)
    (1, 100, 3, 43),        # both plane dimensions ragged above 32: 4 x 5 tiles
    (5, 3, 7, 11),          # C < 32, HW ragged
    (65535, 1, 1, 1),       # the last z index
]
LAYOUT_REFUSED_N = 65536


def layout_grid(case):
    """(tiles along C, tiles along HW, N, C ragged, HW ragged) of transpose_planes_kernel for the case (either direction: the grid is transposed)"""
    n, c, h, w = case
    return (c + 31) // 32, (h * w + 31) // 32, n, c % 32 != 0, (h * w) % 32 != 0


# ---------------------------------------------------------------- B. resampling and skip kernels
# (N, H, W, C, k, s, p)
POOL_CASES = [
    (2, 7, 9, 4, 3, 2, 1),
    (1, 8, 8, 36, 3, 2, 1),
    (2, 5, 6, 8, 2, 2, 1),      # 2 p = k: the divisor is clipped at the far edge
    (1, 1, 1, 4, 3, 2, 1),
    (1, 6, 5, 4, 2, 2, 0),      # last row dropped
    (1, 9, 7, 36, 3, 1, 1),
    (3, 4, 4, 4, 1, 1, 0),
]
POOL_CAP_CASE = (1, 17, 1, 4 * 61681, 1, 1, 0)          # 17 x 61681 = 4096 x 256 + 1 float4 items: the smallest count over the cap
UP_CASES = [(1, 1, 1, 4), (2, 3, 5, 36), (3, 4, 1, 8)]   # (N, H, W, C)
UP_CAP_CASE = (1, 1, 1, 4 * 262145)                      # 4 x 262145 items = cap + 4 (the count is a multiple of 4)
UNSHUF_CASES = [(1, 4, 6, 1), (2, 4, 2, 3), (3, 2, 2, 4), (2, 6, 10, 5)]   # x (N, H, W, C): C = 1; C = 3; H = W = 2; ragged last threads
UNSHUF_CAP_CASE = (1, 2, 2, 1048577)
SHUF_CASES = [(2, 3, 5, 4), (2, 2, 3, 12), (3, 1, 1, 8)]                   # x (N, H, W, C): Co = 1; C = 12; H = W = 1
SHUF_CAP_CASE = (1, 1, 1, 4 * 1048577)


def pool_out_hw(case):
    n, h, w, c, k, s, p = case
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def pool_divisors(case):
    """[Ho, Wo] divisor of every window (clipped to the padded extent) and the count of image cells under it"""
    n, h, w, c, k, s, p = case
    ho, wo = pool_out_hw(case)
    div, cells = torch.zeros((ho, wo)), torch.zeros((ho, wo))
    for oy in range(ho):
        for ox in range(wo):
            hs, ws = oy * s - p, ox * s - p
            he, we = min(hs + k, h + p), min(ws + k, w + p)
            div[oy, ox] = (he - hs) * (we - ws)
            cells[oy, ox] = (min(he, h) - max(hs, 0)) * (min(we, w) - max(ws, 0))
    return div, cells


def avgpool_restated(x: torch.Tensor, k: int, s: int, p: int) -> torch.Tensor:
    """x [N, H, W, C] fp32 -> nn.AvgPool2d(k, s, p) (count_include_pad) as the kernel states it"""
    assert x.dtype == torch.float32
    n, h, w, c = x.shape
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    out = torch.empty((n, ho, wo, c), dtype=torch.float32)
    for oy in range(ho):
        for ox in range(wo):
            hs, ws = oy * s - p, ox * s - p
            he, we = min(hs + k, h + p), min(ws + k, w + p)
            pool = torch.tensor(float((he - hs) * (we - ws)), dtype=torch.float32)
            acc = torch.zeros((n, c), dtype=torch.float32)
            for iy in range(max(hs, 0), min(he, h)):
                for ix in range(max(ws, 0), min(we, w)):
                    acc = acc + x[:, iy, ix, :]
            out[:, oy, ox, :] = acc / pool
    return out


def pool_input(case) -> torch.Tensor:
    n, h, w, c, k, s, p = case
    return scaled("pool", case, (n, h, w, c))


def upsample_expected(x: torch.Tensor) -> torch.Tensor:
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def nhwc(t_nchw: torch.Tensor) -> torch.Tensor:
    return t_nchw.permute(0, 2, 3, 1).contiguous()


def nchw(t_nhwc: torch.Tensor) -> torch.Tensor:
    return t_nhwc.permute(0, 3, 1, 2).contiguous()


def unshuffle_inputs(case):
    n, h, w, c = case
    return scaled("unshuf.x", case, (n, h, w, c)), scaled("unshuf.y", case, (n, h // 2, w // 2, 4 * c))


def unshuffle_expected(x, y):
    return y + nhwc(F.pixel_unshuffle(nchw(x), 2))


def shuffle_inputs(case):
    n, h, w, c = case
    return scaled("shuf.x", case, (n, h, w, c)), scaled("shuf.y", case, (n, 2 * h, 2 * w, c // 4))


def shuffle_expected(x, y):
    return y + nhwc(F.pixel_shuffle(nchw(x), 2))


def blocks_of(kernel: str, case):
    """(work items, cap in blocks or None, blocks launched) of the launch, restated from the extern "C" entry of the kernel"""
    if kernel == "avgpool":
        n, h, w, c, k, s, p = case
        ho, wo = pool_out_hw(case)
        items, cap = n * ho * wo * (c // 4), CAP_EDGE
    elif kernel == "upsample":
        n, h, w, c = case
        items, cap = n * 4 * h * w * (c // 4), CAP_EDGE
    elif kernel == "unshuffle":
        n, h, w, c = case
        items, cap = n * (h // 2) * (w // 2) * c, CAP_EDGE
    elif kernel == "shuffle":
        n, h, w, c = case
        items, cap = n * h * w * (c // 4), CAP_EDGE
    elif kernel == "add":
        items, cap = int(case), CAP_SMALL
    elif kernel == "gather":                 # (S, NCOL, row_len, B)
        items, cap = case[3] * case[2], CAP_SMALL
    elif kernel == "gather_multi":           # ((row lengths), S, NCOL, B): the longest table sets the grid
        items, cap = case[3] * max(case[0]), CAP_SMALL
    elif kernel in ("embedding_add", "learned_sinusoidal", "diag_gaussian", "broadcast", "egress"):
        items, cap = int(case), None         # one thread per element, ragged last block
    else:
        raise KeyError(kernel)
    need = (items + 255) // 256
    return items, cap, need if cap is None else min(need, cap)


def over_cap(kernel: str, case) -> bool:
    items, cap, _ = blocks_of(kernel, case)
    return cap is not None and items > cap * 256


# ---------------------------------------------------------------- C. embedding and table kernels
# (rows, D, idx): B = len(idx)
EMB_CASES = [
    (3, 1, (2, 0, 1)),                      # D = 1
    (4, 65, (3, 3, 0, 1, 3)),               # D = 65, repeated indices
    (5, 257, (4,)),                         # B D = 257: second workgroup with one element
    (7, 16, (0, 6, 0, 6)),                  # indices 0 and rows - 1
]
EMB_OOR_CASE = (4, 33, (1, 4, 0, -1, 3))    # rows 1 and 3 are out of range: left bit-identical (the kernel's documented contract)


def emb_inputs(case):
    rows, d, idx = case
    return scaled("emb.table", case, (rows, d)), torch.tensor(idx, dtype=torch.int64), scaled("emb.io", case, (len(idx), d))


def emb_expected(table, idx, io):
    ok = (idx >= 0) & (idx < table.shape[0])
    out = io.clone()
    out[ok] = io[ok] + table[idx[ok]]
    return out


SIN_DIMS = (2, 16, 33)
SIN_T = (0.0, 0.731, 37.0, 999.0)
PI32 = torch.tensor(3.14159265358979323846, dtype=torch.float32)


def sin_inputs(emb_dim: int):
    return torch.tensor(SIN_T, dtype=torch.float32), torch.randn(emb_dim // 2, generator=_gen("sin.w", (emb_dim,)))


def sin_angles(t: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """[B, half] fp32: ((t w) 2) pi, every product rounded on its own, left to right"""
    a = t[:, None] * w[None, :]
    a = a * torch.tensor(2.0, dtype=torch.float32)
    return a * PI32


def sin_reference(t, w, emb_dim: int):
    """(fp64 [B, row] reference from the fp32 angles, the fp32 CPU chain's row, mask of the sin / cos columns)"""
    a = sin_angles(t, w)
    zero = [torch.zeros((t.shape[0], 1), dtype=torch.float64)] * (emb_dim & 1)
    ref = torch.cat([t.double()[:, None], a.double().sin(), a.double().cos()] + zero, dim=1)
    host = torch.cat([t[:, None], a.sin(), a.cos()] + [z.float() for z in zero], dim=1)
    mask = torch.zeros(ref.shape[1], dtype=torch.bool)
    mask[1:1 + 2 * (emb_dim // 2)] = True
    return ref, host, mask


def sin_bound(ref, host, mask) -> float:
    return max(4.0 * float((host.double() - ref)[:, mask].abs().max()), U24)


# (S, NCOL, row_len, cols)
GATHER_CASES = [
    (3, 2, 1, (1, 0, 1)),
    (2, 3, 4, (2, 2, 0, 1, 2)),             # float-aligned rows, repeated columns
    (4, 2, 257, (0, 1, 1)),                 # the second block of a row
]
GATHER_CAP_CASE = (2, 2, CAP_SMALL * 256 + 1, (1,))
# ((row lengths), S, NCOL, cols)
GATHER_MULTI_CASES = [
    ((64,), 3, 2, (1, 0, 1)),
    ((1, 1280), 2, 3, (2, 0, 2, 1)),
    ((1, 64, 1280), 3, 2, (0, 1, 1, 0, 1)),     # the longest table sets the grid: the short ones have idle blocks
    ((1280, 1, 64), 2, 2, (1, 1)),
]
GATHER_MULTI_CAP_CASE = ((1, CAP_SMALL * 256 + 1), 2, 2, (1,))
BROADCAST_CASES = [(1, 1), (5, 4), (3, 257)]    # (S, n)
ADD_SIZES = (1, 257)
ADD_CAP_SIZE = CAP_SMALL * 256 + 1


def gather_tables(row_lens, S, ncol):
    """tagged tables whose patterns do not overlap"""
    out, start = [], 0
    for ln in row_lens:
        out.append(tagged(S, ncol, ln, start=start))
        start += S * ncol * ln
    return out


# ---------------------------------------------------------------- D. VAE edge
DG_CASES = [(1, 1, 1), (2, 4, 63), (3, 8, 257)]      # (N, C, HW): one element; ragged; second workgroup ... with one ragged tail
DG_5D_CASE = (2, 4, 3, 7, 3)                          # (N, C, D, H, W) of vae.py's view
LOGVAR_PLANTS = (-31.0, -30.0, 20.0, 21.0, 0.0, -0.0)


def dg_inputs(case, hw_shape=None):
    """moments [N, 2C, H, W] (H W = HW as (HW, 1) unless hw_shape) and noise [N, C, H, W]; the first len(LOGVAR_PLANTS) elements of sample 0 (as many
    as it has) and the last ones of the last sample carry the planted logvars and mean 0"""
    n, c, hw = case
    h, w = hw_shape if hw_shape is not None else (hw, 1)
    mean = scaled("dg.mean", case, (n, c, hw), channel_axis=1)
    logvar = 3.0 * torch.randn((n, c, hw), generator=_gen("dg.lv", case))
    noise = torch.randn((n, c, hw), generator=_gen("dg.noise", case))
    k = min(len(LOGVAR_PLANTS), c * hw)
    plants = torch.tensor(LOGVAR_PLANTS[:k])
    for s, sl in ((0, slice(0, k)), (n - 1, slice(c * hw - k, c * hw))):
        logvar[s].view(-1)[sl] = plants
        mean[s].view(-1)[sl] = 0.0
    mom = torch.cat([mean, logvar], dim=1).reshape(n, 2 * c, h, w).contiguous()
    return mom, noise.reshape(n, c, h, w).contiguous()


def dg_terms(mom, noise):
    n, c2 = mom.shape[:2]
    mean, lv = mom.double()[:, :c2 // 2], mom.double()[:, c2 // 2:]
    sn = torch.exp(0.5 * lv.clamp(-30.0, 20.0)) * noise.double()
    z = mean + sn
    return {"out": z, "E": U24 * z.abs() + 4.0 * U24 * sn.abs()}


KL_CASES = [(1, 1, 1), (3, 1, 1), (3, 3, 341), (3, 5, 205), (3, 8, 625)]     # (N, C, HW): C HW = 1, 1023, 1025, 5000 per sample


def kl_inputs(case):
    n, c, hw = case
    mean = scaled("kl.mean", case, (n, c, hw, 1), channel_axis=None) * 4096.0 * 0.25      # samples at 0.25, 2^10, 2^22
    lv = 2.0 * torch.randn((n, c, hw, 1), generator=_gen("kl.lv", case))
    return torch.cat([mean, lv], dim=1).contiguous()


def kl_terms(mom):
    n, c2 = mom.shape[:2]
    mean, lv = mom.double()[:, :c2 // 2], mom.double()[:, c2 // 2:].clamp(-30.0, 20.0)
    m2, ev = mean * mean, torch.exp(lv)
    kl = 0.5 * (m2 + ev - 1.0 - lv).sum() / n
    E = (0.5 / n) * (U24 * m2 + 2.0 * U24 * ev).sum() + U24 * kl.abs() + 2.0 ** -50 * (0.5 / n) * (m2 + ev + 1.0 + lv.abs()).sum()
    return {"out": float(kl), "E": float(E)}


def clamp_plants(numel: int):
    """where the NaN, the +Inf and the -Inf go in a flat tensor of `numel` elements: three distinct positions, the last one in the last element"""
    assert numel >= 3
    return {(numel - 1) // 3: NONFINITE[0], (2 * (numel - 1)) // 3: NONFINITE[1], numel - 1: NONFINITE[2]}


# ---------------------------------------------------------------- E. image egress and the pair operand
EGRESS0_CASES = [(2, 1, 8, 65), (2, 3, 4, 129)]      # (N, C, H, W): C H W >= 512 = both roundings of all 256 grid points; odd W


def egress0_input(case):
    """x = 2 j / 255 - 1 for j = 0..255, each rounded down and up with nextafter: where truncation and rounding part; the rest N(0, 0.9)"""
    n, c, h, w = case
    x = 0.9 * torch.randn((n, c, h, w), generator=_gen("egress0", case))
    g = (2.0 * np.arange(256, dtype=np.float64) / 255.0 - 1.0).astype(np.float32)
    pts = np.concatenate([np.nextafter(g, np.float32(-2.0)), np.nextafter(g, np.float32(2.0))]).astype(np.float32)
    assert c * h * w >= pts.size
    for s in range(n):
        x[s].view(-1)[:pts.size] = torch.from_numpy(pts if s % 2 == 0 else pts[::-1].copy())
    return x


def egress0_expected(x: torch.Tensor) -> np.ndarray:
    img = x.numpy().clip(-1, 1)
    img = (img + 1) / 2 * 255                      # scripts/helpers/sample_dataset.py:46-47 verbatim arithmetic
    return np.moveaxis(img, 1, -1).astype(np.uint8)


EGRESS1_CASES = ["constant", "outside", "chw3", "chw257", "disjoint"]


def egress1_input(name: str) -> torch.Tensor:
    g = _gen("egress1", (name,))
    if name == "constant":                          # max - min = 0: the divisor is 1e-5
        return torch.full((2, 3, 4, 5), 0.25)
    if name == "outside":                           # wholly outside [-1, 1]: every value clamps to 1 (or 0)
        x = 2.0 + torch.rand((2, 1, 5, 7), generator=g)
        x[1] = -x[1]
        return x
    if name == "chw3":                              # 253 idle threads of the min / max reduction hold +-Inf
        return torch.tensor([[-0.5, 0.1, 0.7], [0.3, 0.2, -0.9]]).reshape(2, 3, 1, 1)
    if name == "chw257":
        return 0.8 * torch.randn((2, 1, 1, 257), generator=g)
    if name == "disjoint":                          # samples with disjoint ranges: a min / max taken from the neighbour shows
        x = 0.1 * torch.rand((3, 3, 5, 3), generator=g)
        return x + torch.tensor([-0.9, -0.1, 0.7]).view(3, 1, 1, 1)
    raise KeyError(name)


def egress1_expected(x: torch.Tensor) -> torch.Tensor:
    r = ((x + 1) / 2).clamp(0, 1)                  # scripts/sample.py:49-50, then torchvision norm_ip + save_image
    r = torch.stack([(b.clamp(min=float(b.min()), max=float(b.max())) - b.min()) / max(float(b.max() - b.min()), 1e-5) for b in r])
    return r.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1)


# (N, C, HW, CP)
PACK_CASES = [(1, 1, 1, 32), (3, 3, 35, 32), (2, 8, 64, 32), (2, 12, 9, 32), (2, 40, 5, 64), (2, 4, 33, 32)]
PACK_ZERO_CASE = (2, 4, 33, 32)                      # sample 0 all zero, sample 1 at 2^12
PACK_REFUSED = (1, 1, 2 ** 18 + 1, 32)               # C HW = 2^18 + 1


def pack_input(case) -> torch.Tensor:
    n, c, hw, cp = case
    x = scaled("pack", case, (n, c, hw, 1), channel_axis=1)
    if case == PACK_ZERO_CASE:
        x[0] = 0.0
        x[1] = torch.randn((c, hw, 1), generator=_gen("pack.z", case)) * 4096.0
    return x


def decode_pairs(pairs_i32: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """int32 [N, H, W, CP] fp16-pair tensor + bound [N] -> fp64 [N, H, W, CP]: (hi + lo / 2048) 2^s, s = floor(log2 bound) - 14 (a zero bound: s = 0)"""
    shape = pairs_i32.shape
    raw = pairs_i32.cpu().contiguous().view(torch.int16).view(*shape[:-1], shape[-1] // 8, 2, 8)
    hi = raw[..., 0, :].contiguous().view(torch.float16).double().reshape(shape)
    lo = raw[..., 1, :].contiguous().view(torch.float16).double().reshape(shape)
    b = bound.cpu().double()
    s = torch.where(b > 0, torch.floor(torch.log2(b.clamp_min(1e-300))) - 14, torch.zeros_like(b))
    return (hi + lo / 2048.0) * torch.exp2(s).view(-1, 1, 1, 1), hi, lo


def pack_tolerance(x_nhwc: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    return x_nhwc.double().abs() * 2.0 ** -23 + (bound.double() * 2.0 ** -50).view(-1, 1, 1, 1)
