"""The quantizer (csrc/vq.hip), the window kernels (csrc/window_ops.hip) and the held-out loss kernels (csrc/loss.hip) at their path boundaries:
the inputs, the exact references and the host rules restated in plain Python, shared by tests/test_small_edges_cpu.py (which proves the premises)
and tests/test_small_edges_gpu.py (which holds the kernels to them).  Nothing here touches the device.

The premises, each asserted on the CPU:
  quantizer  z and the codebook are multiples of 2^-6 in [-2, 2] and C <= 16: every product, partial sum, zz + ee and 2 ze of the kernel's formula
             is a multiple of 2^-12 below 2^8, exact in fp32 -- d IS the squared distance, so the index is the integer argmin, no tolerance;
  merge      the tent weights are integers, p a multiple of 2^-4 with |p| <= 8: w p, every fmaf and den are exact while den * 128 < 2^24, and
             float32(acc / den) evaluated in fp64 is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2);
  loss       pred and target multiples of 2^-8 with |v| <= 4 and a pooling factor that is a power of two: the pooled mean, d, |d|, d^2 are
             exact, and the fp64 partial sums (multiples of 2^-16 below 2^44 units) are exact in any order."""
from __future__ import annotations

import torch

from tests.window_cases import RefPlan

SENTINEL = -7777.0            # no input of these cases and no result of a kernel on them equals it
GUARD = 64                    # sentinel floats behind every output


# ================================================================================================ the quantizer
VQ_TILE, VQ_CHUNK, VQ_MAX_SLICES = 256, 512, 16
VQ_GRID = 2.0 ** -6
VQ_SPAN = 128                 # |z|, |e| <= 128 grid units = 2.0
VQ_TWIN_PIXEL = 100           # the pixel that equals the twin codes 4 and 5 (cases with K >= 8)


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def plan_slices(P: int, K: int):
    """vq.hip's plan_slices restated -> (codes per slice S, slices): enough slices that pixel tiles x slices reaches 1024 workgroups, at most 16,
    S a multiple of 64"""
    tiles = cdiv(P, VQ_TILE)
    want = max(1, min(VQ_MAX_SLICES, cdiv(1024, tiles)))
    s = cdiv(cdiv(K, want), 64) * 64
    return s, cdiv(K, s)


# (P, K) -> (S, slices), worked out by hand from the rule above
PLAN_TABLE = {
    (231, 1): (64, 1), (231, 63): (64, 1), (231, 64): (64, 1), (231, 65): (64, 2), (231, 200): (64, 4), (231, 1000): (64, 16),
    (231, 8193): (576, 15), (231, 10000): (640, 16), (231, 16384): (1024, 16), (16384, 8192): (512, 16),
    (25600, 1000): (128, 8),                       # 100 tiles: want 11, ceil(1000 / 11) = 91 -> 128
    (100000, 1500): (512, 3),                      # 391 tiles: want 3
    (262144, 1100): (1152, 1),                     # 1024 tiles: want 1
    (5 * 229 * 229, 1100): (1152, 1),              # 1025 tiles
}


def vq_boundaries(K: int, S: int):
    """every code index b in (0, K) at which a slice or a 512-code chunk of a slice begins: b - 1 and b are scanned by different workgroups, or
    in different staging rounds of one"""
    out = set()
    for k0 in range(0, K, S):
        if k0:
            out.add(k0)
        out.update(range(k0 + VQ_CHUNK, min(K, k0 + S), VQ_CHUNK))
    return sorted(out)


def vq_chunks(K: int, S: int):
    """the chunk lengths of every slice"""
    return [[min(VQ_CHUNK, min(K, k0 + S) - c0) for c0 in range(k0, min(K, k0 + S), VQ_CHUNK)] for k0 in range(0, K, S)]


# name -> z shape, K.  Every C at one tile and four slices; one code, one slice, a one-code last slice, 15 slices, a partial second chunk;
# 391 tiles x 3 slices with a short last one; 1025 tiles x 1 slice of 512 + 512 + 76 codes, 61 live pixels in the last tile, tiles across samples
VQ_CASES = {**{f"C{c}": ((3, c, 7, 11), 200) for c in range(1, 17)},
            **{f"K{k}": ((3, 4, 7, 11), k) for k in (1, 63, 64, 65, 8193, 10000)},
            "three_slices": ((4, 4, 100, 250), 1500),
            "one_slice": ((5, 3, 229, 229), 1100)}


def vq_dyadic_case(name: str):
    """-> dict(z [N,C,H,W] fp32, cb [K,C] fp32, zi [P,C] / ci [K,C] int64 grid units, S, slices, pairs).  Random grid points, plus for every
    boundary b one random vector planted at b - 1 AND b with two pixels equal to it (an exact tie at distance 0 across the boundary), a
    copy of the first planted vector at K - 1, and one vector at the neighbours 4 and 5 of the first chunk with a pixel equal to it."""
    shape, K = VQ_CASES[name]
    n, c, h, w = shape
    P = n * h * w
    g = torch.Generator().manual_seed(7000 + sorted(VQ_CASES).index(name))
    draw = lambda *s: torch.randint(-VQ_SPAN, VQ_SPAN + 1, s, generator=g, dtype=torch.int64)
    zi, ci = draw(P, c), draw(K, c)
    S, slices = plan_slices(P, K)
    pairs = vq_boundaries(K, S)
    assert 2 * len(pairs) + 2 <= P
    for j, b in enumerate(pairs):
        v = draw(c)
        ci[b - 1], ci[b] = v, v
        zi[1 + j], zi[P - 2 - j] = v, v           # in the first and in the last pixel tile
    if pairs and K - 1 not in pairs:
        ci[K - 1] = ci[pairs[0]]
    if K >= 8:
        v = draw(c)
        ci[4], ci[5], zi[VQ_TWIN_PIXEL] = v, v, v  # a tie INSIDE one staging round: only the strict comparison of the scan keeps the first
    zi[0], zi[P - 1] = VQ_SPAN, -VQ_SPAN          # the corners of the grid: the largest sums of the premise
    if K > 3:
        ci[1], ci[2] = -VQ_SPAN, VQ_SPAN
    z = torch.moveaxis((zi.float() * VQ_GRID).view(n, h, w, c), -1, 1).contiguous()
    return dict(z=z, cb=ci.float() * VQ_GRID, zi=zi, ci=ci, S=S, slices=slices, pairs=pairs, P=P, K=K)


def int_distances(zi: torch.Tensor, ci: torch.Tensor) -> torch.Tensor:
    """[pixels, K] int64: the squared distances in units of 2^-12"""
    return (zi * zi).sum(1)[:, None] + (ci * ci).sum(1)[None, :] - 2 * (zi @ ci.t())


def pixel_subset(P: int, seed: int = 5) -> torch.Tensor:
    """every pixel of a small case; of a large one the first tile, the last (partial) tile and 512 seeded pixels"""
    if P <= 4096:
        return torch.arange(P)
    g = torch.Generator().manual_seed(seed)
    last = (P - 1) // VQ_TILE * VQ_TILE
    return torch.unique(torch.cat([torch.arange(VQ_TILE), torch.arange(last, P), torch.randint(0, P, (512,), generator=g)]))


def cpu_formula(z, cb):
    """[pixels, K] fp32 distances by the kernel's stated arithmetic: (sum z^2 + sum e^2) - 2 sum z e, each sum in index order, every
    operation rounded on its own (torch's elementwise fp32 ops: no contraction)"""
    zf = torch.moveaxis(z, 1, -1).reshape(-1, z.shape[1])
    zz, ee, ze = zf[:, 0] * zf[:, 0], cb[:, 0] * cb[:, 0], zf[:, None, 0] * cb[None, :, 0]
    for c in range(1, z.shape[1]):
        zz = zz + zf[:, c] * zf[:, c]
        ee = ee + cb[:, c] * cb[:, c]
        ze = ze + zf[:, None, c] * cb[None, :, c]
    return (zz[:, None] + ee[None, :]) - 2.0 * ze


def sqerr_tolerance(terms: int, total: float) -> float:
    """how far two fp64 sums of the same `terms` non-negative numbers may lie apart: each is within (terms - 1) 2^-53 of the exact sum relative to
    it, whatever its order (Higham, Accuracy and Stability, eq. 4.4; `terms` for `terms - 1` covers the second-order part)"""
    return 2.0 * terms * 2.0 ** -53 * abs(total)


def check_quantizer(z, cb, zq, idx, sq=None):
    """z_q bit-equal to z + (e_idx - z); idx the CPU argmin where the fp64 margin exceeds tau, else within tau of the CPU minimum; the loss
    within the reordering error of an fp64 sum of the same fp32 squares"""
    n, c, h, w = z.shape
    d = cpu_formula(z, cb)
    want = torch.argmin(d, dim=1)
    idx = idx.cpu().long()
    zf = torch.moveaxis(z, 1, -1).reshape(-1, c)
    finite = torch.isfinite(zf).all(1)
    assert torch.equal(idx[~finite], want[~finite])                          # a NaN distance: the first one wins, like torch.argmin
    zd, ed = zf.double(), cb.double()
    d64 = (zd ** 2).sum(1)[:, None] + (ed ** 2).sum(1)[None, :] - 2.0 * zd @ ed.t()   # fp64: error ~1e-16 of the scale, far below tau
    tau = 2.0 ** -20 * ((zd ** 2).sum(1) + float((ed ** 2).sum(1).max()))
    two = torch.topk(d64, min(2, cb.shape[0]), dim=1, largest=False).values
    clear = finite & ((two[:, -1] - two[:, 0] > tau) if cb.shape[0] > 1 else torch.ones_like(finite))
    assert torch.equal(idx[clear], want[clear])
    rows = torch.arange(d.shape[0])
    near = finite & ~clear
    if near.any():
        assert bool(((d[rows, idx] - d[rows, want]).double()[near] <= tau[near]).all())
    zq_want = torch.moveaxis((zf + (cb[idx] - zf)).view(n, h, w, c), -1, 1)
    assert torch.equal(torch.nan_to_num(zq.cpu(), nan=7.0), torch.nan_to_num(zq_want, nan=7.0))
    if sq is not None:
        sq_terms = (cb[idx] - zf) ** 2
        want_sq = float(sq_terms.double().sum())
        assert abs(float(sq) - want_sq) <= sqerr_tolerance(sq_terms.numel(), want_sq)
    return int(clear.sum()), int(near.sum())


def adversarial(K_, C, shape, seed):
    g = torch.Generator().manual_seed(seed)
    cb = torch.rand((K_, C), generator=g) * 2 - 1
    if K_ > 8:
        cb[7] = cb[3]                                   # duplicate rows: ties go to the lower index
        cb[K_ - 1] = cb[3]
    z = torch.randn(shape, generator=g) * 0.7
    n, c, h, w = shape
    zf = torch.moveaxis(z, 1, -1).reshape(-1, c).clone()
    zf[0] = cb[min(3, K_ - 1)]                          # z equal to a (duplicated) code: d rounds to ~0, possibly negative
    zf[1] = cb[K_ - 1]
    zf[2] = cb[min(5, K_ - 1)] * 1000.0 + 0.5           # large norm: the formula cancels
    zf[3] = cb[0] + 1e-4                                # a code plus a hair: tiny, possibly negative d
    zf[4:8] = zf[4:8] * 30.0
    return torch.moveaxis(zf.view(n, h, w, c), -1, 1).contiguous(), cb


# ================================================================================================ the windows
WIN_CAP = 2048 * 256          # work items of one pass of a grid-stride loop behind blocks_for's cap


def vector_eligible(ref: RefPlan) -> bool:
    """window_geometry's by4: the last axis' canvas and window extents and every origin of it a multiple of 4"""
    return ref.canvas[-1] % 4 == 0 and ref.window[-1] % 4 == 0 and all(o % 4 == 0 for o in ref.origins[-1])


def passes(work: int) -> int:
    """passes of the grid-stride loop over `work` items (quads on the 16-byte path, elements otherwise)"""
    return cdiv(work, WIN_CAP)


def prod(v) -> int:
    out = 1
    for x in v:
        out *= int(x)
    return out


# name -> B, C, canvas, window, stride
GATHER_CASES = {
    "cap_vector": dict(B=1, C=9, canvas=(384, 384), window=(256, 256), stride=128),            # 589 824 quads: a second pass on 16-byte loads
    "cap_element": dict(B=1, C=2, canvas=(384, 388), window=(256, 256), stride=(128, 130)),    # origins (0, 130, 132): 786 432 elements
    "origins32_vector": dict(B=2, C=3, canvas=(4, 132), window=(4, 8), stride=(4, 4)),
    "origins32_element": dict(B=2, C=3, canvas=(39, 5), window=(8, 3), stride=(1, 1)),         # 32 origins on the FIRST spatial axis
    "vector3d": dict(B=2, C=3, canvas=(5, 9, 16), window=(3, 5, 8), stride=(1, 2, 4)),         # three origins per axis
    "whole_canvas": dict(B=2, C=3, canvas=(8, 12), window=(8, 12), stride=None),
    "one_cell": dict(B=2, C=3, canvas=(5, 7), window=(1, 1), stride=1),
}
# merge geometries with the largest per-axis cover; `exact`: run on the dyadic grid (den * 128 < 2^24 asserted on the CPU)
MERGE_CASES = {
    "cap": dict(B=2, C=8, canvas=(384, 384), window=(256, 256), stride=128, cover=4),          # 589 824 quads / 2 359 296 cells
    "dense": dict(B=2, C=3, canvas=(20, 20), window=(4, 4), stride=1, cover=16),
    "dense_vector": dict(B=2, C=3, canvas=(14, 40), window=(8, 16), stride=(2, 4), cover=16),
    "origins32_vector": dict(B=2, C=3, canvas=(4, 132), window=(4, 8), stride=(4, 4), cover=2),
    "origins32_element": dict(B=1, C=2, canvas=(4, 39), window=(4, 8), stride=(4, 1), cover=8),
    "clamped_vector": dict(B=2, C=3, canvas=(8, 28), window=(8, 16), stride=(8, 8), cover=3),  # origins (0, 8, 12)
    "clamped_element": dict(B=2, C=3, canvas=(8, 13), window=(8, 8), stride=4, cover=3),       # origins (0, 4, 5)
    "cover8_3d": dict(B=2, C=2, canvas=(6, 12, 12), window=(4, 8, 8), stride=(2, 4, 4), cover=8),
    "dense_3d": dict(B=1, C=2, canvas=(5, 9, 16), window=(3, 5, 8), stride=(1, 2, 4), cover=18),
}
WIN_GRID, WIN_SPAN = 2.0 ** -4, 128            # p = k / 16, |k| <= 128


def ref_plan(case: dict, weight: str = "tent") -> RefPlan:
    return RefPlan(case["canvas"], case["window"], case["stride"], weight)


def bits_input(shape, seed: int) -> torch.Tensor:
    """fp32 of random BITS: NaNs with payloads, infinities, denormals, and -0 / +0 / a quiet and a signalling NaN planted at the ends"""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32)
    flat = bits.view(-1)
    special = torch.tensor([-2 ** 31, 0, 0x7FC00123, 0x7F800001, 0xFFC00001 - 2 ** 32], dtype=torch.int32)   # -0, +0, a quiet, a signalling, a negative NaN
    flat[:5] = special
    flat[-5:] = special
    return bits.view(torch.float32)


def dyadic_windows(shape, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-WIN_SPAN, WIN_SPAN + 1, shape, generator=g, dtype=torch.int64).float() * WIN_GRID


def merge_den(ref: RefPlan) -> torch.Tensor:
    """the integer sum of the covering windows' weights at every canvas cell"""
    w = ref.weights(torch.int64)
    den = torch.zeros(ref.canvas, dtype=torch.int64)
    for m in range(ref.M):
        den[ref.slices(m)] += w
    return den


# ================================================================================================ the held-out loss
LANES, QUAD_SPAN, CHUNK_MIN, PARTS_MAX = 256, 1024, 8192, 256
LOSS_GRID, LOSS_SPAN = 2.0 ** -8, 1024        # v = k / 256, |k| <= 1024
ROWS_MAX = 65535
DIFFUSE_CAP = 2048 * 256
# x_0's shape: 524 296 quads on 16-byte loads (8 past one pass of the capped grid); 524 292 elements in rows of 131 073 (4 past it)
DIFFUSE_CASES = {"vector": (4, 8, 65537), "element": (4, 131073)}


def loss_chunk(per: int) -> int:
    """loss.hip's loss_chunk restated: 8192 elements per partial, or -- from 2 Mi elements per row on -- what keeps a row at 256 partials,
    rounded up to the 1024 elements the lanes take per pass"""
    if cdiv(per, CHUNK_MIN) <= PARTS_MAX:
        return CHUNK_MIN
    return cdiv(cdiv(per, PARTS_MAX), QUAD_SPAN) * QUAD_SPAN


def loss_parts(per: int) -> int:
    return cdiv(per, loss_chunk(per))


# per-row length -> (chunk, partials, the last partial's elements, pred's shape behind the batch axis)
ROW_SIZES = {2097152: (8192, 256, 8192, (8, 512, 512)), 2097156: (9216, 228, 5124, (1, 4, 524289)), 2097153: (9216, 228, 5121, (1, 3, 699051))}


def dyadic_rows(shape, seed: int) -> torch.Tensor:
    """int64 grid units k of v = k / 256, |k| <= 1024, the extremes planted"""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-LOSS_SPAN, LOSS_SPAN + 1, shape, generator=g, dtype=torch.int64)
    k.view(-1)[0], k.view(-1)[-1] = LOSS_SPAN, -LOSS_SPAN
    return k


def pool_sum_int(tk: torch.Tensor, f: int) -> torch.Tensor:
    """[B, C, spatial...] int64 -> the f^dims block SUMS"""
    if f == 1:
        return tk
    B, C = tk.shape[:2]
    sp = [s // f for s in tk.shape[2:]]
    if len(sp) == 2:
        return tk.reshape(B, C, sp[0], f, sp[1], f).sum((3, 5))
    return tk.reshape(B, C, sp[0], f, sp[1], f, sp[2], f).sum((3, 5, 7))


def exact_loss_sums(pk: torch.Tensor, tk: torch.Tensor, f: int) -> torch.Tensor:
    """[B, 2] fp64, exact: per row (sum |d|, sum d^2) of d = pred - block mean for a power-of-two f, from the grid units alone.  n d is an
    integer in units of 2^-8; the sums are divided once, by powers of two"""
    n = f ** (pk.ndim - 2)
    assert n & (n - 1) == 0
    d = n * pk - pool_sum_int(tk, f)
    rows = lambda v: v.reshape(v.shape[0], -1).sum(1)
    s1, s2 = rows(d.abs()), rows(d * d)
    assert int(s2.max()) < 2 ** 62
    return torch.stack((s1.double() / (n / LOSS_GRID), s2.double() / (n / LOSS_GRID) ** 2), dim=1)
