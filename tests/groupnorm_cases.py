"""Cases, fp64 restatement, error bound and host-dispatch census of tests/test_groupnorm_cpu.py and tests/test_groupnorm_gpu.py: the GroupNorm
kernels of csrc/groupnorm.hip and csrc/gn_partial.h against fp64 at the edges of their paths.  Importable without a GPU.

Inputs are functions of the case alone.  Every sample has its own scale, 2^6 apart, and a mean of half that scale; the residual is scaled the
opposite way and the embedding is a slice of a wider tensor (row stride C + 8): a mean, rstd, bound, residual row or embedding row taken from
the wrong sample is off by orders of magnitude, not by rounding.

The restatement `ref_terms` (fp64, NHWC):  mean, biased variance per (sample, group);  z = (x - mean) rstd;  t = z gamma + beta;
s = t sigmoid(t) (act = 1) or t (act = 0);  out = s + r + e.

The elementwise bound `bound_E` of an fp32 evaluation of that chain, u = 2^-24 (one rounding to nearest of a result v costs u |v| at most),
every quantity the fp64 one:

    E = slope |gamma| u (|mean| rstd + 3 |z|)      mean rounded to fp32, times rstd (1 rounding); x - mean, the rounding of rstd, the product
                                                   (3 roundings of z); all of it scaled by gamma and by the slope of the activation
      + slope u (|z gamma| + |t|)                  the product z gamma and the sum with beta (2 roundings; a fused multiply-add makes one)
      + 6 u |s| + 1e-8                             swish_apply (csrc/common.h: 3 ulp of the result = 3 * 2^-23 |s|, or 1e-8 absolute)
      + u (|s + r| + |out|)                        the two final additions (1 rounding each)

slope = 1.1 bounds |d/dt t sigmoid(t)| (its maximum is 1.0998) and is 1 when act = 0, where the swish line drops as well.  A residual read from
its fp16 pairs adds 2 u |r| (csrc/split_f16.h: the last significand bit may be cleared: 2^-23 |r|).  Without normalisation (stats = None) only
the last line remains.  An output that exists as fp16 pairs only adds 2^-22 |out| when decoded (one more cleared bit, with margin for the
scale).  No constant here comes from a run of the kernels; tests/test_groupnorm_cpu.py holds a plain fp32 torch chain to E (it uses 0.3 to 0.9
of it) and checks that E stays of the order of u |out|.

Exact-arithmetic inputs of the statistics (`stats_inputs`): integers times the sample's power of two, with sum x^2 over a whole group below
2^24 in units of the scale squared.  Then every fp32 partial sum and every fmaf of gn_partial_kernel is exact whatever its order, the records
equal the fp64 sums exactly, mean = float(fp64 mean) bit for bit, and rstd lies within one fp32 ulp of float(1 / sqrt(var + eps)) (fp64 sqrt
and divide are correctly rounded on both sides; the ulp is for a tie, should var = q / count - mean^2 be evaluated with a fused multiply-add
on one side).  A dropped, doubled or misplaced element moves a sum by at least one unit, many ulps of the mean.

The census functions restate the host dispatch (stats_chunks, stats_slices, the U / grid cap rule of mf_gn_apply_from_partials_pairs_f32, the
2048-workgroup cap of mf_gn_apply_split_f32) so that the CPU suite can assert which path every case lands on."""
import functools

import torch

from tests import pass_chain_cases as PC

U24 = 2.0 ** -24
EPS = float(torch.tensor(1e-5, dtype=torch.float32))   # the kernels take eps as a float

# (N, H, W, C, G)
STATS_CASES = [
    (2, 1, 1, 32, 8),         # HW = 1: one chunk of one pixel
    (2, 1, 3, 64, 1),         # one group
    (3, 1, 5, 24, 4),         # cpg = 6, C4 = 6, chunks of 3 + 2 pixels
    (2, 1, 67, 96, 32),       # cpg = 3, rowphases = 10 with 16 idle threads, two EMPTY chunks
    (1, 4, 4, 512, 2),        # the cpg-limited slice count (2)
    (1, 4, 4, 512, 32),       # 8 slices
    (2, 3, 3, 1028, 4),       # C4 = 257: the second c4 iteration runs for one lane only
    (1, 5, 5, 2048, 32),      # 8 slices of 256 channels, 4 rowphases
    (1, 5, 5, 2048, 1),       # one slice of 2048 channels: two full c4 iterations
    (1, 2, 2, 1024, 1024),    # cpg = 1 (8 slices of 128 groups)
    (1, 2, 2, 1028, 1028),    # cpg = 1, one slice of 1028 groups: the g += 256 loop, its last turn ragged
    (1, 64, 64, 64, 8),       # 256 pixels per chunk, 16 per thread
]
# the statistics cases that run K.gn_stats only
STATS_ONLY = {(1, 2, 2, 1024, 1024)}

# (N, H, W, C, G, parts) of the from-partials pass
APPLY_CASES = [
    (2, 16, 16, 64, 8, 3),        # baseline
    (2, 16, 16, 96, 8, 3),        # FIXED_C false
    (2, 16, 16, 96, 32, 3),       # cpg = 3
    (3, 5, 7, 24, 3, 1),          # G does not divide 256, idle record threads, one record
    (2, 8, 8, 1024, 256, 4),      # PPT = 1
    (1, 32, 32, 64, 1, 16),       # G = 1, PPT = 256
    (2, 16, 16, 64, 8, 64),       # two records per thread at PPT = 32
    (2, 32, 32, 1024, 32, 9),     # U = 2
    (4, 32, 32, 1024, 32, 9),     # U = 4
    (1, 95, 97, 1024, 32, 16),    # grid capped at 2048 workgroups, a ragged second round
]
# (N, H, W, C, G) of the stats-fed passes
STATS_APPLY_CASES = [(2, 6, 6, 64, 8), (3, 5, 7, 24, 4), (9, 16, 16, 1024, 32)]

APPLY_VARIANTS = PC.APPLY_VARIANTS
APPLY_VARIANTS_LARGE = PC.APPLY_VARIANTS_LARGE
MAXABS_PER_ROW = [4, 4100, 262148, 1048576 + 4]


def case_id(case) -> str:
    return "-".join(str(v) for v in case)


def is_large(case) -> bool:
    return case[0] * case[1] * case[2] * case[3] >= 2048 * 1024


def variants(case):
    return APPLY_VARIANTS_LARGE if is_large(case) else APPLY_VARIANTS


def _gen(tag, case):
    return torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(tag + case_id(case))))


def scales(n):
    return torch.tensor([2.0 ** (6 * i - 3) for i in range(n)])


@functools.lru_cache(maxsize=2)
def apply_inputs(case):
    """(y, gamma, beta, residual, wide) on the CPU, fp32; the embedding is emb_of(wide), a [N, C] slice of the [N, C + 8] tensor (the slice is
    taken after the move to the device: a copy of a slice would be contiguous)"""
    n, h, w, c, G = case[:5]
    g = _gen("apply", case)
    sc = scales(n).view(n, 1, 1, 1)
    y = torch.randn((n, h, w, c), generator=g) * sc + 0.5 * sc
    gamma, beta = 1.0 + 0.3 * torch.randn((c,), generator=g), 0.2 * torch.randn((c,), generator=g)
    r = torch.randn((n, h, w, c), generator=g) * 2.0 * sc.flip(0)
    wide = torch.randn((n, c + 8), generator=g) * 0.5 * sc.view(n, 1)
    return y, gamma, beta, r, wide


def emb_of(wide):
    emb = wide[:, 8:]
    assert emb.stride(0) == wide.shape[1] and emb.shape[1] == wide.shape[1] - 8
    return emb


def bconst_of(gamma, beta, hw, cpg) -> float:
    """the caller's bound of |act(gn(x) gamma + beta)|: |z| <= sqrt(group size)"""
    if gamma is None:
        return float((hw * cpg) ** 0.5)
    return float(gamma.abs().max()) * (hw * cpg) ** 0.5 + float(beta.abs().max())


def cut_records(y, G, parts):
    """the records a convolution would have left: {sum, sum of squares} of `parts` pixel ranges per (sample, group), fp64 [N, parts, G, 2]"""
    n, h, w, c = y.shape
    hw = h * w
    yd = y.double().reshape(n, hw, G, c // G)
    cuts = [hw * k // parts for k in range(parts + 1)]
    rec = torch.stack([torch.stack([yd[:, a:b].sum(dim=(1, 3)), (yd[:, a:b] ** 2).sum(dim=(1, 3))], dim=-1) for a, b in zip(cuts, cuts[1:])], dim=1)
    return rec.contiguous()


# ---------------------------------------------------------------- the fp64 restatement and the bound

def group_stats(x, G):
    """fp64 (mean, rstd-less biased variance) [N, G] over NHWC x"""
    n, h, w, c = x.shape
    xd = x.double().reshape(n, h * w, G, c // G)
    mean = xd.mean(dim=(1, 3))
    var = ((xd - mean.view(n, 1, G, 1)) ** 2).mean(dim=(1, 3))
    return mean, var


def ref_terms(x, G, gamma, beta, act, residual, emb, eps=EPS, stats=None, normalise=True):
    """The quantities of the restatement as fp64 tensors broadcastable to x.  stats [N, G, 2] (mean, rstd) replaces the fp64 statistics;
    normalise=False: s = x (the pass without statistics)."""
    n, h, w, c = x.shape
    xd = x.double()
    one, zero = torch.ones((), dtype=torch.float64, device=x.device), torch.zeros((), dtype=torch.float64, device=x.device)
    ga = gamma.double().view(1, 1, 1, c) if gamma is not None else one
    be = beta.double().view(1, 1, 1, c) if beta is not None else zero
    if normalise:
        if stats is None:
            mean, var = group_stats(x, G)
            rstd = 1.0 / torch.sqrt(var + eps)
        else:
            mean, rstd = stats[..., 0].double(), stats[..., 1].double()
        cpg = c // G
        mean = mean.repeat_interleave(cpg, dim=1).view(n, 1, 1, c)
        rstd = rstd.repeat_interleave(cpg, dim=1).view(n, 1, 1, c)
        z = (xd - mean) * rstd
        t = z * ga + be
    else:
        mean = rstd = z = None
        t = xd
    s = t * torch.sigmoid(t) if act == 1 else t
    r = residual.double() if residual is not None else zero
    e = emb.double().view(n, 1, 1, c) if emb is not None else zero
    return {"mean": mean, "rstd": rstd, "z": z, "t": t, "s": s, "r": r, "e": e, "ga": ga, "out": s + r + e, "act": act, "normalise": normalise}


def ref(x, G, gamma, beta, act, residual, emb, eps=EPS):
    return ref_terms(x, G, gamma, beta, act, residual, emb, eps)["out"]


def bound_E(tm, res_pairs=False):
    """the elementwise bound of the module docstring for the terms `tm` of ref_terms"""
    u = U24
    s, r, out = tm["s"], tm["r"], tm["out"]
    E = u * ((s + r).abs() + out.abs())
    if tm["normalise"]:
        slope = 1.1 if tm["act"] == 1 else 1.0
        g = tm["ga"].abs()
        E = E + slope * g * u * (tm["mean"].abs() * tm["rstd"] + 3.0 * tm["z"].abs()) + slope * u * ((tm["z"] * tm["ga"]).abs() + tm["t"].abs())
        if tm["act"] == 1:
            E = E + 6.0 * u * s.abs() + 1e-8
    if res_pairs:
        E = E + 2.0 * u * r.abs()
    return E


def ratio_rows(got, tm, E):
    """max over each sample of |got - out| / E, as a list of floats"""
    q = (got.double() - tm["out"]).abs() / E
    return [float(v) for v in q.reshape(q.shape[0], -1).amax(dim=1)]


def fp32_chain(x, G, gamma, beta, act, residual, emb, eps=EPS):
    """the same definition evaluated operation by operation in fp32 (statistics from fp64, rounded once)"""
    n, h, w, c = x.shape
    mean, var = group_stats(x, G)
    rstd = (1.0 / torch.sqrt(var + eps)).float().repeat_interleave(c // G, dim=1).view(n, 1, 1, c)
    mean = mean.float().repeat_interleave(c // G, dim=1).view(n, 1, 1, c)
    t = (x - mean) * rstd
    if gamma is not None:
        t = t * gamma.view(1, 1, 1, c)
        t = t + beta.view(1, 1, 1, c)
    s = t * torch.sigmoid(t) if act == 1 else t
    if residual is not None:
        s = s + residual
    if emb is not None:
        s = s + emb.view(n, 1, 1, c)
    return s


def decode_pairs(pairs, bound, shape):
    """the fp16-pair form (csrc/split_f16.h: groups of 8 channels as [hi x 8][lo' x 8], scaled per sample by 2^-(floor(log2 bound) - 14)) in fp64"""
    n = shape[0]
    raw = pairs.contiguous().view(torch.float16).double().reshape(n, -1, 2, 8)
    s = torch.floor(torch.log2(bound.double())) - 14
    return ((raw[:, :, 0] + raw[:, :, 1] / 2048.0) * torch.exp2(s).view(n, 1, 1)).reshape(shape)


# ---------------------------------------------------------------- exact-arithmetic inputs of the statistics

@functools.lru_cache(maxsize=None)
def stats_inputs(case):
    """x (CPU fp32): integers in [-k/2, k] times the sample's scale, k the largest (up to 31) with group size * k^2 < 2^24"""
    n, h, w, c, G = case
    size = h * w * (c // G)
    k = min(31, int((((1 << 24) - 1) // size) ** 0.5))
    assert k >= 4 and size * k * k < (1 << 24), case
    xi = torch.randint(-(k // 2), k + 1, (n, h, w, c), generator=_gen("stats", case)).float()
    assert exact_premise(xi, G) < (1 << 24), case
    return xi * scales(n).view(n, 1, 1, 1)


def exact_premise(xi, G) -> float:
    """max over (sample, group) of sum x^2, x in units of the sample's scale"""
    n, h, w, c = xi.shape
    return float((xi.double() ** 2).reshape(n, h * w, G, c // G).sum(dim=(1, 3)).max())


def stats_chunks(hw):
    return max(1, min(16, (hw + 3) // 4))


def stats_expected(x, G, eps=EPS):
    """(records [N, chunks, G, 2], mean [N, G] fp32, rstd [N, G] fp32) of exact inputs: fp64 sums cut the way gn_partial_kernel cuts the pixels"""
    n, h, w, c = x.shape
    hw = h * w
    chunks = stats_chunks(hw)
    p_per = -(-hw // chunks)
    xd = x.double().reshape(n, hw, G, c // G)
    rec = torch.zeros((n, chunks, G, 2), dtype=torch.float64)
    for k in range(chunks):
        a, b = min(hw, k * p_per), min(hw, (k + 1) * p_per)
        rec[:, k, :, 0] = xd[:, a:b].sum(dim=(1, 3))
        rec[:, k, :, 1] = (xd[:, a:b] ** 2).sum(dim=(1, 3))
    count = float(hw * (c // G))
    tot = rec.sum(dim=1)
    mean = tot[..., 0] / count
    var = (tot[..., 1] / count - mean * mean).clamp_min(0.0)
    return rec, mean.float(), (1.0 / torch.sqrt(var + eps)).float()


def ulp_distance(a, b):
    """largest distance in fp32 units in the last place between two tensors of finite floats of the same sign"""
    return int((a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs().max())


# ---------------------------------------------------------------- the host dispatch, restated

def stats_census(case) -> dict:
    """gn_partial.h: stats_chunks, stats_slices and the loop counts of gn_partial_kernel<false>"""
    n, h, w, c, G = case
    hw, cpg = h * w, c // G
    chunks = stats_chunks(hw)
    sl = 1
    while sl < 8 and n * chunks * sl < 512 and (c // (sl * 2)) % cpg == 0 and (c // (sl * 2)) % 4 == 0 and c // (sl * 2) >= 64:
        sl *= 2
    cs = c // sl
    c4 = cs // 4
    lanes = min(c4, 256)
    rowphases = 256 // lanes
    p_per = -(-hw // chunks)
    sizes = [max(0, min(hw, (k + 1) * p_per) - k * p_per) for k in range(chunks)]
    gs = cs // cpg
    return {"chunks": chunks, "slices": sl, "slices_cpg_limited": sl < 8 and c // (sl * 2) >= 64 and (c // (sl * 2)) % 4 == 0 and (c // (sl * 2)) % cpg != 0,
            "C4": c4, "rowphases": rowphases, "idle_threads": 256 - rowphases * lanes, "c4_iters": -(-c4 // lanes), "c4_last_lanes": c4 - (-(-c4 // lanes) - 1) * lanes,
            "chunk_sizes": sizes, "empty_chunks": sum(1 for s in sizes if s == 0), "px_per_thread": -(-max(sizes) // rowphases), "cpg": cpg, "G": G,
            "groups_per_slice": gs, "g_iters": -(-gs // 256), "lds_bytes": rowphases * cs * 2 * 4}


def apply_census(case) -> dict:
    """mf_gn_apply_from_partials_pairs_f32: U from the workgroup count, the grid cap, the rounds of gn_apply_part_kernel and its record reduction"""
    n, h, w, c, G, parts = case
    per4 = h * w * (c // 4)
    total_blocks = (n * per4 + 255) // 256
    u = 4 if total_blocks >= 4096 else 2 if total_blocks >= 2048 else 1
    bps = -(-per4 // (256 * u))
    cap = (256 * 8 + n - 1) // n
    capped = bps > cap
    bps = min(bps, cap)
    step = bps * 256 * u
    rounds = -(-per4 // step)
    last = per4 - (rounds - 1) * step
    ppt = 256 // G
    return {"U": u, "bps": bps, "capped": capped, "rounds": rounds, "ragged_last_round": last % (256 * u) != 0, "ragged_tail": per4 % (256 * u) != 0,
            "FIXED_C": 256 % (c // 4) == 0, "cpg_mod4": (c // G) % 4, "cpg": c // G, "G": G, "PPT": ppt, "records_per_thread": -(-parts // ppt),
            "idle_record_threads": 256 - ppt * G, "parts": parts}


def stats_apply_census(case) -> dict:
    """mf_gn_apply_split_f32: at most 2048 workgroups of 256 threads; beyond that the grid-stride loop walks on, across samples"""
    n, h, w, c, G = case
    total4 = n * h * w * (c // 4)
    blocks = min(2048, (total4 + 255) // 256)
    per4 = h * w * (c // 4)
    second = total4 > blocks * 256
    return {"total4": total4, "blocks": blocks, "second_iteration": second, "crosses_samples": second and (blocks * 256) // per4 != 0, "cpg_mod4": (c // G) % 4}
