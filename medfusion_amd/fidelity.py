"""Fidelity of a generated set in a feature space: improved precision / recall (k-NN manifolds, Kynkaanniemi et al. 2019) and the Frechet distance,
the figures the reference's evaluate_images.py logs -- everything after the feature extractor (csrc/fidelity.hip, include/medfusion_hip.h
MfFidelityDesc).

The definition is stated HERE (README "Fidelity") and equals the reference's in exact arithmetic.  Features real [N, D], fake [M, D], fp32.  The
pivot c is the fp64 column mean of `real` rounded to fp32, xt = fl32(x - c), n(x) = the fp64 sum of xt_k^2 rounded to fp32,
    d2(x, y) = max(0, fl32(fl32(n(x) + n(y)) - 2 dot(xt, yt))),     dot: ONE fp32 fmaf chain over k ascending (the fp32 matrix cores).
The radius of row i of a bank X is r2_i = the (knn + 1)-th smallest of d2(X_i, X_j) over all j, the j = i entry being exactly 0; query j is inside
the manifold of R when d2(R_i, Q_j) < r2_i for some i (strict, on squared values: no square root on the device).  precision = the share of fake
rows inside the manifold of real, recall = the share of real rows inside the manifold of fake, both with the pivot of real.  The N x M matrix is
never materialised (the reference builds it in full and loops over the generated samples in Python).

frechet_distance is host-side fp64 torch: |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2, the last term as the sum of sqrt(max(lambda_k, 0)) over
the eigenvalues of S1^1/2 S2 S1^1/2 -- two symmetric eigen-decompositions, no general sqrtm, no complex parts.

Neighbours (README "Neighbours"): nearest_neighbours -- the k <= 16 nearest rows of a second bank WITH indices, ordered by (d2, index), optionally
with the candidates' distances recomputed exactly --, density_coverage (Naeem et al. 2020) and memorization_report (authenticity, copy ratio) on the
same d2, tile and pivot; the matrix is not materialised by them either.

Kernel distances (README "Kernel distances"): kid -- the Kernel Inception Distance, the mean and spread of the unbiased MMD^2 under
(gamma x.y + coef0)^degree over seeded subsets --, mmd2 of the full sets under a polynomial or Gaussian kernel, and kernel_matrix; the sums of k are
taken on the same tile while it is in the accumulators (MfKernelSumDesc), all subsets of a term in one launch, the matrix never materialised.

Every argument error is a ValueError that names the argument, raised before anything touches the device."""
from __future__ import annotations

import torch

from . import kernels as K
from . import lib as L

TILE = 128               # rows (and columns) of the distance tile of one workgroup
SLOTS = 512              # workgroups the MI355X holds at once: two per compute unit (registers and LDS of the fused kernels), 256 units.
                         # A model: its choice was timed at ONE shape (10 000 x 10 000 x 2048, profiles/fidelity_bench.txt), nowhere else.


def plan_splits(rows: int, cols: int) -> int:
    """How many splits S of the `cols` axis a launch over `rows` x `cols` distances takes.  A workgroup owns one tile of `rows` and walks
    ceil(col tiles / S) column tiles; the chip runs SLOTS workgroups at a time, so the launch lasts ceil(row tiles * S / SLOTS) rounds of that walk.
    S minimises rounds x walk -- enough workgroups for the chip when the bank has few rows, and no nearly empty last round -- among 1 .. 16 and
    at most the number of column tiles; of equal plans the one with the fewest splits (the smallest workspace)."""
    if rows < 1 or cols < 1:
        raise ValueError(f"plan_splits: rows={rows} cols={cols}")
    row_tiles, col_tiles = -(-rows // TILE), -(-cols // TILE)
    cost = lambda s: -(-row_tiles * s // SLOTS) * -(-col_tiles // s)
    return min(range(1, min(L.FIDELITY_MAX_SPLITS, col_tiles) + 1), key=lambda s: (cost(s), s))


def workspace_bytes(n: int, m: int, splits: int) -> int:
    """the bytes mf_fidelity_workspace_bytes answers for (N, M, splits): the k-NN partial lists or the manifold's partial flags, whichever is more"""
    return max(splits * n * L.FIDELITY_LIST * 4, (splits * m + 15) // 16 * 16)


# ------------------------------------------------------------------------------------------------ argument rules (host only)
def _check_bank(name: str, t, min_rows: int = 2) -> None:
    """the host-side rules of one bank; the device is asked last, by _check_device, when every argument passed these"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: a tensor, got {type(t).__name__}")
    if t.dim() != 2 or t.shape[1] == 0:
        raise ValueError(f"{name}: a 2-D [rows, D] tensor of features, got shape {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: fp32, got {t.dtype}")
    if t.shape[0] < min_rows:
        raise ValueError(f"{name}: at least {min_rows} row(s), got {t.shape[0]}")
    if t.shape[0] >= 1 << 24 or t.shape[1] > 65536:
        raise ValueError(f"{name}: under 2^24 rows of at most 65536 features, got {tuple(t.shape)}")


def _check_device(**named) -> None:
    for name, t in named.items():
        if not t.is_cuda:
            raise ValueError(f"{name}: on a ROCm device -- the fidelity kernels have no CPU path, got a {t.device.type} tensor")


def _check_same_d(name: str, t: torch.Tensor, first_name: str, first: torch.Tensor) -> None:
    if t.shape[1] != first.shape[1]:
        raise ValueError(f"{name}: D = {first.shape[1]} like {first_name}, got {t.shape[1]}")
    if t.device != first.device:
        raise ValueError(f"{name}: on the device of {first_name}")


def _check_knn(knn, rows: int, bank: str) -> None:
    if isinstance(knn, bool) or not isinstance(knn, int) or not 1 <= knn <= L.FIDELITY_LIST - 1:
        raise ValueError(f"knn: an integer in 1 .. {L.FIDELITY_LIST - 1}, got {knn!r}")
    if knn >= rows:
        raise ValueError(f"knn: {knn} neighbours need more than the {rows} rows of {bank}")


def _check_vector(name: str, v, n: int, like: torch.Tensor) -> None:
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.dim() != 1 or v.shape[0] != n:
        raise ValueError(f"{name}: an fp32 [{n}] tensor, got {tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__}")
    if v.device != like.device:
        raise ValueError(f"{name}: on the device of the features")


def _check_splits(splits) -> None:
    if splits is not None and (isinstance(splits, bool) or not isinstance(splits, int) or not 1 <= splits <= L.FIDELITY_MAX_SPLITS):
        raise ValueError(f"_splits: None or 1 .. {L.FIDELITY_MAX_SPLITS}, got {splits!r}")


def _aligned(t: torch.Tensor) -> torch.Tensor:
    """the pivot: contiguous and 16-byte aligned, so that it never decides the load path of the banks"""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _pivot(x: torch.Tensor, pivot) -> torch.Tensor:
    return K.feat_colmean(x) if pivot is None else _aligned(pivot)


# ------------------------------------------------------------------------------------------------ the public functions
def pairwise_sqdist(x: torch.Tensor, y: torch.Tensor = None, *, pivot: torch.Tensor = None) -> torch.Tensor:
    """d2 between the rows of x [N, D] and of y [M, D] -> [N, M] (y=None: x against itself, the diagonal exactly 0).  pivot=None: the column
    mean of x.  For tests and small sets: precision_recall never forms this matrix."""
    _check_bank("x", x)
    if y is not None:
        _check_bank("y", y, min_rows=1)
        _check_same_d("y", y, "x", x)
    if pivot is not None:
        _check_vector("pivot", pivot, x.shape[1], x)
    _check_device(x=x)
    x = x.contiguous()
    c = _pivot(x, pivot)
    nx = K.feat_norms(x, c)
    if y is None:
        return K.feat_sqdist(x, nx, x, nx, c, same_bank=True)
    y = y.contiguous()
    return K.feat_sqdist(x, nx, y, K.feat_norms(y, c), c)


def knn_radii(x: torch.Tensor, knn: int = 3, *, pivot: torch.Tensor = None, squared: bool = False, _splits: int = None) -> torch.Tensor:
    """the k-NN radius of every row of x -> [N]: the distance to its knn-th neighbour (the (knn + 1)-th smallest with the row itself counted, the
    reference's topk(knn + 1)); squared=True: r2 as the device holds it, else its square root"""
    _check_bank("x", x)
    _check_knn(knn, x.shape[0], "x")
    _check_splits(_splits)
    if pivot is not None:
        _check_vector("pivot", pivot, x.shape[1], x)
    _check_device(x=x)
    x = x.contiguous()
    c = _pivot(x, pivot)
    r2 = K.knn_radii_sq(x, K.feat_norms(x, c), c, knn, _splits or plan_splits(x.shape[0], x.shape[0]))
    return r2 if squared else torch.sqrt(r2)


def manifold_hits(ref: torch.Tensor, radii_sq: torch.Tensor, query: torch.Tensor, *, pivot: torch.Tensor = None, _splits: int = None) -> torch.Tensor:
    """is query j inside the manifold of ref: any_i [d2(ref_i, query_j) < radii_sq[i]] -> bool [M].  pivot=None: the column mean of ref."""
    _check_bank("ref", ref)
    _check_vector("radii_sq", radii_sq, ref.shape[0], ref)
    _check_bank("query", query, min_rows=1)
    _check_same_d("query", query, "ref", ref)
    _check_splits(_splits)
    if pivot is not None:
        _check_vector("pivot", pivot, ref.shape[1], ref)
    _check_device(ref=ref)
    ref, query = ref.contiguous(), query.contiguous()
    c = _pivot(ref, pivot)
    hit, _ = K.manifold_hits(ref, K.feat_norms(ref, c), radii_sq.contiguous(), query, K.feat_norms(query, c), c,
                             _splits or plan_splits(query.shape[0], ref.shape[0]))
    return hit.bool()


def _pr_counts(real, fake, knn, splits):
    """the two hit counts as one int32 [2] device tensor: (fake rows inside real's manifold, real rows inside fake's)"""
    c = K.feat_colmean(real)
    nr, nf = K.feat_norms(real, c), K.feat_norms(fake, c)
    n, m = real.shape[0], fake.shape[0]
    r2_real = K.knn_radii_sq(real, nr, c, knn, splits or plan_splits(n, n))
    r2_fake = K.knn_radii_sq(fake, nf, c, knn, splits or plan_splits(m, m))
    _, in_real = K.manifold_hits(real, nr, r2_real, fake, nf, c, splits or plan_splits(m, n), want_hits=False)
    _, in_fake = K.manifold_hits(fake, nf, r2_fake, real, nr, c, splits or plan_splits(n, m), want_hits=False)
    return torch.cat([in_real, in_fake])


def precision_recall(real: torch.Tensor, fake: torch.Tensor, knn: int = 3, *, _splits: int = None) -> dict:
    """improved precision and recall of `fake` against `real` -> {"precision", "recall", "n_real", "n_fake", "knn"}.  Four tiled matrix-core launches (two for the radii, two for the hits),
    no N x M matrix; the host waits exactly once, for the two counts."""
    _check_bank("real", real)
    _check_bank("fake", fake)
    _check_same_d("fake", fake, "real", real)
    _check_knn(knn, real.shape[0], "real")
    _check_knn(knn, fake.shape[0], "fake")
    _check_splits(_splits)
    _check_device(real=real)
    real, fake = real.contiguous(), fake.contiguous()
    in_real, in_fake = _pr_counts(real, fake, knn, _splits).tolist()          # the one copy to the host
    return {"precision": in_real / fake.shape[0], "recall": in_fake / real.shape[0], "n_real": int(real.shape[0]), "n_fake": int(fake.shape[0]), "knn": knn}


# ------------------------------------------------------------------------------------------------ neighbours (README "Neighbours")
def nn_workspace_bytes(m: int, splits: int) -> int:
    """the bytes mf_nn_workspace_bytes answers for M query rows: the partial lists of 16 eight-byte (d2, index) keys per row and split"""
    return splits * m * L.FIDELITY_LIST * 8


def nn_ok(n: int, m: int, d: int, k, splits: int, same_bank: bool = False) -> bool:
    """the rules of the neighbour calls of the C ABI (mf_nn_ok), restated on the host"""
    return (1 <= n < 1 << 24 and 1 <= m < 1 << 24 and 1 <= d <= 65536 and 1 <= k <= L.FIDELITY_LIST and 1 <= splits <= L.FIDELITY_MAX_SPLITS
            and (not same_bank or m == n) and k <= n - int(bool(same_bank)))


def _check_k(name: str, k, rows: int, bank: str, leave_one_out: bool = False) -> None:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= L.FIDELITY_LIST:
        raise ValueError(f"{name}: an integer in 1 .. {L.FIDELITY_LIST}, got {k!r}")
    if k > rows - int(leave_one_out):
        raise ValueError(f"{name}: {k} neighbours need {'more than' if leave_one_out else 'at least'} {k} rows of {bank}, got {rows}")


def _search(query, nq, ref, nref, c, k, splits, exclude_self, refine):
    """-> (d2 fp32 [M, k], index int32 [M, k]) ascending by (d2, index); refine: the k candidates' d2 recomputed exactly and each row sorted again"""
    d2, index = K.nn_search(query, nq, ref, nref, c, k, splits or plan_splits(query.shape[0], ref.shape[0]), exclude_self)
    if not refine:
        return d2, index
    d2 = K.pair_sqdist(query, ref, index)
    if k > 1:                                                                  # by (refined value, index): a stable sort by value of the rows in index order
        index, by_index = torch.sort(index, dim=1, stable=True)
        d2, by_value = torch.sort(d2.gather(1, by_index), dim=1, stable=True)
        index = index.gather(1, by_value)
    return d2, index


def nearest_neighbours(query: torch.Tensor, ref: torch.Tensor = None, k: int = 1, *, pivot: torch.Tensor = None, refine: bool = True,
                       squared: bool = False, _splits: int = None):
    """The k <= 16 nearest rows of ref [N, D] for every row of query [M, D] -> (dist fp32 [M, k], index int64 [M, k]), nearest first.  ref=None:
    the bank against itself, every row's own entry left out (by index: a second row with the same features stays a neighbour at distance 0).
    pivot=None: the column mean of ref (of query when ref is None).  The N x M matrix is never written; nothing synchronises.

    The candidates are the k smallest pairs (d2, index) in lexicographic order -- d2 of pairwise_sqdist compared as a float, then the smaller
    index: with unique indices a total order, so the result does not depend on the tile, the splits or the place of a row in its bank.
    refine=False returns those, the values being the bits of pairwise_sqdist.  refine=True recomputes the k candidates' distances exactly --
    fl32 of the fp64 sum of fl32(x_k - y_k)^2, relative error <= 4 2^-24, equal rows exactly 0 -- and sorts each row again by (refined value,
    index).  The candidate SET is still chosen on d2, which carries the error E_ij = (D + 8) 2^-24 (n_i + n_j): a true neighbour can be missed
    only when it lies within E of the k-th.  squared=False returns the square root."""
    loo = ref is None
    _check_bank("query", query, min_rows=2 if loo else 1)
    if not loo:
        _check_bank("ref", ref, min_rows=1)
        _check_same_d("ref", ref, "query", query)
    bank = query if loo else ref
    _check_k("k", k, bank.shape[0], "query" if loo else "ref", loo)
    _check_splits(_splits)
    if pivot is not None:
        _check_vector("pivot", pivot, query.shape[1], query)
    _check_device(query=query)
    query = query.contiguous()
    ref = query if loo else ref.contiguous()
    c = _pivot(ref, pivot)
    nq = K.feat_norms(query, c)
    nref = nq if loo else K.feat_norms(ref, c)
    d2, index = _search(query, nq, ref, nref, c, k, _splits, loo, bool(refine))
    return (d2 if squared else torch.sqrt(d2)), index.long()


def density_coverage(real: torch.Tensor, fake: torch.Tensor, knn: int = 5, *, _splits: int = None) -> dict:
    """density and coverage (Naeem et al. 2020) of `fake` against `real` -> {"density", "coverage", "n_real", "n_fake", "knn"}, on this module's d2
    and radii with the pivot of real: r2_i = knn_radii(real, knn, squared=True), count_j = #{ i : d2(R_i, F_j) < r2_i },
    density = sum_j count_j / (knn M), coverage = mean_i [ min_j d2(R_i, F_j) < r2_i ] (strict, squared, unrefined values).  Three matrix-core
    launches with their finish launches -- radii, counts, the 1-NN of real in fake --, no N x M matrix; the host waits once."""
    _check_bank("real", real)
    _check_bank("fake", fake)
    _check_same_d("fake", fake, "real", real)
    _check_knn(knn, real.shape[0], "real")
    _check_splits(_splits)
    _check_device(real=real)
    real, fake = real.contiguous(), fake.contiguous()
    n, m = real.shape[0], fake.shape[0]
    c = K.feat_colmean(real)
    nr, nf = K.feat_norms(real, c), K.feat_norms(fake, c)
    r2 = K.knn_radii_sq(real, nr, c, knn, _splits or plan_splits(n, n))
    _, total = K.manifold_counts(real, nr, r2, fake, nf, c, _splits or plan_splits(m, n), want_counts=False)
    nearest, _ = K.nn_search(real, nr, fake, nf, c, 1, _splits or plan_splits(n, m))
    covered = (nearest[:, 0] < r2).sum()
    total, covered = torch.stack([total[0], covered]).tolist()                # the one copy to the host
    return {"density": total / (knn * m), "coverage": covered / n, "n_real": int(n), "n_fake": int(m), "knn": knn}


def memorization_report(train: torch.Tensor, fake: torch.Tensor, *, neighbours: int = 10, _splits: int = None) -> dict:
    """Is a generated row a copy of a training row?  For every row of fake [M, D], as [M] device tensors:
      nearest_index, nearest_dist  the refined 1-NN in train (nearest_neighbours(fake, train), Euclidean distance),
      train_gap                    the refined leave-one-out 1-NN distance of THAT training row inside train,
      authentic                    nearest_dist > train_gap (Alaa et al. 2022),
      copy_ratio                   nearest_dist / the mean of the refined distances to its `neighbours` nearest training rows (Carlini et al. 2023:
                                   small means copied; 0 / 0 = NaN when all of them are exact copies),
    and the float authenticity = mean(authentic).  Two searches, fake -> train with k = neighbours and train -> train leave-one-out with k = 1, with
    the pivot of train; one host sync, for the float.  Features may be flattened pixels: D <= 65536, one channel of 256 x 256; otherwise pool
    them (EmbedderFeatures(pool=...))."""
    _check_bank("train", train)
    _check_bank("fake", fake, min_rows=1)
    _check_same_d("fake", fake, "train", train)
    _check_k("neighbours", neighbours, train.shape[0], "train")
    _check_splits(_splits)
    _check_device(train=train)
    train, fake = train.contiguous(), fake.contiguous()
    c = K.feat_colmean(train)
    nt, nf = K.feat_norms(train, c), K.feat_norms(fake, c)
    d2, index = _search(fake, nf, train, nt, c, neighbours, _splits, False, True)
    gap2, _ = _search(train, nt, train, nt, c, 1, _splits, True, True)
    dist = torch.sqrt(d2)
    nearest_index = index[:, 0].long()
    nearest_dist = dist[:, 0].contiguous()
    train_gap = torch.sqrt(gap2[:, 0])[nearest_index]
    authentic = nearest_dist > train_gap
    out = {"nearest_index": nearest_index, "nearest_dist": nearest_dist, "train_gap": train_gap, "authentic": authentic,
           "copy_ratio": nearest_dist / dist.mean(1), "neighbours": neighbours, "n_train": int(train.shape[0]), "n_fake": int(fake.shape[0])}
    out["authenticity"] = int(authentic.sum()) / fake.shape[0]                # the one copy to the host
    return out


# ------------------------------------------------------------------------------------------------ kernel distances (README "Kernel distances")
KERNELS = {"poly": L.KERNEL_POLY, "rbf": L.KERNEL_RBF}


def _kernel_scalars(kernel, degree, gamma, coef0, D: int):
    """the host-side rules of the kernel's name and scalars -> (kind, degree, gamma, coef0), gamma and coef0 as the fp32 numbers the device uses;
    gamma=None: 1 / D taken in fp64 and rounded to fp32 (poly only)"""
    import ctypes
    import math
    if kernel not in KERNELS:
        raise ValueError(f"kernel: 'poly' or 'rbf', got {kernel!r}")
    if isinstance(degree, bool) or not isinstance(degree, int) or not 1 <= degree <= 4:
        raise ValueError(f"degree: an integer in 1 .. 4, got {degree!r}")
    if gamma is None:
        if kernel == "rbf":
            raise ValueError("gamma: the rbf kernel needs a bandwidth (no median heuristic is built), got None")
        gamma = 1.0 / D
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not math.isfinite(gamma) or gamma <= 0:
        raise ValueError(f"gamma: None or a finite positive number, got {gamma!r}")
    if isinstance(coef0, bool) or not isinstance(coef0, (int, float)) or not math.isfinite(coef0):
        raise ValueError(f"coef0: a finite number, got {coef0!r}")
    gamma32, coef32 = ctypes.c_float(gamma).value, ctypes.c_float(coef0).value
    if not math.isfinite(gamma32) or gamma32 <= 0 or not math.isfinite(coef32):
        raise ValueError(f"gamma: {gamma!r} and coef0: {coef0!r} must be finite (and gamma positive) as fp32 numbers")
    return KERNELS[kernel], degree, gamma32, coef32


def _kernel_operands(kind: int, first: torch.Tensor, pivot, *banks):
    """-> (pivot, the norms of every bank or None): poly runs on the rows themselves -- a pivot of zeros --, rbf on the column mean of `first`"""
    if kind == L.KERNEL_POLY:
        c = torch.zeros((first.shape[1],), dtype=torch.float32, device=first.device) if pivot is None else _aligned(pivot)
        return c, [None] * len(banks)
    c = _pivot(first, pivot)
    return c, [K.feat_norms(b, c) for b in banks]


def kernel_matrix(x: torch.Tensor, y: torch.Tensor = None, *, kernel: str = "poly", degree: int = 3, gamma: float = None, coef0: float = 1.0,
                  pivot: torch.Tensor = None) -> torch.Tensor:
    """k between the rows of x [N, D] and of y [M, D] -> fp32 [N, M] (y=None: x against itself; the diagonal is k(x_i, x_i), not special).
    kernel="poly": (gamma x.y + coef0)^degree, gamma=None: 1 / D; kernel="rbf": exp(-gamma d2) on pairwise_sqdist's d2.  pivot=None: zeros for
    poly (the rows as they are), the column mean of x for rbf.  For tests and small sets: mmd2 and kid never form this matrix."""
    _check_bank("x", x, min_rows=1)
    if y is not None:
        _check_bank("y", y, min_rows=1)
        _check_same_d("y", y, "x", x)
    kind, degree, gamma, coef0 = _kernel_scalars(kernel, degree, gamma, coef0, x.shape[1])
    if pivot is not None:
        _check_vector("pivot", pivot, x.shape[1], x)
    _check_device(x=x)
    x = x.contiguous()
    y = x if y is None else y.contiguous()
    c, (nx, ny) = _kernel_operands(kind, x, pivot, x, y)
    return K.feat_kernel(x, nx, y, ny, c, K.make_ksum_desc(x.shape[0], y.shape[0], x.shape[1], kernel=kind, degree=degree, gamma=gamma, coef0=coef0))


def _ksum_tiles(sa: int, sb: int, same: bool) -> int:
    ta, tb = -(-sa // TILE), -(-sb // TILE)
    return ta * (ta + 1) // 2 if same else ta * tb


def ksum_workspace_bytes(subsets: int, sa: int, sb: int, same_bank: bool = False) -> int:
    """the bytes mf_ksum_workspace_bytes answers: 8 per visited tile, rounded up to 16"""
    return (subsets * _ksum_tiles(sa, sb, same_bank) * 8 + 15) // 16 * 16


def _three_sums(real, fake, ia, ib, S, sa, sb, scalars, diag: bool):
    """-> fp64 [S] x 3: the sums of k over (X, X), (Y, Y) and (X, Y) of every subset; diag: the p == q pairs of the same-bank terms are counted"""
    kind, degree, gamma, coef0 = scalars
    n, m, D = real.shape[0], fake.shape[0], real.shape[1]
    c, (nr, nf) = _kernel_operands(kind, real, None, real, fake)
    kw = dict(kernel=kind, degree=degree, gamma=gamma, coef0=coef0)
    same = 2 if diag else 1
    sxx = K.kernel_sums(real, nr, ia, real, nr, ia, c, K.make_ksum_desc(n, n, D, S, sa, sa, same_bank=same, **kw))
    syy = K.kernel_sums(fake, nf, ib, fake, nf, ib, c, K.make_ksum_desc(m, m, D, S, sb, sb, same_bank=same, **kw))
    sxy = K.kernel_sums(real, nr, ia, fake, nf, ib, c, K.make_ksum_desc(n, m, D, S, sa, sb, **kw))
    return sxx, syy, sxy


def _mmd2_of_sums(sxx, syy, sxy, n: int, m: int, unbiased: bool):
    """-> (MMD^2, the three means), fp64 on the device: sxx / (n (n - 1)) + syy / (m (m - 1)) - 2 sxy / (n m); biased: n^2 and m^2"""
    kxx = sxx / float(n * (n - 1) if unbiased else n * n)
    kyy = syy / float(m * (m - 1) if unbiased else m * m)
    kxy = sxy / float(n * m)
    return kxx + kyy - 2.0 * kxy, (kxx, kyy, kxy)


def _check_mmd_banks(real, fake) -> None:
    _check_bank("real", real)
    _check_bank("fake", fake)
    _check_same_d("fake", fake, "real", real)


def mmd2(real: torch.Tensor, fake: torch.Tensor, *, kernel: str = "poly", degree: int = 3, gamma: float = None, coef0: float = 1.0,
         unbiased: bool = True, return_terms: bool = False):
    """The squared maximum mean discrepancy of the FULL sets under k -> a 0-dim fp64 device tensor:
    sum_{i != j} k(x_i, x_j) / (n (n - 1)) + sum_{i != j} k(y_i, y_j) / (m (m - 1)) - 2 sum_{ij} k(x_i, y_j) / (n m); unbiased=False counts the
    diagonals and divides by n^2 and m^2.  Three matrix-core launches with their finish launches -- the same-bank terms over the upper triangle of
    tiles only --, every sum in fp64 in a fixed order, no N x M matrix, and nothing waits for the device.  return_terms=True: (mmd2, {"kxx", "kyy",
    "kxy"}), the three means as 0-dim fp64 device tensors.  rbf: the pivot is the column mean of real, gamma must be given."""
    _check_mmd_banks(real, fake)
    scalars = _kernel_scalars(kernel, degree, gamma, coef0, real.shape[1])
    _check_device(real=real)
    real, fake = real.contiguous(), fake.contiguous()
    n, m = real.shape[0], fake.shape[0]
    sums = _three_sums(real, fake, None, None, 1, n, m, scalars, diag=not unbiased)
    value, (kxx, kyy, kxy) = _mmd2_of_sums(*sums, n, m, bool(unbiased))
    value = value[0]
    return (value, {"kxx": kxx[0], "kyy": kyy[0], "kxy": kxy[0]}) if return_terms else value


def draw_subsets(n: int, m: int, subsets: int, subset_size: int, seed: int = 0):
    """The index lists of kid -> (ia, ib), int32 [subsets, subset_size] on the host.  ONE host generator of its own, seeded with `seed`; for subset
    s = 0, 1, ... in turn it draws torch.randperm(n), whose first subset_size entries are row s of ia, then torch.randperm(m), whose first
    subset_size entries are row s of ib.  No repeats inside a subset; the subsets are independent draws; torch's global generator is not touched."""
    g = torch.Generator().manual_seed(seed)
    ia, ib = [], []
    for _ in range(subsets):
        ia.append(torch.randperm(n, generator=g)[:subset_size])
        ib.append(torch.randperm(m, generator=g)[:subset_size])
    return torch.stack(ia).to(torch.int32), torch.stack(ib).to(torch.int32)


def _check_kid(subsets, subset_size, seed, n: int, m: int) -> None:
    if subsets is not None and (isinstance(subsets, bool) or not isinstance(subsets, int) or not 1 <= subsets <= L.KSUM_MAX_SUBSETS):
        raise ValueError(f"subsets: None or an integer in 1 .. {L.KSUM_MAX_SUBSETS}, got {subsets!r}")
    if subsets is not None and (isinstance(subset_size, bool) or not isinstance(subset_size, int) or not 2 <= subset_size <= min(n, m)):
        raise ValueError(f"subset_size: an integer in 2 .. min(N, M) = {min(n, m)}, got {subset_size!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < (1 << 62):
        raise ValueError(f"seed: a non-negative integer, got {seed!r}")


def kid(real: torch.Tensor, fake: torch.Tensor, *, subsets: int = 100, subset_size: int = 1000, degree: int = 3, gamma: float = None, coef0: float = 1.0,
        seed: int = 0) -> dict:
    """The Kernel Inception Distance (Binkowski et al. 2018) -> {"kid_mean", "kid_std", "subsets", "subset_size", "n_real", "n_fake"}: the mean and
    the POPULATION standard deviation of the unbiased MMD^2 under (gamma x.y + coef0)^degree over `subsets` pairs of subsets of `subset_size` rows
    (draw_subsets: a seeded host randperm per subset and bank).  The index lists go to the device once as int32 [S, s]; every term of ALL subsets is
    one gathering launch plus its finish launch; the host waits once, for the two figures.  subsets=None: mmd2 of the full sets, the estimate of
    the lowest variance, with kid_std None.  Nothing is drawn from torch's global generator or from a noise source."""
    _check_mmd_banks(real, fake)
    scalars = _kernel_scalars("poly", degree, gamma, coef0, real.shape[1])
    n, m = real.shape[0], fake.shape[0]
    _check_kid(subsets, subset_size, seed, n, m)
    _check_device(real=real)
    real, fake = real.contiguous(), fake.contiguous()
    if subsets is None:
        value = _mmd2_of_sums(*_three_sums(real, fake, None, None, 1, n, m, scalars, diag=False), n, m, True)[0]
        return {"kid_mean": value.tolist()[0], "kid_std": None, "subsets": None, "subset_size": None, "n_real": int(n), "n_fake": int(m)}
    ia, ib = (t.to(real.device) for t in draw_subsets(n, m, subsets, subset_size, seed))
    values = _mmd2_of_sums(*_three_sums(real, fake, ia, ib, subsets, subset_size, subset_size, scalars, diag=False), subset_size, subset_size, True)[0]
    mean, std = torch.stack([values.mean(), values.std(unbiased=False)]).tolist()           # the one copy to the host
    return {"kid_mean": mean, "kid_std": std, "subsets": subsets, "subset_size": subset_size, "n_real": int(n), "n_fake": int(m)}


def plan_kid(n: int, m: int, subsets, subset_size) -> dict:
    """What kid(real [n, D], fake [m, D], subsets, subset_size) launches -> {"launches", "workgroups", "workspace_bytes", "index_bytes",
    "matrix_bytes"}, host only.  workgroups: one per visited tile -- the same-bank terms visit the T (T + 1) / 2 tiles on or above the diagonal --;
    workspace_bytes: the largest of the three launches' (they share it); matrix_bytes: the three fp32 matrices of the materialised form."""
    for name, v in (("n", n), ("m", m)):
        if isinstance(v, bool) or not isinstance(v, int) or not 2 <= v < 1 << 24:
            raise ValueError(f"{name}: an integer in 2 .. 2^24 - 1, got {v!r}")
    _check_kid(subsets, subset_size, 0, n, m)
    S, sa, sb = (1, n, m) if subsets is None else (subsets, subset_size, subset_size)
    terms = (("real x real", sa, sa, True), ("fake x fake", sb, sb, True), ("real x fake", sa, sb, False))
    groups = {name: S * _ksum_tiles(a, b, same) for name, a, b, same in terms}
    launches = [f"ksum_partial_kernel: {name}, {S} subset(s) of {a} x {b} rows, {groups[name]} workgroups" + (" (upper triangle of tiles)" if same else "")
                for name, a, b, same in terms]
    return {"launches": [x for line in launches for x in (line, "ksum_finish_kernel: " + line.split(":")[1].split(",")[0].strip())],
            "workgroups": groups, "workspace_bytes": max(ksum_workspace_bytes(S, a, b, same) for _, a, b, same in terms),
            "index_bytes": 0 if subsets is None else 2 * S * subset_size * 4, "matrix_bytes": S * (sa * sa + sb * sb + sa * sb) * 4}


_density_coverage, _memorization_report = density_coverage, memorization_report     # (FidelityMeter.compute has keywords of these names)
_kid = kid


def _moments(name: str, t: torch.Tensor):
    x = t.to(torch.float64)
    mu = x.mean(0)
    xc = x - mu
    return mu, xc.t() @ xc / (x.shape[0] - 1)


def frechet_distance(real: torch.Tensor, fake: torch.Tensor) -> float:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2 of the two sets' fp64 means and unbiased covariances -> python float.  Works on CPU tensors
    too; the two symmetric eigen-decompositions run on the CPU."""
    _check_bank("real", real)
    _check_bank("fake", fake)
    _check_same_d("fake", fake, "real", real)
    mu1, s1 = _moments("real", real)
    mu2, s2 = _moments("fake", fake)
    s1c, s2c = s1.cpu(), s2.cpu()
    lam, q = torch.linalg.eigh(s1c)
    root = (q * lam.clamp_min(0).sqrt()) @ q.t()                               # S1^1/2, symmetric
    inner = root @ s2c @ root
    lam2 = torch.linalg.eigvalsh((inner + inner.t()) / 2)
    cross = lam2.clamp_min(0).sqrt().sum()
    diff = (mu1 - mu2).cpu()
    return float(diff @ diff + torch.trace(s1c) + torch.trace(s2c) - 2 * cross)


# ------------------------------------------------------------------------------------------------ the extractor and the meter
class EmbedderFeatures:
    """Features from a latent embedder the user already has (the Inception / VGG weights of the reference's extractor cannot be had): for a VAE
    the MEAN half of the encoder's moments, for the codebook embedders encode(x), the encoder's output before quantisation -- nothing is drawn,
    so a noise source's draw_index and torch's generator stay where they were.  pool=p: averaged over p x p cells first; then flattened.  2-D only."""

    def __init__(self, embedder, pool: int = None):
        if pool is not None and (isinstance(pool, bool) or not isinstance(pool, int) or pool < 1):
            raise ValueError(f"pool: None or a positive integer, got {pool!r}")
        self.embedder, self.pool = embedder, pool

    @torch.no_grad()
    def __call__(self, imgs: torch.Tensor) -> torch.Tensor:
        if not isinstance(imgs, torch.Tensor) or imgs.dim() != 4:
            raise ValueError(f"imgs: 2-D images [B, C, H, W], got {tuple(imgs.shape) if isinstance(imgs, torch.Tensor) else type(imgs).__name__}"
                             + (" (3-D features are not built)" if isinstance(imgs, torch.Tensor) and imgs.dim() == 5 else ""))
        if imgs.dtype != torch.float32:
            raise ValueError(f"imgs: fp32, got {imgs.dtype}")
        if not imgs.is_cuda:
            raise ValueError(f"imgs: on a ROCm device, got a {imgs.device.type} tensor")
        model = getattr(self.embedder, "vqvae", self.embedder)              # VQGAN / VAEGAN wrap their autoencoder
        if hasattr(model, "_encode_z"):
            z = model.encode(imgs)
        else:
            K.SyncWords.reset(imgs.device)
            moments = K.with_fused_fallback(imgs.device, lambda: model._encode_moments(imgs))
            z = moments[:, :moments.shape[1] // 2]
        if self.pool is not None:
            z = torch.nn.functional.adaptive_avg_pool2d(z, self.pool)
        return z.reshape(z.shape[0], -1).contiguous()


class FidelityMeter:
    """The reference script's update / compute protocol for FID and precision / recall in one object: update(imgs, real) stores
    features(imgs).reshape(B, -1) on the device, compute() -> {"fd", "precision", "recall", "n_real", "n_fake", "knn"}; its two switches add
    density / coverage and the memorisation report."""

    def __init__(self, features, knn: int = 3, kid=False):
        """kid=True, or a dict of kid()'s keyword arguments, makes compute() add "kid_mean", "kid_std", "kid_subsets" and "kid_subset_size" (the
        switch lives here: compute()'s own keywords are those of the neighbour figures); without it compute() returns what it always did"""
        if isinstance(knn, bool) or not isinstance(knn, int) or not 1 <= knn <= L.FIDELITY_LIST - 1:
            raise ValueError(f"knn: an integer in 1 .. {L.FIDELITY_LIST - 1}, got {knn!r}")
        if not isinstance(kid, (bool, dict)) or (isinstance(kid, dict) and not set(kid) <= {"subsets", "subset_size", "degree", "gamma", "coef0", "seed"}):
            raise ValueError(f"kid: False, True or a dict of kid()'s keyword arguments, got {kid!r}")
        self.features, self.knn, self.kid = features, knn, kid
        self.reset()

    def reset(self) -> None:
        self._real, self._fake = [], []

    @torch.no_grad()
    def update(self, imgs: torch.Tensor, real: bool) -> None:
        f = self.features(imgs)
        if not isinstance(f, torch.Tensor) or f.dtype != torch.float32:
            raise ValueError(f"features: the extractor must return an fp32 tensor, got {getattr(f, 'dtype', type(f).__name__)}")
        (self._real if real else self._fake).append(f.reshape(f.shape[0], -1))

    def banks(self):
        """the features so far, as two device tensors [N, D] and [M, D]"""
        if not self._real or not self._fake:
            raise ValueError("FidelityMeter: update() with real and with generated images first")
        return torch.cat(self._real), torch.cat(self._fake)

    def compute(self, density_coverage: bool = False, memorization: bool = False) -> dict:
        """density_coverage=True adds "density" and "coverage" (density_coverage(real, fake, knn)); memorization=True adds "authenticity" and
        "memorization", the whole memorization_report(real, fake) with the real bank as the training set (10 neighbours, or all the real rows
        when they are fewer)"""
        real, fake = self.banks()
        out = precision_recall(real, fake, self.knn)
        out["fd"] = frechet_distance(real, fake)
        if density_coverage:
            dc = _density_coverage(real, fake, self.knn)
            out["density"], out["coverage"] = dc["density"], dc["coverage"]
        if memorization:
            rep = _memorization_report(real, fake, neighbours=min(10, real.shape[0]))
            out["authenticity"], out["memorization"] = rep["authenticity"], rep
        if self.kid:
            kw = dict(self.kid) if isinstance(self.kid, dict) else {}
            if kw.get("subsets", 100) is not None:
                kw.setdefault("subset_size", min(1000, real.shape[0], fake.shape[0]))      # (kid()'s 1000 where the banks hold that many rows)
            res = _kid(real, fake, **kw)
            out.update(kid_mean=res["kid_mean"], kid_std=res["kid_std"], kid_subsets=res["subsets"], kid_subset_size=res["subset_size"])
        return out
