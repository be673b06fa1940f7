"""The single source of the inputs of the fidelity tests (CPU and GPU) and the fp64 restatement of the definition (README "Fidelity",
medfusion_amd/fidelity.py) they are checked against: seeded Gaussian-mixture feature banks, squared distances, k-NN radii, manifold hits, the
derived error bound of the kernel's d2 and the ambiguity rule of the threshold decisions.  Plain torch on the CPU; nothing here touches a device."""
import functools
from pathlib import Path

import numpy as np
import torch

GOLD = Path(__file__).resolve().parent / "golden"
KNN = 3
CASES = {"c0": (0, 300, 257, 96), "c1": (1, 193, 320, 67), "c2": (2, 130, 129, 8), "c3": (3, 512, 384, 260)}     # seed, N, M, D
OFFSET = 64.0
AMBIGUOUS_CAP = 0.03          # a condition on the INPUTS: at most 3 % of the queries of a case may sit within the error bound of a radius
U = 2.0 ** -24


def make(seed, N, M, D, modes=5, lo=0.7, hi=1.4):
    g = torch.Generator().manual_seed(seed)
    kw = dict(generator=g, dtype=torch.float64)
    centres = torch.randn(modes, D, **kw) * 1.5 + 4.0
    lab_r = torch.randint(0, modes, (N,), generator=g)
    lab_f = torch.randint(0, modes, (M,), generator=g)
    sr = lo + (hi - lo) * torch.rand(N, 1, **kw)
    sf = lo + (hi - lo) * torch.rand(M, 1, **kw)
    real = centres[lab_r] + sr * torch.randn(N, D, **kw)
    fake = centres[lab_f] + 0.95 * sf * torch.randn(M, D, **kw)
    return real.float(), fake.float()


@functools.lru_cache(maxsize=None)
def case(name):
    """(real, fake) of a case; "c0+64": case c0 with 64 added to every feature (in fp32: the inputs ARE these fp32 numbers)"""
    if name.endswith("+64"):
        real, fake = case(name[:-3])
        return real + OFFSET, fake + OFFSET
    return make(*CASES[name])


ALL = tuple(CASES) + ("c0+64",)


def pivot_of(real):
    """the fp64 column mean rounded to fp32"""
    return real.double().mean(0).float()


def centred(x, pivot):
    """xt = fl32(x - c) as fp64 numbers (exact inputs to the fp64 evaluation); pivot=None: x itself"""
    return (x if pivot is None else x - pivot).double()


def norms(xt):
    """n(x): the fp64 sum of xt_k^2 rounded to fp32, returned as fp64 numbers"""
    return (xt * xt).sum(1).float().double()


def sqdist64(a, b):
    """d2 between the rows of two fp64 banks.  Distances do not move under a common shift: both banks are shifted by the mean of `a` first, so that
    |a|^2 + |b|^2 - 2 a.b cancels nothing that matters (relative error ~1e-15 of the norms about that mean)."""
    m = a.mean(0)
    a, b = a - m, b - m
    d = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.t())
    return d.clamp_min(0)


def bound(na, nb, D):
    """E_ij = (D + 8) 2^-24 (n_i + n_j): the rigorous bound of |kernel d2 - fp64 d2 of the same xt| (two fmaf chains' gamma_D |xt||yt| <=
    gamma_D (n_i + n_j) / 2 each, the norm roundings and the two additions in the 8)"""
    return (D + 8) * U * (na[:, None] + nb[None, :])


def radii64(xt, knn=KNN):
    """r2_i: the (knn + 1)-th smallest of row i of the bank's own d2, the diagonal exactly 0"""
    d = sqdist64(xt, xt)
    d.fill_diagonal_(0)
    return d.kthvalue(knn + 1, dim=1).values


def membership(ref_t, query_t, D, knn=KNN):
    """-> (hit [M] bool in fp64, ambiguous [M] bool): query j is ambiguous when some i has |d2_ij - r2_i| <= E_ij + max_j' E_ij' (the second
    term: the radius's own error, over the reference bank)"""
    r2 = radii64(ref_t, knn)
    d = sqdist64(ref_t, query_t)
    nr, nq = norms(ref_t), norms(query_t)
    slack = bound(nr, nq, D) + bound(nr, nr, D).max(dim=1).values[:, None]
    return (d < r2[:, None]).any(0), ((d - r2[:, None]).abs() <= slack).any(0)


def truth(real, fake, pivot, knn=KNN):
    """the fp64 evaluation of the definition on xt = fl32(x - pivot) (pivot=None: on the inputs themselves, the reference's arithmetic in fp64)"""
    rt, ft = centred(real, pivot), centred(fake, pivot)
    D = real.shape[1]
    p_hit, p_amb = membership(rt, ft, D, knn)
    r_hit, r_amb = membership(ft, rt, D, knn)
    return dict(precision_hits=p_hit, precision_ambiguous=p_amb, recall_hits=r_hit, recall_ambiguous=r_amb,
                precision=float(p_hit.double().mean()), recall=float(r_hit.double().mean()),
                radii_real=radii64(rt, knn).sqrt(), radii_fake=radii64(ft, knn).sqrt())


@functools.lru_cache(maxsize=None)
def case_truth(name):
    """truth of a case with the pivot the definition names (shared by the tests; not to be modified)"""
    real, fake = case(name)
    return truth(real, fake, pivot_of(real))


def plain_torch_sqdist(x, y):
    """the reference's un-centred formula in the inputs' own precision: |x|^2 + |y|^2 - 2 x y^T, negatives set to 0"""
    d = (x ** 2).sum(1, keepdim=True) + (y ** 2).sum(1, keepdim=True).t() - 2 * (x @ y.t())
    return d.clamp_min(0)


def golden(name):
    with np.load(GOLD / f"fidelity_{name}.npz") as z:
        return {k: z[k] for k in z.files}
