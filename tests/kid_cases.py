"""The single source of the inputs of the kernel-distance tests (CPU and GPU) and the fp64 restatement of the definition (README "Kernel
distances", medfusion_amd/fidelity.py) they are checked against: the kernel k, the sums over index lists, MMD^2 and kid with the same lists, and the
DERIVED error bounds.  Plain torch on the CPU; nothing here touches a device.

The bounds, first order in u = 2^-24 (one fp32 rounding), derived as fidelity_cases.bound is.

poly.  The device forms dot = ONE fp32 fmaf chain of D terms: |dot - x.y| <= gamma_D sum |x_k y_k| <= D u |x||y| (Cauchy-Schwarz).  v = fmaf(gamma,
dot, c0) is rounded once: |v' - v| <= gamma D u |x||y| + u |v|.  k = v^deg takes deg - 1 rounded products (deg = 4: v2 = fl(v v), k = fl(v2 v2), the
first rounding counted twice: 3 u): |k' - k| <= deg |v|^(deg-1) |v' - v| + (deg - 1) u |v|^deg
    = deg |v|^(deg-1) gamma D u |x||y| + (2 deg - 1) u |v|^deg.
The bound the tests hold the device to is the LOOSER one the issue states, which covers the second-order terms dropped above:
    E_ij = deg |v|^(deg-1) gamma (D + 2) u |x||y| + 2 deg u |v|^deg.

rbf.  d2' is within E^d2_ij = fidelity_cases.bound of the fp64 d2 of the same centred rows.  arg' = fl32(gamma d2') = gamma d2' (1 + e), |e| <= u, so
|arg' - gamma d2| <= delta := gamma E^d2 + gamma d2 u.  k' = expf(-arg') (1 + e2) with |e2| <= c u: the ROCm documentation ("HIP math API", single
precision floating-point functions) lists expf with a maximum error of 1 ULP; one ulp of a result is at most 2^-23 = 2 u of it, so c = 2.  Hence
    E_ij = k (expm1(delta) + 2 u exp(delta))         (= k (gamma E^d2 + gamma d2 u + 2 u) to first order: the issue's form with c = 2 + gamma d2).

A sum of n fp64 terms in ANY fixed order: |sum' - sum| <= (n - 1) 2^-53 sum |k| (first order); the doubling of the off-diagonal tiles is exact.
MMD^2 adds three divisions, a doubling, an addition and a subtraction in fp64: at most 6 2^-53 (|kxx| + |kyy| + 2 |kxy|)."""
import functools

import torch

from tests import fidelity_cases as FC

U = FC.U
U64 = 2.0 ** -53
EXP_REL = 2 * U                     # 1 ULP of expf (ROCm documentation, HIP math API), as a relative error
# (N, M, D): the smallest shapes that cross a tile (128 rows), a chunk (32 features) or a load-path edge (D % 4)
SHAPES = ((129, 257, 33), (5, 130, 35), (128, 128, 36), (17, 16, 1), (257, 257, 64))
DEGREES = (1, 2, 3, 4)
STAT_ROWS = (300, 257, 64)          # N, M, D of the statistics cases


def gamma_default(D):
    """1 / D taken in fp64 and rounded to fp32, as the python float the device gets"""
    return float(torch.tensor(1.0 / D, dtype=torch.float64).float())


def _inception_like(g, rows, D, centres, labels, spread=0.35):
    """non-negative rows, about half of the entries exactly 0, like pooled activations after a ReLU"""
    x = centres[labels] + spread * torch.randn(rows, D, generator=g, dtype=torch.float64)
    return x.clamp_min(0).float()


def make(kind, seed, N, M, D, modes=5):
    """kind "inception": both banks from all the modes with slightly different spreads; "mixture": the generated bank from modes 0 and 1 only (mode
    dropping: KID clearly positive); "same": two draws from one distribution (KID about 0, of either sign)"""
    g = torch.Generator().manual_seed(seed)
    centres = 0.2 * torch.randn(modes, D, generator=g, dtype=torch.float64) + 0.1
    lab_r = torch.randint(0, modes, (N,), generator=g)
    lab_f = torch.randint(0, 2 if kind == "mixture" else modes, (M,), generator=g)
    real = _inception_like(g, N, D, centres, lab_r)
    fake = _inception_like(g, M, D, centres, lab_f, spread=0.35 if kind in ("same", "mixture") else 0.4)
    return real, fake


@functools.lru_cache(maxsize=None)
def case(name):
    """(real, fake): "inception", "mixture", "same" at STAT_ROWS; "<name>+64": 64 added to every feature in fp32 (the inputs ARE these numbers);
    "s<i>": the inception-like banks at SHAPES[i]"""
    if name.endswith("+64"):
        real, fake = case(name[:-3])
        return real + FC.OFFSET, fake + FC.OFFSET
    if name[0] == "s" and name[1:].isdigit():
        return make("inception", 20 + int(name[1:]), *SHAPES[int(name[1:])])
    return make(name, {"inception": 11, "mixture": 12, "same": 13}[name], *STAT_ROWS)


SHAPE_CASES = tuple(f"s{i}" for i in range(len(SHAPES)))


# ------------------------------------------------------------------------------------------------ the kernel and its bounds, fp64
def poly64(x, y, degree, gamma, coef0=1.0):
    """k = (gamma x.y + coef0)^degree on the fp32 inputs as fp64 numbers"""
    return (gamma * (x.double() @ y.double().t()) + coef0) ** degree


def poly_bound(x, y, degree, gamma, coef0=1.0):
    """E_ij of the module header"""
    x, y = x.double(), y.double()
    D = x.shape[1]
    v = (gamma * (x @ y.t()) + coef0).abs()
    xy = x.norm(dim=1)[:, None] * y.norm(dim=1)[None, :]
    return degree * v ** (degree - 1) * gamma * (D + 2) * U * xy + 2 * degree * U * v ** degree


def rbf64(x, y, gamma, pivot):
    """k = exp(-gamma d2) with d2 the fp64 distance of the centred rows xt = fl32(x - pivot)"""
    return torch.exp(-gamma * FC.sqdist64(FC.centred(x, pivot), FC.centred(y, pivot)))


def rbf_bound(x, y, gamma, pivot):
    xt, yt = FC.centred(x, pivot), FC.centred(y, pivot)
    d2 = FC.sqdist64(xt, yt)
    delta = gamma * FC.bound(FC.norms(xt), FC.norms(yt), x.shape[1]) + gamma * d2 * U
    return torch.exp(-gamma * d2) * (torch.expm1(delta) + EXP_REL * torch.exp(delta))


def kernel64(x, y, kernel="poly", degree=3, gamma=None, coef0=1.0, pivot=None):
    """-> (k, E): the fp64 kernel matrix and the elementwise bound of the device's fp32 one"""
    if kernel == "poly":
        gamma = gamma_default(x.shape[1]) if gamma is None else gamma
        return poly64(x, y, degree, gamma, coef0), poly_bound(x, y, degree, gamma, coef0)
    return rbf64(x, y, gamma, pivot), rbf_bound(x, y, gamma, pivot)


# ------------------------------------------------------------------------------------------------ sums, MMD^2, kid
def pair_sum(k, same, diag=False):
    """the sum of a subset pair's matrix; same: A is B -- the p == q entries left out (by position) unless diag"""
    s = k.sum()
    return s - k.diagonal().sum() if same and not diag else s


def sum_bound(k):
    """of the fp64 summation of k's entries in any fixed order"""
    return (k.numel() - 1) * U64 * float(k.abs().sum())


def mmd2_64(real, fake, unbiased=True, **kw):
    """-> (MMD^2, {"kxx", "kyy", "kxy"}, bound): the statistic in fp64 and the summed derived bound of the device's"""
    n, m = real.shape[0], fake.shape[0]
    (kxx, exx), (kyy, eyy), (kxy, exy) = kernel64(real, real, **kw), kernel64(fake, fake, **kw), kernel64(real, fake, **kw)
    dn, dm = (n * (n - 1), m * (m - 1)) if unbiased else (n * n, m * m)
    txx, tyy, txy = float(pair_sum(kxx, True, not unbiased)) / dn, float(pair_sum(kyy, True, not unbiased)) / dm, float(kxy.sum()) / (n * m)
    bound = (float(pair_sum(exx, True, not unbiased)) + sum_bound(kxx)) / dn + (float(pair_sum(eyy, True, not unbiased)) + sum_bound(kyy)) / dm \
        + 2 * (float(exy.sum()) + sum_bound(kxy)) / (n * m) + 6 * U64 * (abs(txx) + abs(tyy) + 2 * abs(txy))
    return txx + tyy - 2 * txy, {"kxx": txx, "kyy": tyy, "kxy": txy}, bound


def kid64(real, fake, ia, ib, **kw):
    """kid with the given index lists [S, s] -> (mean, population std, values [S], bound of the mean, bound of the std).  The std is 1-Lipschitz in
    the vector of values in the norm sqrt(mean (.)^2) <= max: its bound is the largest subset bound (plus the fp64 roundings of mean and std, far
    below it and counted as 8 2^-53 of the largest |value|)."""
    values, bounds = [], []
    for a, b in zip(ia.long(), ib.long()):
        v, _, e = mmd2_64(real[a], fake[b], True, kernel="poly", **kw)
        values.append(v)
        bounds.append(e)
    v = torch.tensor(values, dtype=torch.float64)
    extra = 8 * U64 * float(v.abs().max()) * max(1, len(values))
    return float(v.mean()), float(v.std(unbiased=False)), v, sum(bounds) / len(bounds) + extra, max(bounds) + extra


def closed_form_linear_mmd2(real, fake, gamma=1.0):
    """degree 1, coef0 0: sum_{i != j} x_i.x_j = |sum x|^2 - sum |x_i|^2, so MMD^2_u follows from the bank sums alone"""
    x, y = real.double(), fake.double()
    n, m = x.shape[0], y.shape[0]
    sx, sy = x.sum(0), y.sum(0)
    return gamma * (float(sx @ sx - (x * x).sum()) / (n * (n - 1)) + float(sy @ sy - (y * y).sum()) / (m * (m - 1)) - 2 * float(sx @ sy) / (n * m))


def torch_form(real, fake, degree=3, gamma=None, coef0=1.0, dtype=torch.float32):
    """the plain-torch form of the definition in `dtype`: three matrices, a pow pass and a sum pass over each -> MMD^2_u as a float"""
    x, y = real.to(dtype), fake.to(dtype)
    gamma = gamma_default(x.shape[1]) if gamma is None else gamma
    n, m = x.shape[0], y.shape[0]
    kxx, kyy, kxy = ((gamma * (a @ b.t()) + coef0) ** degree for a, b in ((x, x), (y, y), (x, y)))
    return float((kxx.sum() - kxx.diagonal().sum()) / (n * (n - 1)) + (kyy.sum() - kyy.diagonal().sum()) / (m * (m - 1)) - 2 * kxy.sum() / (n * m))


def rbf_gamma(real):
    """a bandwidth that keeps gamma d2 of order 1 on a case: 1 / (2 x the mean squared distance to the bank's mean), rounded to fp32"""
    x = real.double()
    return float(torch.tensor(0.25 / float(((x - x.mean(0)) ** 2).sum(1).mean()), dtype=torch.float64).float())
