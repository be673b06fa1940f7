"""The single source of the inputs of the neighbour tests (CPU and GPU) and the fp64 restatement of the definitions (README "Neighbours",
medfusion_amd/fidelity.py) they are checked against: the cases of tests/fidelity_cases.py, two mode-dropping cases with planted copies, the k nearest
rows by (d2, index), density / coverage, the memorisation report, and the ambiguity rules.  Plain torch on the CPU; nothing here touches a device.

The bound of the refined distance, derived as fidelity_cases.bound is: out = fl32(S), S = the fp64 sum of v_k^2 with v_k = fl32(x_k - y_k) =
(x_k - y_k)(1 + e_k), |e_k| <= u = 2^-24 (one rounding per difference; none where the difference is exact).  v_k^2 is exact in fp64 (48 bits), so
S = sum (x_k - y_k)^2 (1 + e_k)^2 (1 + g), |g| <= D 2^-53 from the fp64 additions: |S / d2 - 1| <= 2u + u^2 + D 2^-53 (all terms are non-negative:
the relative errors do not amplify).  The final rounding adds u: |out / d2 - 1| <= 3u + O(u^2) + D 2^-53 < 4u for every D <= 65536
(D 2^-53 <= 2^-37).  REFINE_REL = 4 2^-24 is that bound; equal rows give v_k = 0 and exactly 0."""
import functools

import torch

from tests import fidelity_cases as FC

U = FC.U
REFINE_REL = 4 * U
LIST = 16
# seed, N, M, D: the shapes of c0 and c1
DROPPING = {"m4": (4, 300, 257, 96), "m5": (5, 193, 320, 67)}
PLANTED_NEAR = (tuple(range(0, 8)), tuple(range(10, 18)))     # generated rows 0 .. 7 = training rows 10 .. 17 + 1e-3 randn
PLANTED_EXACT = ((8, 9), (20, 21))                            # generated rows 8, 9 = training rows 20, 21 exactly
KNN_DC = 5
NEIGHBOURS = 10
# the issue's table (fp64, WITHOUT the two exact copies): density, coverage, authenticity; the planted copy_ratio is <= 0.0012, the smallest other 0.81
TABLE = {"m4": (1.404, 0.457, 0.813), "m5": (1.182, 0.663, 0.831)}


def make_dropping(seed, N, M, D, exact=True, modes=5, lo=0.7, hi=1.4):
    """fidelity_cases.make with the generated labels drawn from modes 0 and 1 only (the same draws in the same order), then the planted copies:
    the noise of the near-copies is fp64 randn of a generator of its own seeded with `seed`, added in fp64 and rounded to fp32"""
    g = torch.Generator().manual_seed(seed)
    kw = dict(generator=g, dtype=torch.float64)
    centres = torch.randn(modes, D, **kw) * 1.5 + 4.0
    lab_r = torch.randint(0, modes, (N,), generator=g)
    lab_f = torch.randint(0, 2, (M,), generator=g)
    sr = lo + (hi - lo) * torch.rand(N, 1, **kw)
    sf = lo + (hi - lo) * torch.rand(M, 1, **kw)
    train = (centres[lab_r] + sr * torch.randn(N, D, **kw)).float()
    fake = (centres[lab_f] + 0.95 * sf * torch.randn(M, D, **kw)).float()
    noise = torch.randn(len(PLANTED_NEAR[0]), D, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    fake[list(PLANTED_NEAR[0])] = (train[list(PLANTED_NEAR[1])].double() + 1e-3 * noise).float()
    if exact:
        fake[list(PLANTED_EXACT[0])] = train[list(PLANTED_EXACT[1])]
    return train, fake


@functools.lru_cache(maxsize=None)
def case(name):
    """(real / train, fake) of a case: those of fidelity_cases, "m4" / "m5" (the planted copies included), "m4-" / "m5-" (without the two exact copies)"""
    if name.rstrip("-") in DROPPING:
        return make_dropping(*DROPPING[name.rstrip("-")], exact=not name.endswith("-"))
    return FC.case(name)


ALL = FC.ALL + tuple(DROPPING)


def nearest64(qt, rt, k, leave_one_out=False):
    """-> (d2 [M, k], index [M, k], the whole sorted rows [M, N]) of the fp64 d2 between the rows of qt and rt, ascending by (d2, index): a stable
    sort.  leave_one_out: rt is qt and the diagonal is +inf"""
    d = FC.sqdist64(qt, rt)
    if leave_one_out:
        d.fill_diagonal_(float("inf"))
    s, i = torch.sort(d, dim=1, stable=True)
    return s[:, :k], i[:, :k], s


def row_bound(qt, rt, D):
    """max_i E(row, i): the largest error bound of a query row's kernel d2 over the reference bank"""
    return FC.bound(FC.norms(qt), FC.norms(rt), D).max(dim=1).values


def ambiguous_rows(qt, rt, D, k, leave_one_out=False):
    """a row is ambiguous when two neighbouring fp64 order statistics among its first k + 1 are closer than the sum of their bounds E"""
    d = FC.sqdist64(qt, rt)
    E = FC.bound(FC.norms(qt), FC.norms(rt), D)
    if leave_one_out:
        d.fill_diagonal_(float("inf"))
    s, i = torch.sort(d, dim=1, stable=True)
    top = min(k + 1, s.shape[1] - int(leave_one_out))
    s, e = s[:, :top], E.gather(1, i[:, :top])
    return ((s[:, 1:] - s[:, :-1]) < (e[:, 1:] + e[:, :-1])).any(1)


def density_coverage64(rt, ft, D, knn=KNN_DC):
    """fp64 on the centred banks -> dict: count [M], covered [N], density, coverage, and the ambiguity rule of fidelity_cases.membership: the pairs
    with |d2 - r2| <= E_ij + max_j' E_ij' and the rows whose coverage decision such a pair could change"""
    r2 = FC.radii64(rt, knn)
    d = FC.sqdist64(rt, ft)
    nr, nf = FC.norms(rt), FC.norms(ft)
    slack = FC.bound(nr, nf, D) + FC.bound(nr, nr, D).max(dim=1).values[:, None]
    inside = d < r2[:, None]
    amb = (d - r2[:, None]).abs() <= slack
    count, covered = inside.sum(0), inside.any(1)
    # a row's coverage decision is safe when some pair is inside by more than the slack, or every pair is outside by more than the slack
    surely = ((r2[:, None] - d) > slack).any(1)
    never = ((d - r2[:, None]) > slack).all(1)
    return dict(count=count, covered=covered, density=float(count.sum()) / (knn * ft.shape[0]), coverage=float(covered.double().mean()),
                ambiguous_pairs=amb, ambiguous_rows=~(surely | never), r2=r2)


def memorization64(train, fake, neighbours=NEIGHBOURS):
    """fp64 on the fp32 inputs themselves (the refined distance has no pivot) -> dict of [M] tensors and the authenticity"""
    a, b = train.double(), fake.double()

    def exact(x, y, k, loo=False):
        """the k nearest by the expanded form (absolute error ~1e-13 of d2: far below any gap between neighbours here), their d2 again BY
        DIFFERENCES (an exact copy is exactly 0), ascending by (d2, index)"""
        i = nearest64(x.double(), y.double(), k, leave_one_out=loo)[1].sort(dim=1).values
        s, order = torch.sort(pair_d2_64(x, y, i), dim=1, stable=True)
        return s, i.gather(1, order)

    s, i = exact(fake, train, neighbours)
    dist = s.sqrt()
    gap = exact(train, train, 1, loo=True)[0][:, 0].sqrt()
    nearest_dist, nearest_index = dist[:, 0], i[:, 0]
    train_gap = gap[nearest_index]
    authentic = nearest_dist > train_gap
    return dict(nearest_index=nearest_index, nearest_dist=nearest_dist, train_gap=train_gap, authentic=authentic, copy_ratio=nearest_dist / dist.mean(1),
                authenticity=float(authentic.double().mean()), neighbour_index=i, neighbour_dist=dist)


def pair_d2_64(x, y, index):
    """the fp64 squared distance of x[j] and y[index[j, p]] on the fp32 inputs, by differences -> [M, k]"""
    return ((x.double()[:, None, :] - y.double()[index]) ** 2).sum(-1)
