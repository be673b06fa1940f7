"""Improved precision / recall on a real MI355X (medfusion_amd/fidelity.py, csrc/fidelity.hip) against the fp64 restatement of the definition
(tests/fidelity_cases.py).  The distances are held to the DERIVED bound E_ij = (D + 8) 2^-24 (n_i + n_j); the radii and the hits to the kernel's
own matrix bit for bit; precision / recall to fp64 under the ambiguity rule (a decision may differ only where a distance is within the bound of a
radius, and at most 3 % of a case's queries are such); then the memory the fused launches take, and the meter."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import fidelity as F
from medfusion_amd import kernels as K
from oracle import restate as R
from oracle import synth as S
from tests import fidelity_cases as FC


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _random_banks(n, m, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g) * 1.3 + 0.5, torch.randn(m, d, generator=g) * 0.9 + 0.7


def _misaligned(t):
    """the same values, contiguous, one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _held(what, got, x, y, pivot):
    """|kernel d2 - fp64 d2 of the same xt| <= E, element-wise; -> the largest ratio"""
    xt, yt = FC.centred(x, pivot), FC.centred(y, pivot)
    want, E = FC.sqdist64(xt, yt), FC.bound(FC.norms(xt), FC.norms(yt), x.shape[1])
    ratio = float(((got.cpu().double() - want).abs() / E).max())
    print(f"[measured] {what}: max |d2 - fp64| / E = {ratio:.4f}")
    assert ratio <= 1.0, (what, ratio)
    return ratio


# ------------------------------------------------------------------------------------------------ 1. distances
SHAPES = {"tiles128": (128, 128, 32), "tails": (257, 5, 260), "d1": (17, 16, 1)}


@pytest.mark.parametrize("name", list(FC.CASES) + list(SHAPES))
def test_distances_within_the_derived_bound(dev, name):
    x, y = FC.case(name) if name in FC.CASES else _random_banks(*SHAPES[name], seed=11)
    pivot = K.feat_colmean(x.to(dev))
    want_pivot = FC.pivot_of(x)
    assert float((pivot.cpu() - want_pivot).abs().max()) <= float(want_pivot.abs().max()) * 2.0 ** -23      # the fp64 mean, rounded (a tie may fall either way)
    got = M.pairwise_sqdist(x.to(dev), y.to(dev), pivot=pivot)
    assert got.shape == (x.shape[0], y.shape[0]) and got.dtype == torch.float32
    _held(f"sqdist {name} {tuple(x.shape)} x {tuple(y.shape)}", got, x, y, pivot.cpu())
    assert torch.equal(got, M.pairwise_sqdist(x.to(dev), y.to(dev)))                                        # pivot=None is that pivot
    xt = FC.centred(x, pivot.cpu())
    # n(x): an fp64 sum rounded once -- another order of the fp64 additions can move the fp32 rounding by one ulp at most
    assert float((K.feat_norms(x.to(dev), pivot).cpu().double() / FC.norms(xt) - 1).abs().max()) <= 2.0 ** -23


def test_offset_features_stay_within_the_bound_of_the_centred_norms(dev):
    """case c0 + 64: the un-centred fp32 formula (the reference's) loses four digits to |x|^2 ~ 4.4e5; the pivoted kernel keeps E of the CENTRED norms"""
    x, y = FC.case("c0+64")
    pivot = K.feat_colmean(x.to(dev))
    got = M.pairwise_sqdist(x.to(dev), y.to(dev), pivot=pivot)
    want = FC.sqdist64(x.double(), y.double())                                                               # the truth of those fp32 inputs
    xt, yt = FC.centred(x, pivot.cpu()), FC.centred(y, pivot.cpu())
    E = FC.bound(FC.norms(xt), FC.norms(yt), x.shape[1])
    plain = float((FC.plain_torch_sqdist(x, y).double() - want).abs().max())
    kern = float((got.cpu().double() - want).abs().max())
    print(f"[measured] offset +64: max |d2 - fp64| un-centred fp32 formula {plain:.3e}, kernel {kern:.3e}, max E {float(E.max()):.3e}")
    # x - c is exact here (Sterbenz: every feature within a factor 2 of its column mean), so the truth of the inputs is the truth of xt
    assert torch.equal(xt, x.double() - pivot.cpu().double()) and torch.equal(yt, y.double() - pivot.cpu().double())
    assert float(((got.cpu().double() - want).abs() / E).max()) <= 1.0
    assert plain > 10 * kern


def test_the_two_load_paths_give_the_same_bits(dev):
    x, y = (t.to(dev) for t in FC.case("c0"))                                # D = 96: sixteen-byte loads when aligned
    pivot = K.feat_colmean(x)
    a = M.pairwise_sqdist(x, y, pivot=pivot)
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    assert torch.equal(a, M.pairwise_sqdist(_misaligned(x), y, pivot=pivot))
    assert torch.equal(a, M.pairwise_sqdist(x, _misaligned(y), pivot=pivot))
    assert torch.equal(a, M.pairwise_sqdist(x, y, pivot=_misaligned(pivot)))
    r2 = M.knn_radii(x, 3, pivot=pivot, squared=True)
    assert torch.equal(r2, M.knn_radii(_misaligned(x), 3, pivot=pivot, squared=True))
    assert torch.equal(M.manifold_hits(x, r2, y, pivot=pivot), M.manifold_hits(_misaligned(x), r2, _misaligned(y), pivot=pivot))


# ------------------------------------------------------------------------------------------------ 2. position independence
def test_bits_do_not_depend_on_the_position_the_tile_or_the_bank(dev):
    x, y = (t.to(dev) for t in FC.case("c3"))                                # 512 x 384, D = 260: 4 x 3 tiles, nine K chunks with a tail
    pivot = K.feat_colmean(x)
    full = M.pairwise_sqdist(x, y, pivot=pivot)
    assert torch.equal(full, M.pairwise_sqdist(x, y, pivot=pivot))           # two calls
    for (a, b), (c, d) in (((0, 512), (0, 384)), ((37, 301), (129, 200)), ((127, 130), (255, 384)), ((400, 512), (0, 1))):
        sub = M.pairwise_sqdist(x[a:b], y[c:d], pivot=pivot)
        assert torch.equal(sub, full[a:b, c:d]), ((a, b), (c, d))
    assert torch.equal(full.t(), M.pairwise_sqdist(y, x, pivot=pivot))
    own = M.pairwise_sqdist(x, pivot=pivot)
    assert bool((own.diagonal() == 0).all()) and torch.equal(own, own.t())
    two = M.pairwise_sqdist(x, x.clone(), pivot=pivot)                       # the same rows as two banks: the diagonal is COMPUTED
    off = ~torch.eye(512, dtype=torch.bool, device=dev)
    assert torch.equal(own[off], two[off])


# ------------------------------------------------------------------------------------------------ 3. radii
@pytest.mark.parametrize("splits", [1, 2, 16])
@pytest.mark.parametrize("knn", [1, 3, 15])
def test_radii_are_the_order_statistic_of_the_kernels_own_rows(dev, knn, splits):
    for name in ("c1", "c3"):                                                # 193 rows: 2 column tiles under 16 splits (empty splits); 512: 4
        x = FC.case(name)[0].to(dev)
        pivot = K.feat_colmean(x)
        own = M.pairwise_sqdist(x, pivot=pivot)
        want = own.kthvalue(knn + 1, dim=1).values
        got = M.knn_radii(x, knn, pivot=pivot, squared=True, _splits=splits)
        assert torch.equal(got, want), (name, knn, splits)
        assert torch.equal(M.knn_radii(x, knn, pivot=pivot), torch.sqrt(want))
    assert torch.equal(M.knn_radii(x, knn, squared=True), got)               # the planner's own S, the pivot of x


@pytest.fixture(scope="module")
def one_bank(dev):
    """[257, 36]: two full tiles and one row; D = 36 takes the sixteen-byte path with a partial chunk.  -> (x, the same values one float off)"""
    x = _random_banks(257, 1, 36, seed=23)[0].to(dev)
    return x, _misaligned(x)


@pytest.mark.parametrize("splits", [1, 2, 16])
@pytest.mark.parametrize("knn", [1, 3, 15])
def test_radii_are_the_neighbour_search_without_the_row_itself(one_bank, knn, splits):
    """the value list and the key list run one skeleton on one tile: the row itself is the value list's exact 0 and every other d2 >= 0, so the
    (knn + 1)-th smallest with the row equals the knn-th nearest neighbour without it, bit for bit, on either load path"""
    for x in one_bank:
        pivot = K.feat_colmean(x)
        nx = K.feat_norms(x, pivot)
        got = K.knn_radii_sq(x, nx, pivot, knn, splits)
        want = K.nn_search(x, nx, x, nx, pivot, k=knn, splits=splits, exclude_self=True)[0][:, knn - 1]
        assert torch.equal(got, want), (knn, splits, x.data_ptr() % 16)
    assert torch.equal(got, K.knn_radii_sq(one_bank[0], nx, pivot, knn, splits))                    # (and the two paths agree)


def test_radii_of_a_bank_with_two_identical_rows(dev):
    x = FC.case("c2")[0].clone()
    x[77] = x[5]
    x = x.to(dev)
    pivot = K.feat_colmean(x)
    own = M.pairwise_sqdist(x, pivot=pivot)
    n5 = float(K.feat_norms(x, pivot)[5])
    # the twins' distance is fl32(2 n) - 2 dot of the SAME row: within E of 0, clamped at 0 where it comes out negative
    assert 0.0 <= float(own[5, 77]) == float(own[77, 5]) <= (8 + 8) * 2.0 ** -24 * 2 * n5
    assert bool((own >= 0).all()) and not bool(torch.isnan(own).any())
    for knn in (1, 3):
        got = M.knn_radii(x, knn, pivot=pivot, squared=True, _splits=2)
        assert torch.equal(got, own.kthvalue(knn + 1, dim=1).values) and not bool(torch.isnan(got).any())
    assert float(M.knn_radii(x, 1, pivot=pivot, squared=True)[5]) == float(own[5, 77])     # its twin is its nearest neighbour


# ------------------------------------------------------------------------------------------------ 4. hits
@pytest.mark.parametrize("splits", [1, 2, 16])
@pytest.mark.parametrize("name", ["c1", "c3"])
def test_hits_are_the_comparison_on_the_kernels_own_matrix(dev, name, splits):
    real, fake = (t.to(dev) for t in FC.case(name))
    pivot = K.feat_colmean(real)
    for ref, qry in ((real, fake), (fake, real)):
        r2 = M.knn_radii(ref, FC.KNN, pivot=pivot, squared=True, _splits=splits)
        want = (M.pairwise_sqdist(ref, qry, pivot=pivot) < r2[:, None]).any(0)
        got = M.manifold_hits(ref, r2, qry, pivot=pivot, _splits=splits)
        assert got.dtype == torch.bool and torch.equal(got, want), (name, splits)
        hit, count = K.manifold_hits(ref, K.feat_norms(ref, pivot), r2, qry, K.feat_norms(qry, pivot), pivot, splits)
        assert int(count) == int(want.sum()) == int(hit.sum()) and 0 < int(count) < qry.shape[0]
        assert int(K.manifold_hits(ref, K.feat_norms(ref, pivot), r2, qry, K.feat_norms(qry, pivot), pivot, splits, want_hits=False)[1]) == int(count)


# ------------------------------------------------------------------------------------------------ 5. precision / recall
@pytest.mark.parametrize("name", FC.ALL)
def test_precision_recall_against_fp64_under_the_ambiguity_rule(dev, name):
    real, fake = FC.case(name)
    rd, fd = real.to(dev), fake.to(dev)
    pivot = K.feat_colmean(rd)
    want = FC.truth(real, fake, pivot.cpu())                                  # fp64 on the very xt the kernels multiply
    out = M.precision_recall(rd, fd, FC.KNN)
    assert (out["n_real"], out["n_fake"], out["knn"]) == (real.shape[0], fake.shape[0], FC.KNN)
    r2_real, r2_fake = M.knn_radii(rd, FC.KNN, pivot=pivot, squared=True), M.knn_radii(fd, FC.KNN, pivot=pivot, squared=True)
    for key, hits, n in (("precision", M.manifold_hits(rd, r2_real, fd, pivot=pivot), fake.shape[0]),
                         ("recall", M.manifold_hits(fd, r2_fake, rd, pivot=pivot), real.shape[0])):
        amb, w = want[f"{key}_ambiguous"], want[f"{key}_hits"]
        print(f"[measured] {name} {key}: kernel {out[key]:.5f} fp64 {want[key]:.5f}, ambiguous queries {int(amb.sum())} of {n}, "
              f"decisions that differ {int((hits.cpu() != w).sum())}")
        assert int(amb.sum()) <= FC.AMBIGUOUS_CAP * n                         # (c) a condition on the inputs
        assert torch.equal(hits.cpu()[~amb], w[~amb])                        # (a) every other query matches fp64 exactly
        assert out[key] == int(hits.sum()) / n                                # the public figure is the count of those hits
        assert abs(int(hits.sum()) - int(w.sum())) <= int(amb.sum())          # (b)
    for split in (1, 16):
        assert M.precision_recall(rd, fd, FC.KNN, _splits=split) == out
    if name in ("c0", "c1"):                                                  # the reference's own class on these features, in fp64 and in fp32
        g = FC.golden(name)
        for tag in ("f64", "f32"):
            for key, n, a in (("precision", fake.shape[0], "precision_ambiguous"), ("recall", real.shape[0], "recall_ambiguous")):
                ref_count = round(float(g[f"{key}_{tag}"]) * n)
                assert abs(round(out[key] * n) - ref_count) <= int(want[a].sum()), (name, tag, key)
    # the radii: every entry of a row is within E of its fp64 value, so the order statistic is within the row's largest E
    for r2, bank, key in ((r2_real, real, "radii_real"), (r2_fake, fake, "radii_fake")):
        nb = FC.norms(FC.centred(bank, pivot.cpu()))
        assert bool(((r2.cpu().double() - want[key] ** 2).abs() <= FC.bound(nb, nb, real.shape[1]).max(dim=1).values).all()), key


# ------------------------------------------------------------------------------------------------ 6. memory: the fusion is real
def test_precision_recall_never_holds_the_matrix(dev):
    n = m = 4096
    real, fake = (t.to(dev) for t in FC.make(5, n, m, 64))
    K.Workspace.get(16 * n * 16 * 4, dev)                                     # the partial lists at S = 16: 4 MiB, part of the budget below
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = M.precision_recall(real, fake, 3, _splits=16)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(dev) - before + 16 * n * 16 * 4
    print(f"[measured] precision_recall 4096 x 4096 x 64: peak allocation above the inputs {extra / 2 ** 20:.2f} MiB (one fp32 matrix: 64 MiB); "
          f"precision {out['precision']:.4f} recall {out['recall']:.4f}")
    assert extra < n * m * 4 // 4                                             # under a quarter of ONE materialised matrix: 16 MiB
    assert K.fidelity_workspace_bytes(K.make_fidelity_desc(n, m, 64, 3, 16)) == 4 << 20
    r2 = M.knn_radii(real, 3, squared=True)
    assert torch.equal(r2, M.pairwise_sqdist(real).kthvalue(4, dim=1).values)   # 32 x 32 tiles, the planner's splits
    inside = (M.pairwise_sqdist(real, fake) < r2[:, None]).any(0)             # the materialised form of the same decisions, 32 x 32 tiles
    assert out["precision"] == int(inside.sum()) / m and 0 < out["precision"] < 1 and 0 <= out["recall"] < 1


# ------------------------------------------------------------------------------------------------ 7. the meter and the extractor
def _embedder(kind, dev):
    from tests import vq_restate as V
    m = M.VAE(**R.tiny_vae_kwargs()) if kind == "VAE" else M.VQVAE(**V.tiny_vq_kwargs(num_embeddings=100, deep_supervision=0))
    S.synth_state_dict(m, f"metrics.{kind}.")
    return m.to(dev).eval()


@pytest.mark.parametrize("kind", ["VAE", "VQVAE"])
def test_meter_over_embedder_features(dev, kind, monkeypatch):
    emb = _embedder(kind, dev)
    g = torch.Generator().manual_seed(9)
    real = (torch.rand(12, 3, 32, 32, generator=g) * 2 - 1).to(dev)
    fake = (torch.rand(10, 3, 32, 32, generator=g) * 1.6 - 0.8).to(dev)
    # the source an embedder would draw from when none is handed to it: begun, two draws behind it -- an encode() that drew would begin it
    # again (draw_index back to 0) and draw once (1)
    from medfusion_amd import vae as vae_module
    src = M.PhiloxDeviceNoise(11)
    src.begin(2, dev)
    src.draw((2, 4))
    src.draw((2, 4))
    monkeypatch.setattr(vae_module, "default_noise", lambda: src)
    assert src.draw_index == 2
    torch.manual_seed(3)
    state = torch.get_rng_state()
    feats = M.EmbedderFeatures(emb)
    meter = M.FidelityMeter(feats, knn=3)
    meter.update(real[:5], real=True)
    meter.update(fake, real=False)
    meter.update(real[5:], real=True)
    assert src.draw_index == 2 and torch.equal(torch.get_rng_state(), state)              # nothing begun, nothing drawn
    if kind == "VAE":                                                                     # (the spy is live: a plain encode() does draw from it)
        emb.encode(real[:2])
        assert src.draw_index == 1
        src.draw((2, 4))
    if kind == "VAE":
        mom = emb._encode_moments(real)
        by_hand = lambda x: emb._encode_moments(x)[:, :mom.shape[1] // 2].reshape(x.shape[0], -1).contiguous()
    else:
        by_hand = lambda x: emb.encode(x).reshape(x.shape[0], -1).contiguous()
    fr, ff = torch.cat([by_hand(real[:5]), by_hand(real[5:])]), by_hand(fake)
    br, bf = meter.banks()
    assert torch.equal(br, fr) and torch.equal(bf, ff) and br.dtype == torch.float32 and br.shape[0] == 12
    out = meter.compute()
    want = M.precision_recall(fr, ff, 3)
    assert {k: out[k] for k in want} == want and out["fd"] == M.frechet_distance(fr, ff) and out["fd"] == out["fd"] and abs(out["fd"]) < float("inf")
    print(f"[measured] meter {kind}: D {br.shape[1]}, FD {out['fd']:.4f}, precision {out['precision']:.3f}, recall {out['recall']:.3f}")
    c = br.shape[1] // 16                                                    # 32 x 32 images: a [c, 4, 4] latent
    pooled = M.EmbedderFeatures(emb, pool=2)(real)
    assert pooled.shape == (12, 4 * c)
    assert torch.allclose(pooled, torch.nn.functional.avg_pool2d(by_hand(real).view(12, c, 4, 4), 2).reshape(12, -1), atol=1e-6)
    with pytest.raises(ValueError, match="imgs"):
        feats(real[None])
    meter.reset()
    with pytest.raises(ValueError, match="update"):
        meter.compute()
