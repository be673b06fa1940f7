"""spatial_dims=3 on a real MI355X: the 3-D fp16-pair convolution (csrc/conv3d.hip) against an fp64 F.conv3d on the CPU, and the 3-D blocks,
UNet, VAE and sampling pipeline against the reference's fixtures (tests/golden/d3_*, scripts/gen_3d_golden.py)."""

import pytest
import torch
import torch.nn.functional as F

from medfusion_amd import kernels as K
from tests.util import relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rand(seed, shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


def _ref(x1, x2, w, b, stride, pad, up):
    """fp64 on the CPU: torch.cat of the two sources, nearest x2 per axis, F.conv3d"""
    x = torch.cat([x1, x2], 1) if x2 is not None else x1
    if any(up):
        x = F.interpolate(x, scale_factor=tuple(2.0 if u else 1.0 for u in up), mode="nearest")
    return F.conv3d(x, w, b, stride, pad)


def _operand(x, dev):
    """NCDHW fp64 -> the kernel's operand: NDHWC fp32 (C % 32 == 0), or the zero-padded pair operand of pack_nchw_pairs"""
    n, c, d, h, w = x.shape
    xd = x.float().to(dev)
    if c % 32 == 0:
        return xd.permute(0, 2, 3, 4, 1).contiguous(), c
    cp = -(-c // 32) * 32
    return K.pack_nchw_pairs(xd.reshape(n, c, d * h, w), cp), cp


def _run(x1, x2, w, b, stride, pad, up, dev, tile=0, sk=0):
    n, _, d, h, wd = x1.shape
    a1, c1 = _operand(x1, dev)
    a2, c2 = _operand(x2, dev) if x2 is not None else (None, 0)
    co, k = w.shape[0], w.shape[2]
    wh = K.split_weight_f16x2(K.pack_conv3d_weight(w.float().to(dev), c1 + c2 if x2 is not None else c1))
    desc = K.make_conv3d_desc(n, d, h, wd, c1, c2, co, k, stride, pad, up, tile_hint=tile, splitk_hint=sk)
    assert K.conv3d_ok(desc)
    y = K.conv3d_f16x2(a1, wh, b.float().to(dev), desc, x2=a2)
    return y, desc


def _pad_of(k, s):
    return tuple(int((k - a + 1) / 2) for a in s)


GEOMS = [  # (D, H, W), k, stride, upsample
    ((5, 7, 9), 3, (1, 1, 1), (0, 0, 0)),
    ((5, 7, 9), 3, (2, 2, 2), (0, 0, 0)),
    ((5, 7, 9), 3, (1, 2, 2), (0, 0, 0)),
    ((5, 7, 9), 1, (1, 1, 1), (0, 0, 0)),
    ((3, 4, 5), 3, (1, 1, 1), (1, 1, 1)),
    ((3, 4, 5), 3, (1, 1, 1), (0, 1, 1)),
]


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}k{g[1]}s{''.join(map(str, g[2]))}u{''.join(map(str, g[3]))}")
@pytest.mark.parametrize("cin,cout", [(1, 16), (3, 3), (8, 64), (32, 16), (96, 256), (256, 64)])
def test_conv3d_against_fp64(dev, geom, cin, cout):
    dhw, k, stride, up = geom
    seed = hash((dhw, k, stride, up, cin, cout)) % (1 << 30)
    x = _rand(seed, (2, cin, *dhw))
    w = _rand(seed + 1, (cout, cin, k, k, k), 1.0 / (cin * k ** 3) ** 0.5)
    b = _rand(seed + 2, (cout,), 0.1)
    pad = _pad_of(k, stride)
    want = _ref(x, None, w, b, stride, pad, up)
    y, _ = _run(x, None, w, b, stride, pad, up, dev)
    assert y.shape == (2, *want.shape[2:], cout)
    e = relerr(y.permute(0, 4, 1, 2, 3), want)
    assert e < 1e-5, (geom, cin, cout, e)


def test_conv3d_every_tile_and_split(dev):
    """every tile (1..4) and every split-K factor the planner can pick (1, 2, 4, 8, 16) on a fused two-source concat with an odd Cout"""
    x1, x2 = _rand(11, (2, 64, 3, 5, 6)), _rand(12, (2, 32, 3, 5, 6))
    w = _rand(13, (67, 96, 3, 3, 3), 1.0 / (96 * 27) ** 0.5)
    b = _rand(14, (67,), 0.1)
    want = _ref(x1, x2, w, b, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    outs = {}
    for tile in (1, 2, 3, 4):
        for sk in (1, 2, 4, 8, 16):
            y, d = _run(x1, x2, w, b, (1, 1, 1), (1, 1, 1), (0, 0, 0), dev, tile, sk)
            assert K.conv3d_plan(d) == (tile, sk)
            e = relerr(y.permute(0, 4, 1, 2, 3), want)
            assert e < 1e-5, (tile, sk, e)
            outs[(tile, sk)] = y
    # the planner's own choices are among them
    for m in ((1, 3, 5, 6), (4, 8, 16, 16)):
        t, s = K.conv3d_plan(K.make_conv3d_desc(m[0], m[1], m[2], m[3], 64, 32, 67, 3, 1, 1))
        assert 1 <= t <= 4 and s in (1, 2, 4, 8, 16)


def test_conv3d_two_sources_with_their_own_scales(dev):
    """the fused concat: the two sources carry different per-sample scales (x2 ~ 1e3 x1), and the samples of the batch differ by 1e6"""
    x1, x2 = _rand(21, (3, 32, 4, 6, 5)), _rand(22, (3, 64, 4, 6, 5)) * 1e3
    x1[1] *= 1e6
    x2[2] *= 1e-6
    w = _rand(23, (48, 96, 3, 3, 3), 1.0 / (96 * 27) ** 0.5)
    b = _rand(24, (48,), 0.1)
    want = _ref(x1, x2, w, b, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    for sk in (1, 4):
        y, _ = _run(x1, x2, w, b, (1, 1, 1), (1, 1, 1), (0, 0, 0), dev, 0, sk)
        got = y.permute(0, 4, 1, 2, 3)
        for n in range(3):   # per sample: an error in the small sample must not hide behind the large one
            assert relerr(got[n], want[n]) < 1e-5, (sk, n)


def test_conv3d_rows_differ_by_1e6(dev):
    x = _rand(31, (2, 32, 4, 5, 6))
    x[0] *= 1e6
    w = _rand(32, (32, 32, 3, 3, 3), 1.0 / (32 * 27) ** 0.5)
    b = _rand(33, (32,), 0.1)
    want = _ref(x, None, w, b, (2, 2, 2), (1, 1, 1), (0, 0, 0))
    y, _ = _run(x, None, w, b, (2, 2, 2), (1, 1, 1), (0, 0, 0), dev)
    got = y.permute(0, 4, 1, 2, 3)
    for n in range(2):
        assert relerr(got[n], want[n]) < 1e-5, n


def test_conv3d_is_bit_reproducible(dev):
    x1, x2 = _rand(41, (2, 64, 4, 6, 6)), _rand(42, (2, 64, 4, 6, 6))
    w = _rand(43, (128, 128, 3, 3, 3), 1.0 / (128 * 27) ** 0.5)
    b = _rand(44, (128,), 0.1)
    for sk in (0, 1, 8):
        a, _ = _run(x1, x2, w, b, (1, 1, 1), (1, 1, 1), (0, 0, 0), dev, 0, sk)
        c, _ = _run(x1, x2, w, b, (1, 1, 1), (1, 1, 1), (0, 0, 0), dev, 0, sk)
        assert torch.equal(a, c), sk


# ------------------------------------------------------------------------------------------------ models against the reference's fixtures
import medfusion_amd as M  # noqa: E402
from medfusion_amd import blocks3d as B3  # noqa: E402
from oracle import restate as R  # noqa: E402
from oracle import synth as S  # noqa: E402
from tests.d3_cases import BLOCK_CASES, SAMPLE_CASES, UNET_CASES, VAE_CASE, block_kwargs, unet_kwargs  # noqa: E402
from tests.util import T, gold, oracle_noise, to_product_kwargs  # noqa: E402

TOL = 1e-4


def _act(x5, dev):
    """NCDHW (CPU) -> an activation of the 3-D path: the [N, D*H, W, C] view of NDHWC"""
    n, c, d, h, w = x5.shape
    return B3.tag(x5.to(dev).permute(0, 2, 3, 4, 1).contiguous().view(n, d * h, w, c), (d, h, w))


@pytest.mark.parametrize("name", sorted(BLOCK_CASES))
def test_block_matches_reference(dev, name):
    cls, kw, shapes, emb = BLOCK_CASES[name]
    m = getattr(B3, cls)(**block_kwargs(cls, kw))
    S.synth_state_dict(m, f"d3.{name}.")
    m.to(dev).eval()
    xs = [_act(S.synth_input(f"d3.{name}.x{i}", s), dev) for i, s in enumerate(shapes)]
    x = tuple(xs) if len(xs) > 1 else xs[0]   # two sources: torch.cat([h, skip], 1) of the reference, fused into the convolutions
    with torch.no_grad():
        if emb:
            y = m(x, m.local_embed(S.synth_input(f"d3.{name}.emb", (shapes[0][0], emb)).to(dev)))
        else:
            y = m(x)
    want = T(gold("d3_blocks")[f"{name}.y"])
    got = B3.to_ncdhw(y)
    assert got.shape == want.shape
    assert relerr(got, want) < TOL, name


def _unet(dev, strides, prefix, in_ch=8):
    m = M.UNet(**to_product_kwargs(unet_kwargs(strides, in_ch=in_ch)))
    S.synth_state_dict(m, prefix)
    return m.to(dev).eval()


@pytest.mark.parametrize("name", sorted(UNET_CASES))
def test_unet_matches_reference(dev, name):
    strides, shape = UNET_CASES[name]
    m = _unet(dev, strides, f"d3.{name}.")
    g = gold("d3_unet")
    y, _ = m(S.synth_input(f"d3.{name}.x", shape).to(dev), T(g[f"{name}.t"]).to(dev), T(g[f"{name}.c"]).to(dev))
    assert y.shape == shape
    assert relerr(y, T(g[f"{name}.y"])) < TOL, name


def test_vae_encode_decode_match_reference(dev):
    m = M.VAE(**VAE_CASE)
    S.synth_state_dict(m, "d3.vae.")
    m.to(dev).eval()
    g = gold("d3_vae")
    z = m.encode(S.synth_input("d3.vae.img", (2, 1, 16, 32, 32), 0.5).to(dev), noise=oracle_noise(int(g["seed"])))
    assert relerr(z, T(g["z"])) < TOL
    x = m.decode(S.synth_input("d3.vae.z", (2, VAE_CASE["emb_channels"], 2, 4, 4)).to(dev))
    assert x.shape == (2, 1, 16, 32, 32)
    assert relerr(x, T(g["x_dec"])) < TOL


def _pipe(dev, name, objective="x_T", vae=False):
    kw = to_product_kwargs(unet_kwargs([1, 2, 2, 2], in_ch=4))
    pipe = M.DiffusionPipeline(M.GaussianNoiseScheduler, M.UNet, None, R.published_scheduler_kwargs(), kw, estimator_objective=objective, clip_x0=False)
    S.synth_state_dict(pipe.noise_estimator, f"d3.{name}.unet.")
    if vae:
        pipe.latent_embedder = M.VAE(**dict(VAE_CASE, emb_channels=4))
        S.synth_state_dict(pipe.latent_embedder, f"d3.{name}.vae.")
    return pipe.to(dev).eval()


@pytest.mark.parametrize("name", sorted(SAMPLE_CASES))
def test_sample_trajectory_matches_reference(dev, name):
    seed, steps, use_ddim, gs, cond, objective = SAMPLE_CASES[name]
    pipe = _pipe(dev, name, objective)
    g = gold(name)
    extra = {} if cond is None else dict(condition=torch.tensor(cond, device=dev), guidance_scale=gs, un_cond=None)
    img = pipe.sample(int(g["n"]), tuple(int(a) for a in g["size"]), steps=steps, use_ddim=use_ddim, noise=oracle_noise(seed), **extra)
    assert img.shape == tuple(g["image"].shape)
    assert relerr(img, T(g["image"])) < TOL, name


@pytest.mark.parametrize("use_ddim,cond", [(True, [1, 0]), (False, None)], ids=["ddim_cfg", "ddpm"])
def test_the_three_loop_forms_are_bit_identical(dev, use_ddim, cond):
    """eager, command list (the default) and hipGraph give the same bits in 3-D: the 3-D forward is launches of the library only"""
    pipe = _pipe(dev, "loops", vae=True)
    extra = {} if cond is None else dict(condition=torch.tensor(cond, device=dev), guidance_scale=8.0, un_cond=None)
    kw = dict(steps=6, use_ddim=use_ddim, **extra)
    eager = pipe.sample(2, (4, 4, 4, 4), noise=M.PhiloxDeviceNoise(7), loop="eager", **kw)
    listed = pipe.sample(2, (4, 4, 4, 4), noise=M.PhiloxDeviceNoise(7), loop="cmdlist", **kw)
    graph = pipe.sample(2, (4, 4, 4, 4), noise=M.PhiloxDeviceNoise(7), loop="graph", **kw)
    assert eager.shape == (2, 1, 32, 32, 32) and bool(eager.isfinite().all())
    assert torch.equal(eager, listed)
    assert torch.equal(eager, graph)
    assert pipe.last_cmdlist_launches > 20


def test_interpolate_runs_in_3d(dev):
    pipe = _pipe(dev, "interp")
    a = S.synth_input("d3.interp.a", (2, 4, 4, 8, 8)).to(dev)
    b = S.synth_input("d3.interp.b", (2, 4, 4, 8, 8)).to(dev)
    out = pipe.interpolate(a, b, i=5, lam=0.5, noise=oracle_noise(3))
    assert out.shape == a.shape and bool(out.isfinite().all())
