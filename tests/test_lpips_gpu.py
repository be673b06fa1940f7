"""LPIPS on the device against the restatement of tests/lpips_cases.py: the direct convolution, pooling and ReLU, the layer distance, the whole
metric on both trunks and both arithmetics, the meters and the evaluation script."""
import importlib.util
import json
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import medfusion_amd as M
from medfusion_amd import kernels as K
from medfusion_amd import lpips as LP
from oracle import restate as R
from oracle import synth as S
from tests import inception_cases as IC
from tests import lpips_cases as LC

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the direct convolution
@pytest.mark.parametrize("case", LC.DIRECT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_direct_convolution(dev, case):
    n, h, w_, cin, cout, k, s, p = case
    x, w, b, y64, bound = LC.direct_case(case)
    xd, wd, bd = x.to(dev), K.pack_direct_conv_weight(w.to(dev)), b.to(dev)
    plain = K.conv2d_direct(xd, wd, bd, K.make_direct_conv_desc(n, h, w_, cin, cout, k, k, s, p))
    assert plain.shape == y64.shape
    ratio = float(((plain.cpu().double() - y64).abs() / bound).max())
    print(f"[measured] direct conv {case}: max |y - y64| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    fused = K.conv2d_direct(xd, wd, bd, K.make_direct_conv_desc(n, h, w_, cin, cout, k, k, s, p, relu=True))
    assert torch.equal(fused, torch.relu(plain)) and bool((plain < 0).any())
    assert torch.equal(K.conv2d_direct(xd, wd, bd, K.make_direct_conv_desc(n, h, w_, cin, cout, k, k, s, p)), plain)
    nobias = K.conv2d_direct(xd, wd, None, K.make_direct_conv_desc(n, h, w_, cin, cout, k, k, s, p))
    want = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), None, stride=s, padding=p).permute(0, 2, 3, 1)
    assert float(((nobias.cpu().double() - want).abs() / bound).max()) <= 1.0
    # the exact oracle: one fma chain per output from +0 over (kh, kw, cin) ascending, padding taps as zeros; then one fp32 add of the bias
    chain = IC.fma_chain_conv(x, w.permute(2, 3, 1, 0).contiguous(), (p, p), s)
    assert torch.equal(nobias.cpu(), chain) and torch.equal(plain.cpu(), chain + b)


# ------------------------------------------------------------------------------------------------ 2. pooling and ReLU
@pytest.mark.parametrize("channels", LC.POOL_CHANNELS)
@pytest.mark.parametrize("k,side", LC.POOL_CASES)
def test_maxpool_is_exact(dev, k, side, channels):
    x = torch.randn((2, side, side + 1, channels), generator=torch.Generator().manual_seed(side))
    got = K.maxpool_nhwc(x.to(dev), k, 2)
    want = F.max_pool2d(x.permute(0, 3, 1, 2), k, 2).permute(0, 2, 3, 1)
    assert got.shape == want.shape and got.shape[1] == (side - k) // 2 + 1 and torch.equal(got.cpu(), want)


def test_relu_is_exact_on_both_load_paths(dev):
    for n, off in ((1, 0), (7, 0), (4099, 0), (4099, 1), (65 * 1024, 3)):
        x = torch.randn(n + off, generator=torch.Generator().manual_seed(n))
        x[::5] = 0.0
        buf = x.to(dev)
        K.relu_(buf[off:])
        assert torch.equal(buf[off:].cpu(), F.relu(x[off:])) and torch.equal(buf[:off].cpu(), x[:off])


# ------------------------------------------------------------------------------------------------ 3. the layer distance
def _offset(t, dev):
    """the same values at an address 4 bytes past a 16-byte boundary: the element-wise load path"""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
    buf[1:] = t.flatten().to(dev)
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize("P", LC.LAYER_PIXELS)
@pytest.mark.parametrize("C", LC.LAYER_CHANNELS)
def test_layer_distance(dev, C, P):
    fx, fy, w = LC.layer_case(C, P)
    if P > 1:
        fx[0, 0] = 0.0                      # a pixel whose vector is all zero in one map ...
        fx[1, P - 1] = 0.0
        fy[1, P - 1] = 0.0                  # ... and in both
    want, bound = LC.layer_reference(fx, fy, w)
    wd = w.to(dev)
    vec = K.lpips_layer(fx.to(dev), fy.to(dev), wd)[:, 0]
    assert fx.to(dev).data_ptr() % 16 == 0
    ratio = float(((vec.cpu() - want).abs() / bound).max())
    print(f"[measured] layer distance C {C} P {P}: max |term - term64| / bound = {ratio:.3f} (relative error {float(((vec.cpu() - want).abs() / want).max()):.2e})")
    assert ratio <= 1.0 and float(want.min()) > 0
    elem = K.lpips_layer(_offset(fx, dev), _offset(fy, dev), wd)[:, 0]
    assert torch.equal(elem, vec)                                                      # the two load paths: the same bits
    assert torch.equal(K.lpips_layer(fx.to(dev), fx.to(dev), wd), torch.zeros((2, 1), dtype=torch.float64, device=dev))     # identical maps: exactly 0
    assert torch.equal(K.lpips_layer(_offset(fy, dev), fy.to(dev), wd), torch.zeros((2, 1), dtype=torch.float64, device=dev))
    # a pair's bits alone and at each place of a batch of 3
    ox, oy, _ = LC.layer_case(C, P, B=3, seed=1)
    for place in range(3):
        bx, by = ox.clone(), oy.clone()
        bx[place], by[place] = fx[1], fy[1]
        terms = torch.zeros((3, 5), dtype=torch.float64, device=dev)
        total = torch.zeros(3, dtype=torch.float32, device=dev)
        K.lpips_layer(bx.to(dev), by.to(dev), wd, terms, 4, total)
        assert torch.equal(terms[place, 4], vec[1]) and torch.equal(total[place], vec[1].float()) and float(terms[:, :4].abs().max()) == 0


def test_all_zero_maps_give_zero_not_nan(dev):
    z = torch.zeros((1, 9, 64), device=dev)
    f = torch.rand((1, 9, 64), device=dev)
    w = torch.full((64,), 0.5, device=dev)
    assert float(K.lpips_layer(z, z, w)) == 0.0
    got = float(K.lpips_layer(z, f, w))          # a^ = 0, b^ a unit vector: d_p = 0.5 sum b^2 = 0.5
    assert abs(got - 0.5) < 1e-9


# ------------------------------------------------------------------------------------------------ 4. the whole metric
@pytest.mark.parametrize("arithmetic", ["split3", "fp32"])
@pytest.mark.parametrize("net_name", LC.NETS)
def test_whole_metric(dev, net_name, arithmetic):
    bounds = LC.whole_bounds(net_name)
    worst = torch.zeros(5, dtype=torch.float64)
    for seed, std, shape, x, y, t64, _ in LC.whole_cases(net_name):
        net = LC.seeded(net_name, seed, std).with_arithmetic(arithmetic)
        xd, yd = x.to(dev), y.to(dev)
        val, terms = LP.lpips(xd, yd, net, return_terms=True)
        assert val.shape == (shape[0],) and terms.shape == (shape[0], 5) and val.dtype == terms.dtype == torch.float32
        # the fp32 terms the function returns are the roundings of the fp64 terms it holds; the returned ones are held to the bound
        t = torch.empty((shape[0], 5), dtype=torch.float64, device=dev)
        tot = torch.empty(shape[0], dtype=torch.float32, device=dev)
        LP._trunk_pass(xd, yd, net, False, t, tot)
        assert torch.equal(t.float(), terms) and torch.equal(tot, val)
        rel = ((terms.cpu().double() - t64).abs() / t64).max(dim=0).values
        rel64 = ((t.cpu() - t64).abs() / t64).max(dim=0).values
        worst = torch.maximum(worst, rel / bounds)
        print(f"[measured] {net_name} {arithmetic} seed {seed} {shape}: rel err per layer {[f'{v:.2e}' for v in rel.tolist()]} "
              f"(before the rounding to fp32 {[f'{v:.2e}' for v in rel64.tolist()]})")
        assert float(((val.cpu().double() - t64.sum(1)).abs() / t64.sum(1)).max()) < 1e-4
        assert torch.equal(LP.lpips(xd, xd.clone(), net), torch.zeros(shape[0], device=dev))              # lpips(x, x): exactly 0
        assert torch.equal(LP.lpips(xd, yd, net, chunk=1), val)                                           # chunk = 1: the bits of chunk = None
        n01 = LP.lpips((xd + 1) / 2, (yd + 1) / 2, net, normalize=True)
        assert float(((n01 - val).abs() / val).max()) < 1e-4
    print(f"[measured] {net_name} {arithmetic}: worst rel err / bound per layer {[f'{v:.3f}' for v in worst.tolist()]} (bounds {[f'{v:.2e}' for v in bounds.tolist()]})")
    assert bool((worst <= 1.0).all()), (worst.tolist(), bounds.tolist())


@pytest.mark.parametrize("net_name", LC.NETS)
def test_volume_is_the_mean_of_its_slices(dev, net_name):
    net = LC.seeded(net_name, 2, 0.05)
    x, y = (t.to(dev) for t in LC.make_pair((1, 1, 3, 32, 32), 9))
    vol, vterms = LP.lpips(x, y, net, return_terms=True)
    per = [LP.lpips(x[:, :, d], y[:, :, d], net, return_terms=True) for d in range(3)]
    assert vol.shape == (1,) and vterms.shape == (1, 5)
    assert torch.equal(vol, torch.stack([v for v, _ in per], 1).double().mean(1).float())
    want = LC.ref_terms(net, x[0].permute(1, 0, 2, 3).cpu(), y[0].permute(1, 0, 2, 3).cpu(), torch.float64).sum(1).mean()
    assert abs(float(vol) - float(want)) / float(want) < 1e-4


# ------------------------------------------------------------------------------------------------ 5. the meters and the script
def test_reconstruction_meter_accumulates_lpips(dev):
    emb = M.VAE(**R.tiny_vae_kwargs())
    S.synth_state_dict(emb, "lpips.VAE.")
    emb = emb.to(dev).eval()
    net = LC.seeded("alex", 1)
    x = LC.make_pair((3, 3, 176, 176), 4)[0].to(dev)
    src, bare = M.PhiloxDeviceNoise(11), M.PhiloxDeviceNoise(11)
    torch.manual_seed(3)
    want_out = torch.cat([emb(x[i:j], noise=bare)[0].clamp(-1, 1) for i, j in ((0, 2), (2, 3))])
    state_bare = torch.get_rng_state()
    torch.manual_seed(3)
    meter = M.ReconstructionMeter(emb, noise=src, lpips=net)
    meter.update(x[:2])
    meter.update(x[2:])
    assert getattr(src, "draw_index", None) == getattr(bare, "draw_index", None) and torch.equal(torch.get_rng_state(), state_bare)
    lp = meter.lpips_values()
    assert torch.equal(lp, LP.lpips(x, want_out, net)) and float(lp.min()) > 0
    plain = M.ReconstructionMeter(emb, noise=M.PhiloxDeviceNoise(11))
    plain.update(x[:2])
    plain.update(x[2:])
    out, base = meter.compute(), plain.compute()
    assert {k: out[k] for k in base} == base and set(out) - set(base) == {"lpips_mean", "lpips_std", "lpips_score"}
    assert out["lpips_mean"] == float(lp.mean()) and out["lpips_std"] == float(torch.std(lp)) and out["lpips_score"] == 1.0 - out["lpips_mean"]
    with pytest.raises(ValueError, match="LPIPS"):
        plain.lpips_values()


def test_volume_meter_accumulates_lpips(dev):
    net = LC.seeded("vgg", 1)
    x, y = (t.to(dev) for t in LC.make_pair((2, 1, 44, 44, 44), 6))
    rows = iter((y[:1], y[1:]))
    meter = M.VolumeReconstructionMeter(lambda t: (next(rows), None), lpips=net)
    meter.update(x[:1])
    meter.update(x[1:])
    assert torch.equal(meter.lpips_values(), LP.lpips(x, y, net))
    assert meter.compute()["lpips_score"] == 1.0 - float(meter.lpips_values().mean())


def test_evaluation_script_logs_the_lpips_score(dev, tmp_path):
    import numpy as np
    from PIL import Image
    spec = importlib.util.spec_from_file_location("_lpips_evaluate", ROOT / "scripts" / "evaluate_latent_embedder.py")
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    rng = np.random.default_rng(0)
    (tmp_path / "images").mkdir()
    for i in range(3):
        Image.fromarray(rng.integers(0, 256, (176, 176, 3), dtype=np.uint8)).save(tmp_path / "images" / f"im_{i}.png")
    trunk, lin = LC.seeded("alex", 1).state_dicts()
    torch.save(trunk, tmp_path / "trunk.pth")
    torch.save(lin, tmp_path / "lin.pth")
    head = ["--synthetic", "--images", str(tmp_path / "images"), "--batch", "2"]
    res = ev.main(head + ["--out", str(tmp_path / "with"), "--lpips-net", "alex", "--lpips-trunk", str(tmp_path / "trunk.pth"), "--lpips-lin", str(tmp_path / "lin.pth")])
    log = next((tmp_path / "with").glob("metrics_*.log")).read_text()
    assert f"LPIPS Score: {res['lpips_score']}" in log and "not built" not in log and 0 < res["lpips_mean"] and res["lpips_score"] == 1.0 - res["lpips_mean"]
    saved = json.loads(next((tmp_path / "with").glob("metrics_*.json")).read_text())
    assert saved["lpips"] == res["lpips_score"] and saved["lpips_net"] == "alex"
    bare = ev.main(head + ["--out", str(tmp_path / "without")])
    log = next((tmp_path / "without").glob("metrics_*.log")).read_text()
    assert "LPIPS: not built (needs VGG weights)" in log and "LPIPS Score" not in log
    saved = json.loads(next((tmp_path / "without").glob("metrics_*.json")).read_text())
    assert saved["lpips"] is None and not any(k.startswith("lpips_") for k in saved)
    assert {k: bare[k] for k in ("ms_ssim_mean", "mse_mean", "count")} == {k: res[k] for k in ("ms_ssim_mean", "mse_mean", "count")}
