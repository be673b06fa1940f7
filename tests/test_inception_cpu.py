"""The Inception network without a device: the restatement's shapes, the BatchNorm fold, the key list, the state round trip, every refusal, the plan,
the evaluation script's argument rules and its unchanged output without the new options, the Inception Score and the average pool's definition."""
import ctypes as C
import importlib.util
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import medfusion_amd as M
from medfusion_amd import inception as I
from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from tests import inception_cases as IC

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("mf_conv2d_gemm_out_dims", "mf_conv2d_gemm_plan", "mf_conv2d_gemm_f32", "mf_pool2d_nhwc_f32", "mf_inception_prepare_u8", "mf_mean_pixels_f32")


@pytest.fixture(scope="module")
def net():
    return I.InceptionNet.seeded(0, bias_std=0.1)


def _script(name):
    spec = importlib.util.spec_from_file_location(f"_inception_script_{name}", ROOT / "scripts" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ 1. shapes, keys, fold, state
@pytest.mark.parametrize("size", (75, 107, 299))
def test_shapes_of_the_trunk(size):
    shape = I.trace(size)
    assert tuple(shape[b][0] for b in IC.SIDE_BUFFERS) == IC.SIDES[size] and all(h == w for h, w, _ in shape.values())
    assert tuple(shape[b][2] for b in I.BLOCKS) == IC.BLOCK_CHANNELS
    assert shape["Mixed_7c"][0] == shape["Mixed_7b"][0] == IC.SIDES[size][-1] and shape["Mixed_6e"][0] == IC.SIDES[size][-2]
    assert shape["in"] == (size, size, 3) and shape["p64"][2] == 64 and shape["p192"][2] == 192


@pytest.mark.parametrize("size", (75, 107))
def test_the_restatement_runs_at_these_shapes(net, size):
    """forward_ref writes every branch into a buffer of trace()'s shape: a convolution or pool of another output size cannot be assigned"""
    out = IC.forward_ref(net, IC.images(1, 1, size + 3, size, seed=size), size, torch.float32)
    assert {k: v.shape[1] for k, v in out.items()} == {"64": 64, "192": 192, "768": 768, "2048": 2048, "logits_unbiased": 1008, "logits": 1008}
    assert all(bool(torch.isfinite(v).all()) for v in out.values()) and float(out["2048"].abs().max()) > 0


def test_key_list_is_94_basicconvs_and_the_fc(net):
    assert len(I.LAYERS) == 94 and len({name for name, *_ in I.LAYERS}) == 94
    keys = I.state_keys()
    assert len(keys) == 94 * 5 + 2 and keys[-2:] == ["fc.weight", "fc.bias"] and set(keys) == set(net.state_dict())
    assert "Mixed_6b.branch7x7dbl_3.conv.weight" in keys and "Mixed_7c.branch3x3dbl_3b.bn.running_var" in keys and "Conv2d_1a_3x3.bn.weight" in keys
    by = {name: rest for name, *rest in I.LAYERS}
    assert by["Mixed_6b.branch7x7dbl_3"] == [128, 128, 1, 7, 1, 0, 3] and by["Mixed_6c.branch7x7_3"] == [160, 192, 7, 1, 1, 3, 0]
    assert by["Conv2d_1a_3x3"] == [3, 32, 3, 3, 2, 0, 0] and by["Mixed_7c.branch3x3dbl_2"] == [448, 384, 3, 3, 1, 1, 1] and by["Mixed_7a.branch3x3_2"] == [192, 320, 3, 3, 2, 0, 0]
    assert by["Mixed_5b.branch_pool"][:2] == [192, 32] and by["Mixed_5c.branch_pool"][:2] == [256, 64] and by["Mixed_7c.branch1x1"][:2] == [2048, 320]
    assert max(cin * kh * kw for _, cin, _, kh, kw, *_ in I.LAYERS) == 4032 and I.CHAIN == 512


def test_batchnorm_fold_against_the_unfolded_form(net):
    g = torch.Generator().manual_seed(4)
    for index in (0, 10, 93):
        name, cin, cout, kh, kw, s, ph, pw = I.LAYERS[index]
        x = torch.randn((2, cin, 9, 9), generator=g, dtype=torch.float64)
        st = {k: net.state[f"{name}.bn.{k}"].double() for k in I.BN_KEYS}
        assert float(st["weight"].min()) >= 0.5 and float(st["running_var"].min()) >= 0.5 and float(st["bias"].abs().max()) > 0      # a non-trivial BatchNorm
        y = F.conv2d(x, net.state[f"{name}.conv.weight"].double(), None, stride=s, padding=(ph, pw))
        want = F.batch_norm(y, st["running_mean"], st["running_var"], st["weight"], st["bias"], training=False, eps=0.001)
        wf, bf = net.folded(index)
        assert wf.dtype == torch.float32 and bf.dtype == torch.float32
        got = F.conv2d(x, wf.double(), bf.double(), stride=s, padding=(ph, pw))
        # w' and b' are rounded once to fp32: (K + 1) roundings of 2^-24 relative to the magnitudes
        mag = F.conv2d(x.abs(), wf.double().abs(), bf.double().abs(), stride=s, padding=(ph, pw))
        assert bool(((got - want).abs() <= 2.0 ** -24 * mag * 1.01).all())
        s64 = st["weight"] / torch.sqrt(st["running_var"] + 0.001)
        assert torch.equal(wf, (net.state[f"{name}.conv.weight"].double() * s64.view(-1, 1, 1, 1)).float())
        assert torch.equal(bf, (st["bias"] - st["running_mean"] * s64).float())


def test_state_round_trip_and_refusals(net, tmp_path):
    sd = net.state_dict()
    again = I.InceptionNet.from_state(sd)
    assert again.rows == 1008 and all(torch.equal(again.state[k], sd[k]) for k in sd)
    extra = dict(sd)
    extra["AuxLogits.conv0.conv.weight"] = torch.zeros(3)
    extra["Conv2d_1a_3x3.bn.num_batches_tracked"] = torch.tensor(7)
    assert set(I.InceptionNet.from_state(extra).state_dict()) == set(sd)
    torch.save(sd, tmp_path / "net.pth")
    loaded = I.InceptionNet.from_file(tmp_path / "net.pth")
    assert all(torch.equal(loaded.state[k], sd[k]) for k in sd)
    small = I.InceptionNet.from_state({**sd, "fc.weight": sd["fc.weight"][:10], "fc.bias": sd["fc.bias"][:10]})
    assert small.rows == 10
    for key in ("Mixed_6b.branch7x7dbl_3.conv.weight", "Mixed_7c.branch_pool.bn.running_var", "fc.weight", "fc.bias"):
        with pytest.raises(ValueError, match=re.escape(key)):
            I.InceptionNet.from_state({k: v for k, v in sd.items() if k != key})
        with pytest.raises(ValueError, match=re.escape(key)):
            I.InceptionNet.from_state({**sd, key: sd[key][..., None]})
    with pytest.raises(ValueError, match="Conv2d_2a_3x3.conv.weight"):
        I.InceptionNet.from_state({**sd, "Conv2d_2a_3x3.conv.weight": sd["Conv2d_2a_3x3.conv.weight"][:, :5]})
    assert not torch.equal(I.InceptionNet.seeded(1).state["fc.weight"], sd["fc.weight"]) and float(I.InceptionNet.seeded(1).state["fc.bias"].abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_every_refusal_names_its_argument(net):
    x = torch.zeros((2, 3, 80, 80), dtype=torch.uint8)
    for bad, word in ((x.float(), "x: uint8"), (x[0], r"x: a non-empty \[B, C, H, W\]"), (x[:, :2], "x: 1 or 3 channels"), ("x", "x: a tensor"), (x[:0], "x: a non-empty"),
                      (x, "x: on a ROCm device")):
        with pytest.raises(ValueError, match=word):
            net.features(bad)
    for kw, word in (({"size": 74}, "size"), ({"size": 299.0}, "size"), ({"layer": "pool3"}, "layer"), ({"layer": ()}, "layer"), ({"layer": ("2048", "x")}, "layer"),
                     ({"chunk": 0}, "chunk"), ({"chunk": True}, "chunk"), ({"chunk": 1.5}, "chunk")):
        with pytest.raises(ValueError, match=f"^{word}:"):
            net.features(x, **kw)
    with pytest.raises(ValueError, match="^net:"):
        M.InceptionFeatures(object())
    with pytest.raises(ValueError, match="^layer:"):
        M.InceptionFeatures(net, layer=("2048",))
    with pytest.raises(ValueError, match="^value_range:"):
        M.InceptionFeatures(net, value_range=(0, 255))
    with pytest.raises(ValueError, match="^size:"):
        M.InceptionFeatures(net, size=10)
    f = M.InceptionFeatures(net)
    for bad, word in ((torch.zeros((2, 3, 8)), "imgs: 2-D images"), (torch.zeros((1, 3, 80, 80), dtype=torch.float64), "imgs: fp32 or uint8"), (torch.zeros((1, 3, 80, 80)), "imgs: on a ROCm")):
        with pytest.raises(ValueError, match=word):
            f(bad)
    for bad, word in (((torch.zeros(3),), "logits"), ((torch.zeros((4, 3)), 0), "splits"), ((torch.zeros((4, 3)), 5), "splits")):
        with pytest.raises(ValueError, match=f"^{word}:"):
            M.inception_score(*bad)
    with pytest.raises(ValueError, match="^B:"):
        I.plan(0)
    with pytest.raises(RuntimeError, match="no CPU"):
        net.to("cpu")


def test_library_codes_before_any_launch():
    lib = L.load()
    out = (C.c_int32 * 2)()

    def desc(**kw):
        base = dict(N=1, Hin=8, Win=8, Cin=4, Cout=8, kh=3, kw=3, stride=1, pad_h=1, pad_w=1)
        base.update(kw)
        return K.make_gemm_conv_desc(**base)

    assert lib.mf_conv2d_gemm_out_dims(C.byref(desc()), out) == 0 and tuple(out) == (8, 8)
    assert lib.mf_conv2d_gemm_out_dims(C.byref(desc(kh=1, kw=7, pad_h=0, pad_w=3)), out) == 0 and tuple(out) == (8, 8)
    assert lib.mf_conv2d_gemm_out_dims(C.byref(desc(stride=2, pad_h=0, pad_w=0, Hin=19, Win=23)), out) == 0 and tuple(out) == (9, 11)
    for bad in (desc(N=0), desc(Cin=0), desc(Cout=0), desc(kh=12), desc(kw=0), desc(stride=5), desc(stride=0), desc(pad_h=-1), desc(pad_w=-1), desc(chain=-1), desc(tile=4),
                desc(tile=-1), desc(ldy=7), desc(ldy=16, y_offset=9), desc(y_offset=1), desc(y_offset=-1, ldy=16), desc(Hin=2, pad_h=0), desc(Win=1, pad_w=0, kw=3)):
        assert lib.mf_conv2d_gemm_out_dims(C.byref(bad), out) == -1
        assert lib.mf_conv2d_gemm_plan(C.byref(bad), out) == -1
        assert lib.mf_conv2d_gemm_f32(1, 1, None, 1, C.byref(bad), None) == -1 and b"conv2d_gemm" in lib.mf_last_error()
    reserved = desc()
    reserved.reserved = 1
    assert lib.mf_conv2d_gemm_out_dims(C.byref(reserved), out) == -1
    assert lib.mf_conv2d_gemm_out_dims(None, out) == -1 and lib.mf_conv2d_gemm_out_dims(C.byref(desc()), None) == -1 and lib.mf_conv2d_gemm_plan(C.byref(desc()), None) == -1
    assert lib.mf_conv2d_gemm_f32(None, 1, None, 1, C.byref(desc()), None) == -1 and lib.mf_conv2d_gemm_f32(1, None, None, 1, C.byref(desc()), None) == -1
    assert lib.mf_conv2d_gemm_f32(1, 1, None, None, C.byref(desc()), None) == -1
    assert lib.mf_conv2d_gemm_f32(1, 1, None, 1, C.byref(desc(N=1 << 20, Hin=1 << 14, Win=1 << 14, Cin=1 << 10)), None) == -2                  # too large: unsupported
    # the planner: forced tiles are kept, workgroups = pixel tiles x channel tiles
    for tile, (tm, tn) in ((1, (128, 128)), (2, (128, 64)), (3, (64, 64))):
        assert lib.mf_conv2d_gemm_plan(C.byref(desc(N=3, Hin=35, Win=35, Cin=64, Cout=192, tile=tile)), out) == 0
        assert tuple(out) == (tile, math.ceil(3 * 35 * 35 / tm) * math.ceil(192 / tn))
    assert lib.mf_conv2d_gemm_plan(C.byref(desc(N=100, Hin=147, Win=147, Cin=32, Cout=64)), out) == 0 and out[0] in (1, 2, 3)
    # pools, prepare, mean
    for args in ((None, 1, 1, 5, 5, 4, 1, 0, 0, 0, 0), (1, None, 1, 5, 5, 4, 1, 0, 0, 0, 0), (1, 1, 0, 5, 5, 4, 1, 0, 0, 0, 0), (1, 1, 1, 5, 5, 0, 1, 0, 0, 0, 0),
                 (1, 1, 1, 5, 5, 4, 3, 0, 0, 0, 0), (1, 1, 1, 5, 5, 4, 0, 0, 0, 0, 0), (1, 1, 1, 5, 5, 4, 1, 2, 0, 0, 0), (1, 1, 1, 5, 5, 4, 1, -1, 0, 0, 0),
                 (1, 1, 1, 5, 5, 4, 1, 0, 2, 0, 0), (1, 1, 1, 2, 5, 4, 1, 0, 0, 0, 0), (1, 1, 1, 5, 5, 4, 1, 0, 0, 3, 0), (1, 1, 1, 5, 5, 4, 1, 0, 0, 8, 5), (1, 1, 1, 5, 5, 4, 1, 0, 0, 0, 1)):
        assert lib.mf_pool2d_nhwc_f32(*args, None) == -1 and b"pool2d" in lib.mf_last_error(), args
    for args in ((None, 1, 1, 3, 80, 80, 75), (1, None, 1, 3, 80, 80, 75), (1, 1, 0, 3, 80, 80, 75), (1, 1, 1, 2, 80, 80, 75), (1, 1, 1, 4, 80, 80, 75), (1, 1, 1, 3, 0, 80, 75),
                 (1, 1, 1, 3, 80, 16385, 75), (1, 1, 1, 3, 80, 80, 74), (1, 1, 1, 3, 80, 80, 4097)):
        assert lib.mf_inception_prepare_u8(*args, None) == -1 and b"inception_prepare" in lib.mf_last_error(), args
    for args in ((None, 1, 1, 4, 4), (1, None, 1, 4, 4), (1, 1, 0, 4, 4), (1, 1, 1, 0, 4), (1, 1, 1, 4, 0)):
        assert lib.mf_mean_pixels_f32(*args, None) == -1 and b"mean_pixels" in lib.mf_last_error(), args
    assert lib.mf_version() == 250


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    d = K.make_gemm_conv_desc(1, 4, 4, 4, 8, 3, 3, 1, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU"):
        K.conv2d_gemm(torch.zeros((1, 4, 4, 4)), torch.zeros((3, 3, 4, 8)), None, d)
    with pytest.raises(RuntimeError, match="w must have shape"):
        K.conv2d_gemm(torch.zeros((1, 4, 4, 4)), torch.zeros((8, 4, 3, 3)), None, d)
    with pytest.raises(RuntimeError, match="no CPU"):
        K.pool2d_nhwc(torch.zeros((1, 4, 4, 4)), 1, 1, L.POOL_MAX)
    with pytest.raises(RuntimeError, match="stride"):
        K.pool2d_nhwc(torch.zeros((1, 4, 4, 4)), 3, 1, L.POOL_MAX)
    with pytest.raises(RuntimeError, match="uint8"):
        K.inception_prepare(torch.zeros((1, 3, 80, 80)), 75)
    with pytest.raises(RuntimeError, match="no CPU"):
        K.mean_pixels(torch.zeros((1, 4, 4)))


def test_the_entry_points_are_declared_exported_bound_wrapped_and_documented():
    hdr = (ROOT / "include" / "medfusion_hip.h").read_text()
    md = (ROOT / "INTEGRATION.md").read_text()
    wrappers = (ROOT / "medfusion_amd" / "kernels.py").read_text()
    lib = L.load()
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr) and hasattr(lib, name) and name in L.exported_symbols() and name in md and f".{name}(" in wrappers, name
    assert C.sizeof(L.MfGemmConvDesc) == 16 * 4 and "#define MF_VERSION 250" in hdr
    from medfusion_amd import build as B
    assert "inception.hip" in B.SOURCES and "-packed-fp32-ops" in B.EXTRA_CFLAGS["inception.hip"]
    assert "cnn_layers.hip" in B.SOURCES and "-packed-fp32-ops" in B.EXTRA_CFLAGS["cnn_layers.hip"]
    assert (L.POOL_MAX, L.POOL_AVG_VALID, L.INCEPTION_MIN_SIZE) == tuple(int(re.search(rf"#define {n} (\d+)", hdr).group(1)) for n in ("MF_POOL_MAX", "MF_POOL_AVG_VALID", "MF_INCEPTION_MIN_SIZE"))


# ------------------------------------------------------------------------------------------------ 3. the plan
def test_plan_totals():
    p = I.plan(100)
    convs = [r for r in p["layers"] if r["op"] == "conv"]
    pools = [r for r in p["layers"] if r["op"] == "pool"]
    assert len(convs) == 94 and len(pools) == 2 + 3 + 1 + 4 + 1 + 2 and p["conv_launches"] == 95 and p["launches"] == 1 + 94 + 13 + 1 + 1
    assert p["flops"] == sum(r["flops"] for r in p["layers"] if "flops" in r) and p["workgroups"] == sum(r["workgroups"] for r in p["layers"] if "workgroups" in r)
    # 5.7 G multiply-adds per image at 299: the published cost of Inception-v3
    assert 11.3e9 < p["flops"] / 100 < 11.6e9
    first = convs[0]
    assert first["flops"] == 2 * 100 * 149 * 149 * 32 * 27 and first["out"] == (149, 149, 32) and first["into"] == ("c1a", 0)
    assert [r["into"] for r in convs if r["key"].startswith("Mixed_7c.") and r["into"][0] == "Mixed_7c"] == [("Mixed_7c", o) for o in (0, 320, 704, 1088, 1472, 1856)]
    assert p["largest_activation_bytes"] == 100 * 147 * 147 * 64 * 4 and I.default_chunk(299) == (512 << 20) // (147 * 147 * 64 * 4)
    assert p["weight_bytes"] == 4 * (sum(cin * cout * kh * kw + cout for _, cin, cout, kh, kw, *_ in I.LAYERS) + 2048 * 1008 + 1008)
    small = I.plan(3, 75)
    assert small["launches"] == p["launches"] and small["flops"] < p["flops"] and all(r["tile"] in (1, 2, 3) for r in small["layers"] if "tile" in r)
    for op, r in zip([o for o in I.OPS if o[0] == "conv"], convs):                                  # every slice lies inside its buffer, and the slices of a concat tile it
        assert r["into"][1] + r["cout"] <= I.WIDTH[op[3]]
    for block in I.BLOCKS:
        spans = sorted((o[4], o[4] + I.LAYERS[o[1]][2]) for o in I.OPS if o[0] == "conv" and o[3] == block)
        spans += [(o[6], o[6] + I.WIDTH[o[1]]) for o in I.OPS if o[0] == "pool" and o[2] == block]
        spans.sort()
        assert spans[0][0] == 0 and spans[-1][1] == I.WIDTH[block] and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), block


# ------------------------------------------------------------------------------------------------ 4. the Inception Score and the average pool
def test_inception_score_against_a_hand_computed_case():
    p = torch.tensor([[0.75, 0.25], [0.25, 0.75]], dtype=torch.float64)
    want = math.exp(0.75 * math.log(1.5) + 0.25 * math.log(0.5))             # both rows: KL(p || (1/2, 1/2))
    got = M.inception_score(p.log().float() + 3.0)                            # softmax ignores the shift
    assert abs(got["inception_score_mean"] - want) < 1e-6 and got["inception_score_std"] == 0.0
    assert abs(M.inception_score(torch.zeros((5, 7)))["inception_score_mean"] - 1.0) < 1e-12       # uniform predictions: exactly 1
    onehot = torch.eye(4) * 100.0
    assert abs(M.inception_score(onehot)["inception_score_mean"] - 4.0) < 1e-9                     # confident and diverse: the number of classes
    halves = M.inception_score(torch.cat([onehot, torch.zeros((4, 4))]), splits=2)
    assert abs(halves["inception_score_mean"] - 2.5) < 1e-9 and abs(halves["inception_score_std"] - 1.5) < 1e-9


def test_average_pool_of_the_restatement_against_torch():
    """avg = the fp32 sum of the valid taps in ascending (kh, kw) order / their number.  Against F.avg_pool2d(count_include_pad=False) on the CPU the
    values agree to 2 ulp everywhere; recorded: the BITS agree on these inputs with this torch build (ATen sums the window in the same order and
    divides once).  The definition governs either way -- the device kernel is held to the restatement, not to ATen."""
    g = torch.Generator().manual_seed(2)
    agree = True
    for shape in ((2, 5, 8, 8), (1, 3, 17, 17), (2, 4, 3, 3)):
        x = torch.randn(shape, generator=g)
        mine = IC.pool_ref(x, 1, 1, L.POOL_AVG_VALID)
        aten = F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)
        assert mine.shape == aten.shape and bool(((mine - aten).abs() <= 2 * 2.0 ** -23 * F.avg_pool2d(x.abs(), 3, 1, 1, count_include_pad=False)).all())
        agree = agree and torch.equal(mine, aten)
        assert torch.equal(IC.pool_ref(x, 1, 1, L.POOL_MAX), F.max_pool2d(x, 3, 1, 1)) and torch.equal(IC.pool_ref(x, 2, 0, L.POOL_MAX), F.max_pool2d(x, 3, 2))
    print(f"[measured] average pool restatement == F.avg_pool2d(count_include_pad=False) bit for bit: {agree}")
    x64 = torch.randn((1, 2, 6, 6), generator=g, dtype=torch.float64)
    assert torch.allclose(IC.pool_ref(x64, 1, 1, L.POOL_AVG_VALID), F.avg_pool2d(x64, 3, 1, 1, count_include_pad=False), rtol=1e-14, atol=0)


def test_the_single_fma_of_the_oracle_on_a_double_rounding_case():
    """a = 1 + 2^-10, b = 2^-24 (1 - 2^-10 + 2^-20), c = 1: a b = 2^-24 + 2^-54, so a b + c lies just above the fp32 tie 1 + 2^-24 and the fma is
    1 + 2^-23; fp64 rounds the sum to the tie itself and the second rounding, to fp32, takes it to the even neighbour 1.0"""
    a, b, c = np.float32(1 + 2.0 ** -10), np.float32(2.0 ** -24 * (1 - 2.0 ** -10 + 2.0 ** -20)), np.float32(1.0)
    assert float(a) == 1 + 2.0 ** -10 and float(b) == 2.0 ** -24 * (1 - 2.0 ** -10 + 2.0 ** -20)               # both are fp32 values
    for sign in (1.0, -1.0):
        x, z = np.array([sign * a], dtype=np.float32), np.array([sign * c], dtype=np.float32)
        assert float(IC.fma32(x, np.array([b]), z)[0]) == sign * (1 + 2.0 ** -23)
        assert float(np.float32(np.float64(x[0]) * np.float64(b) + np.float64(z[0]))) == sign * 1.0
    exact = np.array([1.5, -2.0, 0.0], dtype=np.float32)                                                       # no rounding at all: the plain value
    assert IC.fma32(exact, exact, exact).tolist() == [3.75, 2.0, 0.0]


def test_the_exact_convolution_oracle_sits_inside_the_fp64_bound():
    """fma_chain_conv against fp64 F.conv2d on every CONV_SHAPES case: |y - y64| <= (K + 2) 2^-24 sum |w||x|, the bound the device is held to"""
    for case in IC.CONV_SHAPES:
        x, w, _, pads = IC.conv_case(case)
        got = IC.conv_oracle(case)
        x64, w64 = x.permute(0, 3, 1, 2).double(), w.permute(3, 2, 0, 1).double()
        y64 = F.conv2d(x64, w64, None, stride=case[3], padding=pads).permute(0, 2, 3, 1)
        mag = F.conv2d(x64.abs(), w64.abs(), None, stride=case[3], padding=pads).permute(0, 2, 3, 1)
        kk = case[0] * case[2][0] * case[2][1]
        assert got.dtype == torch.float32 and got.shape == y64.shape
        assert float(((got.double() - y64).abs() / ((kk + 2) * 2.0 ** -24 * mag)).max()) <= 1.0, case


def test_prepare_restatement_is_the_identity_at_the_networks_size():
    x = IC.images(2, 3, 75, 75, seed=1)
    assert torch.equal(IC.prepare_ref(x, 75), ((x.float() - 128.0) / 128.0).permute(0, 2, 3, 1))
    grey = IC.images(1, 1, 60, 90, seed=2)
    out = IC.prepare_ref(grey, 75)
    assert out.shape == (1, 75, 75, 3) and torch.equal(out[..., 0], out[..., 1]) and torch.equal(out[..., 0], out[..., 2]) and float(out.min()) >= -1 and float(out.max()) < 1
    assert torch.equal(out[0, 0, 0], ((grey[0, 0, 0, 0].float() - 128.0) / 128.0).expand(3))          # no half-pixel offset: output (0, 0) is input (0, 0)


# ------------------------------------------------------------------------------------------------ 5. the scripts
def test_evaluate_images_argument_rules(tmp_path):
    ev = _script("evaluate_images")
    a = ev.parse_args(["--real", "real.pt", "--fake", "fake.npy"])
    assert a.inception_score is None and a.features is None
    assert ev.parse_inception("inception:w.pth") == ("w.pth", "2048") and ev.parse_inception("inception:dir/w.pth:768") == ("dir/w.pth", "768")
    (tmp_path / "imgs").mkdir()
    folder = str(tmp_path / "imgs")
    a = ev.parse_args(["--real", folder, "--fake", folder, "--features", "inception:w.pth:logits_unbiased", "--inception-score"])
    assert a.inception_score == 1 and a.features == "inception:w.pth:logits_unbiased"
    assert ev.parse_args(["--real", folder, "--fake", folder, "--features", "inception:w.pth", "--inception-score", "10"]).inception_score == 10
    for bad in (["--real", folder, "--fake", folder, "--features", "inception:"], ["--real", folder, "--fake", folder, "--features", "inception:w.pth:pool3"],
                ["--real", folder, "--fake", folder, "--features", "inception:w.pth:2048:x"], ["--real", folder, "--fake", folder, "--features", "inception:w.pth", "--inception-score", "0"],
                ["--real", folder, "--fake", folder, "--features", "embedder:x.ckpt", "--inception-score"], ["--real", "a.pt", "--fake", "b.pt", "--inception-score"],
                ["--real", folder, "--fake", "b.pt", "--features", "inception:w.pth", "--inception-score"], ["--real", folder, "--fake", folder, "--features", "inception"]):
        with pytest.raises(SystemExit):
            ev.parse_args(bad)


def test_evaluate_images_output_is_unchanged_without_the_new_options(tmp_path, monkeypatch, capsys):
    """the log and the JSON of a call on feature files, with the device figures stubbed: the lines and keys of the script before the Inception options"""
    ev = _script("evaluate_images")
    feats = torch.randn((6, 4), generator=torch.Generator().manual_seed(0))
    torch.save(feats, tmp_path / "r.pt")
    torch.save(feats[:5] + 1, tmp_path / "f.pt")
    cpu = torch.device("cpu")
    monkeypatch.setattr(torch, "device", lambda *a, **k: cpu)
    monkeypatch.setattr(M, "precision_recall", lambda real, fake, knn: {"precision": 0.5, "recall": 0.25, "n_real": real.shape[0], "n_fake": fake.shape[0], "knn": knn})
    monkeypatch.setattr(M, "frechet_distance", lambda real, fake: 1.5)
    res = ev.main(["--real", str(tmp_path / "r.pt"), "--fake", str(tmp_path / "f.pt"), "--out", str(tmp_path / "out")])
    monkeypatch.undo()
    log = next((tmp_path / "out").glob("metrics_*.log")).read_text().splitlines()
    assert log == ["Samples Real: 6", "Samples Fake: 5", "Inception features: not built (needs downloaded weights); pass precomputed feature files",
                   "FD (features: precomputed feature files, D = 4): 1.5", "Precision: 0.5, Recall 0.25 "]
    saved = json.loads(next((tmp_path / "out").glob("metrics_*.json")).read_text())
    assert saved == res and list(saved) == ["precision", "recall", "n_real", "n_fake", "knn", "fd", "real", "fake", "features", "feature_width", "inception"]
    assert saved["inception"] is None and saved["features"] is None and saved["feature_width"] == 4
    import logging
    for h in list(logging.getLogger("evaluate_images").handlers):
        logging.getLogger("evaluate_images").removeHandler(h)
        h.close()


def test_inception_bench_plans_without_a_device(capsys):
    ib = _script("inception_bench")
    assert ib.main(["--plan", "--batch", "100"]) == 0
    out = capsys.readouterr().out
    assert "launches" in out and "mf_conv2d_gemm_f32" in out and "TFLOP" not in out.split("plan")[0]
    row = json.loads(out.strip().splitlines()[-1])
    assert row["launches"] == 110 and row["conv_launches"] == 95 and row["batch"] == 100 and row["size"] == 299
