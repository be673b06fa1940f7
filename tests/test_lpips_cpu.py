"""LPIPS without a device: the restatement, the seeded nets, the loader, the argument rules, plan() and the C-ABI's refusals."""
import ctypes as C
import importlib.util
from pathlib import Path

import pytest
import torch

import medfusion_amd as M
from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from medfusion_amd import lpips as LP
from tests import lpips_cases as LC

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("net", LC.NETS)
def test_restatement_is_zero_on_identical_images(net):
    x, _ = LC.make_pair((2, 3, 35, 31), 5)
    for dtype in (torch.float64, torch.float32):
        assert torch.equal(LC.ref_terms(LC.seeded(net, 2, 0.05), x, x.clone(), dtype), torch.zeros(2, 5, dtype=dtype))


@pytest.mark.parametrize("net", LC.NETS)
def test_every_term_of_every_case_is_alive(net):
    """a dead layer (all-zero features) would make its term 0 and hide behind any relative bound"""
    smallest = min(float(t64.min()) for *_, t64, _ in LC.whole_cases(net))
    print(f"[measured] {net}: smallest fp64 term {smallest:.3e}; fp32-vs-fp64 bounds per layer {[f'{v:.2e}' for v in LC.whole_bounds(net).tolist()]}")
    assert smallest > 1e-6
    assert all(0 < v < 1e-4 for v in LC.whole_bounds(net).tolist())


def test_seeded_is_one_generator_in_fp64():
    a, b = LP.LPIPSNet.seeded("alex", 3, 0.05), LP.LPIPSNet.seeded("alex", 3, 0.05)
    assert all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(a.convs, b.convs)) and all(torch.equal(p, q) for p, q in zip(a.lins, b.lins))
    g = torch.Generator().manual_seed(3)
    w = (torch.randn((64, 3, 11, 11), generator=g, dtype=torch.float64) * (2.0 / 363) ** 0.5).float()
    assert torch.equal(a.convs[0][0], w) and a.convs[0][0].dtype == torch.float32
    z = LP.LPIPSNet.seeded("vgg", 1)
    assert len(z.convs) == 13 and all(float(bb.abs().max()) == 0 for _, bb in z.convs)
    assert [v.numel() for v in z.lins] == [64, 128, 256, 512, 512] and all(0 <= float(v.min()) and float(v.max()) < 8.0 / v.numel() for v in z.lins)
    std = float(z.convs[5][0].std())
    assert abs(std / (2.0 / (256 * 9)) ** 0.5 - 1) < 0.02


@pytest.mark.parametrize("net", LC.NETS)
def test_loader_round_trip(net, tmp_path):
    src = LC.seeded(net, 2, 0.05)
    trunk, lin = src.state_dicts()
    want = {"vgg": [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28], "alex": [0, 3, 6, 8, 10]}[net]
    assert sorted(trunk) == sorted(f"features.{i}.{n}" for i in want for n in ("weight", "bias"))
    assert sorted(lin) == [f"lin{l}.model.1.weight" for l in range(5)] and all(v.shape == (1, v.numel(), 1, 1) for v in lin.values())
    trunk = dict(trunk, **{"classifier.1.weight": torch.zeros(3, 3), "classifier.1.bias": torch.zeros(3)})
    torch.save(trunk, tmp_path / "trunk.pth")
    torch.save(lin, tmp_path / "lin.pth")
    got = LP.LPIPSNet.from_files(tmp_path / "trunk.pth", tmp_path / "lin.pth", net)
    assert got.net == net and got.arithmetic == "split3" and len(got.convs) == len(src.convs)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got.convs, src.convs))
    assert all(torch.equal(a, b) for a, b in zip(got.lins, src.lins))
    assert LP.LPIPSNet.from_files(tmp_path / "trunk.pth", tmp_path / "lin.pth", net, arithmetic="fp32").arithmetic == "fp32"


def test_loader_errors_name_the_key():
    trunk, lin = LC.seeded("alex", 1).state_dicts()
    missing = {k: v for k, v in trunk.items() if k != "features.6.bias"}
    with pytest.raises(ValueError, match=r"features\.6\.bias"):
        LP.LPIPSNet.from_state(missing, lin, "alex")
    with pytest.raises(ValueError, match=r"features\.3\.weight"):
        LP.LPIPSNet.from_state(dict(trunk, **{"features.3.weight": torch.zeros(192, 64, 3, 3)}), lin, "alex")
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight"):
        LP.LPIPSNet.from_state(trunk, {k: v for k, v in lin.items() if not k.startswith("lin2")}, "alex")
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight"):
        LP.LPIPSNet.from_state(trunk, dict(lin, **{"lin4.model.1.weight": torch.zeros(256)}), "alex")
    with pytest.raises(ValueError, match=r"features\.0\.weight"):          # a VGG file given as AlexNet's
        LP.LPIPSNet.from_state(LC.seeded("vgg", 1).state_dicts()[0], lin, "alex")
    with pytest.raises(ValueError, match="net"):
        LP.LPIPSNet.from_state(trunk, lin, "squeeze")
    with pytest.raises(ValueError, match="arithmetic"):
        LP.LPIPSNet.from_state(trunk, lin, "alex", arithmetic="f16x2")


def test_minimum_sides_and_argument_errors():
    """every refusal the code reaches before it touches the device (CPU tensors get as far as the device rule, which comes last)"""
    net = LC.seeded("alex", 1)
    assert LP.MIN_SIDE == {"vgg": 16, "alex": 31} and L.load().mf_lpips_min_side(L.LPIPS_VGG) == 16 and L.load().mf_lpips_min_side(L.LPIPS_ALEX) == 31
    ok = torch.zeros(2, 3, 31, 40)
    for name, bad, args in (("net", ValueError, (ok, ok, "alex")), ("x", ValueError, ([1.0], ok, net)), ("x", ValueError, (torch.zeros(3, 31, 40), torch.zeros(3, 31, 40), net)),
                            ("x: fp32", ValueError, (ok.double(), ok.double(), net)), ("y: fp32", ValueError, (ok, ok.double(), net)),
                            ("y: of the shape", ValueError, (ok, torch.zeros(2, 3, 31, 41), net)), ("x: 1 or 3 channels", ValueError, (torch.zeros(2, 2, 31, 40),) * 2 + (net,)),
                            ("sides of at least 31", ValueError, (torch.zeros(2, 3, 30, 40),) * 2 + (net,)), ("sides of at least 31", ValueError, (torch.zeros(1, 1, 4, 40, 30),) * 2 + (net,)),
                            ("sides of at least 16", ValueError, (torch.zeros(2, 3, 15, 40),) * 2 + (LC.seeded("vgg", 1),)),
                            ("x: on a ROCm device", ValueError, (ok, ok, net))):
        with pytest.raises(bad, match=name):
            LP.lpips(*args)
    for chunk in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="chunk"):
            LP.lpips(ok, ok, net, chunk=chunk)
    with pytest.raises(ValueError, match="lpips"):
        M.ReconstructionMeter(lambda t: (t, None), lpips="alex")
    with pytest.raises(ValueError, match="lpips"):
        M.VolumeReconstructionMeter(lambda t: (t, None), lpips=object())
    assert M.ReconstructionMeter(lambda t: (t, None)).lpips is None
    with pytest.raises(RuntimeError, match="ROCm"):                       # the wrappers have no CPU path
        K.lpips_layer(torch.zeros(1, 4, 8), torch.zeros(1, 4, 8), torch.zeros(8))
    with pytest.raises(RuntimeError, match="ROCm"):
        K.relu_(torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU"):
        net.to("cpu")


def test_plan_totals():
    v = LP.plan("vgg", 256, 256)
    assert v["taps"] == [(256, 256, 64), (128, 128, 128), (64, 64, 256), (32, 32, 512), (16, 16, 512)]
    convs = [l for l in v["layers"] if l["op"] == "conv"]
    assert [l["kernel"] for l in convs] == ["mf_conv2d_direct_f32"] + ["mf_conv2d_f32"] * 12
    assert [l["splitk"] for l in convs] == [1, 2, 2, 3, 3, 5, 5, 5, 9, 9, 9, 9, 9]     # chains of at most 16 chunks of 32: ceil(9 Cin / 32 / 16)
    # prepare + direct + 12 x (implicit GEMM + split-K reduction + ReLU) + 4 pools + 5 x (distance + finish)
    assert v["launches"] == 1 + 1 + 36 + 4 + 10
    assert v["workspace_bytes"] == 8 * 1024 and v["activation_bytes"] == 2 * 256 * 256 * 64 * 4
    a = LP.plan("alex", 256, 256, arithmetic="fp32")
    assert a["taps"] == [(63, 63, 64), (31, 31, 192), (15, 15, 384), (15, 15, 256), (15, 15, 256)]
    assert [l["kernel"] for l in a["layers"] if l["op"] == "conv"] == ["mf_conv2d_direct_f32"] * 2 + ["mf_conv2d_f32"] * 3
    assert [l["splitk"] for l in a["layers"] if l["op"] == "conv"] == [1, 1, 4, 7, 5]
    assert a["launches"] == 1 + 2 + 6 + 3 + 2 + 10
    assert LP.plan("vgg", 16, 16)["taps"][-1] == (1, 1, 512) and LP.plan("alex", 31, 31)["taps"] == [(7, 7, 64), (3, 3, 192), (1, 1, 384), (1, 1, 256), (1, 1, 256)]
    assert LP.plan("vgg", 35, 31)["taps"] == [(35, 31, 64), (17, 15, 128), (8, 7, 256), (4, 3, 512), (2, 1, 512)]
    for bad in (("vgg", 15, 16), ("alex", 31, 30), ("squeeze", 64, 64), ("vgg", 16.0, 16)):
        with pytest.raises(ValueError):
            LP.plan(*bad)


def test_entry_points_validate_before_any_launch():
    """null pointers, sides below the minimum, C not 1 or 3, a (k, s) pair other than the two -> MF_EINVAL; a workspace too small -> MF_EWORKSPACE"""
    lib = L.load()
    p = 4096    # a stand-in address: every call below is refused before it is read
    assert lib.mf_lpips_prepare_f32(None, p, p, 1, 3, 32, 32, 0, 0, None) == -1 and b"lpips_prepare" in lib.mf_last_error()
    assert lib.mf_lpips_prepare_f32(p, p, p, 1, 2, 32, 32, 0, 0, None) == -1 and b"1 or 3" in lib.mf_last_error()
    assert lib.mf_lpips_prepare_f32(p, p, p, 1, 3, 15, 32, 0, 0, None) == -1 and lib.mf_lpips_prepare_f32(p, p, p, 1, 3, 32, 30, 0, 1, None) == -1
    assert lib.mf_lpips_prepare_f32(p, p, p, 1, 3, 32, 32, 0, 2, None) == -1 and lib.mf_lpips_prepare_f32(p, p, p, 0, 3, 32, 32, 0, 0, None) == -1
    d = K.make_direct_conv_desc(1, 35, 31, 3, 64, 11, 11, 4, 2)
    assert K.direct_conv_out_hw(d) == (8, 7)
    assert lib.mf_conv2d_direct_f32(None, p, None, p, C.byref(d), None) == -1 and lib.mf_conv2d_direct_f32(p, p, None, p, None, None) == -1
    for bad in (K.make_direct_conv_desc(1, 35, 31, 3, 64, 12, 11, 4, 2), K.make_direct_conv_desc(1, 35, 31, 3, 64, 3, 3, 5, 1), K.make_direct_conv_desc(1, 35, 31, 3, 64, 3, 3, 0, 1),
                K.make_direct_conv_desc(1, 2, 2, 3, 64, 5, 5, 1, 0), K.make_direct_conv_desc(1, 8, 8, 0, 64, 3, 3, 1, 1), K.make_direct_conv_desc(1, 8, 8, 3, 4, 3, 3, 1, -1)):
        assert lib.mf_conv2d_direct_f32(p, p, None, p, C.byref(bad), None) == -1 and b"conv2d_direct" in lib.mf_last_error()
    assert lib.mf_relu_f32(None, 8, None) == -1 and lib.mf_relu_f32(p, 0, None) == -1
    assert lib.mf_maxpool_nhwc_f32(p, p, 1, 8, 8, 4, 2, 1, None) == -1 and lib.mf_maxpool_nhwc_f32(p, p, 1, 8, 8, 4, 3, 3, None) == -1
    assert lib.mf_maxpool_nhwc_f32(p, p, 1, 2, 8, 4, 3, 2, None) == -1 and lib.mf_maxpool_nhwc_f32(None, p, 1, 8, 8, 4, 2, 2, None) == -1
    assert lib.mf_lpips_layer_parts(1) == 1 and lib.mf_lpips_layer_parts(65) == 2 and lib.mf_lpips_layer_parts(1 << 20) == 1024 and lib.mf_lpips_layer_parts(0) == 0
    assert lib.mf_lpips_workspace_bytes(3, 1023) == 3 * 16 * 8 and lib.mf_lpips_workspace_bytes(0, 4) == 0
    assert lib.mf_lpips_layer_f32(p, p, p, p, 3 * 16 * 8 - 1, 3, 1023, 64, None) == -4 and b"workspace" in lib.mf_last_error()
    assert lib.mf_lpips_layer_f32(p, None, p, p, 1 << 20, 3, 1023, 64, None) == -1 and lib.mf_lpips_layer_f32(p, p, p, p, 1 << 20, 3, 1023, 0, None) == -1
    assert lib.mf_lpips_layer_f32(p, p, p, p + 4, 1 << 20, 3, 1023, 64, None) == -1
    assert lib.mf_lpips_finish_f32(p, p, None, 3, 1023, 5, 5, None) == -1 and lib.mf_lpips_finish_f32(None, p, None, 3, 1023, 0, 5, None) == -1
    assert C.sizeof(L.MfDirectConvDesc) == 12 * 4


def test_struct_layout_matches_what_a_c_compiler_sees(tmp_path):
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "medfusion_hip.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(MfDirectConvDesc));']
    lines += [f'  printf("{n} %zu\\n", offsetof(MfDirectConvDesc, {n}));' for n, _ in L.MfDirectConvDesc._fields_] + ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(L.MfDirectConvDesc)
    assert all(int(got[n]) == getattr(L.MfDirectConvDesc, n).offset for n, _ in L.MfDirectConvDesc._fields_)


def _script(name):
    spec = importlib.util.spec_from_file_location(f"_lpips_script_{name}", ROOT / "scripts" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_scripts_take_the_three_flags_together(tmp_path, capsys):
    trunk, lin = LC.seeded("alex", 1).state_dicts()
    torch.save(trunk, tmp_path / "t.pth")
    torch.save(lin, tmp_path / "l.pth")
    ev, vol = _script("evaluate_latent_embedder"), _script("evaluate_volumes")
    assert ev.parse_args(["--synthetic", "--images", "x"]).lpips is None
    a = ev.parse_args(["--synthetic", "--images", "x", "--lpips-net", "alex", "--lpips-trunk", str(tmp_path / "t.pth"), "--lpips-lin", str(tmp_path / "l.pth")])
    assert isinstance(a.lpips, LP.LPIPSNet) and a.lpips.net == "alex"
    v = vol.parse_args(["--checkpoint", "c", "--volumes", "x", "--lpips-net", "alex", "--lpips-trunk", str(tmp_path / "t.pth"), "--lpips-lin", str(tmp_path / "l.pth")])
    assert isinstance(v.lpips, LP.LPIPSNet)
    for mod, head in ((ev, ["--synthetic", "--images", "x"]), (vol, ["--checkpoint", "c", "--volumes", "x"])):
        for bad in (["--lpips-net", "alex"], ["--lpips-trunk", str(tmp_path / "t.pth"), "--lpips-lin", str(tmp_path / "l.pth")], ["--lpips-net", "squeeze"]):
            with pytest.raises(SystemExit):
                mod.parse_args(head + bad)
    with pytest.raises(SystemExit):
        vol.parse_args(["--volumes", "x", "--pairs", "3", "--lpips-net", "alex", "--lpips-trunk", str(tmp_path / "t.pth"), "--lpips-lin", str(tmp_path / "l.pth")])
    capsys.readouterr()
    bench = _script("lpips_bench")
    rows = bench.plan_rows()
    assert any("vgg" in r and "52 launches" in r for r in rows) and any("alex" in r and "24 launches" in r for r in rows)
