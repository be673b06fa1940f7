"""spatial_dims=3 without a GPU: the 3-D constructors reproduce the reference's state-dict layout (tests/golden/d3_keys.json), the options that
are not built raise NotImplementedError naming them, a 3-D pipeline checkpoint loads through the shape inference, the 3-D descriptor's layout
and host-side validation, and the fixtures load."""

import ctypes as C
import json
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import medfusion_amd as M
from medfusion_amd import blocks as BLK
from medfusion_amd import blocks3d as B3
from medfusion_amd import kernels as K
from medfusion_amd import lib as L
from oracle import restate as R
from oracle import synth as S
from tests.d3_cases import BLOCK_CASES, SAMPLE_CASES, UNET_CASES, VAE_CASE, block_kwargs, unet_kwargs
from tests.test_vq_cpu import _fake_reference
from tests.util import GOLD, gold, to_product_kwargs

ROOT = GOLD.parents[1]
KEYS = json.loads((GOLD / "d3_keys.json").read_text())


def _layout(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


@pytest.mark.parametrize("name", sorted(BLOCK_CASES))
def test_block_layout_is_the_references(name):
    cls, kw, _, _ = BLOCK_CASES[name]
    assert _layout(getattr(B3, cls)(**block_kwargs(cls, kw))) == KEYS[name]


@pytest.mark.parametrize("name", sorted(UNET_CASES))
def test_unet_layout_is_the_references(name):
    m = M.UNet(**to_product_kwargs(unet_kwargs(UNET_CASES[name][0])))
    assert _layout(m) == KEYS[name]
    assert m.in_conv.conv.weight.dim() == 5


def test_vae_layout_is_the_references():
    m = M.VAE(**VAE_CASE)
    assert _layout(m) == KEYS["vae"]
    assert m.scale3 == (8, 8, 8)


@pytest.mark.parametrize("make,option", [
    (lambda: M.UNet(**to_product_kwargs(unet_kwargs([1, 2, 2, 2]) | {"use_attention": "linear"})), "use_attention"),
    (lambda: M.UNet(**to_product_kwargs(unet_kwargs([1, 2, 2, 2]) | {"use_attention": ["none", "none", "spatial", "none"]})), "use_attention"),
    (lambda: M.UNet(**to_product_kwargs(unet_kwargs([1, 2, 2, 2]) | {"use_self_conditioning": True})), "use_self_conditioning"),
    (lambda: M.UNet(**to_product_kwargs(unet_kwargs([1, 2, 2, 2]) | {"estimate_variance": True})), "estimate_variance"),
    (lambda: M.UNet(**to_product_kwargs(unet_kwargs([1, 2, 2, 2]) | {"kernel_sizes": [3, 5, 3, 3]})), "kernel_size"),
    (lambda: M.UNet(**to_product_kwargs(unet_kwargs([1, 2, 2, 2]) | {"spatial_dims": 1})), "spatial_dims"),
    (lambda: M.VAE(**(VAE_CASE | {"use_attention": "linear"})), "use_attention"),
    (lambda: M.VAE(**(VAE_CASE | {"kernel_sizes": [3, 3, 2, 3]})), "kernel_size"),
    (lambda: M.VQVAE(spatial_dims=3), "spatial_dims"),
    (lambda: M.VQGAN(spatial_dims=3), "spatial_dims"),
    (lambda: M.VAEGAN(spatial_dims=3), "spatial_dims"),
    (lambda: B3.BasicUp(3, 32, 8, 2, 2, use_res=True), "use_res"),
    (lambda: B3.BasicDown(3, 32, 128, 3, 2, use_res=True), "use_res"),
    (lambda: B3.BasicUp(3, 32, 32, 2, 2, learnable_interpolation=False), "learnable_interpolation"),
    (lambda: B3.BasicBlock(3, 32, 32, (3, 3, 1)), "kernel_size"),
])
def test_options_that_are_not_built_raise(make, option):
    with pytest.raises(NotImplementedError, match=option):
        make()


def test_other_arithmetic_raises_at_forward():
    blk = B3.BasicBlock(3, 32, 32, 3)
    x = B3.tag(torch.zeros(1, 4, 2, 32), (2, 2, 2))
    old = BLK.CONV_PRECISION
    try:
        for prec in (0, 1, 4, 6):
            BLK.CONV_PRECISION = prec
            with pytest.raises(NotImplementedError, match="MF_CONV_FP32_F16X2"):
                blk(x)
    finally:
        BLK.CONV_PRECISION = old


def test_padding_per_axis_is_monai_get_padding():
    assert B3.monai_padding3(3, (1, 2, 2)) == (1, 1, 1)
    assert B3.monai_padding3((1, 2, 2), (1, 2, 2)) == (0, 0, 0)
    assert B3.monai_padding3(1, 1) == (0, 0, 0)
    assert B3.monai_padding3(3, 2) == (1, 1, 1)


def test_descriptor_layout_matches_what_a_c_compiler_sees(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "medfusion_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(MfConv3dDesc));']
    for fname, _ in L.MfConv3dDesc._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(MfConv3dDesc, {fname}));')
    lines += ['  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(tmp_path / "l.c"), "-o", str(tmp_path / "l")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(L.MfConv3dDesc) == 20 * 4
    for fname, _ in L.MfConv3dDesc._fields_:
        assert int(got[fname]) == getattr(L.MfConv3dDesc, fname).offset, fname


def test_host_validation_and_planning_without_gpu():
    lib = L.load()
    d = K.make_conv3d_desc(2, 5, 7, 9, 32, 0, 16, 3, (1, 2, 2), (1, 1, 1))
    assert K.conv3d_ok(d) and K.conv3d_out_dims(d) == (5, 4, 5)
    t, s = K.conv3d_plan(d)
    assert 1 <= t <= 4 and s in (1, 2, 4, 8, 16)
    assert K.conv3d_out_dims(K.make_conv3d_desc(2, 3, 4, 5, 32, 0, 16, 3, 1, 1, (0, 1, 1))) == (3, 8, 10)
    for bad in (dict(C1=3), dict(C1=32, C2=16), dict(k=5), dict(precision=1), dict(stride=(3, 1, 1)), dict(upsample=(2, 0, 0)), dict(Cout=0),
                dict(tile_hint=5), dict(splitk_hint=17)):
        a = dict(N=2, D=5, H=7, W=9, C1=32, C2=0, Cout=16, k=3, stride=(1, 1, 1), pad=(1, 1, 1), upsample=(0, 0, 0))
        a.update(bad)
        hints = {h: a.pop(h) for h in ("tile_hint", "splitk_hint", "precision") if h in a}
        dd = K.make_conv3d_desc(a["N"], a["D"], a["H"], a["W"], a["C1"], a["C2"], a["Cout"], a["k"], a["stride"], a["pad"], a["upsample"], **hints)
        assert not K.conv3d_ok(dd), bad
        rc = lib.mf_conv3d_f16x2(None, None, None, None, None, None, None, 1.0, None, 0, C.byref(dd), None)
        assert rc == -2 and b"unsupported" in lib.mf_last_error(), bad
    # split-K slabs: workspace sized by the host
    d = K.make_conv3d_desc(1, 2, 2, 2, 1024, 1024, 1024, 3, 1, 1, splitk_hint=4)
    assert lib.mf_conv3d_workspace_bytes(C.byref(d)) == 4 * 8 * 1024 * 4
    d = K.make_conv3d_desc(1, 2, 2, 2, 1024, 0, 1024, 3, 1, 1, splitk_hint=1)
    assert lib.mf_conv3d_workspace_bytes(C.byref(d)) == 0


def test_fixtures_load():
    g = gold("d3_blocks")
    for name in BLOCK_CASES:
        assert g[f"{name}.y"].dtype == np.float32 and g[f"{name}.y"].ndim == 5
    g = gold("d3_unet")
    for name, (_, shape) in UNET_CASES.items():
        assert g[f"{name}.y"].shape == shape
    g = gold("d3_vae")
    assert g["x_dec"].shape == (2, 1, 16, 32, 32) and g["z"].shape == (2, VAE_CASE["emb_channels"], 2, 4, 4)
    for name in SAMPLE_CASES:
        g = gold(name)
        assert g["image"].shape == (int(g["n"]), *g["size"])
    for p in GOLD.glob("d3_*"):
        assert p.stat().st_size < 400 * 1024, p


def _write_pipeline_3d(tmp_path, vae_kw, prefix):
    ukw = dict(unet_kwargs([1, 2, 2, 2], in_ch=vae_kw["emb_channels"]), cond_embedder=None, cond_embedder_kwargs={})
    emb = M.VAE(**vae_kw)
    S.synth_state_dict(emb, prefix + "vae.")
    src = M.DiffusionPipeline(M.GaussianNoiseScheduler, M.UNet, emb, R.published_scheduler_kwargs(), to_product_kwargs(ukw), clip_x0=False)
    S.synth_state_dict(src.noise_estimator, prefix + "unet.")
    names, mods, made = _fake_reference(["VAE"])
    hp = dict(noise_scheduler=made["GaussianNoiseScheduler"], noise_estimator=made["UNet"], latent_embedder=made["VAE"],
              noise_scheduler_kwargs=R.published_scheduler_kwargs(), noise_estimator_kwargs=dict(ukw, time_embedder=made["TimeEmbbeding"]),
              latent_embedder_checkpoint="gone/last_vae.ckpt", estimator_objective="x_T", clip_x0=False)
    sys.modules.update(mods)
    try:
        torch.save({"state_dict": src.state_dict(), "hyper_parameters": hp, "pytorch-lightning_version": "1.8.6"}, tmp_path / "last.ckpt")
    finally:
        for n in names:
            sys.modules.pop(n, None)
    return src


def test_3d_pipeline_checkpoint_loads_through_shape_inference(tmp_path):
    """the UNet takes spatial_dims=3 from the hyper-parameters; the VAE (its checkpoint gone) is rebuilt from the pipeline checkpoint's
    latent_embedder.* tensors, spatial_dims from the rank of its convolution weights"""
    src = _write_pipeline_3d(tmp_path, VAE_CASE, "d3ckpt.")
    pipe = M.DiffusionPipeline.load_from_checkpoint(tmp_path / "last.ckpt")
    assert pipe.noise_estimator.spatial_dims == 3 and pipe.latent_embedder.spatial_dims == 3
    got, want = pipe.state_dict(), src.state_dict()
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    from medfusion_amd.checkpoint import infer_vae_kwargs
    vsd = {k[len("latent_embedder."):]: v for k, v in src.state_dict().items() if k.startswith("latent_embedder.")}
    inf = infer_vae_kwargs(vsd, "VAE")
    assert inf["spatial_dims"] == 3 and inf["hid_chs"] == VAE_CASE["hid_chs"] and inf["in_channels"] == 1
    inf2 = infer_vae_kwargs({k: v for k, v in M.VAE(**R.tiny_vae_kwargs()).state_dict().items()}, "VAE")
    assert inf2["spatial_dims"] == 2
