"""Harness-level parity on a real MI355X and the BASELINE configs at their per-GPU sizes:
 * a checkpoint written by the REFERENCE's classes (tests/golden/ckpt/, oracle/gen_ckpt_fixture.py) loads and samples like the reference,
   with EMA and with live weights;
 * scripts/sample.py runs as a subprocess and its output is pinned against the oracle driven with the same Philox draws;
 * scripts/sample_dataset.py writes exactly the uint8 pixels of the reference's host formula, through the asynchronous egress;
 * cfg3 at its per-GPU workload (16 rows, 3 classes, guidance 8 = a 32-row CFG pair at 32x32), cfg4 as a captured hipGraph
   (100 iterations == eager bit for bit at B=8 / 32x32, 1000 iterations finish finite).
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import medfusion_amd as M
from medfusion_amd import published as P
from oracle import restate as R
from oracle import synth as S
from tests.test_oracle_cpu import build_oracle_pipe
from tests.util import T, ckpt_runs, gold, oracle_noise, relerr

ROOT = Path(__file__).resolve().parents[1]
TOL = 1e-4
GUIDED_HARNESS_TOL = 1e-4   # guidance 8 on the published widths, 6 iterations: measured on MI355X 7.1e-6 / 8.9e-6 (f16x2), 7.9e-6 / 8.6e-6 (split3), cfg3 rows 5.5e-6 / 7.0e-6 (the prints)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ckpt_dir(tmp_path_factory):
    return ckpt_runs(tmp_path_factory.mktemp("ckpt"))


@pytest.fixture(params=[5, 1], ids=["f16x2", "split3"], autouse=True)
def conv_precision(request):
    from medfusion_amd import blocks as BLK
    old = BLK.CONV_PRECISION
    BLK.CONV_PRECISION = request.param
    yield request.param
    BLK.CONV_PRECISION = old


@torch.no_grad()
def test_reference_written_checkpoint_samples_like_the_reference(dev, ckpt_dir):
    """rows f1 + E: DiffusionPipeline.load_from_checkpoint on the reference-written fixture (nested VAE checkpoint, use_ema=True in the
    hyper-parameters), then sample() against what the reference produced from the same file -- with the EMA weights
    (diffusion_pipeline.py:234-235) and with the live ones."""
    g = gold("ckpt_sample")
    pipe = M.DiffusionPipeline.load_from_checkpoint(ckpt_dir / "tiny_diffusion" / "last.ckpt").to(dev)
    assert pipe.use_ema
    cond = T(g["condition"]).to(dev)
    imgs = {}
    for tag, use_ema in (("ema", True), ("live", False)):
        pipe.use_ema = use_ema
        noise = oracle_noise(int(g["seed"]))
        imgs[tag] = pipe.sample(3, (8, 8, 8), steps=int(g["steps"]), use_ddim=True, condition=cond, guidance_scale=1.0, un_cond=None, noise=noise)
        assert noise.draw_index == int(g["draws"])
        assert relerr(imgs[tag], T(g[f"image_{tag}"])) < TOL, tag
    assert relerr(imgs["ema"], imgs["live"]) > 1e-2   # the two weight sets really differ


@torch.no_grad()
def test_default_noise_moves_on_between_calls(dev, ckpt_dir):
    """two sample() calls in a row differ, reseeding reproduces the first (like the reference's default generator)"""
    pipe = M.DiffusionPipeline.load_from_checkpoint(ckpt_dir / "tiny_diffusion" / "last.ckpt").to(dev)
    torch.manual_seed(0)
    a = pipe.sample(2, (8, 8, 8), steps=2, decode=False)
    b = pipe.sample(2, (8, 8, 8), steps=2, decode=False)
    torch.manual_seed(0)
    c = pipe.sample(2, (8, 8, 8), steps=2, decode=False)
    assert not torch.equal(a, b) and torch.equal(a, c)


def _run(cmd, **env):
    e = dict(os.environ, **{k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, *cmd], cwd=str(ROOT), env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@torch.no_grad()
def test_sample_script_is_pinned_against_the_oracle(dev, tmp_path, conv_precision):
    """row H: scripts/sample.py (the reference's flow: seed 0, conditions [0, 1, None], guidance 8, save_image) as a subprocess on the
    published architecture with seeded weights; its raw tensors must equal the oracle's, driven with the Philox key the script's
    `torch.manual_seed(0)` produces, and a second run must reproduce the first bit for bit."""
    out = tmp_path / "samples"
    _run(["scripts/sample.py", "--synthetic", "--steps", "3", "--n", "4", "--out", str(out)], MEDFUSION_CONV_PRECISION=conv_precision)
    raw = torch.load(out / "samples_raw.pt")
    assert sorted(raw) == ["0", "1", "None"] and all((out / f"test_{c}.png").exists() or (out / f"test_{c}.png.npy").exists() for c in (0, 1, None))
    torch.manual_seed(0)
    key = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())   # what PhiloxDeviceNoise.begin() draws after manual_seed(0)
    ora = build_oracle_pipe(R.published_unet_kwargs(2), R.published_vae_kwargs(8), "published")
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    for cond in (0, 1, None):
        ora.set_noise_fn(S.PhiloxNoise(key))
        c = torch.tensor([cond] * 4) if cond is not None else None
        want = ora.sample(4, (8, 32, 32), guidance_scale=8, condition=c, un_cond=None, steps=3, use_ddim=True)
        got = raw[str(cond)]
        assert got.shape == (4, 3, 256, 256)
        e = relerr(got, want)
        print(f"[measured] sample.py harness, condition {cond}: {e:.1e}")
        assert e < (GUIDED_HARNESS_TOL if cond is not None else TOL), cond   # guidance 8 (tests/test_parity_gpu.py has the measured values)
    stats = {k: (float(v.min()), float(v.max()), float(v.mean())) for k, v in raw.items()}
    out2 = tmp_path / "samples2"
    _run(["scripts/sample.py", "--synthetic", "--steps", "3", "--n", "4", "--out", str(out2)], MEDFUSION_CONV_PRECISION=conv_precision)
    raw2 = torch.load(out2 / "samples_raw.pt")
    assert all(torch.equal(raw[k], raw2[k]) for k in raw), stats


@torch.no_grad()
def test_bulk_generation_writes_the_reference_pixels(dev, tmp_path, conv_precision):
    """rows H (bulk) + f2: scripts/sample_dataset.py -- chunks of `sample_batch`, guidance 1, device clip -> uint8 -> channel-last,
    pinned buffers + asynchronous copy, writer thread.  The files must hold exactly the pixels of the reference's host formula
    (sample_dataset.py:44-53) applied to the same samples."""
    out = tmp_path / "gen"
    txt = _run(["scripts/sample_dataset.py", "--synthetic", "--steps-list", "2", "--labels", "No_Cardiomegaly:0,Cardiomegaly:1", "--n-samples", "5",
                "--sample-batch", "2", "--out", str(out), "--compare-no-egress"], MEDFUSION_CONV_PRECISION=conv_precision)
    st = json.loads(txt.strip().splitlines()[-1])["bulk_generation"]
    assert st["with_egress"]["images"] == 10 and st["images_left_on_device"]["images"] == 10
    pipe = P.build_published_pipeline(dev, num_classes=2)
    try:
        from PIL import Image
        load = lambda p: np.asarray(Image.open(p))
        ext = ""
    except ImportError:
        load = lambda p: np.load(str(p) + ".npy")
        ext = None
    for name, label in (("No_Cardiomegaly", 0), ("Cardiomegaly", 1)):
        torch.manual_seed(0)
        counter = 0
        for n in (2, 2, 1):   # 5 samples in chunks of 2
            cond = torch.tensor([label] * n, device=dev)
            res = pipe.sample(n, (8, 32, 32), guidance_scale=1, condition=cond, un_cond=1 - cond, steps=2).cpu().numpy()
            for image in res:
                image = image.clip(-1, 1)
                image = (image + 1) / 2 * 255
                image = np.moveaxis(image, 0, -1).astype(np.uint8)
                got = load(out.parent / f"{out.name}_2" / name / f"fake_{counter}.png")
                assert got.shape == image.shape and np.array_equal(got, image), (name, counter)
                counter += 1


@torch.no_grad()
def test_cfg3_at_the_per_gpu_workload(dev):
    """BASELINE configs[2] at the size ONE GPU sees: 16 rows, 3-class LabelEmbedder, guidance 8 => a 32-row classifier-free-guidance pair
    at latent 32x32.  Rows 0 and 1 against the oracle (4 iterations); every other row through row independence (a shard of the batch
    equals the rows of the full run) and determinism."""
    pipe = P.build_published_pipeline(dev, num_classes=3)
    ora = build_oracle_pipe(R.published_unet_kwargs(3), R.published_vae_kwargs(8), "published")
    cond = (torch.arange(16) % 3).to(dev)
    kw = dict(steps=4, use_ddim=True, guidance_scale=8.0, un_cond=None, decode=False)
    full = pipe.sample(16, (8, 32, 32), condition=cond, noise=M.PhiloxDeviceNoise(99), **kw)
    assert torch.equal(full, pipe.sample(16, (8, 32, 32), condition=cond, noise=M.PhiloxDeviceNoise(99), **kw))
    for shard in ((1, 4), (7, 16)):
        part = pipe.sample(16, (8, 32, 32), condition=cond, noise=M.PhiloxDeviceNoise(99), shard=shard, **kw)
        lo = shard[0] * 16 // shard[1]
        assert relerr(part, full[lo:lo + part.shape[0]]) < 1e-4
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    nz = S.PhiloxNoise(99)
    ora.set_noise_fn(lambda like: nz(torch.empty((16, *like.shape[1:])))[:2])    # rows 0, 1 of the 16-row draws
    want = ora.sample(2, (8, 32, 32), condition=cond[:2].cpu(), guidance_scale=8.0, un_cond=None, steps=4, use_ddim=True, decode=False) \
        if "decode" in ora.sample.__code__.co_varnames else None
    if want is None:
        tr = []
        ora.sample(2, (8, 32, 32), condition=cond[:2].cpu(), guidance_scale=8.0, un_cond=None, steps=4, use_ddim=True, trace=tr)
        want = tr[-1][1]
    e = relerr(full[:2], want)
    print(f"[measured] cfg3 at the per-GPU workload, rows 0-1 vs oracle: {e:.1e}")
    assert e < GUIDED_HARNESS_TOL
    g1 = pipe.sample(16, (8, 32, 32), condition=cond, noise=M.PhiloxDeviceNoise(99), steps=2, use_ddim=True, guidance_scale=1.0, un_cond=None)
    assert g1.shape == (16, 3, 256, 256) and bool(g1.isfinite().all())


@torch.no_grad()
def test_cfg4_graph_replay_at_full_size(dev, conv_precision):
    """BASELINE configs[3]: the DDPM schedule as ONE captured hipGraph replayed per iteration at B=8, latent 32x32, published widths:
    100 iterations equal the eager loop bit for bit; the full 1000-iteration replay finishes finite (1001 noise draws)."""
    pipe = P.build_published_pipeline(dev, num_classes=None)
    kw = dict(use_ddim=False, decode=False)
    eager = pipe.sample(8, (8, 32, 32), steps=100, noise=M.PhiloxDeviceNoise(4), loop="eager", **kw)
    graph = pipe.sample(8, (8, 32, 32), steps=100, noise=M.PhiloxDeviceNoise(4), use_graph=True, **kw)
    assert torch.equal(eager, graph)
    listed = pipe.sample(8, (8, 32, 32), steps=100, noise=M.PhiloxDeviceNoise(4), loop="cmdlist", **kw)    # the default loop of sample()
    assert torch.equal(eager, listed) and pipe.last_cmdlist_launches > 60    # (the whole iteration: 84 launches at this revision -- 92 minus the 8 conv_res that share their 3x3's launch at B = 8)
    if conv_precision == 5:
        src = M.PhiloxDeviceNoise(4)
        img = pipe.sample(8, (8, 32, 32), steps=None, use_ddim=False, noise=src, use_graph=True)
        assert src.draw_index == 1001 and img.shape == (8, 3, 256, 256) and bool(img.isfinite().all())
