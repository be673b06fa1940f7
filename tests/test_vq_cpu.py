"""The codebook embedders on the CPU: state-dict layout against the reference's recorded key lists, the test-side restatement against the
reference's fixtures (tests/golden/vq_*, scripts/gen_vq_golden.py), and checkpoint loading of pipelines whose latent embedder is a VQVAE, VQGAN or
VAEGAN (latent_embedders.py:191-340, 408-490, 860-940)."""
import json
import sys
import types

import pytest
import torch

import medfusion_amd as M
from oracle import restate as R
from oracle import synth as S
from tests import vq_restate as V
from tests.util import T, gold, to_product_kwargs

ROOT = __import__("pathlib").Path(__file__).resolve().parents[1]
KEYS = json.loads((ROOT / "tests" / "golden" / "vq_keys.json").read_text())
PRODUCT = {"VQVAE": M.VQVAE, "VQGAN": M.VQGAN, "VAEGAN": M.VAEGAN}
REF_MOD = "medical_diffusion.models.embedders.latent_embedders"


def _inference_keys(tag):
    return [(k, tuple(s)) for k, s in KEYS["keys"][tag] if not k.startswith("discriminator.")]


@pytest.mark.parametrize("tag,n", [("VQVAE_tiny", 89), ("VQGAN_tiny", 89), ("VAEGAN_tiny", 90), ("VQVAE_default", 85), ("VQGAN_default", 85),
                                   ("VAEGAN_default", 86)])
def test_state_dict_layout_is_the_references(tag, n):
    cls, size = tag.split("_")
    m = PRODUCT[cls](**(KEYS["kwargs"][tag] if size == "tiny" else {}))
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert len(got) == n
    assert got == _inference_keys(tag)
    if cls != "VQVAE":   # the reference's GAN variants carry their discriminators besides: training-only, not built here
        assert len(KEYS["keys"][tag]) > n and all(k.startswith(("vqvae.", "discriminator.")) for k, _ in KEYS["keys"][tag])


def test_group_defaults_and_geometry():
    q, g, v = M.VQVAE(), M.VQGAN(), M.VAEGAN()
    assert q.inc.block_seq[0].basic_block.norm.num_groups == 32 and g.vqvae.inc_dec.block_seq[0].basic_block.norm.num_groups == 32
    assert v.vqvae.inc.block_seq[0].basic_block.norm.num_groups == 8
    assert q.quantizer.embedder.weight.shape == (8192, 4) and q.scale == 8 and g.scale == 8 and v.scale == 8
    assert (g.emb_channels, g.out_channels, v.emb_channels, v.out_channels) == (4, 3, 4, 3)
    assert isinstance(g.vqvae, M.VQVAE) and type(v.vqvae) is M.VAE


def _restated(cls, kw, prefix):
    m = cls(**kw).eval()
    S.synth_state_dict(m, prefix)
    return m


@pytest.mark.parametrize("name,cls,kwtag,prefix", [("vq_vqvae_tiny", V.VQVAE, "VQVAE_tiny", "vqvae_tiny."),
                                                    ("vq_vqgan_tiny", V.VQGAN, "VQGAN_tiny", "vqgan_tiny.")])
@torch.no_grad()
def test_restatement_reproduces_the_reference_fixtures(name, cls, kwtag, prefix):
    """bit for bit, on one thread like the generator (the fixtures' summation order)"""
    g = gold(name)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        m = _restated(cls, KEYS["kwargs"][kwtag], prefix)
        q = m.vqvae.quantizer if hasattr(m, "vqvae") else m.quantizer
        assert torch.equal(q.indices(T(g["z"])).int(), T(g["idx_dec"]))
        assert torch.equal(m.decode(T(g["z"])), T(g["x_dec"]))
        assert torch.equal(m.encode(T(g["img"])), T(g["z_enc"]))
        assert torch.equal(q.indices(T(g["z_enc"])).int(), T(g["idx_fwd"]))
        out, hor, loss = m(T(g["img"]))
        assert torch.equal(out, T(g["out"])) and len(hor) == 2
        assert all(torch.equal(h, T(g[f"hor{i}"])) for i, h in enumerate(hor))
        assert torch.equal(loss.reshape(1), T(g["emb_loss"]))
    finally:
        torch.set_num_threads(threads)
    assert float(g["margin_dec"]) >= 1e-3 and float(g["margin_fwd"]) >= 1e-3


# ----------------------------------------------------------------------------- checkpoints
def _fake_reference(clsnames):
    """the reference's module tree, just long enough to pickle class references into a file (tests/test_host_logic_cpu.py's technique)"""
    names = ["medical_diffusion", "medical_diffusion.models", "medical_diffusion.models.estimators", "medical_diffusion.models.estimators.unet2",
             "medical_diffusion.models.noise_schedulers", "medical_diffusion.models.noise_schedulers.gaussian_scheduler",
             "medical_diffusion.models.embedders", "medical_diffusion.models.embedders.time_embedder", REF_MOD]
    mods = {n: types.ModuleType(n) for n in names}
    made = {}
    for modname, clsname in [("medical_diffusion.models.estimators.unet2", "UNet"),
                             ("medical_diffusion.models.noise_schedulers.gaussian_scheduler", "GaussianNoiseScheduler"),
                             ("medical_diffusion.models.embedders.time_embedder", "TimeEmbbeding")] + [(REF_MOD, c) for c in clsnames]:
        c = type(clsname, (), {})
        c.__module__, c.__qualname__ = modname, clsname
        setattr(mods[modname], clsname, c)
        made[clsname] = c
    return names, mods, made


def _embedder(cls_name, kw, prefix):
    m = PRODUCT[cls_name](**kw) if cls_name in PRODUCT else M.VAE(**kw)
    S.synth_state_dict(m, prefix)
    return m


def _disc(sd, prefix=""):
    """a discriminator's tensors, as a GAN checkpoint carries them"""
    sd = dict(sd)
    sd[prefix + "discriminator.0.inc.conv.weight"] = torch.ones(8, 3, 3, 3)
    sd[prefix + "discriminator.0.outc.conv.bias"] = torch.ones(1)
    return sd


def _write_pipeline(tmp_path, cls_name, emb_kw, emb, baked="", embedder_ckpt=True, drop=None):
    ukw = R.tiny_unet_kwargs(None, "none", in_ch=emb_kw["emb_channels"], out_ch=emb_kw["emb_channels"])
    src = M.DiffusionPipeline(M.GaussianNoiseScheduler, M.UNet, emb, R.published_scheduler_kwargs(), to_product_kwargs(ukw), clip_x0=False)
    S.synth_state_dict(src.noise_estimator, "vqckpt.unet.")
    names, mods, made = _fake_reference([cls_name])
    hp = dict(noise_scheduler=made["GaussianNoiseScheduler"], noise_estimator=made["UNet"], latent_embedder=made[cls_name],
              noise_scheduler_kwargs=R.published_scheduler_kwargs(), noise_estimator_kwargs=dict(ukw, time_embedder=made["TimeEmbbeding"]),
              latent_embedder_checkpoint=baked, estimator_objective="x_T", clip_x0=False, optimizer=torch.optim.AdamW)
    sd = _disc(src.state_dict(), "latent_embedder.")
    if drop:
        sd.pop(drop)
    sys.modules.update(mods)
    try:
        if embedder_ckpt:
            esd = _disc(emb.state_dict())
            torch.save({"state_dict": esd, "hyper_parameters": dict(emb_kw, optimizer_vqvae=torch.optim.Adam, gan_loss_weight=1.0)},
                       tmp_path / "emb.ckpt")
        torch.save({"state_dict": sd, "hyper_parameters": hp, "pytorch-lightning_version": "1.8.6"}, tmp_path / "last.ckpt")
    finally:
        for n in names:
            sys.modules.pop(n, None)
    return src


@pytest.mark.parametrize("cls_name,kw", [("VQGAN", V.tiny_vq_kwargs(num_embeddings=100, deep_supervision=1)),
                                         ("VQVAE", V.tiny_vq_kwargs(num_embeddings=70, emb_channels=3, deep_supervision=0)),
                                         ("VAEGAN", V.tiny_vaegan_kwargs())])
def test_pipeline_checkpoint_with_a_codebook_or_gan_embedder_loads_it(tmp_path, cls_name, kw):
    emb = _embedder(cls_name, kw, f"vqckpt.{cls_name}.")
    src = _write_pipeline(tmp_path, cls_name, kw, emb, baked=str(tmp_path / "emb.ckpt"))

    def check(pipe):
        assert type(pipe.latent_embedder) is PRODUCT[cls_name]
        got, want = pipe.state_dict(), src.state_dict()
        assert list(got) == list(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k
        assert not any("discriminator" in k for k in got)

    # through the readable embedder checkpoint named in the hyper-parameters (its discriminator tensors are ignored)
    check(M.DiffusionPipeline.load_from_checkpoint(tmp_path / "last.ckpt"))
    # through the shape inference: the baked path is gone, the weights come from the pipeline checkpoint's latent_embedder.* tensors
    (tmp_path / "emb.ckpt").unlink()
    check(M.DiffusionPipeline.load_from_checkpoint(tmp_path / "last.ckpt"))
    from medfusion_amd.checkpoint import infer_vae_kwargs
    inf = infer_vae_kwargs({k[len("latent_embedder."):]: v for k, v in src.state_dict().items() if k.startswith("latent_embedder.")}, cls_name)
    assert inf["hid_chs"] == kw["hid_chs"] and inf["emb_channels"] == kw["emb_channels"] and inf["deep_supervision"] == kw["deep_supervision"]
    assert inf.get("num_embeddings") == kw.get("num_embeddings") and "norm_name" not in inf


def test_pipeline_checkpoint_missing_autoencoder_tensors_is_refused(tmp_path):
    kw = V.tiny_vq_kwargs(num_embeddings=100)
    emb = _embedder("VQGAN", kw, "vqckpt.missing.")
    _write_pipeline(tmp_path, "VQGAN", kw, emb, baked="", embedder_ckpt=False, drop="latent_embedder.vqvae.quantizer.embedder.weight")
    with pytest.raises(RuntimeError, match="quantizer.embedder.weight"):
        M.DiffusionPipeline.load_from_checkpoint(tmp_path / "last.ckpt")
    _write_pipeline(tmp_path, "VQGAN", kw, emb, baked="", embedder_ckpt=False, drop="latent_embedder.vqvae.outc.conv.weight")
    with pytest.raises(RuntimeError, match="outc.conv.weight"):
        M.DiffusionPipeline.load_from_checkpoint(tmp_path / "last.ckpt")
    # a GAN embedder checkpoint missing one autoencoder tensor: refused, not filled with random weights (`vqvae` is not training-only)
    from medfusion_amd.checkpoint import _check_missing
    with pytest.raises(RuntimeError, match="missing"):
        _check_missing(["vqvae.inc.block_seq.0.basic_block.conv.weight"], "VQGAN")
    _check_missing(["discriminator.0.inc.conv.weight", "perceiver.net.x"], "VQGAN")


def test_pipeline_checkpoint_with_an_unknown_embedder_raises(tmp_path):
    kw = V.tiny_vq_kwargs(num_embeddings=100)
    emb = _embedder("VQGAN", kw, "vqckpt.unknown.")
    ukw = R.tiny_unet_kwargs(None, "none", in_ch=4, out_ch=4)
    src = M.DiffusionPipeline(M.GaussianNoiseScheduler, M.UNet, emb, R.published_scheduler_kwargs(), to_product_kwargs(ukw), clip_x0=False)
    names, mods, made = _fake_reference(["SomeOtherEmbedder"])
    hp = dict(noise_scheduler=made["GaussianNoiseScheduler"], noise_estimator=made["UNet"], latent_embedder=made["SomeOtherEmbedder"],
              noise_scheduler_kwargs=R.published_scheduler_kwargs(), noise_estimator_kwargs=dict(ukw, time_embedder=made["TimeEmbbeding"]),
              latent_embedder_checkpoint="gone.ckpt", loss=torch.nn.L1Loss)
    sys.modules.update(mods)
    try:
        torch.save({"state_dict": src.state_dict(), "hyper_parameters": hp}, tmp_path / "last.ckpt")
    finally:
        for n in names:
            sys.modules.pop(n, None)
    with pytest.raises(RuntimeError, match="SomeOtherEmbedder"):
        M.DiffusionPipeline.load_from_checkpoint(tmp_path / "last.ckpt")
    # the other training-only references stay placeholders: the hyper-parameters still read
    from medfusion_amd.checkpoint import read_checkpoint
    assert "loss" in read_checkpoint(tmp_path / "last.ckpt")["hyper_parameters"]
