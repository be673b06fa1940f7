"""The data set's transform (mf_image_resample: csrc/ingest.hip, medfusion_amd/ingest.py) on a real MI355X, held bit for bit to the numpy
restatement of PIL's resampler (tests/ingest_cases.py, itself held to Pillow with 0 mismatches by tests/test_ingest_cpu.py): every case of the list
for uint8 (1 and 3 channels), uint16 and float32; the value maps against torch's chains; a ragged batch against its single-image calls; fused crops
against resize-then-slice; a same-size image against K.image_ingress; a repeated call; ImageFolder and the harness loader.  Nothing here has a
tolerance: every comparison is equality of bits."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from medfusion_amd import ingest as I
from medfusion_amd import kernels as K
from tests import ingest_cases as IC

ROOT = Path(__file__).resolve().parents[1]
CASE_IDS = ["%dx%d-%dx%d" % (c[0] + c[1]) for c in IC.CASES]
BITS = {"u8": np.uint8, "u16": np.uint16, "f32": np.uint32}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def raw(arrays, dev, kind, **kw):
    """the resampled values of a batch as [N, h, w, C] of the element type: the byte path for uint8, the fp32 NCHW output for the others (a uint16
    value is exact in fp32)"""
    if kind == "u8":
        return I.resample_bytes(arrays, device=dev, **kw).cpu().numpy()
    y = I.transform(arrays, normalize=None, device=dev, **kw).cpu().numpy().transpose(0, 2, 3, 1)
    if kind == "u16":
        assert np.array_equal(y, np.floor(y)) and y.min() >= 0 and y.max() <= 65535
    return np.ascontiguousarray(y.astype(IC.NP_DTYPE[kind]))


def same_bits(a, b, kind):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(BITS[kind]), np.ascontiguousarray(b).view(BITS[kind]))


@pytest.mark.parametrize("kind,C_", IC.DTYPES, ids=lambda v: str(v))
@pytest.mark.parametrize("case", range(len(IC.CASES)), ids=CASE_IDS)
def test_kernel_equals_the_restatement_bit_for_bit(dev, case, kind, C_):
    got = raw([IC.data(case, kind, C_)], dev, kind, resize=IC.CASES[case][1])
    assert same_bits(got[0], IC.want(case, kind, C_), kind)


@pytest.mark.parametrize("kind,C_", IC.DTYPES, ids=lambda v: str(v))
@pytest.mark.parametrize("case", range(len(IC.CASES)), ids=CASE_IDS)
def test_kernel_equals_pillow_where_it_imports(dev, case, kind, C_):
    pytest.importorskip("PIL")
    oh, ow = IC.CASES[case][1]
    got = raw([IC.data(case, kind, C_)], dev, kind, resize=(oh, ow))
    assert same_bits(got[0], IC.pil_resize(IC.data(case, kind, C_), oh, ow, kind), kind)


@pytest.mark.parametrize("case", [0, 2, 4, 8], ids=lambda c: CASE_IDS[c])
def test_value_maps_equal_torchs_chains(dev, case):
    size = IC.CASES[case][1]
    for kind, C_, full in (("u8", 1, 255), ("u8", 3, 255), ("u16", 1, 65535)):
        v = torch.from_numpy(IC.want(case, kind, C_).astype(np.int32)).permute(2, 0, 1)[None]
        want = ((v / full) - 0.5) / 0.5
        got = I.transform([IC.data(case, kind, C_)], resize=size, device=dev)
        assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got.cpu(), want.contiguous())
    for kind, C_ in IC.DTYPES:
        v = torch.from_numpy(IC.want(case, kind, C_).astype(np.float32)).permute(2, 0, 1).contiguous()
        unit = (v - v.min()) / (v.max() - v.min())
        got = I.transform([IC.data(case, kind, C_)], resize=size, normalize="minmax", center=False, device=dev)
        assert torch.equal(got.cpu()[0], unit)
        got = I.transform([IC.data(case, kind, C_)], resize=size, normalize="minmax", device=dev)
        assert torch.equal(got.cpu()[0], (unit - 0.5) / 0.5)
        assert torch.equal(I.transform([IC.data(case, kind, C_)], resize=size, normalize=None, device=dev).cpu()[0], v)


@pytest.mark.parametrize("kind,C_", IC.DTYPES, ids=lambda v: str(v))
@pytest.mark.parametrize("geom", [dict(resize=(24, 20)), dict(resize=12, crop=8), dict(resize=(33, 10))], ids=["to24x20", "short12crop8", "to33x10"])
def test_ragged_batch_equals_its_single_image_calls(dev, kind, C_, geom):
    """every source of the case list in ONE batch (sizes 1 x 9 .. 320 x 390, up- and downscales, images at odd byte offsets, one whose axis or whole
    size is the target's), each against its own single-image call; a permuted batch permutes the outputs"""
    arrays = [IC.data(c, kind, C_) for c in range(len(IC.CASES))]
    if kind == "u8":
        offs = [d.src_off for d in I.pack(arrays, pin=False, **geom).geom.descs]
        assert any(o % 2 for o in offs) and any(o % 4 for o in offs)
    got = raw(arrays, dev, kind, **geom)
    for i, a in enumerate(arrays):
        assert same_bits(got[i:i + 1], raw([a], dev, kind, **geom), kind), i
    perm = [5, 0, 8, 3, 1, 7, 2, 6, 4]
    assert same_bits(raw([arrays[p] for p in perm], dev, kind, **geom), got[perm], kind)
    if "crop" not in geom:                                     # and against the restatement itself
        oh, ow = geom["resize"]
        for i in (0, 3, 8):
            assert same_bits(got[i], IC.resize(arrays[i], oh, ow, kind), kind)


@pytest.mark.parametrize("kind,C_", IC.DTYPES, ids=lambda v: str(v))
@pytest.mark.parametrize("case", [0, 1, 2, 4, 6], ids=lambda c: CASE_IDS[c])
def test_fused_crop_equals_resize_then_slice(dev, case, kind, C_):
    oh, ow = IC.CASES[case][1]
    a, full = IC.data(case, kind, C_), IC.want(case, kind, C_)
    ch, cw = max(oh // 2, 1), max(ow // 3, 1)
    boxes = [(0, 0, ch, cw), (oh - ch, ow - cw, ch, cw), (0, ow - cw, oh, cw), (oh - ch, 0, ch, ow), I.center_crop_box(oh, ow, (ch, cw))]
    for top, left, h, w in boxes:
        got = raw([a], dev, kind, resize=(oh, ow), crop=(top, left, h, w))
        assert same_bits(got[0], full[top:top + h, left:left + w], kind), (top, left, h, w)
    top, left, h, w = I.center_crop_box(oh, ow, (ch, cw))
    assert same_bits(raw([a], dev, kind, resize=(oh, ow), crop=(ch, cw))[0], full[top:top + h, left:left + w], kind)


def test_same_size_images_equal_image_ingress(dev):
    rng = np.random.default_rng(5)
    for shape in ((3, 17, 23, 1), (2, 16, 16, 3), (1, 1, 1, 3)):
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        want = K.image_ingress(torch.from_numpy(x).to(dev))
        assert torch.equal(I.transform(list(x), device=dev), want)
        assert torch.equal(I.transform(list(x), resize=shape[1:3], device=dev), want)
    # in a ragged batch: the image that already has the target's size, between two that are resampled
    arrays = [IC.data(0, "u8", 3), rng.integers(0, 256, (16, 16, 3), dtype=np.uint8), IC.data(2, "u8", 3)]
    got = I.transform(arrays, resize=(16, 16), device=dev)
    assert torch.equal(got[1:2], K.image_ingress(torch.from_numpy(arrays[1][None]).to(dev)))
    # a skipped axis rounds nothing twice: 64 x 64 -> 64 x 31 is the horizontal pass alone
    assert same_bits(raw([IC.data(4, "u16", 1)], dev, "u16", resize=(64, 31))[0], IC.want(4, "u16", 1), "u16")


def test_repeated_call_with_cached_tables_and_reused_buffers(dev):
    arrays = [IC.data(c, "u8", 3) for c in (0, 1, 5)]
    p = I.plan([a.shape[:2] for a in arrays], resize=(32, 32), dtype=np.uint8, channels=3)
    assert p["launches"] == 2 and p["workspace_bytes"] > 0
    ws = torch.full((p["workspace_bytes"] + 64,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((3, 3, 32, 32), float("nan"), device=dev)
    first = I.transform(arrays, resize=(32, 32), device=dev).clone()
    tables = {k: v[1] for k, v in I._TABLES.items()}
    assert I.transform(arrays, resize=(32, 32), device=dev, workspace=ws, out=out) is out and torch.equal(out, first)
    out.fill_(float("nan"))
    packed = I.pack(arrays, resize=(32, 32))
    assert torch.equal(I.transform(packed, device=dev, workspace=ws, out=out), first) and torch.equal(I.transform(packed, device=dev), first)
    assert all(I._TABLES[k][1] is v for k, v in tables.items())                       # no table was built again
    with pytest.raises(ValueError, match="workspace"):
        I.transform(arrays, resize=(32, 32), device=dev, workspace=ws[:16])
    with pytest.raises(ValueError, match="out"):
        I.transform(arrays, resize=(32, 32), device=dev, out=out[:2])


def test_image_folder_and_the_harness_loader(dev, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(9)
    shapes = {"a.png": (40, 57), "b.png": (64, 33), "c.png": (32, 32)}
    for name, (h, w) in shapes.items():
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(tmp_path / name)
    files = sorted(tmp_path.glob("*.png"))
    for channels in (3, 1):
        decoded = [I.decode(f, channels) for f in files]
        assert [d.shape for d in decoded] == [shapes[f.name] + (channels,) for f in files]
        want = I.transform(decoded, resize=32, crop=32, device=dev)
        batches = list(I.ImageFolder(tmp_path, channels=channels, resize=32, crop=32, batch=2, device=dev))
        assert [names for _, names in batches] == [["a.png", "b.png"], ["c.png"]]
        assert torch.equal(torch.cat([b for b, _ in batches]), want) and want.shape == (3, channels, 32, 32)
        assert same_bits(I.resample_bytes(decoded[:1], resize=32, crop=32, device=dev).cpu().numpy()[0],
                         IC.resize(decoded[0], 32, 45, "u8")[:, 6:38], "u8")          # 32 * 57 / 40 = 45.6 -> 45; round(13 / 2) = 6
    with pytest.raises(ValueError, match=r"b\.png \(64 x 33\) gives an output of 62 x 32, a\.png one of 32 x 45"):
        next(iter(I.ImageFolder(tmp_path, resize=32, device=dev)))
    # scripts/img2img.py's loader: --resize 32 --crop 32 over the three sizes; without the flags files of one size take the byte ingress as before
    import argparse
    sys.path.insert(0, str(ROOT / "scripts"))
    try:
        import img2img
    finally:
        sys.path.pop(0)
    ap = argparse.ArgumentParser()
    I.add_ingest_arguments(ap)
    for channels in (3, 1):
        x = img2img.load_images(files, channels, dev, ap.parse_args(["--resize", "32", "--crop", "32"]))
        assert x.shape == (3, channels, 32, 32) and torch.equal(x, I.transform([I.decode(f, channels) for f in files], resize=32, crop=32, device=dev))
    plain = img2img.load_images(files[2:], 3, dev, ap.parse_args([]))
    assert torch.equal(plain, K.image_ingress(torch.from_numpy(img2img.load_png(files[2], 3)[None].copy()).to(dev)))
    mask = np.zeros((40, 57), np.uint8)
    mask[10:20, 30:] = 255
    Image.fromarray(mask, "L").save(tmp_path / "mask_file.png")
    m = I.load_mask(tmp_path / "mask_file.png", dev, ap.parse_args(["--resize", "32", "--crop", "32"]))
    assert m.shape == (1, 1, 32, 32) and m.dtype == torch.uint8 and 0 < int((m != 0).sum()) < 32 * 32
    m0 = I.load_mask(tmp_path / "mask_file.png", dev, ap.parse_args([]))
    assert m0.shape == (1, 1, 40, 57) and torch.equal(m0.cpu()[0, 0], torch.from_numpy(mask))
