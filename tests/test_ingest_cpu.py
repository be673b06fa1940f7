"""The data set's transform without a GPU: the numpy restatement (tests/ingest_cases.py) against Pillow itself, the library's coefficient tables
against the restatement's, the size rules against hand-computed values, the plan's totals, and every argument rule of medfusion_amd/ingest.py and
of the library entries (refused on the host before any launch)."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from medfusion_amd import ingest as I
from medfusion_amd import lib as L
from tests import ingest_cases as IC

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("mf_resample_table", "mf_resample_plan", "mf_image_resample", "mf_minmax_apply_f32")
FAKE = 1 << 12       # a non-null "device pointer" for calls that must be refused before any launch


@pytest.mark.parametrize("kind,C_", IC.DTYPES, ids=lambda v: str(v))
@pytest.mark.parametrize("case", range(len(IC.CASES)), ids=lambda c: "%dx%d-%dx%d" % (IC.CASES[c][0] + IC.CASES[c][1]))
def test_restatement_equals_pillow(case, kind, C_):
    """Image.resize(..., BILINEAR) in modes L, RGB, I;16 and F: 0 mismatching pixels (uint8, uint16), 0 mismatching bits (float32)"""
    oh, ow = IC.CASES[case][1]
    ref = IC.pil_resize(IC.data(case, kind, C_), oh, ow, kind)
    got = IC.want(case, kind, C_)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    bits = {"u8": np.uint8, "u16": np.uint16, "f32": np.uint32}[kind]
    assert int((np.ascontiguousarray(ref).view(bits) != got.view(bits)).sum()) == 0


def _axes():
    pairs = set()
    for (H, W), (oh, ow) in IC.CASES:
        pairs |= {(W, ow), (H, oh)}
    return sorted(pairs | {(17, 17), (1, 1), (1, 5), (1000, 1)})


@pytest.mark.parametrize("n_in,n_out", _axes(), ids=str)
def test_library_table_equals_the_restatement(n_in, n_out):
    """fp64 bits, the 22-bit integers, the bounds and ksize of every axis of the list, of in = out and of in = 1"""
    kk, b, ks = IC.coeffs(n_in, n_out)
    lib = L.load()
    assert lib.mf_resample_table(n_in, n_out, None, None, None) == ks
    wf, wi, bb = np.full((n_out, ks), 7.0), np.full((n_out, ks), 7, np.int32), np.full((n_out, 2), 7, np.int32)
    assert lib.mf_resample_table(n_in, n_out, wf.ctypes.data, wi.ctypes.data, bb.ctypes.data) == ks
    assert np.array_equal(wf.view(np.uint64), kk.view(np.uint64))
    assert np.array_equal(wi, IC.fixed(kk)) and np.array_equal(bb, b)
    ks2, wf2, wi2, b2 = I.resample_table(n_in, n_out)
    assert ks2 == ks and np.array_equal(wf2, kk) and np.array_equal(wi2, wi) and np.array_equal(b2, b)
    assert I.resample_table(n_in, n_out)[1] is wf2            # built once, kept across calls


def test_size_rules_against_hand_computed_values():
    assert I.resized_size(390, 320, 256) == (312, 256)        # shorter side 320 -> 256, 256 * 390 / 320 = 312.0
    assert I.resized_size(320, 390, 256) == (256, 312)
    assert I.resized_size(100, 333, 50) == (50, 166)          # 50 * 333 / 100 = 166.5 -> truncated
    assert I.resized_size(333, 100, 50) == (166, 50)
    assert I.resized_size(64, 64, 32) == (32, 32)
    assert I.resized_size(2828, 2320, 256) == (312, 256)      # 256 * 2828 / 2320 = 312.05...
    assert I.resized_size(37, 53, (16, 20)) == (16, 20) and I.resized_size(37, 53, [16]) == (16, 22) and I.resized_size(37, 53, None) == (37, 53)
    # odd differences 1, 3, 5: (d / 2) = 0.5, 1.5, 2.5 -> Python's round: 0, 2, 2
    assert I.center_crop_box(33, 32, 32) == (0, 0, 32, 32)
    assert I.center_crop_box(35, 32, 32) == (2, 0, 32, 32)
    assert I.center_crop_box(37, 32, 32) == (2, 0, 32, 32)
    assert I.center_crop_box(32, 39, 32) == (0, 4, 32, 32)    # 7 / 2 = 3.5 -> 4
    assert I.center_crop_box(312, 256, 256) == (28, 0, 256, 256)
    assert I.center_crop_box(40, 50, (30, 20)) == (5, 15, 30, 20)
    for bad in (41, (30, 51), 0):
        with pytest.raises(ValueError, match="crop"):
            I.center_crop_box(40, 50, bad)
    with pytest.raises(ValueError, match="resize"):
        I.resized_size(8, 8, 0)


def test_plan_totals():
    # one image, both passes: 37 x 53 -> 16 x 16, uint8 C = 3
    p = I.plan([(37, 53)], resize=(16, 16), dtype=np.uint8, channels=3)
    assert p["launches"] == 2 and p["out_size"] == (16, 16) and p["tables"] == 2
    assert p["workspace_bytes"] == 37 * 16 * 3 and p["workgroups"] == ((37 * 16 + 255) // 256, 1)
    ksh, ksv = IC.coeffs(53, 16)[2], IC.coeffs(37, 16)[2]
    assert p["table_bytes"] == 16 * (ksh + ksv) * 4 + 2 * 16 * 8 and p["source_bytes"] == 37 * 53 * 3
    # a ragged batch: the second image keeps its width (no horizontal pass, no workspace), the third is the first's geometry again (tables shared)
    p = I.plan([(37, 53), (40, 16), (37, 53)], resize=(16, 16), dtype=np.float32)
    assert p["launches"] == 2 and p["tables"] == 3 and p["workspace_bytes"] == 2 * 37 * 16 * 4 and p["workgroups"] == (2 * 3, 3)
    # a crop keeps the horizontal pass to the rows the surviving rows reach: 300 x 200 -> 30 x 20, rows 10 .. 19 of it
    _, b, _ = IC.coeffs(300, 30)
    rows = int((b[10:20, 0] + b[10:20, 1]).max() - b[10:20, 0].min())
    p = I.plan([(300, 200)], resize=(30, 20), crop=(10, 8), dtype=np.uint16)
    assert rows < 300 and p["workspace_bytes"] == rows * 8 * 2 and p["out_size"] == (10, 8)
    # nothing to resample: one launch, no tables, no workspace
    p = I.plan([(8, 9), (8, 9)], dtype=np.uint8, channels=3)
    assert p == {"launches": 1, "workgroups": (0, 2), "workspace_bytes": 0, "table_bytes": 0, "tables": 0, "source_bytes": 2 * 8 * 9 * 3,
                 "descriptor_bytes": 2 * C.sizeof(L.MfResampleImage), "out_size": (8, 9)}
    p = I.plan([(64, 64)], resize=(64, 31))                    # one axis skipped: the horizontal pass alone resamples
    assert p["tables"] == 1 and p["launches"] == 2 and p["workspace_bytes"] == 64 * 31


def test_pack_places_images_back_to_back():
    a = [np.arange(3 * 5, dtype=np.uint8).reshape(3, 5), np.arange(2 * 7, dtype=np.uint8).reshape(2, 7) + 100]
    p = I.pack(a, resize=(4, 4), pin=False)
    assert [d.src_off for d in p.geom.descs] == [0, 15]        # the second image starts at an odd byte
    buf = p.host.numpy()
    assert np.array_equal(buf[:15], a[0].reshape(-1)) and np.array_equal(buf[15:29], a[1].reshape(-1))
    o_desc, o_bounds, o_weights = p.sections
    assert o_desc % 16 == 0 and o_bounds % 16 == 0 and o_weights % 16 == 0 and o_desc >= 29
    assert bytes(buf[o_desc:o_desc + C.sizeof(p.geom.descs)]) == bytes(p.geom.descs)
    assert np.array_equal(buf[o_bounds:o_bounds + p.geom.bounds.nbytes].view(np.int32).reshape(-1, 2), p.geom.bounds)
    b = [np.zeros((3, 5), np.uint16), np.zeros((2, 7), np.uint16)]
    assert [d.src_off for d in I.pack(b, resize=(4, 4), pin=False).geom.descs] == [0, 30]


def test_value_errors_name_the_argument_before_any_device_work():
    u8 = np.zeros((8, 8), np.uint8)
    with pytest.raises(ValueError, match="mixed dtypes"):
        I.transform([u8, np.zeros((8, 8), np.uint16)], device="cuda")
    with pytest.raises(ValueError, match="4 channels"):
        I.transform([np.zeros((8, 8, 4), np.uint8)], device="cuda")
    with pytest.raises(ValueError, match="not contiguous"):
        I.transform([np.zeros((8, 16), np.uint8)[:, ::2]], device="cuda")
    with pytest.raises(ValueError, match="mixed channel"):
        I.transform([u8, np.zeros((8, 8, 3), np.uint8)], device="cuda")
    with pytest.raises(ValueError, match="dtype"):
        I.transform([np.zeros((8, 8), np.int16)], device="cuda")
    with pytest.raises(ValueError, match="channels"):
        I.transform([np.zeros((8, 8, 3), np.float32)], normalize=None, device="cuda")
    with pytest.raises(ValueError, match="channels"):
        I.transform([np.zeros((8, 8, 2), np.uint8)], device="cuda")
    with pytest.raises(ValueError, match="arrays"):
        I.transform([], device="cuda")
    with pytest.raises(ValueError, match="normalize"):
        I.transform([u8], normalize="zscore", device="cuda")
    with pytest.raises(ValueError, match="normalize"):
        I.transform([np.zeros((8, 8), np.float32)], device="cuda")
    with pytest.raises(ValueError, match="crop"):
        I.transform([u8], resize=6, crop=7, device="cuda")
    with pytest.raises(ValueError, match="byte path"):
        I.resample_bytes([np.zeros((8, 8), np.uint16)], device="cuda")
    # every output of a batch has one size: the first offending file and both sizes are named
    with pytest.raises(ValueError, match=r"b\.png \(10 x 30\) gives an output of 16 x 48, a\.png one of 16 x 32"):
        I.transform([np.zeros((10, 20), np.uint8), np.zeros((10, 30), np.uint8), np.zeros((10, 40), np.uint8)], resize=16, names=["a.png", "b.png", "c.png"],
                    device="cuda")
    with pytest.raises(ValueError, match="Packed"):
        I.transform(I.pack([u8], pin=False), resize=4, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        I.transform([u8], device="cpu")


def _one_image(H=8, W=8, Hr=4, Wr=4, top=0, left=0):
    d = (L.MfResampleImage * 1)()
    d[0].H, d[0].W, d[0].Hr, d[0].Wr, d[0].top, d[0].left = H, W, Hr, Wr, top, left
    parts, nw, nb = [], 0, 0
    for axis, n_in, n_out in (("h", W, Wr), ("v", H, Hr)):
        if n_in != n_out:
            ks, _, _, b = I.resample_table(n_in, n_out)
            setattr(d[0], "tw_" + axis, nw), setattr(d[0], "tb_" + axis, nb), setattr(d[0], "ksize_" + axis, ks)
            parts.append(b)
            nw, nb = nw + n_out * ks, nb + n_out
    bounds = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((1, 2), np.int32)
    return d, bounds, nw, nb


def test_library_error_codes_without_a_device():
    lib = L.load()
    plan = L.MfResamplePlan()

    def do_plan(d, bounds, nw, nb, C_=1, dt=L.INGEST_U8, h=4, w=4, src=64):
        return lib.mf_resample_plan(d, 1, C_, dt, h, w, bounds.ctypes.data, nb, nw, src, C.byref(plan))

    d, bounds, nw, nb = _one_image()
    assert do_plan(d, bounds, nw, nb) == 0 and plan.launches == 2 and plan.workspace_bytes == 8 * 4 and (plan.wg_h, plan.wg_v) == (1, 1)
    assert lib.mf_resample_plan(None, 1, 1, 0, 4, 4, None, 0, 0, 64, C.byref(plan)) == -1 and b"null" in lib.mf_last_error()
    assert lib.mf_resample_plan(d, 1, 1, 0, 4, 4, bounds.ctypes.data, nb, nw, 64, None) == -1
    assert do_plan(d, bounds, nw, nb, C_=2) == -1 and b"1 or 3" in lib.mf_last_error()
    assert do_plan(d, bounds, nw, nb, C_=4) == -1
    assert do_plan(d, bounds, nw, nb, C_=3, dt=L.INGEST_U16, src=1 << 20) == -2 and do_plan(d, bounds, nw, nb, C_=3, dt=L.INGEST_F32, src=1 << 20) == -2
    assert do_plan(d, bounds, nw, nb, dt=3) == -1 and do_plan(d, bounds, nw, nb, h=0) == -1
    assert do_plan(d, bounds, nw, nb, h=5) == -1 and b"crop" in lib.mf_last_error()          # a crop outside the resized image
    assert do_plan(d, bounds, nw, nb, src=63) == -1 and b"outside the buffer" in lib.mf_last_error()
    assert do_plan(d, bounds, nw, nb - 1) == -1 and do_plan(d, bounds, nw - 1, nb) == -1     # table rows outside the tables given
    for field, bad in (("H", 0), ("Wr", 0), ("top", -1), ("left", 1), ("ksize_h", 7), ("src_off", -1), ("reserved", 1)):
        d2, bounds, nw, nb = _one_image()
        setattr(d2[0], field, bad)
        assert do_plan(d2, bounds, nw, nb) == -1, field
    d2, bounds, nw, nb = _one_image()
    d2[0].src_off = 1
    assert do_plan(d2, bounds, nw, nb, dt=L.INGEST_U16, src=1 << 20) == -1                   # a uint16 image at an odd byte
    bad_bounds = bounds.copy()
    bad_bounds[1, 0] = 7                                                                     # (xmin, n) reaching past the source
    assert do_plan(d, bad_bounds, nw, nb) == -1 and b"bounds" in lib.mf_last_error()

    def args(d_, b_, nw_, nb_, **kw):
        a = L.MfResampleArgs()
        a.src, a.images, a.images_host, a.weights_i32, a.weights_f64, a.bounds, a.bounds_host = FAKE, FAKE, C.addressof(d_), FAKE, FAKE, FAKE, b_.ctypes.data
        a.workspace, a.workspace_bytes, a.out, a.bounds_count, a.weights_count, a.src_bytes = FAKE, 1 << 20, FAKE, nb_, nw_, 64
        a.N, a.C, a.dtype, a.h, a.w, a.out_mode = 1, 1, L.INGEST_U8, 4, 4, L.INGEST_CENTERED
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    d, bounds, nw, nb = _one_image()
    assert do_plan(d, bounds, nw, nb) == 0
    run = lambda **kw: lib.mf_image_resample(C.byref(args(d, bounds, nw, nb, **kw)), None)
    assert lib.mf_image_resample(None, None) == -1
    for ptr in ("src", "images", "images_host", "out", "bounds", "bounds_host", "weights_i32", "workspace"):
        assert run(**{ptr: None}) == -1, ptr
    assert run(dtype=L.INGEST_F32, weights_f64=None, out_mode=L.INGEST_RAW) == -1
    assert run(C=2) == -1 and run(C=3, dtype=L.INGEST_U16, src_bytes=1 << 20) == -2
    assert run(out_mode=3) == -1 and run(out_mode=L.INGEST_BYTES, dtype=L.INGEST_U16) == -1 and run(out_mode=L.INGEST_CENTERED, dtype=L.INGEST_F32) == -1
    assert run(h=5) == -1 and run(N=0) == -1 and run(reserved=1) == -1
    assert run(workspace_bytes=8 * 4 - 1) == -4 and b"workspace" in lib.mf_last_error()      # a workspace too small
    assert run(workspace=FAKE + 8) == -1
    raw = (L.MfResampleImage * 1)()                                                          # descriptors the plan did not fill
    C.memmove(raw, d, C.sizeof(raw))
    raw[0].rows -= 1
    a = args(raw, bounds, nw, nb)
    assert lib.mf_image_resample(C.byref(a), None) == -1 and b"mf_resample_plan" in lib.mf_last_error()
    assert lib.mf_resample_table(0, 4, None, None, None) == -1 and lib.mf_resample_table(4, 0, None, None, None) == -1
    assert lib.mf_minmax_apply_f32(None, FAKE, 1, 16, 1, None) == -1 and lib.mf_minmax_apply_f32(FAKE, FAKE, 0, 16, 1, None) == -1
    assert lib.mf_minmax_apply_f32(FAKE, None, 1, 16, 1, None) == -1 and lib.mf_minmax_apply_f32(FAKE, FAKE, 1, 0, 1, None) == -1


def test_new_entry_points_are_declared_exported_bound_and_documented():
    hdr = (ROOT / "include" / "medfusion_hip.h").read_text()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    md = (ROOT / "INTEGRATION.md").read_text()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.exported_symbols() and hasattr(lib, name), name
        assert name in md, f"INTEGRATION.md does not list {name}"
    assert lib.mf_version() == 250 and "#define MF_VERSION 250" in hdr       # additive within ABI 250
    from medfusion_amd import build as B
    assert "ingest.hip" in B.SOURCES and "-packed-fp32-ops" in B.EXTRA_CFLAGS["ingest.hip"]


def test_struct_layouts_match_what_a_c_compiler_sees(tmp_path):
    assert C.sizeof(L.MfResampleImage) == 6 * 8 + 12 * 4 and C.sizeof(L.MfResamplePlan) == 8 + 4 * 4 and C.sizeof(L.MfResampleArgs) == 9 * 8 + 4 * 8 + 8 * 4
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    structs = {"MfResampleImage": L.MfResampleImage, "MfResamplePlan": L.MfResamplePlan, "MfResampleArgs": L.MfResampleArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "medfusion_hip.h"', 'int main(void) {']
    for name, cls in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for name, cls in structs.items():
        assert int(got[name]) == C.sizeof(cls), name
        for fname, _ in cls._fields_:
            assert int(got[f"{name}.{fname}"]) == getattr(cls, fname).offset, f"{name}.{fname}"


def test_harness_flags_leave_the_default_path_alone():
    """without --resize / --crop / --ext a script lists *.png and takes the byte ingress as before"""
    import argparse
    ap = argparse.ArgumentParser()
    I.add_ingest_arguments(ap)
    a = ap.parse_args([])
    assert (a.resize, a.crop, a.ext) == (None, None, None) and not I.ingest_requested(a)
    a = ap.parse_args(["--resize", "256", "--crop", "224", "200", "--ext", "png", "JPG"])
    assert I.ingest_requested(a) and I._size_arg(a.resize) == 256 and I._size_arg(a.crop) == (224, 200) and a.ext == ["png", "JPG"]


def test_list_images_and_decode(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    Image.fromarray(rng.integers(0, 256, (5, 7, 3), dtype=np.uint8), "RGB").save(tmp_path / "b.png")
    Image.fromarray(rng.integers(0, 256, (6, 4), dtype=np.uint8), "L").save(tmp_path / "a.JPG")
    Image.fromarray(rng.integers(0, 65536, (3, 3), dtype=np.uint16)).save(tmp_path / "c.tif")
    (tmp_path / "notes.txt").write_text("x")
    assert [f.name for f in I.list_images(tmp_path)] == ["b.png"]
    assert [f.name for f in I.list_images(tmp_path, ("png", "jpg", "tif"))] == ["a.JPG", "b.png", "c.tif"]
    assert I.decode(tmp_path / "b.png", 3).shape == (5, 7, 3) and I.decode(tmp_path / "b.png", 1).shape == (5, 7, 1)
    assert I.decode(tmp_path / "a.JPG", 3).shape == (6, 4, 3) and I.decode(tmp_path / "a.JPG", 3).dtype == np.uint8
    c16 = I.decode(tmp_path / "c.tif", 1)
    assert c16.dtype == np.uint16 and c16.shape == (3, 3, 1) and c16.flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError, match="path"):
        I.ImageFolder(tmp_path, exts=("bmp",))
