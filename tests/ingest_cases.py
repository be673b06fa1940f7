"""The data set's transform (medfusion_amd/ingest.py, csrc/ingest.hip) without a device: the numpy restatement of PIL's bilinear resampler
(ImagingResample: antialiased when reducing, horizontal pass first, intermediate rounded to the element type) for uint8, uint16 and float32, the
case list and the seeded data of tests/test_ingest_cpu.py and tests/test_ingest_gpu.py.  The CPU test holds the restatement to Pillow itself with 0
mismatches; the GPU test holds the kernels to the restatement bit for bit."""
import math

import numpy as np

PRECISION_BITS = 22

# (H, W) -> (h', w')
CASES = [((37, 53), (16, 16)), ((320, 390), (256, 312)), ((5, 7), (11, 13)), ((1, 9), (4, 3)), ((64, 64), (64, 31)), ((257, 129), (32, 32)),
         ((300, 200), (7, 200)), ((2, 2), (64, 64)), ((33, 1000), (33, 10))]
DTYPES = [("u8", 1), ("u8", 3), ("u16", 1), ("f32", 1)]
NP_DTYPE = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}


def coeffs(in_size, out_size):
    """the coefficient table of one axis: fp64 weights [out][ksize] (entries n.. are 0), (xmin, n) [out][2], ksize"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), np.float64)
    bounds = np.zeros((out_size, 2), np.int64)
    ss = 1.0 / fs
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        ww = 0.0
        for x in range(n):
            a = abs((x + xmin - center + 0.5) * ss)
            w = 1.0 - a if a < 1.0 else 0.0
            kk[xx, x] = w
            ww += w
        if ww != 0.0:
            for x in range(n):
                kk[xx, x] /= ww
        bounds[xx] = (xmin, n)
    return kk, bounds, ksize


def fixed(kk):
    """the 22-bit integer coefficients of the 8-bit resampler"""
    out = np.where(kk < 0, -0.5 + kk * (1 << PRECISION_BITS), 0.5 + kk * (1 << PRECISION_BITS))
    return np.trunc(out).astype(np.int64)


def _pass(img, out_size, kind):
    """one pass along axis 1 of img [R, S, C]"""
    kk, b, _ = coeffs(img.shape[1], out_size)
    ki = fixed(kk)
    out = np.zeros((img.shape[0], out_size, img.shape[2]), img.dtype)
    for xx in range(out_size):
        x0, n = b[xx]
        if kind == "u8":
            acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(img[:, x0:x0 + n].astype(np.int64), ki[xx, :n], axes=([1], [0]))
            out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
            continue
        ss = np.zeros((img.shape[0], img.shape[2]), np.float64)
        for x in range(n):
            ss = ss + img[:, x0 + x].astype(np.float64) * kk[xx, x]       # (numpy rounds the product and the sum separately)
        out[:, xx] = ss.astype(np.float32) if kind == "f32" else np.clip(np.floor(ss + 0.5), 0, 65535)
    return out


def resize(img, oh, ow, kind):
    """img [H, W, C] -> [oh, ow, C]: horizontal pass, rounded, then vertical; an axis whose size does not change is skipped"""
    H, W = img.shape[:2]
    t = _pass(img, ow, kind) if ow != W else img
    if oh != H:
        t = _pass(t.transpose(1, 0, 2), oh, kind).transpose(1, 0, 2)
    return np.ascontiguousarray(t)


_DATA, _WANT = {}, {}


def data(case, kind, C, seed=0):
    """seeded noise [H, W, C] whose top half is a random field of the two extreme values: the rounding and the clamp are both exercised"""
    key = (case, kind, C, seed)
    if key not in _DATA:
        (H, W), _ = CASES[case]
        rng = np.random.default_rng(1000 * seed + 10 * case + C + {"u8": 0, "u16": 100, "f32": 200}[kind])
        if kind == "f32":
            a = (rng.standard_normal((H, W, C)) * 1000).astype(np.float32)
            a[:H // 2] = rng.choice(np.array([-3.0e4, 3.0e4], np.float32), (H // 2, W, C))
        else:
            top = 255 if kind == "u8" else 65535
            a = rng.integers(0, top + 1, (H, W, C)).astype(NP_DTYPE[kind])
            a[:H // 2] = rng.choice(np.array([0, top], NP_DTYPE[kind]), (H // 2, W, C))
        a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def want(case, kind, C, seed=0):
    """the restatement's result of a case, computed once and left unchanged"""
    key = (case, kind, C, seed)
    if key not in _WANT:
        oh, ow = CASES[case][1]
        r = resize(data(case, kind, C, seed), oh, ow, kind)
        r.setflags(write=False)
        _WANT[key] = r
    return _WANT[key]


def pil_resize(a, oh, ow, kind):
    """Pillow's own result for a [H, W, C] array: modes L / RGB / I;16 / F, Image.resize(..., BILINEAR)"""
    from PIL import Image
    C = a.shape[2]
    if kind == "u8":
        im = Image.fromarray(a[..., 0], "L") if C == 1 else Image.fromarray(a, "RGB")
    elif kind == "u16":
        im = Image.frombytes("I;16", (a.shape[1], a.shape[0]), np.ascontiguousarray(a[..., 0]).astype("<u2").tobytes())
    else:
        im = Image.fromarray(a[..., 0], "F")
    r = im.resize((ow, oh), Image.BILINEAR)
    if kind == "u16":
        return np.frombuffer(r.tobytes(), "<u2").reshape(oh, ow, 1).astype(np.uint16)
    return np.asarray(r).reshape(oh, ow, C)
