"""The data set's transform on the device: T.Resize (PIL bilinear, antialiased when reducing) -> T.CenterCrop -> T.ToTensor -> T.Normalize(0.5, 0.5)
of the reference's loaders (medical_diffusion/data/datasets/dataset_simple_2d.py:34-45) for a batch of images of ANY sizes: raw bytes, their
descriptors and the coefficient tables go up in one copy, one pair of launches resamples, crops and maps the values (mf_image_resample,
csrc/ingest.hip; the definition is in include/medfusion_hip.h, "dataset transform").  Decoding PNG / JPEG / TIFF files stays on the host (PIL).

Everything up to the copy runs without a device: sizes, crop boxes, tables, the plan and every argument rule."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np
import torch

from . import lib as L

_KINDS = {np.dtype(np.uint8): ("u8", L.INGEST_U8), np.dtype(np.uint16): ("u16", L.INGEST_U16), np.dtype(np.float32): ("f32", L.INGEST_F32)}
_TABLES = {}      # (in, out) -> (ksize, weights f64 [out, ksize], fixed i32 [out, ksize], bounds i32 [out, 2]): built once, kept across calls


def _pair(v, what):
    if isinstance(v, (int, np.integer)):
        return int(v), int(v)
    v = tuple(int(s) for s in v)
    if len(v) == 1:
        return v[0], v[0]
    if len(v) != 2:
        raise ValueError(f"{what}: one size or (h, w), got {v}")
    return v


def resized_size(h, w, resize):
    """torchvision's T.Resize: an int makes the SHORTER side `resize` and the longer int(resize * long / short); (h, w) is taken as it is"""
    if resize is None:
        return int(h), int(w)
    if isinstance(resize, (int, np.integer)) or len(resize) == 1:
        s = int(resize if isinstance(resize, (int, np.integer)) else resize[0])
        if s < 1:
            raise ValueError(f"resize: {s}")
        if w <= h:
            return int(s * h / w), s
        return s, int(s * w / h)
    rh, rw = _pair(resize, "resize")
    if rh < 1 or rw < 1:
        raise ValueError(f"resize: {(rh, rw)}")
    return rh, rw


def center_crop_box(h, w, crop):
    """torchvision's T.CenterCrop of an h x w image -> (top, left, ch, cw); Python's round: a half goes to the even integer.  No padding.
    Four numbers are an explicit box (top, left, ch, cw), returned as it is when it lies in the image."""
    if not isinstance(crop, (int, np.integer)) and len(crop) == 4:      # an explicit box (top, left, ch, cw) of the resized image
        top, left, ch, cw = (int(v) for v in crop)
        if top < 0 or left < 0 or ch < 1 or cw < 1 or top + ch > h or left + cw > w:
            raise ValueError(f"crop: the box {(top, left, ch, cw)} does not lie in the resized image {h} x {w}")
        return top, left, ch, cw
    ch, cw = _pair(crop, "crop")
    if ch < 1 or cw < 1 or ch > h or cw > w:
        raise ValueError(f"crop: {ch} x {cw} does not fit the resized image {h} x {w} (padding crops are not built)")
    return int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0)), ch, cw


def resample_table(n_in, n_out):
    """the coefficient table of one axis (mf_resample_table, host only), cached: (ksize, weights, fixed, bounds)"""
    key = (int(n_in), int(n_out))
    if key not in _TABLES:
        lib = L.load()
        ks = lib.mf_resample_table(key[0], key[1], None, None, None)
        if ks < 0:
            raise ValueError(f"resample_table: {key[0]} -> {key[1]}: {L.last_error()}")
        wf, wi, b = np.zeros((key[1], ks), np.float64), np.zeros((key[1], ks), np.int32), np.zeros((key[1], 2), np.int32)
        L.check(min(lib.mf_resample_table(key[0], key[1], wf.ctypes.data, wi.ctypes.data, b.ctypes.data), 0), "mf_resample_table")
        for a in (wf, wi, b):
            a.setflags(write=False)
        _TABLES[key] = (ks, wf, wi, b)
    return _TABLES[key]


def _kind(dtype):
    try:
        return _KINDS[np.dtype(dtype)]
    except (KeyError, TypeError):
        raise ValueError(f"dtype: uint8, uint16 or float32, got {dtype}") from None


def _up16(n):
    return (n + 15) // 16 * 16


class _Geometry:
    """descriptors, concatenated tables and the plan of one batch (host only)"""

    def __init__(self, shapes, dtype, channels, resize, crop, names=None):
        self.kind, self.dt = _kind(dtype)
        self.C, self.N = int(channels), len(shapes)
        if self.N < 1:
            raise ValueError("shapes: an empty batch")
        if self.C > 3 or self.C < 1:
            raise ValueError(f"channels: {self.C}; 1 or 3 (RGBA is not built)")
        if self.C == 2 or (self.C == 3 and self.kind != "u8"):
            raise ValueError(f"channels: {self.C} channels of {self.kind}; 3 channels are read as uint8 only, 2 not at all")
        esz = np.dtype(dtype).itemsize
        name = (lambda i: str(names[i])) if names is not None else (lambda i: f"image {i}")
        self.descs = (L.MfResampleImage * self.N)()
        placed, wparts, bparts, nw, nb, off, self.out_size = {}, [], [], 0, 0, 0, None
        for i, (H, W) in enumerate(shapes):
            H, W = int(H), int(W)
            if H < 1 or W < 1:
                raise ValueError(f"shapes: {name(i)} is {H} x {W}")
            Hr, Wr = resized_size(H, W, resize)
            if Hr < 1 or Wr < 1:
                raise ValueError(f"resize: {name(i)} ({H} x {W}) would become {Hr} x {Wr}")
            top, left, h, w = (0, 0, Hr, Wr) if crop is None else center_crop_box(Hr, Wr, crop)
            if self.out_size is None:
                self.out_size = (h, w)
            elif (h, w) != self.out_size:
                raise ValueError(f"{name(i)} ({H} x {W}) gives an output of {h} x {w}, {name(0)} one of {self.out_size[0]} x {self.out_size[1]}: "
                                 "every output of a batch must have one size (resize= / crop=)")
            d = self.descs[i]
            d.H, d.W, d.Hr, d.Wr, d.top, d.left = H, W, Hr, Wr, top, left
            off = (off + esz - 1) // esz * esz       # back to back: an image starts at a multiple of its element size, else anywhere
            d.src_off = off
            off += H * W * self.C * esz
            for axis, n_in, n_out in (("h", W, Wr), ("v", H, Hr)):
                if n_in == n_out:
                    continue
                if (n_in, n_out) not in placed:
                    ks, wf, wi, b = resample_table(n_in, n_out)
                    placed[(n_in, n_out)] = (nw, nb, ks)
                    wparts.append(wi if self.kind == "u8" else wf)
                    bparts.append(b)
                    nw, nb = nw + n_out * ks, nb + n_out
                tw, tb, ks = placed[(n_in, n_out)]
                setattr(d, "tw_" + axis, tw), setattr(d, "tb_" + axis, tb), setattr(d, "ksize_" + axis, ks)
        self.src_bytes = off
        self.n_weights, self.n_bounds, self.tables = nw, nb, len(placed)
        wdt = np.int32 if self.kind == "u8" else np.float64
        self.weights = np.concatenate([p.reshape(-1) for p in wparts]) if wparts else np.zeros(0, wdt)
        self.bounds = np.ascontiguousarray(np.concatenate(bparts)) if bparts else np.zeros((0, 2), np.int32)
        self.plan = L.MfResamplePlan()
        h, w = self.out_size
        L.check(L.load().mf_resample_plan(self.descs, self.N, self.C, self.dt, h, w, self.bounds.ctypes.data, nb, nw, self.src_bytes, C.byref(self.plan)),
                "mf_resample_plan")

    @property
    def table_bytes(self):
        return self.weights.nbytes + self.bounds.nbytes


def plan(shapes, resize=None, crop=None, dtype=np.uint8, channels=1):
    """Host only: what transform() of images of these (H, W) would launch -- launches, workgroups of the two passes, workspace / table / source /
    descriptor bytes and the output size."""
    g = _Geometry(list(shapes), dtype, channels, resize, crop)
    return {"launches": g.plan.launches, "workgroups": (g.plan.wg_h, g.plan.wg_v), "workspace_bytes": g.plan.workspace_bytes, "table_bytes": g.table_bytes,
            "tables": g.tables, "source_bytes": g.src_bytes, "descriptor_bytes": C.sizeof(g.descs), "out_size": g.out_size}


class Packed:
    """a batch ready to go up: ONE host buffer (pinned where a device exists) holding the images back to back, their descriptors and the tables"""

    def __init__(self, host, geom, sections, names):
        self.host, self.geom, self.sections, self.names, self.dev = host, geom, sections, names, None

    def to(self, device):
        """upload now and keep the device copy: transform() of this batch then copies nothing"""
        self.dev = self.host.to(torch.device(device), non_blocking=True)
        return self


def _check_arrays(arrays):
    if isinstance(arrays, np.ndarray) or not len(arrays):
        raise ValueError("arrays: a non-empty list of [H, W] / [H, W, C] numpy arrays")
    first = None
    for i, a in enumerate(arrays):
        if not isinstance(a, np.ndarray) or a.ndim not in (2, 3):
            raise ValueError(f"arrays: item {i} is not a [H, W] / [H, W, C] numpy array")
        c = 1 if a.ndim == 2 else a.shape[2]
        if c > 3:
            raise ValueError(f"arrays: item {i} has {c} channels; 1 or 3 (RGBA is not built)")
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError(f"arrays: item {i} is not contiguous")
        if first is None:
            first = (a.dtype, c)
            _kind(a.dtype)
        elif a.dtype != first[0]:
            raise ValueError(f"arrays: mixed dtypes ({first[0]} and {a.dtype} at item {i})")
        elif c != first[1]:
            raise ValueError(f"arrays: mixed channel counts ({first[1]} and {c} at item {i})")
    return first


def pack(arrays, *, resize=None, crop=None, names=None, pin=None):
    """[H, W] / [H, W, C] arrays of one dtype and channel count but any sizes -> Packed: the bytes back to back (an image starts at a multiple of its
    element size, else unaligned), then the descriptors and the tables of this resize / crop.  No device is touched (pin=None pins the buffer when a
    device exists: the copy is then asynchronous)."""
    dtype, c = _check_arrays(arrays)
    g = _Geometry([a.shape[:2] for a in arrays], dtype, c, resize, crop, names=names)
    o_desc = _up16(g.src_bytes)
    o_bounds = o_desc + _up16(C.sizeof(g.descs))
    o_weights = o_bounds + _up16(g.bounds.nbytes)
    total = o_weights + _up16(g.weights.nbytes)
    pin = torch.cuda.is_available() if pin is None else pin
    host = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=bool(pin))
    buf = host.numpy()
    for a, d in zip(arrays, g.descs):
        buf[d.src_off:d.src_off + a.nbytes] = a.reshape(-1).view(np.uint8)
    buf[o_desc:o_desc + C.sizeof(g.descs)] = np.frombuffer(g.descs, np.uint8)
    buf[o_bounds:o_bounds + g.bounds.nbytes] = g.bounds.reshape(-1).view(np.uint8)
    buf[o_weights:o_weights + g.weights.nbytes] = g.weights.view(np.uint8)
    return Packed(host, g, (o_desc, o_bounds, o_weights), names)


def _run(x, resize, crop, mode, out, device, workspace, names):
    if isinstance(x, Packed):
        if resize is not None or crop is not None:
            raise ValueError("resize / crop: a Packed batch carries the geometry pack() was given")
        p = x
    else:
        p = pack(x, resize=resize, crop=crop, names=names)
    g = p.geom
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError("medfusion_amd: tensors must live on a ROCm device -- the product path has no CPU fallback")
    (h, w), n, c = g.out_size, g.N, g.C
    shape, odt = ((n, h, w, c), torch.uint8) if mode == L.INGEST_BYTES else ((n, c, h, w), torch.float32)
    if out is not None and (tuple(out.shape) != shape or out.dtype != odt or not out.is_contiguous() or out.device.type != "cuda"):
        raise ValueError(f"out: a contiguous {odt} tensor of shape {shape} on the device")
    need = int(g.plan.workspace_bytes)
    if workspace is not None and (workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.device.type != "cuda"):
        raise ValueError(f"workspace: a uint8 device tensor of at least {need} bytes")
    from .kernels import stream
    if p.dev is not None and p.dev.device == (device if device.index is not None else torch.device("cuda", torch.cuda.current_device())):
        dev = p.dev
    else:
        dev = p.host.to(device, non_blocking=True)      # the one copy: bytes, descriptors, tables
    if out is None:
        out = torch.empty(shape, dtype=odt, device=device)
    if workspace is None and need:
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
    o_desc, o_bounds, o_weights = p.sections
    base = dev.data_ptr()
    a = L.MfResampleArgs()
    a.src, a.images, a.images_host = base, base + o_desc, C.addressof(g.descs)
    a.weights_f64 = base + o_weights if g.kind != "u8" and g.n_weights else None
    a.weights_i32 = base + o_weights if g.kind == "u8" and g.n_weights else None
    a.bounds, a.bounds_host = (base + o_bounds, g.bounds.ctypes.data) if g.n_bounds else (None, None)
    a.workspace, a.workspace_bytes = (workspace.data_ptr(), workspace.numel()) if need else (None, 0)
    a.out, a.bounds_count, a.weights_count, a.src_bytes = out.data_ptr(), g.n_bounds, g.n_weights, g.src_bytes
    a.N, a.C, a.dtype, a.h, a.w, a.out_mode = n, c, g.dt, h, w, mode
    with torch.cuda.device(device):
        L.check(L.load().mf_image_resample(C.byref(a), stream()), "mf_image_resample")
    return out


def transform(x, *, resize=None, crop=None, normalize="centered", center=True, out=None, device=None, workspace=None, names=None):
    """A list of arrays (or a Packed batch) -> [N, C, h, w] fp32 on the device: resized, cropped and normalised like the reference's loader.
    normalize: "centered" (uint8 / uint16: ((v / full) - 0.5) / 0.5, full = 255 / 65535), "minmax" (the reference's Normalize, (v - min) / (max - min)
    per image over the cropped result, then the centring when center=True) or None (the resampled values).  Every argument rule is checked before
    anything touches the device; `workspace` (plan()'s workspace_bytes, uint8) and `out` may be reused across calls."""
    if normalize not in ("centered", "minmax", None):
        raise ValueError(f"normalize: 'centered', 'minmax' or None, got {normalize!r}")
    kind = x.geom.kind if isinstance(x, Packed) else _kind(_check_arrays(x)[0])[0]
    if normalize == "centered" and kind == "f32":
        raise ValueError("normalize: 'centered' divides by the full scale of an integer type; float32 images take 'minmax' or None")
    mode = L.INGEST_CENTERED if normalize == "centered" else L.INGEST_RAW
    y = _run(x, resize, crop, mode, out, device, workspace, names)
    if normalize == "minmax":
        from . import kernels as K
        n = y.shape[0]
        mm = K.rows_minmax(y)
        with torch.cuda.device(y.device):
            L.check(L.load().mf_minmax_apply_f32(y.data_ptr(), mm.data_ptr(), n, y.numel() // n, int(bool(center)), K.stream()), "mf_minmax_apply_f32")
    return y


def resample_bytes(x, *, resize=None, crop=None, out=None, device=None, workspace=None, names=None):
    """the byte path: uint8 arrays -> [N, h, w, C] uint8 on the device, the resampled and cropped pixels themselves (what PIL's resize returns)"""
    kind = x.geom.kind if isinstance(x, Packed) else _kind(_check_arrays(x)[0])[0]
    if kind != "u8":
        raise ValueError("arrays: the byte path reads uint8 images")
    return _run(x, resize, crop, L.INGEST_BYTES, out, device, workspace, names)


def decode(path, channels):
    """one file -> [H, W, C] array on the host (PIL): 3 channels like the reference's load_item (.convert('RGB')); 1 channel keeps a 16-bit or
    float image's values (uint16 / float32) and reads everything else as 8-bit grey"""
    from PIL import Image
    with Image.open(path) as img:
        if channels == 3:
            arr = np.asarray(img.convert("RGB"), dtype=np.uint8)
        elif channels != 1:
            raise ValueError(f"channels: {channels}; 1 or 3")
        elif img.mode in ("I;16", "I;16L", "I;16B", "I;16N"):
            arr = np.asarray(img).astype(np.uint16)
        elif img.mode == "F":
            arr = np.asarray(img, dtype=np.float32)
        else:
            arr = np.asarray(img.convert("L"), dtype=np.uint8)
    return np.ascontiguousarray(arr[..., None] if arr.ndim == 2 else arr)


def list_images(folder, exts=None):
    """the files of a folder by name; exts=None: *.png, as the harnesses always listed them"""
    folder = Path(folder)
    if exts is None:
        return sorted(folder.glob("*.png"))
    want = {"." + e.lower().lstrip(".") for e in exts}
    return sorted(f for f in folder.iterdir() if f.is_file() and f.suffix.lower() in want)


class ImageFolder:
    """Iterates (batch [n, C, h, w] fp32 on the device, file names) over a folder of images of any sizes and formats: PIL decodes on the host, the
    transform runs on the device."""

    def __init__(self, path, exts=("png", "jpg", "jpeg", "tif", "tiff"), channels=3, resize=None, crop=None, batch=16, normalize="centered", center=True,
                 device=None):
        self.files = list_images(path, exts)
        if not self.files:
            raise ValueError(f"path: no {'/'.join(exts)} files in {path}")
        self.channels, self.resize, self.crop, self.batch, self.normalize, self.center, self.device = channels, resize, crop, int(batch), normalize, center, device

    def __len__(self):
        return (len(self.files) + self.batch - 1) // self.batch

    def __iter__(self):
        for lo in range(0, len(self.files), self.batch):
            chunk = self.files[lo:lo + self.batch]
            arrays = [decode(f, self.channels) for f in chunk]
            yield transform(arrays, resize=self.resize, crop=self.crop, normalize=self.normalize, center=self.center, device=self.device,
                            names=[f.name for f in chunk]), [f.name for f in chunk]


# ----------------------------------------------------------------------------- the harnesses' shared flags
def add_ingest_arguments(ap):
    """--resize / --crop / --ext of the scripts that read a folder of images; without them a script reads *.png of one size as before"""
    ap.add_argument("--resize", type=int, nargs="+", default=None, metavar="S",
                    help="resize every image on the device like the reference's loader (PIL bilinear): one size = the shorter side, two = height width")
    ap.add_argument("--crop", type=int, nargs="+", default=None, metavar="S", help="then centre-crop to this size (one size, or height width)")
    ap.add_argument("--ext", nargs="+", default=None, help="file extensions to read (default: png); with --resize / --crop the sizes may differ")


def ingest_requested(args):
    return getattr(args, "resize", None) is not None or getattr(args, "crop", None) is not None


def _size_arg(v):
    return None if v is None else (v[0] if len(v) == 1 else tuple(v))


def load_batch(files, channels, device, args=None, loader=None):
    """files -> [n, C, h, w] fp32 in [-1, 1] on the device.  Without --resize / --crop: the bytes of equal-sized images through mf_image_ingress_u8,
    exactly as before; with them: images of any sizes through the transform."""
    from . import kernels as K
    if args is None or not ingest_requested(args):
        load = loader or decode
        return K.image_ingress(torch.from_numpy(np.stack([load(f, channels) for f in files])).to(device))
    arrays = [decode(f, channels) for f in files]
    return transform(arrays, resize=_size_arg(args.resize), crop=_size_arg(args.crop), device=device, names=[Path(f).name for f in files])


def load_mask(path, device, args=None, loader=None):
    """a mask file -> uint8 [1, 1, h, w] on the device (non-zero = regenerate); with --resize / --crop it takes the images' transform (bilinear; a
    mask is thresholded after: a pixel the resampler leaves above zero is regenerated)"""
    if args is None or not ingest_requested(args):
        load = loader or decode
        return torch.from_numpy(load(path, 1)[..., 0].copy())[None, None].to(device)
    m = resample_bytes([decode(path, 1)], resize=_size_arg(args.resize), crop=_size_arg(args.crop), device=device, names=[Path(path).name])
    return m.permute(0, 3, 1, 2).contiguous()
