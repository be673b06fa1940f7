"""Tensor-level wrappers over the C-ABI.  torch is plumbing only: device memory, streams.

Activations inside the path are NHWC torch tensors of shape [N, H, W, C] (contiguous).  Every wrapper
launches on torch's current stream and raises if a tensor is not on the GPU -- there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import lib as L


def _gpu(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("medfusion_amd: tensors must live on a ROCm device -- the product path has no CPU fallback")
        if t.dtype not in (torch.float32, torch.float64, torch.int64, torch.int32, torch.uint8, torch.int16):
            raise RuntimeError(f"medfusion_amd: unsupported dtype {t.dtype}")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def stream(device_index: Optional[int] = None) -> int:
    """the hipStream_t torch launches on right now (current device, or `device_index`): the raw C entry points when this torch has them --
    `torch.cuda.current_stream()` builds a Stream object per call, a quarter of the host time of a launch (scripts/host_profile.py)"""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device() if device_index is None else device_index)
    return (torch.cuda.current_stream() if device_index is None else torch.cuda.current_stream(device_index)).cuda_stream


_growths = 0   # how often a Workspace / SyncWords buffer was (re)allocated: the command-list recorder compares before / after (pipeline.py)


def scratch_growth_count() -> int:
    return _growths


class _StreamBuf:
    """A grow-only buffer per (device, stream), owned by torch (the library never allocates): launches on one stream are serialised, so sharing is
    safe; concurrent streams must not share scratch.  Grown -- zeroed again where `zeroed` -- outside graph capture only (the eager warm-up run does it);
    every growth is counted (scratch_growth_count).  Subclasses: what the buffer is called in the error, its smallest size, its element type."""
    what, floor, dtype, zeroed = "", 0, torch.uint8, False

    @classmethod
    def get(cls, size: int, device) -> torch.Tensor:
        key = (device.index, stream(device.index))
        buf = cls._bufs.get(key)
        if buf is None or buf.numel() < size:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"medfusion_amd: {cls.what} growth during graph capture; run one eager warm-up first")
            buf = cls._bufs[key] = (torch.zeros if cls.zeroed else torch.empty)(max(size, cls.floor), dtype=cls.dtype, device=device)
            global _growths
            _growths += 1
        return buf


class Workspace(_StreamBuf):
    """Scratch bytes: split-K slabs and hand-off regions, the Winograd GEMM's output in the transform domain."""
    _bufs, what, floor = {}, "workspace", 1 << 20


class SyncWords(_StreamBuf):
    """Zero-initialised 32-bit counters the in-launch split-K reduction of mf_conv2d_f16x2 meets through (every launch leaves them zero)."""
    _bufs, what, floor, dtype, zeroed = {}, "sync-counter", 1 << 14, torch.int32, True

    @classmethod
    def reset(cls, device) -> None:
        """Zero the counters of the current stream again (one memset): a launch that died half-way -- a device fault, an interrupted
        process -- would otherwise leave a pair's counter at 1 and the next launch would take a stale tile.  Called once per sampling loop /
        VAE pass, never per launch."""
        buf = cls._bufs.get((device.index, stream(device.index)))
        if buf is not None and not torch.cuda.is_current_stream_capturing():
            buf.zero_()


class Rendezvous(_StreamBuf):
    """Counters of the convolutions that apply their GroupNorm inside their own launch (mf_conv2d_f16x2_gn_apply): word 0 is the ERROR FLAG
    (a wait that did not complete: another process's waiting workgroups filled the device), the [N][2] arrive / depart counters start at
    word 4.  One array per (device, stream); zero before the first launch, left zero by every launch.  `failed(device)` reads the flags of
    the device (a host sync): DiffusionPipeline checks once per sampling loop, VAE once per pass, and on a hit zero everything, switch the
    fused form off for the process (`disabled`) and re-run on the two-launch form."""

    _bufs, what, floor, dtype, zeroed = {}, "rendezvous-counter", 1 << 12, torch.int32, True
    # OPT-IN (MEDFUSION_FUSED_APPLY=1): built, bit-identical to the two-launch form, and measured NOT faster -- same-process A/B on cfg2,
    # profiles/r04_fused_gn_apply_ab.txt: -0.2 % (fused at 32 x 32 only) ... -2.2 % (everywhere); the tail costs what the boundary + the
    # apply launch cost (profiles/r04_conv_timeline_fused.txt).  So the default is the two-launch form, which also never waits in a kernel.
    disabled = os.environ.get("MEDFUSION_FUSED_APPLY", "0") != "1"
    used = {}          # device index -> a fused launch went out since the last check
    launches = 0       # fused launches issued by this process (tests, diagnostics)

    @classmethod
    def get(cls, words: int, device) -> torch.Tensor:
        buf = super().get(words + 4, device)
        cls.used[device.index] = True
        cls.launches += 1
        return buf

    @classmethod
    def failed(cls, device) -> bool:
        """did a rendezvous of this device time out since the last check?  (host sync; clears flag and counters on a hit)"""
        if not cls.used.get(device.index):
            return False
        cls.used[device.index] = False
        torch.cuda.synchronize(device)   # (every stream of the device: .item() below would wait for the current one only)
        bad = False
        for (di, _), buf in list(cls._bufs.items()):
            if di == device.index and int(buf[0].item()) != 0:
                bad = True
        if bad:
            for (di, _), buf in list(cls._bufs.items()):
                if di == device.index:
                    buf.zero_()
        return bad


# Policy (blocks.py): a convolution applies its GroupNorm itself only from this many output pixels per sample on.  Below, the tiles of a
# sample finish too far apart (deep in-launch split-K trees at 8 x 8) for the wait to beat a separate apply launch (scripts/conv_timeline.py
# --fused, profiles/r04_conv_timeline_fused.txt).  The C-ABI query (mf_conv2d_f16x2_fuse_words) answers capability only.
FUSE_MIN_HW = int(os.environ.get("MEDFUSION_FUSE_MIN_HW", "256"))
_fused = __import__("threading").local()   # .depth: nesting of with_fused_fallback on THIS thread (two threads may drive two streams)


def with_fused_fallback(device, fn, rewind=None):
    """Run fn() -- a whole sampling loop, a VAE pass -- and, if one of the convolutions that apply their GroupNorm inside their own launch
    timed out waiting for its sample (Rendezvous: only when another process's waiting workgroups fill the device), switch that form off for
    the process, call `rewind()` (restore whatever fn consumed: noise counters) and run fn() again on the two-launch form.  Nested calls
    (the decode inside a sampling loop) leave the check to the outermost one: a failure anywhere invalidates everything after it."""
    if getattr(_fused, "depth", 0) > 0 or Rendezvous.disabled or torch.cuda.is_current_stream_capturing():
        return fn()
    _fused.depth = 1
    try:
        out = fn()
    finally:
        _fused.depth = 0
    if Rendezvous.failed(device):
        import warnings
        Rendezvous.disabled = True
        warnings.warn("medfusion_amd: a convolution's in-launch GroupNorm rendezvous timed out (the device is shared with another process whose "
                      "workgroups were waiting too); the fused form is switched off for this process and the pass is re-run on the two-launch form")
        if rewind is not None:
            rewind()
        SyncWords.reset(device)
        out = fn()
    return out


def pack_conv_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """OIHW -> [Cout][KH][KW][Cin] (device, once at load)."""
    _gpu(w_oihw)
    w = w_oihw.contiguous()
    co, ci, kh, kw = w.shape
    out = torch.empty((co, kh, kw, ci), dtype=torch.float32, device=w.device)
    L.check(L.load().mf_pack_conv_weight_f32(w.data_ptr(), out.data_ptr(), co, ci, kh, kw, stream()), "mf_pack_conv_weight_f32")
    return out


def pack_upconv_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """OIHW 3x3 -> [4 phases][Cout][2][2][Cin]: weights of the sub-pixel form of nearest-x2 + 3x3 conv."""
    _gpu(w_oihw)
    w = w_oihw.contiguous()
    co, ci, kh, kw = w.shape
    assert (kh, kw) == (3, 3)
    out = torch.empty((4, co, 2, 2, ci), dtype=torch.float32, device=w.device)
    L.check(L.load().mf_pack_upconv_weight_f32(w.data_ptr(), out.data_ptr(), co, ci, stream()), "mf_pack_upconv_weight_f32")
    return out


def subpixel_ok(d: L.MfConvDesc) -> bool:
    return bool(L.load().mf_conv2d_subpixel_ok(C.byref(d)))


def conv_is_igemm(d: L.MfConvDesc) -> bool:
    return bool(L.load().mf_conv2d_is_igemm(C.byref(d)))


def split_conv_weight(w_packed: torch.Tensor) -> torch.Tensor:
    """packed fp32 weights (either packing; rows = all leading dims but the K = kh*kw*cin of the last three) -> the bf16-triplet
    form of MF_CONV_FP32_SPLIT3_W3: [rows][K/8][3][8] bf16 as an opaque int16 tensor [rows, 3K]."""
    _gpu(w_packed)
    w = w_packed.contiguous()
    k = w.shape[-1] * w.shape[-2] * w.shape[-3]
    rows = w.numel() // k
    out = torch.empty((rows, 3 * k), dtype=torch.int16, device=w.device)
    L.check(L.load().mf_split_conv_weight_bf16x3(w.data_ptr(), out.data_ptr(), rows, k, stream()), "mf_split_conv_weight_bf16x3")
    return out


# ----------------------------------------------------------------------------- fp16-pair operands (MF_CONV_FP32_F16X2)
# The fp16-pair form of an activation travels as attributes of the fp32 tensor it mirrors: `t._mf_split` (an int32 tensor of the same
# shape) and `t._mf_bound` (float [N]: the per-sample upper bound of |t| whose exponent scaled the pairs -- fp16 stops at 65504, an
# un-normalised residual stream does not; csrc/split_f16.h).  Producers that know a bound for free set both (gn_apply(split=True)); the
# fp16-pair convolution can MEASURE the bound of its output (measure_out=True); a consumer that finds neither runs the stand-alone
# passes (max |t| per sample, then the split) once and caches the result on the tensor.  Every wrapper that writes INTO an existing
# tensor (`out=`) drops stale mirrors first.
# Bound-slack audit (diagnostic, MEDFUSION_AUDIT_BOUNDS=1 or kernels.AUDIT = True; tests/test_parity_gpu.py::test_trained_like_weights_and_bound_slack):
# every producer that attaches an fp16-pair mirror under a DERIVED bound records (site, shape, bound / true max per sample) in AUDIT_LOG.  A derived
# bound sits above the data (the pair format keeps its 23 bits down to 2^-28 of the bound); the audit shows by how much, across a whole network.
AUDIT = os.environ.get("MEDFUSION_AUDIT_BOUNDS", "0") == "1"
AUDIT_LOG = []


def _audit(t: torch.Tensor, site: str) -> None:
    """diagnostic only (torch arithmetic, a host sync): decode the pair mirror of `t`, compare its per-sample max with the bound it was scaled by"""
    if not AUDIT or getattr(t, "_mf_split", None) is None or getattr(t, "_mf_bound", None) is None or torch.cuda.is_current_stream_capturing():
        return
    n = t.shape[0]
    raw = t._mf_split.view(torch.float16).reshape(n, -1, 2, 8).float()
    bound = t._mf_bound.double()
    s = torch.floor(torch.log2(bound.clamp_min(1e-300))) - 14
    amax = (raw[:, :, 0] + raw[:, :, 1] / 2048.0).abs().amax(dim=(1, 2)).double() * torch.exp2(s)
    slack = (bound / amax.clamp_min(1e-300)).cpu()
    AUDIT_LOG.append((site, tuple(t.shape), float(slack.max()), float(slack.min()), bool(torch.isfinite(raw).all())))


def _stamp(t: torch.Tensor) -> None:
    """remember the tensor's version counter next to its mirrors: a torch in-place op on `t` bumps `_version`, and stale() sees it (writes
    through this library go by raw pointer and do not: every wrapper that writes INTO an existing tensor calls drop_split itself)"""
    t._mf_ver = t._version


def stale(t: torch.Tensor) -> bool:
    return getattr(t, "_mf_ver", None) is not None and t._mf_ver != t._version


def _fresh(t: torch.Tensor, name: str):
    """attribute `name` of t (a mirror), or None -- dropping every mirror first when a torch in-place op has touched t since they were made"""
    if stale(t):
        if getattr(t, "_mf_pairs_only", False):
            # the pairs are the ONLY valid copy of this tensor (its fp32 storage was never written): a torch in-place op on it has just
            # modified garbage, and dropping the mirror would make every later reader take that garbage for the values
            raise RuntimeError("medfusion_amd: a torch in-place op touched a tensor that exists only as fp16 pairs (the output of a GroupNorm-apply "
                               "pass between two convolutions); its fp32 storage holds no values")
        drop_split(t)
        t._mf_ver = None
    return getattr(t, name, None)


def pairs_only(t) -> bool:
    """this tensor's values exist only in its fp16-pair mirror (gn_apply(out_fp32=False)): its fp32 storage was never written"""
    return t is not None and getattr(t, "_mf_pairs_only", False)


def _need_f32(*ts):
    for t in ts:
        if pairs_only(t):
            raise RuntimeError("medfusion_amd: this tensor exists only as fp16 pairs (the output of a GroupNorm-apply pass between two convolutions); "
                               "its fp32 form was never written -- only the fp16-pair convolution and the apply pass (as a residual) can read it")


def _f32(what: str, *ts):
    """the entry reads and writes these by raw pointer as floats (_gpu lets the other dtypes of the library through)"""
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"medfusion_amd: {what}: fp32 tensors only, got {t.dtype}")


_DTYPE_NAMES = {torch.float32: "fp32", torch.float64: "fp64", torch.int64: "int64", torch.int32: "int32"}


def _dense(what: str, name: str, t, dtype=torch.float32, shape=None, dim: Optional[int] = None, contiguous: bool = True, written: bool = False) -> None:
    """`t` is read or written by raw pointer as `dtype`: refuse another dtype, a tensor that exists only as fp16 pairs, a strided view
    (contiguous=False: the wrapper copies) and -- where given -- another rank or shape.  Pure host logic: the check_* functions below are built
    from it and take CPU tensors as well (tests/test_edge_cpu.py); every wrapper calls its check before _gpu and before any launch."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"medfusion_amd: {what}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise RuntimeError(f"medfusion_amd: {what}: {name} must be {_DTYPE_NAMES[dtype]}, got {t.dtype}")
    if dtype == torch.float32 and not written:      # (written: an output that is only written may be pairs-only storage; drop_split hands it to the writer)
        _need_f32(t)
    if contiguous and not t.is_contiguous():
        raise RuntimeError(f"medfusion_amd: {what}: {name} must be contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
    if dim is not None and t.dim() != dim:
        raise RuntimeError(f"medfusion_amd: {what}: {name} must have {dim} dimensions, got shape {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"medfusion_amd: {what}: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")


# every mirror attribute a producer may attach (_attach) and a writer must drop (drop_split).  Not mirrors, and left alone by drop_split: `_mf_ver` (the
# stamp; _fresh clears it), `_mf_wino_site` / `_mf_wino_site_f32` (where to report a wanted transform: they describe the producer, not the values);
# `_mf_pairs_only` is a flag of the storage that drop_split clears by its own rule.  A new mirror kind goes HERE (tests/test_host_logic_cpu.py checks)
MIRRORS = ("_mf_split", "_mf_bound", "_mf_slots", "_mf_wino", "_mf_wino_bound", "_mf_wino_f32")


def drop_split(t: Optional[torch.Tensor]) -> None:
    if t is not None:
        attrs = t.__dict__   # (the tensor's Python attributes: most tensors written into carry none, and this runs per launch)
        if attrs:
            if attrs.get("_mf_pairs_only"):
                attrs["_mf_pairs_only"] = False   # (an fp32 writer is about to fill the storage)
            for name in MIRRORS:
                if attrs.get(name) is not None:
                    attrs[name] = None


def _attach(t: torch.Tensor, site: Optional[str] = None, split=None, bound=None, slots=None, wino=None, wino_f32=None, pairs_only: bool = False) -> torch.Tensor:
    """Attach the mirrors a producer has just made to its tensor `t` -- split (fp16 pairs) / bound / slots (slot maxima, a bound still to be reduced) / wino
    = (V as pairs, its bounds) / wino_f32 (V in fp32); None: not produced -- and stamp t's version next to them.  site: the producer scaled the pairs by
    a bound of its own: the text under which the bound-slack audit records it (None: nothing to audit).  pairs_only: t's fp32 storage was never written"""
    if split is not None:
        t._mf_split = split
    if bound is not None:
        t._mf_bound = bound
    if slots is not None:
        t._mf_slots = slots
    if wino is not None:
        t._mf_wino, t._mf_wino_bound = wino
    if wino_f32 is not None:
        t._mf_wino_f32 = wino_f32
    t._mf_ver = t._version   # (_stamp)
    if AUDIT and site is not None:
        _audit(t, site)
    if pairs_only:
        t._mf_pairs_only = True
    return t


def maxabs_rows(x: torch.Tensor) -> torch.Tensor:
    """x [N, ...] contiguous fp32 -> bound [N] = max |x[n]| (measured on the device: two small launches, no atomics, no host sync)"""
    _gpu(x)
    _need_f32(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise RuntimeError("maxabs_rows: contiguous fp32")
    n = x.shape[0]
    lib = L.load()
    per = x.numel() // n
    partial = torch.empty((n, lib.mf_maxabs_rows_slots(per)), dtype=torch.float32, device=x.device)
    bound = torch.empty((n,), dtype=torch.float32, device=x.device)
    L.check(lib.mf_maxabs_rows_f32(x.data_ptr(), partial.data_ptr(), bound.data_ptr(), n, per, stream()), "mf_maxabs_rows_f32")
    return bound


def bound_of(x: torch.Tensor) -> torch.Tensor:
    b = _fresh(x, "_mf_bound")
    if b is None:
        sl = _fresh(x, "_mf_slots")
        if sl is not None:   # per-(tile, wave) maxima the producing convolution left: one wave per sample reduces them
            b = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
            L.check(L.load().mf_bound_finalize_f32(sl.data_ptr(), b.data_ptr(), sl.shape[0], sl.shape[1], stream()), "mf_bound_finalize_f32")
        else:
            b = maxabs_rows(x)
        _attach(x, bound=b)
    return b


def split_f16x2(x: torch.Tensor, bound: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 tensor [N, ...] (innermost extent % 8 == 0) -> its fp16-pair form, an opaque int32 tensor of the same shape; row n is scaled
    by the power of two that `bound[n]` implies (None: unscaled)"""
    _gpu(x, bound)
    _need_f32(x)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.shape[-1] % 8:
        raise RuntimeError("split_f16x2: contiguous fp32 with innermost extent % 8 == 0")
    rows = x.shape[0] if bound is not None else 1
    if bound is not None and bound.numel() != rows:
        raise RuntimeError("split_f16x2: one bound per leading index")
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    L.check(L.load().mf_split_f16x2(x.data_ptr(), out.data_ptr(), _ptr(bound), rows, x.numel() // rows, stream()), "mf_split_f16x2")
    return out


def split_of(x: torch.Tensor) -> torch.Tensor:
    s = _fresh(x, "_mf_split")
    if s is None:
        b = None
        if _fresh(x, "_mf_bound") is None and x.dim() >= 2 and x.shape[-1] % 8 == 0 and x.is_contiguous() and x.dtype == torch.float32:
            # no bound yet: the slot maxima the producing convolution left -- or those of a measuring pass -- are reduced inside the split
            # itself (mf_split_f16x2_slots: no bound-finalize launch), which publishes the bound as well
            _need_f32(x)
            lib = L.load()
            n, per = x.shape[0], x.numel() // x.shape[0]
            sl = _fresh(x, "_mf_slots")
            if sl is None:
                sl = torch.empty((n, lib.mf_maxabs_rows_slots(per)), dtype=torch.float32, device=x.device)
                L.check(lib.mf_maxabs_rows_f32(x.data_ptr(), sl.data_ptr(), None, n, per, stream()), "mf_maxabs_rows_f32")
            s = torch.empty(x.shape, dtype=torch.int32, device=x.device)
            b = torch.empty((n,), dtype=torch.float32, device=x.device)
            L.check(lib.mf_split_f16x2_slots(x.data_ptr(), s.data_ptr(), sl.data_ptr(), sl.shape[1], b.data_ptr(), n, per, stream()), "mf_split_f16x2_slots")
        else:
            s = split_f16x2(x, bound_of(x))
        _attach(x, "split of a measured tensor", split=s, bound=b)
    return s


def _pair_operands(x1: torch.Tensor, x2: Optional[torch.Tensor]):
    """(pairs of x1, bound of x1, pairs of x2, bound of x2) -- the operands of an fp16-pair convolution of x1 | x2, made on demand; x2 may be None"""
    if x2 is None:
        return split_of(x1), bound_of(x1), None, None
    return split_of(x1), bound_of(x1), split_of(x2), bound_of(x2)


def _tail_operands(residual: Optional[torch.Tensor], emb: Optional[torch.Tensor], bounds: bool = True, slots: bool = True, pairs: bool = True):
    """What a GroupNorm tail / apply pass reads besides its input: (fp32 pointer of the residual, its pairs, its bound, its slot maxima, the bound of the
    embedding rows).  A residual that exists as pairs only is read from them (pairs=False: this pass cannot -- _need_f32 raises); one whose bound is
    still the slot maxima of the convolution that measured it hands those over (slots=False: this pass cannot reduce them -- bound_of does);
    bounds=False: the pass emits no pair mirror and needs no bound.  Call BEFORE the output may alias the residual: the bounds describe what is READ."""
    res_pairs = rb = rslots = eb = None
    if pairs_only(residual):
        if not pairs:
            _need_f32(residual)
        res_pairs, rb = residual._mf_split, bound_of(residual)
    elif residual is not None and bounds:
        if slots and _fresh(residual, "_mf_bound") is None and _fresh(residual, "_mf_slots") is not None:
            rslots = residual._mf_slots
        else:
            rb = bound_of(residual)
    if emb is not None and bounds:
        eb = _fresh(emb, "_mf_bound")
        if eb is None:
            eb = maxabs_rows(emb.contiguous())
    return (None if res_pairs is not None else _ptr(residual)), res_pairs, rb, rslots, eb


def _pair_outputs(shape, dev, wino: Optional[bool] = None):
    """uninitialised (fp32 NHWC output, its pair mirror, its bound [N]) and -- wino given -- (V of the output for the next Winograd convolution, its bounds
    [16 N]), both None unless wanted"""
    n, h, w, c = shape
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    outs = torch.empty(shape, dtype=torch.int32, device=dev)
    ob = torch.empty((n,), dtype=torch.float32, device=dev)
    if wino is None:
        return out, outs, ob
    ov = torch.empty((16, n, (h // 2) * (w // 2), c), dtype=torch.int32, device=dev) if wino else None
    ovb = torch.empty((16 * n,), dtype=torch.float32, device=dev) if wino else None
    return out, outs, ob, ov, ovb


def _scratch(dev, need: int, words: int, need_g: Optional[int] = None, words_g: int = 0, wino: bool = False):
    """Device pointers to the scratch of one launch: (workspace of `need` bytes, `words` sync counters) and -- need_g given: a guest convolution shares the
    launch -- (the guest's workspace, the guest's counters): its region lies behind the host's at the next multiple of 256 bytes, its counters behind the
    host's.  None where a convolution needs none.  wino: the host is a Winograd component GEMM, whose workspace is never empty (its output in the
    transform domain) and which is handed the counter array whenever the launch has one"""
    off = (need + 255) & ~255
    total, wtotal = (need, words) if need_g is None else (off + need_g, words + words_g)
    ws = Workspace.get(total, dev).data_ptr() if (wino or total) else None
    sync = SyncWords.get(wtotal, dev).data_ptr() if wtotal else None
    host = (ws if (wino or need) else None, sync if (wino or words) else None)
    if need_g is None:
        return host
    return (*host, ws + off if need_g else None, sync + 4 * words if words_g else None)


def split_weight_f16x2(w_packed: torch.Tensor):
    """packed fp32 conv weights -> (fp16-pair form scaled by their own max, that max as a float); load-time work (one host sync)"""
    if torch.cuda.is_current_stream_capturing():
        #  the split needs max |w| on the HOST: a weight tensor whose first use falls inside a graph capture -- a shape first seen there
        # -- cannot be packed; every loop form runs its first iteration eagerly for exactly this reason
        raise RuntimeError("medfusion_amd: conv weights must be packed (a host sync) before a hipGraph capture starts: run one eager evaluation of this "
                           "input shape first (DiffusionPipeline.denoise does: its iteration 0 is eager in every loop form)")
    w = w_packed.contiguous()
    wmax = float(w.abs().max().item())
    bound = torch.full((1,), wmax, dtype=torch.float32, device=w.device)
    return split_f16x2(w.view(1, -1), bound).view(w.shape), wmax


def conv_f16x2_ok(d: L.MfConvDesc) -> bool:
    return bool(L.load().mf_conv2d_f16x2_ok(C.byref(d)))


def conv_plan(d: L.MfConvDesc):
    """(tile id, split-K factor) the planner picks for `d`; (0, 0) if it is not on an implicit-GEMM kernel"""
    t, k = C.c_int32(), C.c_int32()
    L.check(L.load().mf_conv2d_plan_query(C.byref(d), C.byref(t), C.byref(k)), "mf_conv2d_plan_query")
    return t.value, k.value


def pin_conv_plan(d: L.MfConvDesc):
    """Fix the planner's choice for `d` in its hint fields (later calls with this descriptor skip the table lookup and the cost model) and
    return what a caller needs per launch: (workspace bytes, slots of the measured-bound array, sync words of an in-launch split-K)."""
    lib = L.load()
    if d.precision in (5, 6) and not (d.tile_hint and d.splitk_hint):
        t, k = conv_plan(d)
        if t > 0 and k > 0:
            d.tile_hint, d.splitk_hint = t, k
    return (lib.mf_conv2d_workspace_bytes(C.byref(d)), (lib.mf_conv2d_f16x2_bound_slots(C.byref(d)) if d.precision in (5, 6) else 0),
            (lib.mf_conv2d_f16x2_sync_words(C.byref(d)) if d.precision in (5, 6) else 0))


def conv2d_f16x2(x1: torch.Tensor, w_split, bias: Optional[torch.Tensor], d: L.MfConvDesc, x2: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, measure_out: bool = False, gn_groups: int = 0, gn_parts: int = 0, pinned=None):
    """MF_CONV_FP32_F16X2 (d.precision = 5; or the opt-in single-term MF_CONV_F16 = 6) convolution of fp32 NHWC tensors whose fp16-pair
    mirrors are made on demand.  w_split = split_weight_f16x2(...).
    measure_out: also measure the per-sample max |y| (-> y._mf_bound: the output feeds a convolution or a residual add un-normalised).
    pinned: pin_conv_plan(d), computed once by callers that launch the same descriptor every iteration.
    Returns y, or (y, partial [N, parts, G, 2]) when gn_groups > 0 (statistics of the GroupNorm that follows)."""
    check_conv2d("conv2d_f16x2", x1, x2, w_split[0], bias, out, d)
    wh, wmax = w_split
    _gpu(x1, x2, wh, bias)
    lib = L.load()
    x1s, b1, x2s, b2 = _pair_operands(x1, x2)
    ho, wo = conv_out_hw(d)
    if out is None:
        out = torch.empty((d.N, ho, wo, d.Cout), dtype=torch.float32, device=x1.device)
    else:
        drop_split(out)
    if pinned is None:
        pinned = (lib.mf_conv2d_workspace_bytes(C.byref(d)), lib.mf_conv2d_f16x2_bound_slots(C.byref(d)) if measure_out and not gn_groups else 0,
                  lib.mf_conv2d_f16x2_sync_words(C.byref(d)))
    need, slots, words = pinned
    if not measure_out or gn_groups:
        slots = 0
    yb = torch.empty((d.N, slots), dtype=torch.float32, device=x1.device) if slots else None
    partial = torch.empty((d.N, gn_parts, gn_groups, 2), dtype=torch.float64, device=x1.device) if gn_groups else None
    ws, sync = _scratch(x1.device, need, words)
    rc = lib.mf_conv2d_f16x2(x1s.data_ptr(), _ptr(x2s), wh.data_ptr(), _ptr(bias), out.data_ptr(), b1.data_ptr(), _ptr(b2), wmax, _ptr(yb), ws, need,
                             sync, _ptr(partial), gn_groups, C.byref(d), stream())
    L.check(rc, "mf_conv2d_f16x2")
    if slots:   # per-(tile, wave) maxima: reduced to the bound of each sample by the first consumer that asks (bound_of), or inside the
        _attach(out, slots=yb)   # GroupNorm-apply pass that takes this tensor as its residual (without slots a consumer measures on demand)
    return (out, partial) if gn_groups else out


def conv_group_ok(da: L.MfConvDesc, Ga: int, db: L.MfConvDesc, Gb: int) -> bool:
    """can the two fp16-pair convolutions share one launch (mf_conv2d_f16x2_group_ok)?"""
    return bool(L.load().mf_conv2d_f16x2_group_ok(C.byref(da), Ga, C.byref(db), Gb))


def conv2d_f16x2_group(x1: torch.Tensor, x2: Optional[torch.Tensor], a, b):
    """TWO independent fp16-pair convolutions of the same input (x1 | x2) in ONE launch (mf_conv2d_f16x2_group): a = the large one, followed by a
    GroupNorm -- dict(w_split, bias, d, gn_groups, gn_parts, pinned) -> (y, partial records) --, b = the small one whose output is measured --
    dict(w_split, bias, d, pinned) -> y with its bound slots attached.  Bit for bit what conv2d_f16x2(.., gn_groups=..) and
    conv2d_f16x2(.., measure_out=True) return."""
    _gpu(x1, x2, a["w_split"][0], b["w_split"][0], a["bias"], b["bias"])
    dev = x1.device
    ops = _pair_operands(x1, x2)
    (need_a, _, words_a), (need_b, _, words_b) = a["pinned"], b["pinned"]
    ws_a, sync_a, ws_b, sync_b = _scratch(dev, need_a, words_a, need_b, words_b)   # b's hand-off region behind a's, its counters behind a's
    G, parts = a["gn_groups"], a["gn_parts"]
    partial = torch.empty((a["d"].N, parts, G, 2), dtype=torch.float64, device=dev)
    ca, ya = _conv_call(ops, a, ws_a, sync_a, dev, partial=partial, G=G)
    cb, yb = _conv_call(ops, b, ws_b, sync_b, dev, measured=True)
    L.check(L.load().mf_conv2d_f16x2_group(C.byref(ca), C.byref(cb), stream()), "mf_conv2d_f16x2_group")
    return (ya, partial), yb


def _conv_call(ops, c, ws, sync, dev, partial=None, G: int = 0, measured: bool = False):
    """One member of a launch that several convolutions share, as (its MfConvF16x2Call record, the output the record points at).  ops = _pair_operands
    of the common input, c = dict(w_split, bias, d, pinned, ...) as conv2d_f16x2_group documents, ws / sync = its pointers from _scratch.
    measured: the output carries the slot maxima of its bound (the plan permitting: pinned[1] slots), like conv2d_f16x2(measure_out=True)"""
    x1s, b1, x2s, b2 = ops
    wh, wmax = c["w_split"]
    d = c["d"]
    need, nslots, _ = c["pinned"]
    ho, wo = conv_out_hw(d)
    y = torch.empty((d.N, ho, wo, d.Cout), dtype=torch.float32, device=dev)
    slots = torch.empty((d.N, nslots), dtype=torch.float32, device=dev) if measured and nslots else None
    call = L.MfConvF16x2Call(x1s.data_ptr(), _ptr(x2s), wh.data_ptr(), _ptr(c["bias"]), y.data_ptr(), b1.data_ptr(), _ptr(b2), wmax, _ptr(slots),
                             ws, need, sync, _ptr(partial), G, C.pointer(d))
    if slots is not None:
        _attach(y, slots=slots)
    return call, y


def check_pack_nchw_pairs(x_nchw, cp: int) -> None:
    _dense("pack_nchw_pairs", "x", x_nchw, dim=4, contiguous=False)
    n, c, h, w = x_nchw.shape
    if cp % 32 or not 0 < c <= cp or n < 1 or h * w < 1:
        raise RuntimeError(f"medfusion_amd: pack_nchw_pairs: x {tuple(x_nchw.shape)} needs 1 <= C <= cp = {cp}, cp a multiple of 32")
    if c * h * w > 1 << 18:
        raise RuntimeError(f"medfusion_amd: pack_nchw_pairs: one workgroup per sample -- at most 2^18 values per sample, got {c * h * w}")


def pack_nchw_pairs(x_nchw: torch.Tensor, cp: int = 32) -> torch.Tensor:
    """NCHW fp32 [N, C, H, W] (C <= cp) -> an NHWC [N, H, W, cp] tensor that exists ONLY as fp16 pairs (channels C.. zero), scaled per sample by
    the max |x| the same launch measures (mf_pack_nchw_pairs_f32): the operand form of the network input"""
    check_pack_nchw_pairs(x_nchw, cp)
    _gpu(x_nchw)
    x = x_nchw.contiguous()
    n, c, h, w = x.shape
    out, outs, ob = _pair_outputs((n, h, w, cp), x.device)     # (out's storage is never written: pairs only)
    L.check(L.load().mf_pack_nchw_pairs_f32(x.data_ptr(), outs.data_ptr(), ob.data_ptr(), n, c, h * w, cp, stream()), "mf_pack_nchw_pairs_f32")
    return _attach(out, "pack_nchw_pairs (measured)", split=outs, bound=ob, pairs_only=True)


def conv_pairs_out_ok(d: L.MfConvDesc) -> bool:
    return bool(L.load().mf_conv2d_f16x2_pairs_out_ok(C.byref(d)))


def conv2d_f16x2_pairs_out(x1: torch.Tensor, w_split, bias: Optional[torch.Tensor], d: L.MfConvDesc, l1, bias_max: float, x2: Optional[torch.Tensor] = None,
                           pinned=None) -> torch.Tensor:
    """the fp16-pair convolution writing its output as fp32 AND as fp16 pairs under a bound derived from the operands
    (mf_conv2d_f16x2_pairs_out): l1 = (largest filter L1 norm over the channels of x1, ... of x2), bias_max = max |bias|.  The result carries
    its mirror and bound like the output of gn_apply(split=True): no measuring pass, no split launch in front of its consumers."""
    check_conv2d("conv2d_f16x2_pairs_out", x1, x2, w_split[0], bias, None, d)
    wh, wmax = w_split
    _gpu(x1, x2, wh, bias)
    lib = L.load()
    x1s, b1, x2s, b2 = _pair_operands(x1, x2)
    out, outs, ob = _pair_outputs((d.N, *conv_out_hw(d), d.Cout), x1.device)
    if pinned is None:
        pinned = (lib.mf_conv2d_workspace_bytes(C.byref(d)), 0, lib.mf_conv2d_f16x2_sync_words(C.byref(d)))
    need, _, words = pinned
    ws, sync = _scratch(x1.device, need, words)
    rc = lib.mf_conv2d_f16x2_pairs_out(x1s.data_ptr(), _ptr(x2s), wh.data_ptr(), _ptr(bias), out.data_ptr(), outs.data_ptr(), ob.data_ptr(), b1.data_ptr(), _ptr(b2),
                                       wmax, float(l1[0]), float(l1[1]), float(bias_max), ws, need, sync, C.byref(d), stream())
    L.check(rc, "mf_conv2d_f16x2_pairs_out")
    return _attach(out, "conv pairs_out (derived: bound(x) L1(w) + max|bias|)", split=outs, bound=ob)


# ----------------------------------------------------------------------------- Winograd F(2x2, 3x3) form of the 3x3 stride-1 convolutions
# The transform-domain mirror of an activation travels as attributes of the tensor, like the plain fp16-pair mirror: `t._mf_wino` (int32
# [16, N, T, C]: V = B^T d B as fp16 pairs) and `t._mf_wino_bound` (float [16 N]).  Producers that write it themselves set both; a consumer that
# finds neither runs the stand-alone input transform once (mf_wino_input_f16x2, from the plain pair mirror) and caches the result on the tensor.
def wino_ok(d: L.MfConvDesc) -> bool:
    return bool(L.load().mf_wino_ok(C.byref(d)))


def wino_preferred(d: L.MfConvDesc) -> bool:
    """is the Winograd form the faster one for `d` on MI355X?  (mf_wino_preferred: since ABI 240 a rule in (Cin, Cout, H W, N) that holds at any batch --
    csrc/conv_f16x2_wino.inc; the host switch is blocks.WINOGRAD / MEDFUSION_WINOGRAD = 0 never | 1 where preferred | 2 wherever mf_wino_ok)"""
    return bool(L.load().mf_wino_preferred(C.byref(d)))


def wino_gn_parts(d: L.MfConvDesc, G: int) -> int:
    return L.load().mf_wino_gn_parts(C.byref(d), G)


def wino_pack_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """OIHW 3x3 -> U = G g G^T as [16, Cout, 1, 1, Cin] fp32 (device, once at load)"""
    _gpu(w_oihw)
    w = w_oihw.contiguous()
    co, ci, kh, kw = w.shape
    assert (kh, kw) == (3, 3)
    out = torch.empty((16, co, 1, 1, ci), dtype=torch.float32, device=w.device)
    L.check(L.load().mf_wino_pack_weight_f32(w.data_ptr(), out.data_ptr(), co, ci, stream()), "mf_wino_pack_weight_f32")
    return out


def wino_input(x: torch.Tensor):
    """(V as fp16 pairs [16, N, T, C], bounds [16 N]) of the NHWC activation x, cached on x.  A tensor whose producer could have written V
    itself (conv2d_wino_gn_apply: `_mf_wino_site`) tells it so here: from its next call on that producer emits V with its output -- the
    stand-alone transform below runs once per site (the eager warm-up iteration of a sampling loop), never in the recorded iteration."""
    v = _fresh(x, "_mf_wino")
    if v is None:
        site = getattr(x, "_mf_wino_site", None)
        if site is not None:
            site[0][site[1]] = True
        xs, xb = split_of(x), bound_of(x)
        n, h, w, c = x.shape
        v = torch.empty((16, n, (h // 2) * (w // 2), c), dtype=torch.int32, device=x.device)
        vb = torch.empty((16 * n,), dtype=torch.float32, device=x.device)
        L.check(L.load().mf_wino_input_f16x2(xs.data_ptr(), xb.data_ptr(), v.data_ptr(), vb.data_ptr(), n, h, w, c, stream()), "mf_wino_input_f16x2")
        _attach(x, wino=(v, vb))
    return v, x._mf_wino_bound


def _wino_operands(x1: torch.Tensor, x2: Optional[torch.Tensor]):
    """(V of x1, its bounds, V of x2, its bounds): the operands of a Winograd convolution of x1 | x2 (wino_input); x2 may be None"""
    return (*wino_input(x1), *(wino_input(x2) if x2 is not None else (None, None)))


def pin_wino_plan(d: L.MfConvDesc):
    """(workspace bytes, sync words) of the Winograd form of `d`, computed once by callers that launch the same descriptor every iteration"""
    lib = L.load()
    return lib.mf_wino_workspace_bytes(C.byref(d)), lib.mf_wino_sync_words(C.byref(d))


def check_wino(what: str, x1, x2, u, bias, d: L.MfConvDesc, G: int = 0, gamma=None, beta=None, residual=None, emb=None, emb_stride: int = 0) -> None:
    """The sizes mf_conv2d_wino_f16x2 / mf_conv2d_wino_gn_apply_f16x2 / mf_wino_tail_f32 take on trust, against the descriptor, in the style of
    check_conv2d: x1 / x2 are contiguous fp32 NHWC [N, Hin, Win, C1 / C2] (x2 present iff C2 > 0; a tensor that exists as pairs only still has
    that shape), `u` holds the 16 slabs of Cout (C1 + C2) transformed weights (fp16 pairs: int32 storage; fp32; the bf16 triplets of precision 3
    three times as many), bias / gamma / beta Cout contiguous fp32 values (gamma and beta together), the residual N Hin Win Cout values, the
    embedding rows [N, Cout] with unit channel stride and the row stride the caller states.  G > 0: the group count of the tail divides Cout.
    Host arithmetic on shapes only: no device call, no sync."""
    def bad(msg):
        raise RuntimeError(f"medfusion_amd: {what}: {msg}")
    for name, x, ch in (("x1", x1, d.C1), ("x2", x2, d.C2)):
        if (x is not None) != (ch > 0):
            bad(f"{name} is {'given' if x is not None else 'missing'} but the descriptor has {ch} channels for it")
        if x is not None and (tuple(x.shape) != (d.N, d.Hin, d.Win, ch) or x.dtype != torch.float32 or not x.is_contiguous()):
            bad(f"{name} {tuple(x.shape)} {x.dtype} must be contiguous fp32 NHWC of the descriptor's N Hin Win C = {(d.N, d.Hin, d.Win, ch)}")
    want = 16 * d.Cout * (d.C1 + d.C2) * (3 if d.precision == 3 else 1)
    udt = {5: torch.int32, 3: torch.int16}.get(d.precision, torch.float32)   # fp16 pairs / bf16 triplets are opaque integer storage
    if u is None or u.numel() != want or not u.is_contiguous() or u.dtype != udt:
        bad(f"the transformed weights hold {None if u is None else (u.numel(), u.dtype)}, 16 Cout (C1 + C2) = 16 {d.Cout} ({d.C1} + {d.C2})"
            f"{' in three bf16 terms' if d.precision == 3 else ''} needs {want} contiguous {udt} values")
    for name, t in (("bias", bias), ("gamma", gamma), ("beta", beta)):
        if t is not None and (t.numel() != d.Cout or t.dtype != torch.float32 or not t.is_contiguous()):
            bad(f"{name} {tuple(t.shape)} {t.dtype} must be contiguous fp32 of Cout = {d.Cout} values")
    if (gamma is None) != (beta is None):
        bad("gamma and beta go together")
    if G and (G < 0 or d.Cout % G):
        bad(f"{G} groups do not divide Cout = {d.Cout}")
    if residual is not None and (tuple(residual.shape) != (d.N, d.Hin, d.Win, d.Cout) or residual.dtype != torch.float32 or not residual.is_contiguous()):
        bad(f"the residual {tuple(residual.shape)} {residual.dtype} must be contiguous fp32 NHWC {(d.N, d.Hin, d.Win, d.Cout)}")
    if emb is not None:
        if emb.dim() != 2 or tuple(emb.shape) != (d.N, d.Cout) or emb.dtype != torch.float32 or emb.stride(1) != 1:
            bad(f"the embedding {tuple(emb.shape)} {emb.dtype} (strides {emb.stride()}) must be fp32 rows [N, Cout] = {(d.N, d.Cout)} with unit channel stride")
        if emb_stride % 4 or emb_stride < d.Cout or (d.N > 1 and emb_stride != emb.stride(0)):
            bad(f"emb_stride {emb_stride} must be the embedding's row stride {emb.stride(0)}, a multiple of 4 and >= Cout = {d.Cout}")


def conv2d_wino_f16x2(x1: torch.Tensor, u_split, bias: Optional[torch.Tensor], d: L.MfConvDesc, x2: Optional[torch.Tensor] = None,
                      gn_groups: int = 0, gn_parts: int = 0, pinned=None):
    """The 3x3 stride-1 convolution `d` in its Winograd form (mf_conv2d_wino_f16x2): u_split = split_weight_f16x2(wino_pack_weight(w)).
    Returns y fp32 NHWC, or (y, partial [N, parts, G, 2]) when gn_groups > 0 (gn_parts = wino_gn_parts(d, G) > 0)."""
    uh, umax = u_split
    check_wino("conv2d_wino_f16x2", x1, x2, uh, bias, d, gn_groups)
    _gpu(x1, x2, uh, bias)
    lib = L.load()
    v1, b1, v2, b2 = _wino_operands(x1, x2)
    dev = x1.device
    out = torch.empty((d.N, d.Hin, d.Win, d.Cout), dtype=torch.float32, device=dev)
    partial = torch.empty((d.N, gn_parts, gn_groups, 2), dtype=torch.float64, device=dev) if gn_groups else None
    need, words = pinned if pinned is not None else pin_wino_plan(d)
    ws, sync = _scratch(dev, need, words, wino=True)
    rc = lib.mf_conv2d_wino_f16x2(v1.data_ptr(), _ptr(v2), uh.data_ptr(), _ptr(bias), out.data_ptr(), b1.data_ptr(), _ptr(b2), umax, ws, need,
                                  sync, _ptr(partial), gn_groups, C.byref(d), stream())
    L.check(rc, "mf_conv2d_wino_f16x2")
    return (out, partial) if gn_groups else out


def wino_tail_ok(d: L.MfConvDesc, G: int) -> bool:
    return bool(L.load().mf_wino_tail_ok(C.byref(d), G))


def wino_group_ok(d: L.MfConvDesc, guest: L.MfConvDesc) -> bool:
    """can the fp16-pair convolution `guest` share the launch of d's component GEMM (mf_wino_group_ok)?"""
    return bool(L.load().mf_wino_group_ok(C.byref(d), C.byref(guest)))


def conv2d_wino_gn_apply(x1: torch.Tensor, u_split, bias: Optional[torch.Tensor], d: L.MfConvDesc, gamma, beta, G: int, eps: float, act: int = 1,
                         residual: Optional[torch.Tensor] = None, emb: Optional[torch.Tensor] = None, emb_stride: int = 0,
                         x2: Optional[torch.Tensor] = None, bconst: float = 0.0, out_fp32: bool = True, want_wino: bool = False, pinned=None,
                         guest=None) -> torch.Tensor:
    """Winograd conv -> GroupNorm -> Swish -> (+ residual) -> (+ emb) (-> the input transform of the next Winograd convolution) in two launches
    (mf_conv2d_wino_gn_apply_f16x2): the component GEMM and one tail.  Returns the result with its fp16-pair mirror and bound attached (out_fp32 =
    False: pairs only, like gn_apply) and, with want_wino, its transform-domain mirror as well.
    guest = dict(w_split, bias, d, pinned): conv_res of the same ResBlock (a 1x1 on the same x1 | x2) in the GEMM's grid; its measured output IS the
    residual of the tail (`residual` must be None then)."""
    uh, umax = u_split
    check_wino("conv2d_wino_gn_apply", x1, x2, uh, bias, d, G, gamma, beta, residual, emb, emb_stride)
    _gpu(x1, x2, uh, bias, gamma, beta, residual, emb)
    lib = L.load()
    v1, b1, v2, b2 = _wino_operands(x1, x2)
    dev = x1.device
    need, words = pinned if pinned is not None else pin_wino_plan(d)
    gcall = None
    if guest is not None:
        if residual is not None:
            raise RuntimeError("conv2d_wino_gn_apply: the guest's output is the residual")
        need_g, _, words_g = guest["pinned"]
        ws, sync, ws_g, sync_g = _scratch(dev, need, words, need_g, words_g, wino=True)   # the guest's hand-off region behind the GEMM's workspace, its counters behind the GEMM's
        gcall, residual = _conv_call(_pair_operands(x1, x2), guest, ws_g, sync_g, dev, measured=True)
    else:
        ws, sync = _scratch(dev, need, words, wino=True)
    tail_ops = _tail_operands(residual, emb)
    out, outs, ob, ov, ovb = _pair_outputs((d.N, d.Hin, d.Win, d.Cout), dev, wino=want_wino)
    t = _tail_struct(L.MfWinoTail, gamma, beta, tail_ops, emb, emb_stride, out if out_fp32 else None, outs, ob, _ptr(ov), _ptr(ovb), act, bconst, eps)
    rc = lib.mf_conv2d_wino_gn_apply_f16x2(v1.data_ptr(), _ptr(v2), uh.data_ptr(), _ptr(bias), b1.data_ptr(), _ptr(b2), umax, ws, need, sync, G,
                                           C.byref(t), None if gcall is None else C.byref(gcall), C.byref(d), stream())
    L.check(rc, "mf_conv2d_wino_gn_apply_f16x2")
    return _attach(out, "Winograd tail (derived: bconst + residual + embedding)", split=outs, bound=ob, wino=(ov, ovb) if want_wino else None,
                   pairs_only=not out_fp32)


def _tail_struct(cls, gamma, beta, tail_ops, emb, emb_stride, out, outs, ob, p11, p12, act, bconst, eps):
    """MfGnFuse / MfWinoTail (`cls`): what the GroupNorm tail of a convolution reads and writes.  tail_ops = _tail_operands(residual, emb); out None: the
    fp32 form is not written (pairs only).  The two structs differ in their pointer fields 11 and 12 alone: (rendezvous counters, error flag) of the
    convolution that waits for its sample inside its launch, (V of the output, its bounds) of the Winograd tail"""
    rp, res_pairs, rb, rslots, eb = tail_ops
    return cls(_ptr(gamma), _ptr(beta), rp, _ptr(res_pairs), _ptr(rb), _ptr(rslots), _ptr(emb), _ptr(eb), _ptr(out), outs.data_ptr(), ob.data_ptr(), p11, p12,
               int(emb_stride), 0 if rslots is None else rslots.shape[1], int(act), float(bconst), float(eps))


# ----------------------------------------------------------------------------- the Winograd form on the EXACT arithmetics (round 6, ABI 250)
def wino_f32_ok(d: L.MfConvDesc, G: int) -> bool:
    """can the 3x3 `d` (precision 0 = fp32 MFMA or 3 = exact bf16 triplets) with the G-group GroupNorm behind it run as fp32 transforms + component GEMMs
    on the exact arithmetic's own kernel + the tail?  (mf_wino_f32_ok)"""
    return bool(L.load().mf_wino_f32_ok(C.byref(d), G))


def wino_input_f32(x: torch.Tensor) -> torch.Tensor:
    """V = B^T d B of the fp32 NHWC activation x as fp32 [16, N, T, C], cached on x; a tensor whose producer could have written V itself
    (conv2d_wino_gn_apply_f32: `_mf_wino_site_f32`) tells it so here, like wino_input does for the fp16-pair form"""
    v = _fresh(x, "_mf_wino_f32")
    if v is None:
        _need_f32(x)
        site = getattr(x, "_mf_wino_site_f32", None)
        if site is not None:
            site[0][site[1]] = True
        n, h, w, c = x.shape
        v = torch.empty((16, n, (h // 2) * (w // 2), c), dtype=torch.float32, device=x.device)
        L.check(L.load().mf_wino_input_f32(x.data_ptr(), v.data_ptr(), n, h, w, c, stream()), "mf_wino_input_f32")
        _attach(x, wino_f32=v)
    return v


def conv2d_wino_gn_apply_f32(x1: torch.Tensor, u_packed: torch.Tensor, bias: Optional[torch.Tensor], d: L.MfConvDesc, gamma, beta, G: int, eps: float,
                             act: int = 1, residual: Optional[torch.Tensor] = None, emb: Optional[torch.Tensor] = None, emb_stride: int = 0,
                             x2: Optional[torch.Tensor] = None, want_wino: bool = False) -> torch.Tensor:
    """conv3x3 -> GroupNorm -> Swish -> + residual -> + emb on the Winograd form of an EXACT arithmetic (d.precision 0 or 3): the 16 component GEMMs run on
    that arithmetic's own implicit-GEMM kernel (mf_conv2d_f32 on the upsample = 3 descriptor; u_packed = U = G g G^T [16, Cout, 1, 1, Cin], pre-split for
    precision 3), the transforms and the tail are fp32.  Returns y fp32 NHWC; want_wino: it also carries V of y for the next Winograd convolution."""
    check_wino("conv2d_wino_gn_apply_f32", x1, x2, u_packed, bias, d, G, gamma, beta, residual, emb, emb_stride)
    _gpu(x1, x2, u_packed, bias, gamma, beta, residual, emb)
    lib = L.load()
    n, h, w, c1 = x1.shape
    c2 = 0 if x2 is None else x2.shape[-1]
    co, t = d.Cout, (h // 2) * (w // 2)
    v1 = wino_input_f32(x1)
    v2 = wino_input_f32(x2) if x2 is not None else None
    g = make_conv_desc(16 * n, 1, t, c1, c2, co, 1, 1, 0, 3, precision=d.precision)
    m = conv2d(v1.view(16 * n, 1, t, c1), u_packed, None, g, x2=None if v2 is None else v2.view(16 * n, 1, t, c2))
    assert m.numel() == 16 * n * t * co, (tuple(m.shape), n, t, co)   # M [16][n T][Cout]: what the tail reads, no more
    if residual is not None:
        _need_f32(residual)
    out = torch.empty((n, h, w, co), dtype=torch.float32, device=x1.device)
    ov = torch.empty((16, n, t, co), dtype=torch.float32, device=x1.device) if want_wino else None
    L.check(lib.mf_wino_tail_f32(m.data_ptr(), _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(residual), _ptr(emb), emb_stride, out.data_ptr(), _ptr(ov),
                                 n, h, w, co, G, act, eps, stream()), "mf_wino_tail_f32")
    return _attach(out, wino_f32=ov) if want_wino else out


def conv_fuse_words(d: L.MfConvDesc, G: int) -> int:
    """rendezvous words mf_conv2d_f16x2_gn_apply needs for `d` followed by a G-group GroupNorm; 0: this convolution cannot apply it itself
    (capability; whether blocks.py uses the form is Rendezvous.disabled / FUSE_MIN_HW)"""
    return L.load().mf_conv2d_f16x2_fuse_words(C.byref(d), G)


def conv2d_f16x2_gn_apply(x1: torch.Tensor, w_split, bias: Optional[torch.Tensor], d: L.MfConvDesc, gamma, beta, G: int, eps: float, parts: int,
                          words: int, act: int = 1, residual: Optional[torch.Tensor] = None, emb: Optional[torch.Tensor] = None, emb_stride: int = 0,
                          x2: Optional[torch.Tensor] = None, bconst: float = 0.0, out_fp32: bool = True, pinned=None) -> torch.Tensor:
    """conv -> GroupNorm -> Swish -> (+ residual) -> (+ emb) in ONE launch (mf_conv2d_f16x2_gn_apply): what conv2d_f16x2(gn_groups=G) followed
    by gn_apply(GnPartials, split=True) computes, bit for bit.  words = conv_fuse_words(d, G) > 0, parts = conv_gn_parts(d, G) > 0.
    Returns the result with its fp16-pair mirror and bound attached (out_fp32=False: pairs only, like gn_apply)."""
    wh, wmax = w_split
    _gpu(x1, x2, wh, bias, gamma, beta, residual, emb)
    lib = L.load()
    x1s, b1, x2s, b2 = _pair_operands(x1, x2)
    dev = x1.device
    tail_ops = _tail_operands(residual, emb)
    out, outs, ob = _pair_outputs((d.N, *conv_out_hw(d), d.Cout), dev)
    partial = torch.empty((d.N, parts, G, 2), dtype=torch.float64, device=dev)
    if pinned is None:
        pinned = (lib.mf_conv2d_workspace_bytes(C.byref(d)), 0, lib.mf_conv2d_f16x2_sync_words(C.byref(d)))
    need, _, swords = pinned
    ws, sync = _scratch(dev, need, swords)
    rv = Rendezvous.get(words, dev)
    f = _tail_struct(L.MfGnFuse, gamma, beta, tail_ops, emb, emb_stride, out if out_fp32 else None, outs, ob, rv.data_ptr() + 16, rv.data_ptr(), act, bconst, eps)
    rc = lib.mf_conv2d_f16x2_gn_apply(x1s.data_ptr(), _ptr(x2s), wh.data_ptr(), _ptr(bias), b1.data_ptr(), _ptr(b2), wmax, ws, need, sync,
                                      partial.data_ptr(), G, C.byref(f), C.byref(d), stream())
    L.check(rc, "mf_conv2d_f16x2_gn_apply")
    return _attach(out, "conv + GroupNorm tail in one launch (derived)", split=outs, bound=ob, pairs_only=not out_fp32)


def make_conv3d_desc(N, D, H, W, C1, C2, Cout, k, stride=(1, 1, 1), pad=(0, 0, 0), upsample=(0, 0, 0), tile_hint=0, splitk_hint=0,
                     precision=5) -> L.MfConv3dDesc:
    """descriptor of a 3-D convolution (mf_conv3d_f16x2): per-axis stride / pad / upsample as 3-tuples (an int: the same on every axis)"""
    t3 = lambda v: (int(v),) * 3 if isinstance(v, int) else tuple(int(a) for a in v)
    A = C.c_int32 * 3
    return L.MfConv3dDesc(N, D, H, W, C1, C2, Cout, k, A(*t3(stride)), A(*t3(pad)), A(*t3(upsample)), tile_hint, splitk_hint, precision)


def conv3d_ok(d: L.MfConv3dDesc) -> bool:
    """True: mf_conv3d_f16x2 accepts `d` (with the workspace mf_conv3d_workspace_bytes names)"""
    return bool(L.load().mf_conv3d_ok(C.byref(d)))


def conv3d_out_dims(d: L.MfConv3dDesc):
    out = (C.c_int32 * 3)()
    L.check(L.load().mf_conv3d_out_dims(C.byref(d), out), "mf_conv3d_out_dims")
    return tuple(out)


def conv3d_plan(d: L.MfConv3dDesc):
    """(tile id 1..4, split-K slices) the planner picks for `d` (the hints of `d` win)"""
    t, k = C.c_int32(), C.c_int32()
    L.check(L.load().mf_conv3d_plan_query(C.byref(d), C.byref(t), C.byref(k)), "mf_conv3d_plan_query")
    return t.value, k.value


def pack_conv3d_weight(w_oidhw: torch.Tensor, cin_pad: int = 0) -> torch.Tensor:
    """OIDHW fp32 [Cout, Cin, k, k, k] -> [Cout, k, k, k, cin_pad] fp32 (input channels Cin.. zero; cin_pad 0: Cin)"""
    _gpu(w_oidhw)
    w = w_oidhw.detach().contiguous()
    co, ci, k = w.shape[0], w.shape[1], w.shape[2]
    if w.dim() != 5 or tuple(w.shape[2:]) != (k, k, k):
        raise RuntimeError(f"pack_conv3d_weight: OIDHW weights with a cubic kernel, got {tuple(w.shape)}")
    cp = cin_pad or ci
    out = torch.empty((co, k, k, k, cp), dtype=torch.float32, device=w.device)
    L.check(L.load().mf_pack_conv3d_weight_f32(w.data_ptr(), out.data_ptr(), co, ci, k, cp, stream()), "mf_pack_conv3d_weight_f32")
    return out


def check_conv3d(x1, x2, w_split, bias, out, d: L.MfConv3dDesc) -> None:
    """The sizes mf_conv3d_f16x2 takes on trust, against the descriptor: x1 / x2 hold N D H W voxels of C1 / C2 channels (x2 present iff C2 > 0), the
    bias Cout values, the split weights Cout k^3 (C1 + C2), and `out` -- None: the wrapper allocates it -- is contiguous fp32 of N Do Ho Wo Cout values"""
    def bad(msg):
        raise RuntimeError(f"medfusion_amd: conv3d_f16x2: {msg}")
    vox = d.N * d.D * d.H * d.W
    if x1 is None or x1.numel() != vox * d.C1:
        bad(f"x1 holds {None if x1 is None else x1.numel()} values, the descriptor's N D H W C1 = {d.N} {d.D} {d.H} {d.W} {d.C1} needs {vox * d.C1}")
    if (x2 is not None) != (d.C2 > 0):
        bad(f"the second source is {'given' if x2 is not None else 'missing'} but the descriptor has C2 = {d.C2}")
    if x2 is not None and x2.numel() != vox * d.C2:
        bad(f"x2 holds {x2.numel()} values, the descriptor's N D H W C2 = {d.N} {d.D} {d.H} {d.W} {d.C2} needs {vox * d.C2}")
    if bias is not None and (bias.numel() != d.Cout or bias.dtype != torch.float32 or not bias.is_contiguous()):
        bad(f"bias {tuple(bias.shape)} {bias.dtype} must be contiguous fp32 of Cout = {d.Cout} values")
    wh = w_split[0]
    if wh.numel() != d.Cout * d.k ** 3 * (d.C1 + d.C2) or not wh.is_contiguous():
        bad(f"the split weights hold {wh.numel()} values, Cout k^3 (C1 + C2) = {d.Cout} {d.k}^3 ({d.C1} + {d.C2}) needs {d.Cout * d.k ** 3 * (d.C1 + d.C2)}")
    if out is not None:
        od = [((e << u) + 2 * p - d.k) // s + 1 if s > 0 else 0 for e, s, p, u in zip((d.D, d.H, d.W), d.stride, d.pad, d.upsample)]
        want = d.N * od[0] * od[1] * od[2] * d.Cout
        if out.numel() != want or out.dtype != torch.float32 or not out.is_contiguous():
            bad(f"out {tuple(out.shape)} {out.dtype} must be contiguous fp32 of N Do Ho Wo Cout = {d.N} {od[0]} {od[1]} {od[2]} {d.Cout} = {want} values")


def conv3d_f16x2(x1: torch.Tensor, w_split, bias: Optional[torch.Tensor], d: L.MfConv3dDesc, x2: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MF_CONV_FP32_F16X2 3-D convolution of NDHWC fp32 tensors (any shape with N leading and d.C1 / d.C2 innermost, e.g. the [N, D*H, W, C]
    view) whose fp16-pair mirrors are made on demand (or that exist as pairs only: pack_nchw_pairs).  w_split = split_weight_f16x2(
    pack_conv3d_weight(...)).  Returns y fp32 [N, Do, Ho, Wo, Cout] (or fills `out`, any shape of that size)."""
    check_conv3d(x1, x2, w_split, bias, out, d)
    wh, wmax = w_split
    _gpu(x1, x2, wh, bias)
    lib = L.load()
    if not lib.mf_conv3d_ok(C.byref(d)):
        raise RuntimeError("conv3d_f16x2: descriptor not supported (mf_conv3d_ok)")
    x1s, b1, x2s, b2 = _pair_operands(x1, x2)
    do, ho, wo = conv3d_out_dims(d)
    if out is None:
        out = torch.empty((d.N, do, ho, wo, d.Cout), dtype=torch.float32, device=x1.device)
    else:
        drop_split(out)
    need = lib.mf_conv3d_workspace_bytes(C.byref(d))
    ws, _ = _scratch(x1.device, need, 0)
    rc = lib.mf_conv3d_f16x2(x1s.data_ptr(), _ptr(x2s), wh.data_ptr(), _ptr(bias), out.data_ptr(), b1.data_ptr(), _ptr(b2), wmax, ws, need,
                             C.byref(d), stream())
    L.check(rc, "mf_conv3d_f16x2")
    return out


def make_conv_desc(N, Hin, Win, C1, C2, Cout, k, stride, pad, upsample=0, in_layout=L.LAYOUT_NHWC, out_layout=L.LAYOUT_NHWC,
                   tile_hint=0, splitk_hint=0, precision=0) -> L.MfConvDesc:
    return L.MfConvDesc(N, Hin, Win, C1, C2, Cout, k, k, stride, pad, upsample, in_layout, out_layout, tile_hint, splitk_hint, precision)


def convert_conv_weight_bf16(w_packed: torch.Tensor) -> torch.Tensor:
    """packed fp32 weights -> bf16 (round to nearest even) for the opt-in MF_CONV_BF16 mode: opaque int16 tensor [rows, K]"""
    _gpu(w_packed)
    w = w_packed.contiguous()
    k = w.shape[-1] * w.shape[-2] * w.shape[-3]
    rows = w.numel() // k
    out = torch.empty((rows, k), dtype=torch.int16, device=w.device)
    L.check(L.load().mf_convert_conv_weight_bf16(w.data_ptr(), out.data_ptr(), rows, k, stream()), "mf_convert_conv_weight_bf16")
    return out


def conv_out_hw(d: L.MfConvDesc):
    up = 1 if d.upsample in (1, 2) else 0   # (upsample = 3, the component GEMM of a Winograd convolution, is a plain 1 x T 1x1: csrc/conv_plan.h)
    he, we = d.Hin << up, d.Win << up
    return (he + 2 * d.pad - d.KH) // d.stride + 1, (we + 2 * d.pad - d.KW) // d.stride + 1


def check_conv2d(what: str, x1, x2, w, bias, out, d: L.MfConvDesc) -> None:
    """The sizes mf_conv2d_f32 / mf_conv2d_f16x2 / mf_conv2d_f16x2_pairs_out take on trust, against the descriptor: x1 / x2 hold N Hin Win pixels of
    C1 / C2 channels in either layout (x2 present iff C2 > 0), the bias Cout contiguous fp32 values, the weights Cout KH KW (C1 + C2) values -- the
    sub-pixel packing (upsample = 2) 4 phases of Cout 2 2 (C1 + C2), the component GEMMs of a Winograd convolution (upsample = 3) 16 slabs of Cout
    (C1 + C2), the bf16-triplet form (precision 3) three times as many -- and `out` -- None: the wrapper allocates it -- is contiguous fp32 of
    N Ho Wo Cout values.  Host arithmetic on shapes only: no device call, no sync."""
    def bad(msg):
        raise RuntimeError(f"medfusion_amd: {what}: {msg}")
    lay = "NCHW" if d.in_layout == L.LAYOUT_NCHW else "NHWC"
    pix = d.N * d.Hin * d.Win
    if x1 is None or x1.numel() != pix * d.C1:
        bad(f"x1 holds {None if x1 is None else x1.numel()} values, the descriptor's N Hin Win C1 = {d.N} {d.Hin} {d.Win} {d.C1} ({lay}) needs {pix * d.C1}")
    if (x2 is not None) != (d.C2 > 0):
        bad(f"the second source is {'given' if x2 is not None else 'missing'} but the descriptor has C2 = {d.C2}")
    if x2 is not None and x2.numel() != pix * d.C2:
        bad(f"x2 holds {x2.numel()} values, the descriptor's N Hin Win C2 = {d.N} {d.Hin} {d.Win} {d.C2} ({lay}) needs {pix * d.C2}")
    if bias is not None and (bias.numel() != d.Cout or bias.dtype != torch.float32 or not bias.is_contiguous()):
        bad(f"bias {tuple(bias.shape)} {bias.dtype} must be contiguous fp32 of Cout = {d.Cout} values")
    cin = d.C1 + d.C2
    if d.upsample == 2:
        want, form = 4 * d.Cout * 4 * cin, f"the sub-pixel packing 4 Cout 2 2 (C1 + C2) = 4 {d.Cout} 2 2 ({d.C1} + {d.C2})"
    elif d.upsample == 3:
        want, form = 16 * d.Cout * cin, f"16 Cout (C1 + C2) = 16 {d.Cout} ({d.C1} + {d.C2})"
    else:
        want, form = d.Cout * d.KH * d.KW * cin, f"Cout KH KW (C1 + C2) = {d.Cout} {d.KH} {d.KW} ({d.C1} + {d.C2})"
    if d.precision == 3:
        want, form = 3 * want, "three bf16 terms of " + form
    if w is None or w.numel() != want or not w.is_contiguous():
        bad(f"the weights hold {None if w is None else w.numel()} values{'' if w is None or w.is_contiguous() else ' (not contiguous)'}, {form} needs {want}")
    if out is not None:
        ho, wo = conv_out_hw(d) if d.stride > 0 else (0, 0)
        n_out = d.N * ho * wo * d.Cout
        if out.numel() != n_out or out.dtype != torch.float32 or not out.is_contiguous():
            bad(f"out {tuple(out.shape)} {out.dtype} must be contiguous fp32 of N Ho Wo Cout = {d.N} {ho} {wo} {d.Cout} = {n_out} values")


def conv2d(x1: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], d: L.MfConvDesc, x2: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = conv(x1 ++ x2) + bias per descriptor `d`.  Output NHWC [N,Ho,Wo,Cout] or NCHW [N,Cout,Ho,Wo]."""
    check_conv2d("conv2d", x1, x2, w_packed, bias, out, d)
    _gpu(x1, x2, w_packed, bias)
    _need_f32(x1, x2)
    lib = L.load()
    ho, wo = conv_out_hw(d)
    if out is None:
        shape = (d.N, d.Cout, ho, wo) if d.out_layout == L.LAYOUT_NCHW else (d.N, ho, wo, d.Cout)
        out = torch.empty(shape, dtype=torch.float32, device=x1.device)
    else:
        drop_split(out)
    need = lib.mf_conv2d_workspace_bytes(C.byref(d))
    ws, _ = _scratch(x1.device, need, 0)
    rc = lib.mf_conv2d_f32(x1.data_ptr(), _ptr(x2), w_packed.data_ptr(), _ptr(bias), out.data_ptr(), ws, need, C.byref(d), stream())
    L.check(rc, "mf_conv2d_f32")
    return out


def conv_gn_parts(d: L.MfConvDesc, G: int) -> int:
    """How many per-sample partial GroupNorm records this convolution emits itself (0: it cannot)."""
    return L.load().mf_conv2d_gn_parts(C.byref(d), G)


def conv2d_gn(x1: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], d: L.MfConvDesc, G: int, parts: int,
              x2: Optional[torch.Tensor] = None):
    """Convolution + the partial statistics of the GroupNorm that follows (conv epilogue or split-K reducer) -> (y NHWC, partial)."""
    _gpu(x1, x2, w_packed, bias)
    _need_f32(x1, x2)
    lib = L.load()
    ho, wo = conv_out_hw(d)
    out = torch.empty((d.N, ho, wo, d.Cout), dtype=torch.float32, device=x1.device)
    partial = torch.empty((d.N, parts, G, 2), dtype=torch.float64, device=x1.device)
    need = lib.mf_conv2d_workspace_bytes(C.byref(d))
    ws, _ = _scratch(x1.device, need, 0)
    rc = lib.mf_conv2d_gn_f32(x1.data_ptr(), _ptr(x2), w_packed.data_ptr(), _ptr(bias), out.data_ptr(), ws, need, partial.data_ptr(), G, C.byref(d),
                              stream())
    L.check(rc, "mf_conv2d_gn_f32")
    return out, partial


def gn_stats_partial(x: torch.Tensor, G: int):
    """x NHWC -> (partial [N, parts, G, 2] float64 {sum, sumsq}, parts)"""
    if x.dtype != torch.float32:
        raise RuntimeError("gn_stats_partial: fp32 only")
    _gpu(x)
    _need_f32(x)
    n, h, w, c = x.shape
    lib = L.load()
    parts = lib.mf_gn_partial_parts(h * w)
    partial = torch.empty((n, parts, G, 2), dtype=torch.float64, device=x.device)
    L.check(lib.mf_gn_stats_partial_f32(x.data_ptr(), partial.data_ptr(), n, h * w, c, G, stream()), "mf_gn_stats_partial_f32")
    return partial, parts


def gn_finalize(partial: torch.Tensor, parts: int, HW: int, C: int, G: int, eps: float = 1e-5) -> torch.Tensor:
    """partial [N, parts, G, 2] -> stats [N, G, 2] = (mean, rstd)"""
    _gpu(partial)
    n = partial.shape[0]
    stats = torch.empty((n, G, 2), dtype=torch.float32, device=partial.device)
    L.check(L.load().mf_gn_finalize_f32(partial.data_ptr(), parts, stats.data_ptr(), n, HW, C, G, eps, stream()), "mf_gn_finalize_f32")
    return stats


def gn_stats(x: torch.Tensor, G: int, eps: float = 1e-5) -> torch.Tensor:
    """x NHWC [N,H,W,C] -> stats [N,G,2] = (mean, rstd)."""
    _gpu(x)
    _need_f32(x)
    n, h, w, c = x.shape
    lib = L.load()
    stats = torch.empty((n, G, 2), dtype=torch.float32, device=x.device)
    need = lib.mf_gn_stats_workspace_bytes(n, h * w, c, G)
    ws = Workspace.get(need, x.device)
    L.check(lib.mf_gn_stats_f32(x.data_ptr(), stats.data_ptr(), ws.data_ptr(), need, n, h * w, c, G, eps, stream()), "mf_gn_stats_f32")
    return stats


class GnPartials:
    """the partial GroupNorm sums a convolution left ([N, parts, G, 2] fp64) handed to gn_apply un-finalised: the apply pass reduces them itself"""
    __slots__ = ("records", "parts", "eps")

    def __init__(self, records, parts, eps):
        self.records, self.parts, self.eps = records, parts, eps


def gn_apply(x: torch.Tensor, stats, gamma, beta, G: int, act: int = 1, residual: Optional[torch.Tensor] = None,
             emb: Optional[torch.Tensor] = None, emb_stride: int = 0, out: Optional[torch.Tensor] = None, split: bool = False,
             bconst: float = 0.0, out_fp32: bool = True) -> torch.Tensor:
    """stats: [N, G, 2] mean / rstd (gn_stats / gn_finalize), a GnPartials (mf_gn_apply_from_partials_f32: no finalize launch) or None.
    split=True: also emit the fp16-pair mirror of the result (operand of a following MF_CONV_FP32_F16X2 convolution), scaled per sample
    by the bound the pass derives: bconst (>= max |act(gn(x) gamma + beta)|, from the caller; the bound of x when nothing is normalised)
    + the bounds of the residual and of the embedding rows.
    out_fp32=False (a REQUEST, honoured on the from-partials pass with split=True): the result is wanted as fp16 pairs only -- every consumer
    is an fp16-pair convolution or the residual input of another such pass -- and its fp32 form is not written (12 instead of 16 bytes per
    element); the returned tensor says so (pairs_only).  A `residual` that is itself pairs-only is read from its pairs."""
    part = stats if isinstance(stats, GnPartials) else None
    if part is not None:
        stats = None
    _gpu(x, stats, gamma, beta, residual, emb)
    _need_f32(x)
    n, h, w, c = x.shape
    split = split and c % 8 == 0
    want_pairs_only = (not out_fp32) and split and part is not None
    ob = outs = None
    # (before `out` may alias x or the residual: their bounds describe the values this pass READS.  Only the from-partials pass reduces slot maxima
    # itself, and only it, emitting pairs, reads a residual that exists as pairs only)
    xb = bound_of(x) if (split and stats is None and part is None) else None
    rp, res_pairs, rb, rslots, eb = _tail_operands(residual, emb, bounds=split, slots=part is not None, pairs=split and part is not None)
    if out is None:
        out = torch.empty_like(x)
    else:
        drop_split(out)
    if split:
        outs = torch.empty(out.shape, dtype=torch.int32, device=x.device)
        ob = torch.empty((n,), dtype=torch.float32, device=x.device)
    if part is not None:
        rc = L.load().mf_gn_apply_from_partials_pairs_f32(x.data_ptr(), part.records.data_ptr(), part.parts, float(part.eps), _ptr(gamma), _ptr(beta),
                                                          rp, _ptr(res_pairs), _ptr(emb), emb_stride,
                                                          None if want_pairs_only else out.data_ptr(), _ptr(outs), _ptr(rb), _ptr(rslots),
                                                          0 if rslots is None else rslots.shape[1], _ptr(eb), float(bconst), _ptr(ob), n, h * w, c, G,
                                                          act, stream())
        L.check(rc, "mf_gn_apply_from_partials_pairs_f32")
    else:
        rc = L.load().mf_gn_apply_split_f32(x.data_ptr(), _ptr(stats), _ptr(gamma), _ptr(beta), rp, _ptr(emb), emb_stride, out.data_ptr(),
                                            _ptr(outs), _ptr(xb), _ptr(rb), _ptr(eb), float(bconst), _ptr(ob), n, h * w, c, G, act, stream())
        L.check(rc, "mf_gn_apply_split_f32")
    if split:
        _attach(out, "GroupNorm apply (derived: bconst + residual + embedding)" if (stats is not None or part is not None) else "apply without norm (bound(x) + residual + embedding)",
                split=outs, bound=ob, pairs_only=want_pairs_only)
    return out


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], act_in: bool = False, act_out: bool = False,
           out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """x [B, In] (row stride may exceed In), w [Out, In] -> [B, Out]."""
    _gpu(x, w, bias, out)
    _need_f32(x)
    _f32("linear", x, w, bias, out)
    assert x.dim() == 2 and w.dim() == 2, "linear: x [B, In], w [Out, In]"
    b, inn = x.shape
    o = w.shape[0]
    assert w.shape[1] == inn and x.stride(1) == 1 and w.is_contiguous()
    assert bias is None or (bias.shape == (o,) and bias.is_contiguous()), "linear: bias [Out], contiguous"
    if out is None:
        out = torch.empty((b, o), dtype=torch.float32, device=x.device)
    else:
        assert out.shape == (b, o) and out.stride(1) == 1, "linear: out [B, Out] with unit column stride"
        drop_split(out)
    rc = L.load().mf_linear_f32(x.data_ptr(), x.stride(0), w.data_ptr(), _ptr(bias), out.data_ptr(), out.stride(0), b, inn, o, int(act_in),
                                int(act_out), int(accumulate), stream())
    L.check(rc, "mf_linear_f32")
    return out


def sinusoidal(t: torch.Tensor, dim: int, max_period: float = 10000.0, shift: float = 1.0, flip: bool = False,
               freqs: Optional[torch.Tensor] = None) -> torch.Tensor:
    _gpu(t, freqs)
    t = t.to(torch.float32).contiguous()
    out = torch.empty((t.shape[0], dim), dtype=torch.float32, device=t.device)
    L.check(L.load().mf_sinusoidal_f32(t.data_ptr(), _ptr(freqs), out.data_ptr(), t.shape[0], dim, max_period, shift, int(flip), stream()),
            "mf_sinusoidal_f32")
    return out


def check_learned_sinusoidal(t, weights, emb_dim: int) -> None:
    """t [B] of any real dtype (the wrapper converts it); weights: the emb_dim // 2 learned frequencies, fp32"""
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.shape[0] < 1 or t.is_complex() or t.dtype == torch.bool:
        raise RuntimeError("medfusion_amd: learned_sinusoidal: t must be a non-empty [B] tensor of timesteps")
    if int(emb_dim) < 2:
        raise RuntimeError(f"medfusion_amd: learned_sinusoidal: emb_dim = {emb_dim} must be >= 2")
    _dense("learned_sinusoidal", "weights", weights, shape=(int(emb_dim) // 2,), contiguous=False)


def learned_sinusoidal(t: torch.Tensor, weights: torch.Tensor, emb_dim: int) -> torch.Tensor:
    """LearnedSinusoidalPosEmb.forward (time_embedder.py:42-49): [B] -> [B, 1 + 2 (emb_dim // 2) + (emb_dim & 1)]"""
    check_learned_sinusoidal(t, weights, emb_dim)
    _gpu(t, weights)
    t = t.to(torch.float32).contiguous()
    w = weights.detach().contiguous()
    out = torch.empty((t.shape[0], 1 + 2 * (emb_dim // 2) + (emb_dim & 1)), dtype=torch.float32, device=t.device)
    L.check(L.load().mf_learned_sinusoidal_f32(t.data_ptr(), w.data_ptr(), out.data_ptr(), t.shape[0], emb_dim, stream()), "mf_learned_sinusoidal_f32")
    return out


def check_embedding_add(table, idx, io) -> None:
    """io [B, D] += table[idx]: table [rows, D] and io fp32, contiguous; idx [B] int64 or int32 (the wrapper converts and copies it)"""
    _dense("embedding_add", "table", table, dim=2)
    _dense("embedding_add", "io", io, dim=2)
    if io.shape[1] != table.shape[1] or io.shape[0] < 1 or table.shape[0] < 1 or table.shape[1] < 1:
        raise RuntimeError(f"medfusion_amd: embedding_add: io {tuple(io.shape)} must be [B, D] for the table {tuple(table.shape)} = [rows, D]")
    if not isinstance(idx, torch.Tensor) or idx.dtype not in (torch.int64, torch.int32):
        raise RuntimeError(f"medfusion_amd: embedding_add: idx must be int64 (or int32), got {getattr(idx, 'dtype', type(idx).__name__)}")
    if idx.numel() != io.shape[0]:
        raise RuntimeError(f"medfusion_amd: embedding_add: idx must hold one index per row of io = {io.shape[0]}, got shape {tuple(idx.shape)}")


def embedding_add(table: torch.Tensor, idx: torch.Tensor, io: torch.Tensor) -> torch.Tensor:
    check_embedding_add(table, idx, io)
    _gpu(table, idx, io)
    idx = idx.to(torch.int64).contiguous()
    drop_split(io)
    L.check(L.load().mf_embedding_add_f32(table.data_ptr(), idx.data_ptr(), io.data_ptr(), io.shape[0], io.shape[1], table.shape[0], stream()),
            "mf_embedding_add_f32")
    return io


def philox_normal(out: torch.Tensor, seed: int, draw: int, sample_offset: int = 0, step_dev: Optional[torch.Tensor] = None,
                  draw_stride: int = 0) -> torch.Tensor:
    """Fill out [B, ...] with N(0,1): draw index = draw + draw_stride * (*step_dev or 0)."""
    _gpu(out, step_dev)
    b = out.shape[0]
    per = out.numel() // b
    drop_split(out)
    rc = L.load().mf_philox_normal_f32(out.data_ptr(), seed & 0xFFFFFFFFFFFFFFFF, draw, draw_stride, _ptr(step_dev), 0, sample_offset, b, per, stream())
    L.check(rc, "mf_philox_normal_f32")
    return out


def rows_axpby(x: torch.Tensor, a: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None, c: Optional[torch.Tensor] = None,
               d: Optional[torch.Tensor] = None, clamp: Optional[tuple] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b] = clamp((a[b]*x[b] + c[b]*y[b]) / d[b]); a, c, d are [B] fp32 device vectors (or None)."""
    _gpu(x, a, y, c, d)
    x = x.contiguous()
    if y is not None:
        y = y.contiguous()
    b = x.shape[0]
    if out is None:
        out = torch.empty_like(x)
    else:
        drop_split(out)
    lo, hi = clamp if clamp is not None else (0.0, 0.0)
    rc = L.load().mf_rows_axpby_f32(x.data_ptr(), _ptr(y), _ptr(a), _ptr(c), _ptr(d), out.data_ptr(), b, x.numel() // b, int(clamp is not None),
                                    float(lo), float(hi), stream())
    L.check(rc, "mf_rows_axpby_f32")
    return out


def image_to_uint8(x_nchw: torch.Tensor, normalize_each: bool = False) -> torch.Tensor:
    """[N,C,H,W] float in ~[-1,1] -> [N,H,W,C] uint8 on the device (mode 0: sample_dataset.py; mode 1: sample.py + save_image)."""
    _dense("image_to_uint8", "x", x_nchw, dim=4, contiguous=False)
    _gpu(x_nchw)
    x = x_nchw.contiguous()
    n, c, h, w = x.shape
    out = torch.empty((n, h, w, c), dtype=torch.uint8, device=x.device)
    ws = torch.empty((n, 2), dtype=torch.float32, device=x.device) if normalize_each else None
    L.check(L.load().mf_image_egress_u8(x.data_ptr(), out.data_ptr(), _ptr(ws), n, c, h, w, int(normalize_each), stream()), "mf_image_egress_u8")
    return out


def _drop_outputs(outputs) -> None:
    """the tensors a scheduler / solver step writes (x_t, x0, ...): the call goes by raw pointers, their fp16-pair mirrors (if any) are stale after it"""
    for t in outputs:
        drop_split(t)


def sched_step(args: L.MfSchedArgs, outputs=()) -> None:
    """`outputs`: the tensors the step writes (x_t, x0, ...): the call goes by raw pointers, their fp16-pair mirrors (if any) are stale after it"""
    _drop_outputs(outputs)
    L.check(L.load().mf_sched_step_f32(C.byref(args), stream()), "mf_sched_step_f32")


def sched_step_philox(args: L.MfSchedArgs, seed: int, draw_base: int, draw_stride: int, sample_offset: int, B: int, counter: torch.Tensor, outputs=()) -> None:
    """the tail of a denoise iteration in one launch (mf_sched_step_philox_f32): both noise draws in registers, the scheduler step, the
    step counter += 1.  counter: int32 [2] on the device = (step, ticket word)."""
    _gpu(counter)
    _drop_outputs(outputs)
    L.check(L.load().mf_sched_step_philox_f32(C.byref(args), seed & 0xFFFFFFFFFFFFFFFF, draw_base, draw_stride, sample_offset, B, counter.data_ptr(),
                                              counter.data_ptr() + 4, stream()), "mf_sched_step_philox_f32")


def image_ingress(x_nhwc: torch.Tensor) -> torch.Tensor:
    """[N,H,W,C] uint8 -> [N,C,H,W] float in [-1,1] on the device: (x/255 - 0.5)/0.5, bit-exact vs tF.normalize(x/255, 0.5, 0.5) (mf_image_ingress_u8)."""
    _gpu(x_nhwc)
    if x_nhwc.dtype != torch.uint8 or x_nhwc.dim() != 4:
        raise ValueError("image_ingress: a [N, H, W, C] uint8 tensor")
    x = x_nhwc.contiguous()
    n, h, w, c = x.shape
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_image_ingress_u8(x.data_ptr(), out.data_ptr(), n, c, h, w, stream()), "mf_image_ingress_u8")
    return out


def mask_maxpool(mask: torch.Tensor, factors) -> torch.Tensor:
    """[N,1,H,W] / [N,1,D,H,W] mask (bool / uint8: != 0; floating point: > 0.5) -> uint8 0 / 1 at 1 / factors of the size by max over each block
    (mf_mask_maxpool_u8); factors: one int per spatial axis"""
    if mask.dtype == torch.bool:
        mask = mask.to(torch.uint8)
    _gpu(mask)
    if mask.dim() not in (4, 5) or mask.shape[1] != 1 or len(factors) != mask.dim() - 2:
        raise ValueError(f"mask_maxpool: a [N, 1, ...] mask and one factor per spatial axis, got {tuple(mask.shape)} and {tuple(factors)}")
    is_f = mask.is_floating_point()
    m = (mask.to(torch.float32) if is_f else mask.to(torch.uint8)).contiguous()
    sp, f = list(m.shape[2:]), [int(v) for v in factors]
    if len(sp) == 2:
        sp, f = [1] + sp, [1] + f
    if any(v <= 0 or a % v for a, v in zip(sp, f)):
        raise ValueError(f"mask_maxpool: {tuple(mask.shape[2:])} is not a whole number of {tuple(factors)} blocks")
    out = torch.empty((m.shape[0], 1, *(a // v for a, v in zip(m.shape[2:], factors))), dtype=torch.uint8, device=m.device)
    L.check(L.load().mf_mask_maxpool_u8(m.data_ptr(), int(is_f), out.data_ptr(), m.shape[0], *sp, *f, stream()), "mf_mask_maxpool_u8")
    return out


def select_cells(mask: torch.Tensor, a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = where(mask, a, b): mask uint8 [N,1,...] one byte per cell, broadcast over the channels of a, b [N,C,...] fp32 (mf_select_cells_f32).
    `out` may be a or b."""
    _gpu(mask, a, b, out)
    a, b = a.contiguous(), b.contiguous()
    n, c = a.shape[0], a.shape[1]
    cells = a.numel() // max(1, n * c)
    if mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.numel() != n * cells or a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(f"select_cells: mask uint8 [N,1,cells...] against fp32 [N,C,cells...], got {tuple(mask.shape)} {mask.dtype} and {tuple(a.shape)}")
    if out is None:
        out = torch.empty_like(a)
    else:
        drop_split(out)
    L.check(L.load().mf_select_cells_f32(mask.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), n, c, cells, stream()), "mf_select_cells_f32")
    return out


def _window_rows(what: str, canvas_shape, windows_shape, plan):
    """the canvas rows of a windowed launch, after the shapes were checked against the plan"""
    sp = len(plan.canvas)
    ok = (len(canvas_shape) == 2 + sp and len(windows_shape) == 2 + sp and tuple(canvas_shape[2:]) == plan.canvas and tuple(windows_shape[2:]) == plan.window
          and canvas_shape[1] == windows_shape[1] and windows_shape[0] == canvas_shape[0] * plan.M and canvas_shape[0] > 0)
    if not ok:
        raise ValueError(f"{what}: canvas [B,C,{plan.canvas}] against windows [B*{plan.M},C,{plan.window}], got {tuple(canvas_shape)} and {tuple(windows_shape)}")
    return canvas_shape[0]


def window_gather(canvas: torch.Tensor, plan, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """canvas [B,C,(D,)H,W] fp32 -> windows [B*M,C,(d,)h,w]: row b*M + m is window m of `plan` (medfusion_amd.window.WindowPlan) cropped from
    canvas row b, bit for bit (mf_window_gather_f32)"""
    _gpu(canvas, out)
    if canvas.dtype != torch.float32:
        raise ValueError(f"window_gather: an fp32 canvas, got {canvas.dtype}")
    canvas = canvas.contiguous()
    if out is None:
        out = torch.empty((canvas.shape[0] * plan.M, canvas.shape[1], *plan.window), dtype=torch.float32, device=canvas.device)
    else:
        drop_split(out)
    B = _window_rows("window_gather", canvas.shape, out.shape, plan)
    if out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("window_gather: a contiguous fp32 output")
    desc = plan.desc(B, canvas.shape[1])
    L.check(L.load().mf_window_gather_f32(canvas.data_ptr(), out.data_ptr(), C.byref(desc), stream()), "mf_window_gather_f32")
    return out


def window_merge(windows: torch.Tensor, plan, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """windows [B*M,C,(d,)h,w] fp32 -> canvas [B,C,(D,)H,W]: per cell the weighted average of the covering windows in ascending window order, a
    cell under exactly one window that window's value bit for bit (mf_window_merge_f32)"""
    _gpu(windows, out)
    if windows.dtype != torch.float32 or windows.shape[0] % plan.M:
        raise ValueError(f"window_merge: fp32 windows, a whole number of canvases of {plan.M}, got {tuple(windows.shape)} {windows.dtype}")
    windows = windows.contiguous()
    if out is None:
        out = torch.empty((windows.shape[0] // plan.M, windows.shape[1], *plan.canvas), dtype=torch.float32, device=windows.device)
    else:
        drop_split(out)
    B = _window_rows("window_merge", out.shape, windows.shape, plan)
    if out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("window_merge: a contiguous fp32 output")
    desc = plan.desc(B, windows.shape[1])
    L.check(L.load().mf_window_merge_f32(windows.data_ptr(), out.data_ptr(), C.byref(desc), stream()), "mf_window_merge_f32")
    return out


def rows_minmax(x: torch.Tensor) -> torch.Tensor:
    """[N, ...] fp32 -> [N, 2]: the min and the max of every row (mf_rows_minmax_f32)"""
    _gpu(x)
    _need_f32(x)
    x = x.contiguous()
    n = x.shape[0]
    out = torch.empty((n, 2), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_rows_minmax_f32(x.data_ptr(), out.data_ptr(), n, x.numel() // n, stream()), "mf_rows_minmax_f32")
    return out


def avgpool2_planes(x: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] fp32 -> [N, C, H // 2, W // 2] by 2 x 2 means, an odd trailing row or column dropped (mf_avgpool2_planes_f32)"""
    _gpu(x)
    _need_f32(x)
    x = x.contiguous()
    n, c, h, w = x.shape
    out = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_avgpool2_planes_f32(x.data_ptr(), out.data_ptr(), n * c, h, w, stream()), "mf_avgpool2_planes_f32")
    return out


def make_ssim_desc(P: int, C_: int, H: int, W: int, Nx: int, Ny: int, taps, k1: float, k2: float, data_range: Optional[float], indexed: int = 0,
                   want_mse: bool = False) -> L.MfSsimDesc:
    """data_range=None: L of every pair from the banks' min / max rows on the device"""
    d = L.MfSsimDesc(P=P, C=C_, H=H, W=W, Nx=Nx, Ny=Ny, k=len(taps), indexed=indexed, want_mse=int(want_mse), range_on_device=int(data_range is None),
                     k1=k1, k2=k2, data_range=0.0 if data_range is None else data_range)
    for j, v in enumerate(taps[:L.SSIM_MAX_K]):
        d.taps[j] = v
    return d


def ssim_ok(d: L.MfSsimDesc) -> bool:
    return bool(L.load().mf_ssim_ok(C.byref(d)))


def ssim_pairs(xbank: torch.Tensor, ybank: torch.Tensor, d: L.MfSsimDesc, sim: Optional[torch.Tensor], cs: Optional[torch.Tensor],
               mse: Optional[torch.Tensor] = None, ix: Optional[torch.Tensor] = None, iy: Optional[torch.Tensor] = None,
               minmax_x: Optional[torch.Tensor] = None, minmax_y: Optional[torch.Tensor] = None) -> None:
    """One scale of d.P pairs (mf_ssim_pairs_f32 + mf_ssim_finish_f32): pair p is xbank[ix[p]] against ybank[iy[p]] (contiguous fp32 [N, C, H, W] banks,
    int32 indices or None for the identity); sim / cs: fp32 views with one element per pair (any stride: a column of a [P, S] table), mse: [P]."""
    _gpu(xbank, ybank, sim, cs, mse, ix, iy, minmax_x, minmax_y)
    _need_f32(xbank, ybank)
    if not (xbank.is_contiguous() and ybank.is_contiguous()) or tuple(xbank.shape[1:]) != (d.C, d.H, d.W) or tuple(ybank.shape[1:]) != (d.C, d.H, d.W) \
            or xbank.shape[0] != d.Nx or ybank.shape[0] != d.Ny:
        raise ValueError(f"ssim_pairs: contiguous banks [{d.Nx}|{d.Ny}, {d.C}, {d.H}, {d.W}], got {tuple(xbank.shape)} and {tuple(ybank.shape)}")
    for name, idx in (("ix", ix), ("iy", iy)):
        if idx is not None and (idx.dtype != torch.int32 or not idx.is_contiguous() or idx.numel() != d.P):
            raise ValueError(f"ssim_pairs: {name} is a contiguous int32 [{d.P}]")
    stride = None
    for name, o in (("sim", sim), ("cs", cs)):
        if o is None:
            continue
        if o.dtype != torch.float32 or o.dim() != 1 or o.shape[0] != d.P or (stride is not None and o.stride(0) != stride and d.P > 1):
            raise ValueError(f"ssim_pairs: {name} is an fp32 view of {d.P} elements, of sim's stride")
        stride = o.stride(0) if d.P > 1 else 1
    if mse is not None and (mse.dtype != torch.float32 or not mse.is_contiguous() or mse.numel() != d.P):
        raise ValueError(f"ssim_pairs: mse is a contiguous fp32 [{d.P}]")
    h = L.load()
    need = h.mf_ssim_workspace_bytes(C.byref(d))
    if need == 0:
        raise ValueError(f"ssim_pairs: descriptor refused: {L.last_error()}")
    ws = Workspace.get(need, xbank.device)
    L.check(h.mf_ssim_pairs_f32(xbank.data_ptr(), ybank.data_ptr(), _ptr(ix), _ptr(iy), _ptr(minmax_x), _ptr(minmax_y), ws.data_ptr(), ws.numel(),
                                C.byref(d), stream()), "mf_ssim_pairs_f32")
    L.check(h.mf_ssim_finish_f32(ws.data_ptr(), _ptr(sim), _ptr(cs), _ptr(mse), stride or 1, C.byref(d), stream()), "mf_ssim_finish_f32")


def avgpool2_volumes(x: torch.Tensor) -> torch.Tensor:
    """[N, C, D, H, W] fp32 -> [N, C, D // 2, H // 2, W // 2] by 2 x 2 x 2 means, an odd trailing plane, row or column dropped (mf_avgpool2_volumes_f32)"""
    _gpu(x)
    _need_f32(x)
    x = x.contiguous()
    n, c, d, h, w = x.shape
    out = torch.empty((n, c, d // 2, h // 2, w // 2), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_avgpool2_volumes_f32(x.data_ptr(), out.data_ptr(), n * c, d, h, w, stream()), "mf_avgpool2_volumes_f32")
    return out


def make_ssim3d_desc(P: int, C_: int, D: int, H: int, W: int, Nx: int, Ny: int, taps, k1: float, k2: float, data_range: Optional[float],
                     indexed: int = 0, want_mse: bool = False) -> L.MfSsim3dDesc:
    """data_range=None: L of every pair from the banks' min / max rows on the device"""
    d = L.MfSsim3dDesc(P=P, C=C_, D=D, H=H, W=W, Nx=Nx, Ny=Ny, k=len(taps), indexed=indexed, want_mse=int(want_mse),
                       range_on_device=int(data_range is None), k1=k1, k2=k2, data_range=0.0 if data_range is None else data_range)
    for j, v in enumerate(taps[:L.SSIM_MAX_K]):
        d.taps[j] = v
    return d


def ssim3d_ok(d: L.MfSsim3dDesc) -> bool:
    return bool(L.load().mf_ssim3d_ok(C.byref(d)))


def ssim3d_pairs(xbank: torch.Tensor, ybank: torch.Tensor, d: L.MfSsim3dDesc, sim: Optional[torch.Tensor], cs: Optional[torch.Tensor],
                 mse: Optional[torch.Tensor] = None, ix: Optional[torch.Tensor] = None, iy: Optional[torch.Tensor] = None,
                 minmax_x: Optional[torch.Tensor] = None, minmax_y: Optional[torch.Tensor] = None) -> None:
    """One scale of d.P volume pairs (mf_ssim3d_pairs_f32 + mf_ssim3d_finish_f32): pair p is xbank[ix[p]] against ybank[iy[p]] (contiguous fp32
    [N, C, D, H, W] banks, int32 indices or None for the identity); sim / cs: fp32 views with one element per pair (any stride), mse: [P]."""
    _gpu(xbank, ybank, sim, cs, mse, ix, iy, minmax_x, minmax_y)
    _need_f32(xbank, ybank)
    want = (d.C, d.D, d.H, d.W)
    if not (xbank.is_contiguous() and ybank.is_contiguous()) or tuple(xbank.shape[1:]) != want or tuple(ybank.shape[1:]) != want \
            or xbank.shape[0] != d.Nx or ybank.shape[0] != d.Ny:
        raise ValueError(f"ssim3d_pairs: contiguous banks [{d.Nx}|{d.Ny}, {d.C}, {d.D}, {d.H}, {d.W}], got {tuple(xbank.shape)} and {tuple(ybank.shape)}")
    for name, idx in (("ix", ix), ("iy", iy)):
        if idx is not None and (idx.dtype != torch.int32 or not idx.is_contiguous() or idx.numel() != d.P):
            raise ValueError(f"ssim3d_pairs: {name} is a contiguous int32 [{d.P}]")
    stride = None
    for name, o in (("sim", sim), ("cs", cs)):
        if o is None:
            continue
        if o.dtype != torch.float32 or o.dim() != 1 or o.shape[0] != d.P or (stride is not None and o.stride(0) != stride and d.P > 1):
            raise ValueError(f"ssim3d_pairs: {name} is an fp32 view of {d.P} elements, of sim's stride")
        stride = o.stride(0) if d.P > 1 else 1
    if mse is not None and (mse.dtype != torch.float32 or not mse.is_contiguous() or mse.numel() != d.P):
        raise ValueError(f"ssim3d_pairs: mse is a contiguous fp32 [{d.P}]")
    h = L.load()
    need = h.mf_ssim3d_workspace_bytes(C.byref(d))
    if need == 0:
        raise ValueError(f"ssim3d_pairs: descriptor refused: {L.last_error()}")
    ws = Workspace.get(need, xbank.device)
    L.check(h.mf_ssim3d_pairs_f32(xbank.data_ptr(), ybank.data_ptr(), _ptr(ix), _ptr(iy), _ptr(minmax_x), _ptr(minmax_y), ws.data_ptr(), ws.numel(),
                                  C.byref(d), stream()), "mf_ssim3d_pairs_f32")
    L.check(h.mf_ssim3d_finish_f32(ws.data_ptr(), _ptr(sim), _ptr(cs), _ptr(mse), stride or 1, C.byref(d), stream()), "mf_ssim3d_finish_f32")


def make_fidelity_desc(N: int, M: int, D: int, knn: int = 1, splits: int = 1, same_bank: bool = False) -> L.MfFidelityDesc:
    return L.MfFidelityDesc(N=N, M=M, D=D, knn=knn, splits=splits, same_bank=int(same_bank))


def fidelity_ok(d: L.MfFidelityDesc) -> bool:
    return bool(L.load().mf_fidelity_ok(C.byref(d)))


def fidelity_workspace_bytes(d: L.MfFidelityDesc) -> int:
    """0 for a descriptor the library refuses (host only)"""
    return int(L.load().mf_fidelity_workspace_bytes(C.byref(d)))


def _feature_bank(what: str, x: torch.Tensor) -> None:
    _gpu(x)
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous():
        raise ValueError(f"{what}: a contiguous fp32 [rows, D] bank, got {tuple(x.shape)} {x.dtype}")


def _feature_rows(what: str, v: torch.Tensor, n: int) -> None:
    _gpu(v)
    if v.dtype != torch.float32 or not v.is_contiguous() or v.numel() != n:
        raise ValueError(f"{what}: a contiguous fp32 [{n}]")


def feat_colmean(x: torch.Tensor) -> torch.Tensor:
    """[N, D] -> [D]: the fp64 column means rounded to fp32, the pivot of the distances (mf_feat_colmean_f32)"""
    _feature_bank("feat_colmean", x)
    out = torch.empty((x.shape[1],), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_feat_colmean_f32(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], stream()), "mf_feat_colmean_f32")
    return out


def feat_norms(x: torch.Tensor, pivot: torch.Tensor) -> torch.Tensor:
    """[N, D], [D] -> [N]: the fp64 sums of fl32(x - pivot)^2 rounded to fp32 (mf_feat_norms_f32)"""
    _feature_bank("feat_norms", x)
    _feature_rows("feat_norms: pivot", pivot, x.shape[1])
    out = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_feat_norms_f32(x.data_ptr(), pivot.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], stream()), "mf_feat_norms_f32")
    return out


def feat_sqdist(x: torch.Tensor, nx: torch.Tensor, y: torch.Tensor, ny: torch.Tensor, pivot: torch.Tensor, same_bank: bool = False) -> torch.Tensor:
    """the [N, M] matrix of squared distances between the rows of x and of y (mf_feat_sqdist_f32); same_bank: y is x, the diagonal exactly 0"""
    _feature_bank("feat_sqdist", x)
    _feature_bank("feat_sqdist", y)
    d = make_fidelity_desc(x.shape[0], y.shape[0], x.shape[1], 1, 1, same_bank)
    if y.shape[1] != d.D or not fidelity_ok(d):
        raise ValueError(f"feat_sqdist: banks {tuple(x.shape)} and {tuple(y.shape)}: {L.last_error() if y.shape[1] == d.D else 'D differs'}")
    _feature_rows("feat_sqdist: nx", nx, d.N)
    _feature_rows("feat_sqdist: ny", ny, d.M)
    _feature_rows("feat_sqdist: pivot", pivot, d.D)
    out = torch.empty((d.N, d.M), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_feat_sqdist_f32(x.data_ptr(), nx.data_ptr(), y.data_ptr(), ny.data_ptr(), pivot.data_ptr(), out.data_ptr(), C.byref(d), stream()),
            "mf_feat_sqdist_f32")
    return out


def knn_radii_sq(x: torch.Tensor, nx: torch.Tensor, pivot: torch.Tensor, knn: int, splits: int) -> torch.Tensor:
    """[N]: the (knn + 1)-th smallest squared distance of every row of x to the rows of x, itself included as 0 (mf_knn_partial_f32 +
    mf_knn_finish_f32); the matrix is never written"""
    _feature_bank("knn_radii_sq", x)
    d = make_fidelity_desc(x.shape[0], x.shape[0], x.shape[1], knn, splits, True)
    h = L.load()
    need = h.mf_fidelity_workspace_bytes(C.byref(d))
    if need == 0:
        raise ValueError(f"knn_radii_sq: descriptor refused: {L.last_error()}")
    _feature_rows("knn_radii_sq: nx", nx, d.N)
    _feature_rows("knn_radii_sq: pivot", pivot, d.D)
    ws = Workspace.get(need, x.device)
    out = torch.empty((d.N,), dtype=torch.float32, device=x.device)
    L.check(h.mf_knn_partial_f32(x.data_ptr(), nx.data_ptr(), pivot.data_ptr(), ws.data_ptr(), ws.numel(), C.byref(d), stream()), "mf_knn_partial_f32")
    L.check(h.mf_knn_finish_f32(ws.data_ptr(), out.data_ptr(), C.byref(d), stream()), "mf_knn_finish_f32")
    return out


def manifold_hits(ref: torch.Tensor, nref: torch.Tensor, radii_sq: torch.Tensor, query: torch.Tensor, nquery: torch.Tensor, pivot: torch.Tensor,
                  splits: int, want_hits: bool = True):
    """-> (hit uint8 [M] or None, count int32 [1]): is query j closer to some ref row i than that row's radius, squared values, strict
    (mf_manifold_partial_f32 + mf_manifold_finish_f32); the matrix is never written"""
    _feature_bank("manifold_hits", ref)
    _feature_bank("manifold_hits", query)
    d = make_fidelity_desc(ref.shape[0], query.shape[0], ref.shape[1], 1, splits, False)
    h = L.load()
    need = h.mf_fidelity_workspace_bytes(C.byref(d)) if query.shape[1] == d.D else 0
    if need == 0:
        raise ValueError(f"manifold_hits: banks {tuple(ref.shape)} and {tuple(query.shape)}: {L.last_error() if query.shape[1] == d.D else 'D differs'}")
    _feature_rows("manifold_hits: nref", nref, d.N)
    _feature_rows("manifold_hits: radii_sq", radii_sq, d.N)
    _feature_rows("manifold_hits: nquery", nquery, d.M)
    _feature_rows("manifold_hits: pivot", pivot, d.D)
    ws = Workspace.get(need, ref.device)
    hit = torch.empty((d.M,), dtype=torch.uint8, device=ref.device) if want_hits else None
    count = torch.empty((1,), dtype=torch.int32, device=ref.device)
    L.check(h.mf_manifold_partial_f32(ref.data_ptr(), nref.data_ptr(), radii_sq.data_ptr(), query.data_ptr(), nquery.data_ptr(), pivot.data_ptr(),
                                      ws.data_ptr(), ws.numel(), C.byref(d), stream()), "mf_manifold_partial_f32")
    L.check(h.mf_manifold_finish_f32(ws.data_ptr(), _ptr(hit), count.data_ptr(), C.byref(d), stream()), "mf_manifold_finish_f32")
    return hit, count


def nn_ok(d: L.MfFidelityDesc) -> bool:
    return bool(L.load().mf_nn_ok(C.byref(d)))


def nn_workspace_bytes(d: L.MfFidelityDesc) -> int:
    """0 for a descriptor the neighbour calls refuse (host only)"""
    return int(L.load().mf_nn_workspace_bytes(C.byref(d)))


def nn_search(query: torch.Tensor, nquery: torch.Tensor, ref: torch.Tensor, nref: torch.Tensor, pivot: torch.Tensor, k: int, splits: int,
              exclude_self: bool = False):
    """-> (d2 fp32 [M, k], index int32 [M, k]): the k nearest rows of ref for every row of query, ascending by (d2, index) (mf_nn_partial_f32 +
    mf_nn_finish_f32); exclude_self: ref IS query and a row is not its own neighbour.  The matrix is never written"""
    _feature_bank("nn_search", query)
    _feature_bank("nn_search", ref)
    d = make_fidelity_desc(ref.shape[0], query.shape[0], ref.shape[1], k, splits, exclude_self)
    h = L.load()
    need = h.mf_nn_workspace_bytes(C.byref(d)) if query.shape[1] == d.D else 0
    if need == 0:
        raise ValueError(f"nn_search: banks {tuple(query.shape)} and {tuple(ref.shape)}, k={k}: {L.last_error() if query.shape[1] == d.D else 'D differs'}")
    _feature_rows("nn_search: nquery", nquery, d.M)
    _feature_rows("nn_search: nref", nref, d.N)
    _feature_rows("nn_search: pivot", pivot, d.D)
    ws = Workspace.get(need, ref.device)
    d2 = torch.empty((d.M, k), dtype=torch.float32, device=ref.device)
    index = torch.empty((d.M, k), dtype=torch.int32, device=ref.device)
    L.check(h.mf_nn_partial_f32(query.data_ptr(), nquery.data_ptr(), ref.data_ptr(), nref.data_ptr(), pivot.data_ptr(), ws.data_ptr(), ws.numel(),
                                C.byref(d), stream()), "mf_nn_partial_f32")
    L.check(h.mf_nn_finish_f32(ws.data_ptr(), d2.data_ptr(), index.data_ptr(), C.byref(d), stream()), "mf_nn_finish_f32")
    return d2, index


def pair_sqdist(query: torch.Tensor, ref: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """[M, k]: the exact squared distance of query row j and ref row index[j, p], the sum in fp64, rounded once (mf_pair_sqdist_f32)"""
    _feature_bank("pair_sqdist", query)
    _feature_bank("pair_sqdist", ref)
    _gpu(index)
    if index.dtype != torch.int32 or index.dim() != 2 or index.shape[0] != query.shape[0] or not index.is_contiguous():
        raise ValueError(f"pair_sqdist: a contiguous int32 [{query.shape[0]}, k] index, got {tuple(index.shape)} {index.dtype}")
    d = make_fidelity_desc(ref.shape[0], query.shape[0], ref.shape[1], index.shape[1], 1, False)
    if query.shape[1] != d.D or not nn_ok(d):
        raise ValueError(f"pair_sqdist: banks {tuple(query.shape)} and {tuple(ref.shape)}, k={d.knn}: {L.last_error() if query.shape[1] == d.D else 'D differs'}")
    out = torch.empty(tuple(index.shape), dtype=torch.float32, device=ref.device)
    L.check(L.load().mf_pair_sqdist_f32(query.data_ptr(), ref.data_ptr(), index.data_ptr(), out.data_ptr(), C.byref(d), stream()), "mf_pair_sqdist_f32")
    return out


def manifold_counts(ref: torch.Tensor, nref: torch.Tensor, radii_sq: torch.Tensor, query: torch.Tensor, nquery: torch.Tensor, pivot: torch.Tensor,
                    splits: int, want_counts: bool = True):
    """-> (count int32 [M] or None, total int64 [1]): how many ref rows i hold query j inside their ball, d2 < radii_sq[i], strict
    (mf_manifold_count_partial_f32 + mf_manifold_count_finish_f32); the matrix is never written"""
    _feature_bank("manifold_counts", ref)
    _feature_bank("manifold_counts", query)
    d = make_fidelity_desc(ref.shape[0], query.shape[0], ref.shape[1], 1, splits, False)
    h = L.load()
    if query.shape[1] != d.D or not nn_ok(d):
        raise ValueError(f"manifold_counts: banks {tuple(ref.shape)} and {tuple(query.shape)}: {L.last_error() if query.shape[1] == d.D else 'D differs'}")
    _feature_rows("manifold_counts: nref", nref, d.N)
    _feature_rows("manifold_counts: radii_sq", radii_sq, d.N)
    _feature_rows("manifold_counts: nquery", nquery, d.M)
    _feature_rows("manifold_counts: pivot", pivot, d.D)
    ws = Workspace.get((splits * d.M * 4 + 15) // 16 * 16, ref.device)         # int32 [splits][M]: a part of mf_nn_workspace_bytes
    count = torch.empty((d.M,), dtype=torch.int32, device=ref.device) if want_counts else None
    total = torch.empty((1,), dtype=torch.int64, device=ref.device)
    L.check(h.mf_manifold_count_partial_f32(ref.data_ptr(), nref.data_ptr(), radii_sq.data_ptr(), query.data_ptr(), nquery.data_ptr(), pivot.data_ptr(),
                                            ws.data_ptr(), ws.numel(), C.byref(d), stream()), "mf_manifold_count_partial_f32")
    L.check(h.mf_manifold_count_finish_f32(ws.data_ptr(), _ptr(count), total.data_ptr(), C.byref(d), stream()), "mf_manifold_count_finish_f32")
    return count, total


def make_ksum_desc(N: int, M: int, D: int, S: int = 1, sa: int = None, sb: int = None, kernel: int = L.KERNEL_POLY, degree: int = 3,
                   gamma: float = 1.0, coef0: float = 1.0, same_bank: int = 0) -> L.MfKernelSumDesc:
    """sa / sb None: the whole bank"""
    return L.MfKernelSumDesc(N=N, M=M, D=D, S=S, sa=N if sa is None else sa, sb=M if sb is None else sb, kernel=kernel, degree=degree, gamma=gamma,
                             coef0=coef0, same_bank=int(same_bank), reserved=0)


def ksum_ok(d: L.MfKernelSumDesc) -> bool:
    return bool(L.load().mf_ksum_ok(C.byref(d)))


def ksum_workspace_bytes(d: L.MfKernelSumDesc) -> int:
    """0 for a descriptor the kernel sums refuse (host only)"""
    return int(L.load().mf_ksum_workspace_bytes(C.byref(d)))


def _index_lists(what: str, index, S: int, rows: int, like: torch.Tensor) -> None:
    if index is None:
        return
    _gpu(index)
    if index.dtype != torch.int32 or not index.is_contiguous() or tuple(index.shape) != (S, rows) or index.device != like.device:
        raise ValueError(f"{what}: a contiguous int32 [{S}, {rows}] index list on the banks' device, got {tuple(index.shape)} {index.dtype}")


def kernel_sums(a: torch.Tensor, na, ia, b: torch.Tensor, nb, ib, pivot: torch.Tensor, d: L.MfKernelSumDesc) -> torch.Tensor:
    """fp64 [S]: the sum of k over the pairs of rows ia[s] of a and ib[s] of b (mf_ksum_partial_f32 + mf_ksum_finish_f64); na / nb: the norms, for
    the rbf kernel; ia / ib None: the identity.  The matrix is never written"""
    _feature_bank("kernel_sums", a)
    _feature_bank("kernel_sums", b)
    h = L.load()
    fits = a.shape == (d.N, d.D) and b.shape == (d.M, d.D)
    need = h.mf_ksum_workspace_bytes(C.byref(d)) if fits else 0
    if need == 0:
        raise ValueError(f"kernel_sums: banks {tuple(a.shape)} and {tuple(b.shape)}: {L.last_error() if fits else 'not the shapes of the descriptor'}")
    _feature_rows("kernel_sums: pivot", pivot, d.D)
    if d.kernel == L.KERNEL_RBF:
        _feature_rows("kernel_sums: na", na, d.N)
        _feature_rows("kernel_sums: nb", nb, d.M)
    _index_lists("kernel_sums: ia", ia, d.S, d.sa, a)
    _index_lists("kernel_sums: ib", ib, d.S, d.sb, b)
    ws = Workspace.get(need, a.device)
    out = torch.empty((d.S,), dtype=torch.float64, device=a.device)
    L.check(h.mf_ksum_partial_f32(a.data_ptr(), _ptr(na), _ptr(ia), b.data_ptr(), _ptr(nb), _ptr(ib), pivot.data_ptr(), ws.data_ptr(), ws.numel(),
                                  C.byref(d), stream()), "mf_ksum_partial_f32")
    L.check(h.mf_ksum_finish_f64(ws.data_ptr(), out.data_ptr(), C.byref(d), stream()), "mf_ksum_finish_f64")
    return out


def feat_kernel(x: torch.Tensor, nx, y: torch.Tensor, ny, pivot: torch.Tensor, d: L.MfKernelSumDesc) -> torch.Tensor:
    """the [N, M] matrix of k between the rows of x and of y (mf_feat_kernel_f32); nx / ny: the norms, for the rbf kernel"""
    _feature_bank("feat_kernel", x)
    _feature_bank("feat_kernel", y)
    fits = x.shape == (d.N, d.D) and y.shape == (d.M, d.D)
    if not fits or not ksum_ok(d):
        raise ValueError(f"feat_kernel: banks {tuple(x.shape)} and {tuple(y.shape)}: {L.last_error() if fits else 'not the shapes of the descriptor'}")
    _feature_rows("feat_kernel: pivot", pivot, d.D)
    if d.kernel == L.KERNEL_RBF:
        _feature_rows("feat_kernel: nx", nx, d.N)
        _feature_rows("feat_kernel: ny", ny, d.M)
    out = torch.empty((d.N, d.M), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_feat_kernel_f32(x.data_ptr(), _ptr(nx), y.data_ptr(), _ptr(ny), pivot.data_ptr(), out.data_ptr(), C.byref(d), stream()),
            "mf_feat_kernel_f32")
    return out


def sched_step_blend(args: L.MfSchedArgs, blend: L.MfSchedBlend, outputs=()) -> None:
    """sched_step with the kept cells of x_t_out replaced by the known latent at the next timestep (mf_sched_step_blend_f32)"""
    _drop_outputs(outputs)
    L.check(L.load().mf_sched_step_blend_f32(C.byref(args), C.byref(blend), stream()), "mf_sched_step_blend_f32")


def sched_step_philox_blend(args: L.MfSchedArgs, blend: L.MfSchedBlend, seed: int, draw_base: int, draw_stride: int, sample_offset: int, B: int,
                            counter: torch.Tensor, outputs=()) -> None:
    """sched_step_philox with the same select, still one launch (mf_sched_step_philox_blend_f32)"""
    _gpu(counter)
    _drop_outputs(outputs)
    L.check(L.load().mf_sched_step_philox_blend_f32(C.byref(args), seed & 0xFFFFFFFFFFFFFFFF, draw_base, draw_stride, sample_offset, B, counter.data_ptr(),
                                                    counter.data_ptr() + 4, C.byref(blend), stream()), "mf_sched_step_philox_blend_f32")


def solver_step(args: L.MfSolverArgs, blend: Optional[L.MfSchedBlend] = None, outputs=()) -> None:
    """the deterministic solver step in one launch (mf_solver_step_f32; with `blend` mf_solver_step_blend_f32: the inpainting select on x_t_out).
    `outputs` as in sched_step."""
    _drop_outputs(outputs)
    if blend is None:
        L.check(L.load().mf_solver_step_f32(C.byref(args), stream()), "mf_solver_step_f32")
    else:
        L.check(L.load().mf_solver_step_blend_f32(C.byref(args), C.byref(blend), stream()), "mf_solver_step_blend_f32")


def solver_step_traj(args: L.MfSolverArgs, traj: L.MfSolverTraj, outputs=()) -> None:
    """the solver step that records its x_t_out into, or takes its kept cells from, a slot of a trajectory buffer indexed by the step
    (mf_solver_step_traj_f32).  `outputs` as in sched_step."""
    _drop_outputs(outputs)
    L.check(L.load().mf_solver_step_traj_f32(C.byref(args), C.byref(traj), stream()), "mf_solver_step_traj_f32")


def solver_step_noise(args: L.MfSolverArgs, nz: L.MfSolverNoise, blend: Optional[L.MfSchedBlend] = None, outputs=()) -> None:
    """the stochastic solver step in one launch (mf_solver_step_noise_f32): solver_step, then x_t_out += scale[step] * eps, eps the caller's draw
    or Philox inside the launch (nz.noise None), then the inpainting select when `blend` is given.  `outputs` as in sched_step."""
    _drop_outputs(outputs)
    L.check(L.load().mf_solver_step_noise_f32(C.byref(args), C.byref(nz), None if blend is None else C.byref(blend), stream()), "mf_solver_step_noise_f32")


def check_rows_t(what: str, t, B: int) -> None:
    """t: the timestep of every row as the loss kernels read it -- contiguous int32 [B]"""
    _dense(what, "t", t, dtype=torch.int32, shape=(B,))


def philox_in_launch_ok(*ts) -> bool:
    """may a launch over these [B, ...] tensors generate its draw in registers?  mf_solver_step_noise_f32's rule: elements per sample a multiple
    of 4 and every tensor 16-byte aligned (None: absent)"""
    ts = [t for t in ts if t is not None]
    return all(t.data_ptr() % 16 == 0 for t in ts) and (ts[0].numel() // max(1, ts[0].shape[0])) % 4 == 0


def diffuse_rows(x_0: torch.Tensor, t: torch.Tensor, sqrt_ac: torch.Tensor, sqrt_1m_ac: torch.Tensor, eps: Optional[torch.Tensor] = None, philox=None,
                 eps_out: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, outputs=()) -> torch.Tensor:
    """x_t[b] = sqrt_ac[t_b] x_0[b] + sqrt_1m_ac[t_b] eps[b] in one launch (mf_diffuse_rows_f32; rows with t < 0 return x_0, t >= T eps).  eps: the
    caller's draw, or philox = (seed, draw, sample_offset): the draw is generated in registers (eps_out, optional, receives it).  t: int32 [B] on
    the device; the two tables fp32 [T].  `outputs` as in sched_step."""
    what = "diffuse_rows"
    _dense(what, "x_0", x_0)
    B = x_0.shape[0]
    check_rows_t(what, t, B)
    _dense(what, "sqrt_ac", sqrt_ac, dim=1)
    _dense(what, "sqrt_1m_ac", sqrt_1m_ac, shape=sqrt_ac.shape)
    if (eps is None) == (philox is None):
        raise RuntimeError("medfusion_amd: diffuse_rows: either eps or philox=(seed, draw, sample_offset)")
    for name, v in (("eps", eps), ("eps_out", eps_out), ("out", out)):
        if v is not None:
            _dense(what, name, v, shape=x_0.shape, written=name != "eps")
    _gpu(x_0, t, sqrt_ac, sqrt_1m_ac, eps, eps_out, out)
    if out is None:
        out = torch.empty_like(x_0)
    _drop_outputs((out, eps_out, *outputs))
    seed, draw, offset = philox if philox is not None else (0, 0, 0)
    a = L.MfDiffuseArgs(x_0.data_ptr(), _ptr(eps), out.data_ptr(), _ptr(eps_out), t.data_ptr(), sqrt_ac.data_ptr(), sqrt_1m_ac.data_ptr(), x_0.numel() // B,
                        seed & 0xFFFFFFFFFFFFFFFF, offset, draw, sqrt_ac.shape[0], B, 0)
    L.check(L.load().mf_diffuse_rows_f32(C.byref(a), stream()), "mf_diffuse_rows_f32")
    return out


def loss_pool_factor(pred_shape, target_shape) -> int:
    """the integer factor f by which a [B, C, spatial...] target is average-pooled onto pred: every spatial side of the target f times pred's
    (ValueError otherwise: F.interpolate(mode='area') between sides that do not divide is not this pooling)"""
    ps, ts = tuple(pred_shape), tuple(target_shape)
    if len(ps) != len(ts) or len(ps) not in (4, 5) or ps[:2] != ts[:2]:
        raise ValueError(f"denoise_loss: pred {ps} against target {ts}: [B, C, spatial...] tensors of one rank, batch and channel count")
    if any(p < 1 for p in ps[2:]) or ts[2] % ps[2] or ts[2] < ps[2]:
        raise ValueError(f"denoise_loss: pred {ps} against target {ts}: the target's side must be a multiple of pred's")
    f = ts[2] // ps[2]
    if any(tt != f * pp for pp, tt in zip(ps[2:], ts[2:])):
        raise ValueError(f"denoise_loss: pred {ps} against target {ts}: every side of the target must be {f} times pred's")
    return f


def _loss_sums(entry: str, finish: str, launch, B: int, per: int, values: int, device) -> torch.Tensor:
    lib = L.load()
    need = lib.mf_loss_workspace_bytes(B, per, values)
    ws = Workspace.get(need, device)
    out = torch.empty((B, values), dtype=torch.float64, device=device)
    L.check(launch(lib, ws.data_ptr(), need), entry)
    L.check(getattr(lib, finish)(ws.data_ptr(), out.data_ptr(), B, per, stream()), finish)
    return out


def denoise_loss(pred: torch.Tensor, target: Optional[torch.Tensor] = None, philox=None, target_shape=None) -> torch.Tensor:
    """[B, 2] fp64 = per row (sum |pred - target|, sum (pred - target)^2), the target average-pooled on the fly onto pred's extents
    (mf_denoise_loss_f32 + mf_denoise_loss_finish_f32; partials in the per-stream workspace).  target: a [B, C, spatial...] tensor, or
    philox = (seed, draw, sample_offset) with target_shape: the draw mf_philox_normal_f32 would write there, regenerated in registers."""
    what = "denoise_loss"
    _dense(what, "pred", pred)
    if (target is None) == (philox is None):
        raise RuntimeError("medfusion_amd: denoise_loss: either target or philox=(seed, draw, sample_offset) with target_shape")
    if target is not None:
        _dense(what, "target", target)
        target_shape = target.shape
    f = loss_pool_factor(pred.shape, target_shape)
    _gpu(pred, target)
    B, Cc = pred.shape[0], pred.shape[1]
    sp = tuple(pred.shape[2:])
    seed, draw, offset = philox if philox is not None else (0, 0, 0)
    d = L.MfLossDesc(B, Cc, len(sp), (C.c_int32 * 3)(*((1,) * (3 - len(sp)) + sp)), f, draw, seed & 0xFFFFFFFFFFFFFFFF, offset)
    return _loss_sums("mf_denoise_loss_f32", "mf_denoise_loss_finish_f32",
                      lambda lib, ws, n: lib.mf_denoise_loss_f32(pred.data_ptr(), _ptr(target), C.byref(d), ws, n, stream()), B, pred.numel() // B, 2, pred.device)


VARIANCE_TABLES = ("betas", "posterior_variance", "posterior_mean_coef1", "posterior_mean_coef2", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")


def variance_loss(x_0: torch.Tensor, x_t: torch.Tensor, x_T: torch.Tensor, pred: torch.Tensor, pred_var: torch.Tensor, t: torch.Tensor, tables: dict,
                  objective: int, clip_x0: bool) -> torch.Tensor:
    """[B, 3] fp64 = per row (sum kl, sum nll, sum var_scale) of the learned-variance terms of the validation step (mf_variance_loss_f32 +
    mf_variance_loss_finish_f32).  tables: the scheduler's device tables by buffer name (VARIANCE_TABLES); t int32 [B] on the device."""
    what = "variance_loss"
    _dense(what, "x_0", x_0)
    for name, v in (("x_t", x_t), ("x_T", x_T), ("pred", pred), ("pred_var", pred_var)):
        _dense(what, name, v, shape=x_0.shape)
    B = x_0.shape[0]
    check_rows_t(what, t, B)
    tabs = [tables[n] for n in VARIANCE_TABLES]
    for n, v in zip(VARIANCE_TABLES, tabs):
        _dense(what, n, v, shape=tabs[0].shape, dim=1)
    _gpu(x_0, x_t, x_T, pred, pred_var, t, *tabs)
    a = L.MfVarianceLossArgs(x_0.data_ptr(), x_t.data_ptr(), x_T.data_ptr(), pred.data_ptr(), pred_var.data_ptr(), t.data_ptr(), *(v.data_ptr() for v in tabs),
                             x_0.numel() // B, tabs[0].shape[0], B, int(objective), int(bool(clip_x0)))
    return _loss_sums("mf_variance_loss_f32", "mf_variance_loss_finish_f32", lambda lib, ws, n: lib.mf_variance_loss_f32(C.byref(a), ws, n, stream()), B,
                      x_0.numel() // B, 3, x_0.device)


def guide_table(rows, device) -> torch.Tensor:
    """the device table of the guidance stage: a list of L.MfGuideStep, one per executed iteration -> uint8 tensor"""
    arr = (L.MfGuideStep * len(rows))(*rows)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone().to(device)


def guide_workspace(B: int, n: int, device) -> Optional[torch.Tensor]:
    """the caller-owned workspace of mf_guide_f32 for B rows of n elements (None: a row fits one workgroup, none is needed).  A tensor of its own,
    not the per-stream scratch: it is made before a recorded iteration and must not move under it."""
    need = L.load().mf_guide_workspace_bytes(B, n)
    return torch.empty(need, dtype=torch.uint8, device=device) if need else None


def guide(pred: torch.Tensor, table: torch.Tensor, *, pred_uncond: Optional[torch.Tensor] = None, x_t: Optional[torch.Tensor] = None, step=0,
          objective: int = 0, stages: int = 0, out: Optional[torch.Tensor] = None, scale_out: Optional[torch.Tensor] = None,
          limit_out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The guidance stage on B rows (mf_guide_f32; include/medfusion_hip.h): the classifier-free combine with the scale of table row `step`, then
    -- stages & L.GUIDE_RESCALE -- the guidance rescale and -- stages & L.GUIDE_THRESHOLD -- dynamic thresholding of the x_0 estimate.  pred /
    pred_uncond / x_t: fp32 [B, ...] tensors of one shape (they may start at any 4-byte offset); step: a host int, or an int32 device tensor
    (the loop's counter); out: None = in place on `pred`.  scale_out / limit_out: fp32 [B], the k and s used.  workspace: guide_workspace(B, n),
    made here when None and needed (not inside a recorded iteration).  Returns `out`."""
    what = "guide"
    _dense(what, "pred", pred)
    B = pred.shape[0]
    n = pred.numel() // max(1, B)
    for name, v in (("pred_uncond", pred_uncond), ("x_t", x_t), ("out", out)):
        if v is not None:
            _dense(what, name, v, shape=pred.shape, written=name == "out")
    for name, v in (("scale_out", scale_out), ("limit_out", limit_out)):
        if v is not None:
            _dense(what, name, v, shape=(B,), written=True)
    step_dev = step if torch.is_tensor(step) else None
    if step_dev is not None:
        _dense(what, "step", step_dev, dtype=torch.int32)
    _gpu(pred, table, pred_uncond, x_t, out, scale_out, limit_out, step_dev, workspace)
    if out is None:
        out = pred
    if workspace is None and stages:
        workspace = guide_workspace(B, n, pred.device)
    _drop_outputs((out,))
    a = L.MfGuideArgs(_ptr(x_t), pred.data_ptr(), _ptr(pred_uncond), out.data_ptr(), _ptr(scale_out), _ptr(limit_out), table.data_ptr(), _ptr(step_dev),
                      _ptr(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size(), n, 0 if step_dev is not None else int(step),
                      int(objective), B, int(stages), 0, 0)
    L.check(L.load().mf_guide_f32(C.byref(a), stream()), "mf_guide_f32")
    return out


def lpips_prepare(x: torch.Tensor, y: torch.Tensor, normalize: bool, net: int) -> torch.Tensor:
    """x, y NCHW [B, 1|3, H, W] -> the scaling layer's output of both as one NHWC batch [2B, H, W, 3] (mf_lpips_prepare_f32)"""
    _dense("lpips_prepare", "x", x, dim=4)
    _dense("lpips_prepare", "y", y, shape=x.shape)
    _gpu(x, y)
    B, Cc, H, W = x.shape
    out = torch.empty((2 * B, H, W, 3), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_lpips_prepare_f32(x.data_ptr(), y.data_ptr(), out.data_ptr(), B, Cc, H, W, int(bool(normalize)), net, stream()), "mf_lpips_prepare_f32")
    return out


def make_direct_conv_desc(N, Hin, Win, Cin, Cout, kh, kw, stride, pad, relu=False) -> L.MfDirectConvDesc:
    return L.MfDirectConvDesc(N, Hin, Win, Cin, Cout, kh, kw, stride, pad, int(bool(relu)), 0, 0)


def direct_conv_out_hw(d: L.MfDirectConvDesc):
    out = (C.c_int32 * 2)()
    L.check(L.load().mf_conv2d_direct_out_dims(C.byref(d), out), "mf_conv2d_direct_out_dims")
    return int(out[0]), int(out[1])


def pack_direct_conv_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """OIHW -> [KH][KW][Cin][Cout], the layout mf_conv2d_direct_f32 reads (a copy at load time)"""
    return w_oihw.detach().permute(2, 3, 1, 0).contiguous()


def conv2d_direct(x: torch.Tensor, w_hwio: torch.Tensor, bias: Optional[torch.Tensor], d: L.MfDirectConvDesc) -> torch.Tensor:
    """y = conv(x, w) + bias (+ ReLU with d.relu), NHWC [N, Ho, Wo, Cout] (mf_conv2d_direct_f32: any Cin / Cout, kernels up to 11 x 11, stride 1 .. 4)"""
    what = "conv2d_direct"
    _dense(what, "x", x, shape=(d.N, d.Hin, d.Win, d.Cin))
    _dense(what, "w", w_hwio, shape=(d.KH, d.KW, d.Cin, d.Cout))
    if bias is not None:
        _dense(what, "bias", bias, shape=(d.Cout,))
    _gpu(x, w_hwio, bias)
    ho, wo = direct_conv_out_hw(d)
    out = torch.empty((d.N, ho, wo, d.Cout), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_conv2d_direct_f32(x.data_ptr(), w_hwio.data_ptr(), _ptr(bias), out.data_ptr(), C.byref(d), stream()), "mf_conv2d_direct_f32")
    return out


def relu_(x: torch.Tensor) -> torch.Tensor:
    """x = max(x, 0) in place (mf_relu_f32)"""
    _dense("relu_", "x", x)
    _gpu(x)
    drop_split(x)
    if x.numel():
        L.check(L.load().mf_relu_f32(x.data_ptr(), x.numel(), stream()), "mf_relu_f32")
    return x


def maxpool_nhwc(x: torch.Tensor, k: int, stride: int) -> torch.Tensor:
    """max-pool of an NHWC tensor, (k, stride) = (2, 2) or (3, 2), floor mode, no padding (mf_maxpool_nhwc_f32)"""
    _dense("maxpool_nhwc", "x", x, dim=4)
    _gpu(x)
    N, H, W, Cc = x.shape
    if (k, stride) not in ((2, 2), (3, 2)) or H < k or W < k:
        raise RuntimeError(f"medfusion_amd: maxpool_nhwc: window {k} stride {stride} on sides {H} x {W}: (2, 2) or (3, 2), sides of at least the window")
    out = torch.empty((N, (H - k) // stride + 1, (W - k) // stride + 1, Cc), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_maxpool_nhwc_f32(x.data_ptr(), out.data_ptr(), N, H, W, Cc, k, stride, stream()), "mf_maxpool_nhwc_f32")
    return out


def lpips_layer(fx: torch.Tensor, fy: torch.Tensor, w: torch.Tensor, terms: Optional[torch.Tensor] = None, layer: int = 0,
                total: Optional[torch.Tensor] = None) -> torch.Tensor:
    """term_l of B pairs of feature maps fx, fy [B, ..., C] (NHWC) under the linear weights w [C] -> terms[:, layer] (fp64 [B, layers]; None: a fresh
    [B, 1]); with `total` (fp32 [B]) also the sum of the pair's terms (mf_lpips_layer_f32 + mf_lpips_finish_f32; partials in the per-stream workspace)"""
    what = "lpips_layer"
    _dense(what, "fx", fx)
    _dense(what, "fy", fy, shape=fx.shape)
    if fx.dim() < 2:
        raise RuntimeError(f"medfusion_amd: {what}: fx must be [B, ..., C], got shape {tuple(fx.shape)}")
    B, Cc = fx.shape[0], fx.shape[-1]
    _dense(what, "w", w, shape=(Cc,))
    if terms is None:
        terms = torch.empty((B, 1), dtype=torch.float64, device=fx.device)
    _dense(what, "terms", terms, dtype=torch.float64, dim=2, written=True)
    if terms.shape[0] != B or not 0 <= layer < terms.shape[1]:
        raise RuntimeError(f"medfusion_amd: {what}: terms {tuple(terms.shape)} must be [B = {B}, layers > {layer}]")
    if total is not None:
        _dense(what, "total", total, shape=(B,), written=True)
    _gpu(fx, fy, w, terms, total)
    P = fx.numel() // (B * Cc)
    lib = L.load()
    need = lib.mf_lpips_workspace_bytes(B, P)
    ws = Workspace.get(need, fx.device)
    L.check(lib.mf_lpips_layer_f32(fx.data_ptr(), fy.data_ptr(), w.data_ptr(), ws.data_ptr(), need, B, P, Cc, stream()), "mf_lpips_layer_f32")
    L.check(lib.mf_lpips_finish_f32(ws.data_ptr(), terms.data_ptr(), _ptr(total), B, P, layer, terms.shape[1], stream()), "mf_lpips_finish_f32")
    return terms


def make_gemm_conv_desc(N, Hin, Win, Cin, Cout, kh, kw, stride=1, pad_h=0, pad_w=0, relu=False, ldy=0, y_offset=0, chain=0, tile=0) -> L.MfGemmConvDesc:
    return L.MfGemmConvDesc(N, Hin, Win, Cin, Cout, kh, kw, stride, pad_h, pad_w, int(bool(relu)), ldy, y_offset, chain, tile, 0)


def gemm_conv_out_hw(d: L.MfGemmConvDesc):
    out = (C.c_int32 * 2)()
    L.check(L.load().mf_conv2d_gemm_out_dims(C.byref(d), out), "mf_conv2d_gemm_out_dims")
    return int(out[0]), int(out[1])


def gemm_conv_plan(d: L.MfGemmConvDesc):
    """(tile id, workgroups) of the launch mf_conv2d_gemm_f32 makes for `d` (host only)"""
    out = (C.c_int32 * 2)()
    L.check(L.load().mf_conv2d_gemm_plan(C.byref(d), out), "mf_conv2d_gemm_plan")
    return int(out[0]), int(out[1])


def _sliced_out(what: str, out: Optional[torch.Tensor], shape, ldy: int, y_offset: int, device) -> torch.Tensor:
    """the output of a launch that writes channels [y_offset, y_offset + shape[-1]) of pixels of `ldy` channels: a fresh dense tensor without `out`"""
    width = ldy if ldy else shape[-1]
    if out is None:
        return torch.empty((*shape[:-1], width), dtype=torch.float32, device=device)
    _dense(what, "out", out, shape=(*shape[:-1], width), written=True)
    _gpu(out)
    drop_split(out)
    return out


def conv2d_gemm(x: torch.Tensor, w_hwio: torch.Tensor, bias: Optional[torch.Tensor], d: L.MfGemmConvDesc, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = conv(x, w) + bias (+ ReLU with d.relu) on the fp32 matrix cores, NHWC; channels [d.y_offset, d.y_offset + Cout) of `out` [N, Ho, Wo, d.ldy or
    Cout] are written, the others left alone (mf_conv2d_gemm_f32: any Cin / Cout, kernels up to 11 x 11 per axis, stride 1 .. 4)"""
    what = "conv2d_gemm"
    _dense(what, "x", x, shape=(d.N, d.Hin, d.Win, d.Cin))
    _dense(what, "w", w_hwio, shape=(d.KH, d.KW, d.Cin, d.Cout))
    if bias is not None:
        _dense(what, "bias", bias, shape=(d.Cout,))
    _gpu(x, w_hwio, bias)
    ho, wo = gemm_conv_out_hw(d)
    out = _sliced_out(what, out, (d.N, ho, wo, d.Cout), d.ldy, d.y_offset, x.device)
    L.check(L.load().mf_conv2d_gemm_f32(x.data_ptr(), w_hwio.data_ptr(), _ptr(bias), out.data_ptr(), C.byref(d), stream()), "mf_conv2d_gemm_f32")
    return out


def pool2d_nhwc(x: torch.Tensor, stride: int, pad: int, mode: int, out: Optional[torch.Tensor] = None, ldy: int = 0, y_offset: int = 0) -> torch.Tensor:
    """the 3 x 3 pool of an NHWC tensor, stride 1 or 2, pad 0 or 1, mode L.POOL_MAX or L.POOL_AVG_VALID, into channels [y_offset, y_offset + C) of `out`
    (mf_pool2d_nhwc_f32)"""
    what = "pool2d_nhwc"
    _dense(what, "x", x, dim=4)
    N, H, W, Cc = x.shape
    if stride not in (1, 2) or pad not in (0, 1) or H + 2 * pad < 3 or W + 2 * pad < 3:
        raise RuntimeError(f"medfusion_amd: {what}: stride {stride} (1 or 2), pad {pad} (0 or 1) on sides {H} x {W} (padded sides of at least 3)")
    _gpu(x)
    out = _sliced_out(what, out, (N, (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1, Cc), ldy, y_offset, x.device)
    L.check(L.load().mf_pool2d_nhwc_f32(x.data_ptr(), out.data_ptr(), N, H, W, Cc, stride, pad, mode, ldy, y_offset, stream()), "mf_pool2d_nhwc_f32")
    return out


def inception_prepare(x: torch.Tensor, size: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 NCHW [B, 1|3, H, W] -> the network's operand, fp32 NHWC [B, size, size, 3] (mf_inception_prepare_u8)"""
    what = "inception_prepare"
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 4 or not x.is_contiguous():
        raise RuntimeError(f"medfusion_amd: {what}: x must be a contiguous uint8 [B, C, H, W] tensor, got {getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    _gpu(x)
    B, Cc, H, W = x.shape
    out = _sliced_out(what, out, (B, size, size, 3), 0, 0, x.device)
    L.check(L.load().mf_inception_prepare_u8(x.data_ptr(), out.data_ptr(), B, Cc, H, W, size, stream()), "mf_inception_prepare_u8")
    return out


def mean_pixels(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, ..., C] fp32 (NHWC) -> [B, C]: the mean over the pixels, summed in fp64 (mf_mean_pixels_f32)"""
    what = "mean_pixels"
    _dense(what, "x", x)
    if x.dim() < 2 or x.numel() == 0:
        raise RuntimeError(f"medfusion_amd: {what}: x must be a non-empty [B, ..., C], got shape {tuple(x.shape)}")
    _gpu(x)
    B, Cc = x.shape[0], x.shape[-1]
    out = _sliced_out(what, out, (B, Cc), 0, 0, x.device)
    L.check(L.load().mf_mean_pixels_f32(x.data_ptr(), out.data_ptr(), B, x.numel() // (B * Cc), Cc, stream()), "mf_mean_pixels_f32")
    return out


def absdiff_mean_c(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[N,C,...] fp32 x 2 -> [N,1,...]: the mean over the channels of |a - b| (mf_absdiff_mean_c_f32)"""
    _gpu(a, b)
    if a.shape != b.shape or a.dim() < 3 or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(f"absdiff_mean_c: two fp32 [N,C,cells...] tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    a, b = a.contiguous(), b.contiguous()
    n, c = a.shape[0], a.shape[1]
    out = torch.empty((n, 1, *a.shape[2:]), dtype=torch.float32, device=a.device)
    L.check(L.load().mf_absdiff_mean_c_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), n, c, a.numel() // max(1, n * c), stream()), "mf_absdiff_mean_c_f32")
    return out


def check_gather_step_rows(tables, step, cols) -> None:
    """tables: one to three contiguous fp32 [S, NCOL, L_i] that share S and NCOL; cols [B] int64, contiguous; step: a host int in [0, S) or a
    device int32 counter (read on the device: its value cannot be checked here)"""
    what = "gather_step_rows"
    if not 1 <= len(tables) <= 3:
        raise RuntimeError(f"medfusion_amd: {what}: one to three tables, got {len(tables)}")
    for i, t in enumerate(tables):
        _dense(what, f"table {i}", t, dim=3)
        if t.numel() == 0 or tuple(t.shape[:2]) != tuple(tables[0].shape[:2]):
            raise RuntimeError(f"medfusion_amd: {what}: table {i} {tuple(t.shape)} must be a non-empty [S, NCOL, L] with the [S, NCOL] of table 0 {tuple(tables[0].shape)}")
    _dense(what, "cols", cols, dtype=torch.int64, dim=1)
    if cols.shape[0] < 1:
        raise RuntimeError(f"medfusion_amd: {what}: cols must have shape [B], B >= 1")
    if isinstance(step, torch.Tensor):
        _dense(what, "the device step", step, dtype=torch.int32)
        if step.numel() < 1:
            raise RuntimeError(f"medfusion_amd: {what}: the device step is empty")
    elif isinstance(step, bool) or not hasattr(step, "__index__") or not 0 <= int(step) < tables[0].shape[0]:
        raise RuntimeError(f"medfusion_amd: {what}: host step {step!r} is outside [0, {tables[0].shape[0]}): the table has that many steps")


def gather_step_rows_multi(tables, step, cols: torch.Tensor):
    """gather_step_rows for up to three [S, NCOL, L_i] tables that share `cols` and the step, in ONE launch -> list of [B, L_i]"""
    tables = list(tables)
    check_gather_step_rows(tables, step, cols)
    _gpu(cols, *tables)
    n = len(tables)
    B, ncol = cols.shape[0], tables[0].shape[1]
    outs = [torch.empty((B, t.shape[2]), dtype=torch.float32, device=t.device) for t in tables]
    tp = (L.c_fp * n)(*[t.data_ptr() for t in tables])
    op = (L.c_fp * n)(*[o.data_ptr() for o in outs])
    rl = (C.c_int64 * n)(*[t.shape[2] for t in tables])
    dev_step = isinstance(step, torch.Tensor)
    rc = L.load().mf_gather_step_rows3_f32(tp, rl, op, n, cols.data_ptr(), step.data_ptr() if dev_step else None, 0 if dev_step else int(step), ncol, B, stream())
    L.check(rc, "mf_gather_step_rows3_f32")
    return outs


def gather_step_rows(table: torch.Tensor, step, cols: torch.Tensor) -> torch.Tensor:
    """table [S, NCOL, L] fp32, cols [B] int64 -> [B, L] = table[step, cols[b]]; `step`: a host int or a device int32 counter (graph replay)"""
    check_gather_step_rows([table], step, cols)
    _gpu(table, cols)
    s_, ncol, ln = table.shape
    out = torch.empty((cols.shape[0], ln), dtype=torch.float32, device=table.device)
    dev_step = isinstance(step, torch.Tensor)
    rc = L.load().mf_gather_step_rows_f32(table.data_ptr(), cols.data_ptr(), step.data_ptr() if dev_step else None, 0 if dev_step else int(step), ncol, ln,
                                          out.data_ptr(), cols.shape[0], stream())
    L.check(rc, "mf_gather_step_rows_f32")
    return out


def check_broadcast_from_table(table, step_dev, out) -> None:
    """out [B] fp32 <- table[*step_dev]: table [S] fp32, step_dev a device int32 counter"""
    what = "broadcast_from_table"
    _dense(what, "table", table, dim=1)
    _dense(what, "the device step", step_dev, dtype=torch.int32)
    _dense(what, "out", out, dim=1, written=True)
    if table.numel() < 1 or step_dev.numel() < 1 or out.numel() < 1:
        raise RuntimeError(f"medfusion_amd: {what}: table {tuple(table.shape)}, step {tuple(step_dev.shape)} and out {tuple(out.shape)} must be non-empty")


def broadcast_from_table(table: torch.Tensor, step_dev: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    check_broadcast_from_table(table, step_dev, out)
    _gpu(table, step_dev, out)
    drop_split(out)
    L.check(L.load().mf_broadcast_from_table_f32(table.data_ptr(), step_dev.data_ptr(), 0, out.data_ptr(), out.numel(), stream()), "mf_broadcast_from_table_f32")
    return out


def counter_add(counter: torch.Tensor, inc: int = 1) -> None:
    _gpu(counter)
    L.check(L.load().mf_counter_add_i32(counter.data_ptr(), inc, stream()), "mf_counter_add_i32")


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """q [B,Nq,C], k/v [B,Nk,C] -> [B,Nq,C]."""
    _gpu(q, k, v)
    _need_f32(q, k, v)
    _f32("attention", q, k, v)
    assert q.dim() == 3 and k.dim() == 3 and q.is_contiguous() and k.is_contiguous() and v.is_contiguous(), "attention: contiguous q [B, Nq, C], k / v [B, Nk, C]"
    b, nq, c = q.shape
    nk = k.shape[1]
    assert k.shape == (b, nk, c) and v.shape == k.shape, f"attention: k {tuple(k.shape)} and v {tuple(v.shape)} must both be [{b}, Nk, {c}]"
    assert heads > 0 and c % heads == 0, f"attention: C={c} is no multiple of heads={heads}"
    out = torch.empty_like(q)
    L.check(L.load().mf_attention_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), b, heads, nq, nk, c // heads, scale, stream()),
            "mf_attention_f32")
    return out


def layernorm(x: torch.Tensor, gamma, beta, eps: float = 1e-5) -> torch.Tensor:
    _gpu(x, gamma, beta)
    _need_f32(x)
    _f32("layernorm", x, gamma, beta)
    c = x.shape[-1]
    assert x.is_contiguous() and gamma.shape == (c,) and beta.shape == (c,) and gamma.is_contiguous() and beta.is_contiguous(), "layernorm: contiguous x [..., C], gamma / beta [C]"
    out = torch.empty_like(x)
    L.check(L.load().mf_layernorm_f32(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), x.numel() // c, c, eps, stream()), "mf_layernorm_f32")
    return out


def geglu(h: torch.Tensor) -> torch.Tensor:
    _gpu(h)
    _need_f32(h)
    _f32("geglu", h)
    assert h.is_contiguous() and h.shape[-1] % 2 == 0, "geglu: contiguous h [..., 2 C]"
    c = h.shape[-1] // 2
    out = torch.empty((*h.shape[:-1], c), dtype=torch.float32, device=h.device)
    L.check(L.load().mf_geglu_f32(h.data_ptr(), out.data_ptr(), h.numel() // (2 * c), c, stream()), "mf_geglu_f32")
    return out


def check_add(a, b, out=None) -> None:
    """out = a + b elementwise: three contiguous fp32 tensors of one shape (out may be a or b)"""
    _dense("add", "a", a)
    _dense("add", "b", b, shape=a.shape)
    if out is not None:
        _dense("add", "out", out, shape=a.shape, written=out is not a and out is not b)
    if a.numel() < 1:
        raise RuntimeError("medfusion_amd: add: empty tensors")


def check_layout(what: str, x, copies: bool) -> None:
    """a 4-D fp32 tensor with at most 65535 samples (the sample index is blockIdx.z); copies=False: the wrapper reads it in place"""
    _dense(what, "x", x, dim=4, contiguous=not copies)
    if x.numel() < 1 or x.shape[0] > 65535:
        raise RuntimeError(f"medfusion_amd: {what}: x {tuple(x.shape)} must be non-empty with N <= 65535 (one grid plane per sample)")


def check_avgpool2d(x, k: int, stride: int, pad: int):
    """x [N, H, W, C] fp32, C % 4 == 0; nn.AvgPool2d's own rule 2 pad <= k -> (Ho, Wo), both >= 1"""
    _dense("avgpool2d", "x", x, dim=4, contiguous=False)
    n, h, w, c = x.shape
    if min(n, h, w, c) < 1 or c % 4:
        raise RuntimeError(f"medfusion_amd: avgpool2d: x {tuple(x.shape)} must be a non-empty [N, H, W, C] with C % 4 == 0")
    if k < 1 or stride < 1 or pad < 0 or 2 * pad > k:
        raise RuntimeError(f"medfusion_amd: avgpool2d: kernel {k}, stride {stride}, pad {pad}: needs k >= 1, stride >= 1, 0 <= 2 pad <= k")
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    if ho < 1 or wo < 1:
        raise RuntimeError(f"medfusion_amd: avgpool2d: x {tuple(x.shape)} with kernel {k}, stride {stride}, pad {pad} has an empty output")
    return ho, wo


def check_upsample_nearest2x(x) -> None:
    _dense("upsample_nearest2x", "x", x, dim=4, contiguous=False)
    if x.numel() < 1 or x.shape[3] % 4:
        raise RuntimeError(f"medfusion_amd: upsample_nearest2x: x {tuple(x.shape)} must be a non-empty [N, H, W, C] with C % 4 == 0")


def check_pixel_shuffle_pair(what: str, x, y, unshuffle: bool) -> None:
    """x fp32 [N, H, W, C] (the wrapper copies a strided one); y fp32, contiguous (written in place), of the shuffled shape"""
    _dense(what, "x", x, dim=4, contiguous=False)
    n, h, w, c = x.shape
    ok = x.numel() > 0 and ((h % 2 == 0 and w % 2 == 0) if unshuffle else c % 4 == 0)
    want = (n, h // 2, w // 2, 4 * c) if unshuffle else (n, 2 * h, 2 * w, c // 4)
    if not ok or not isinstance(y, torch.Tensor) or tuple(y.shape) != want:
        raise RuntimeError(f"medfusion_amd: {what}: x {tuple(x.shape)} does not {'unshuffle' if unshuffle else 'shuffle'} onto y {tuple(getattr(y, 'shape', ()))}")
    _dense(what, "y", y)


def check_diag_gaussian(what: str, moments, noise=None):
    """moments [N, 2C, H, W] fp32 (mean | logvar); noise, where the op takes one: [N, C, H, W] fp32; both contiguous -> (N, C, H W)"""
    _dense(what, "moments", moments, dim=4, contiguous=noise is not None)
    n, c2, h, w = moments.shape
    if moments.numel() < 1 or c2 % 2:
        raise RuntimeError(f"medfusion_amd: {what}: moments {tuple(moments.shape)} must be a non-empty [N, 2 C, H, W]")
    if noise is not None:
        _dense(what, "noise", noise, shape=(n, c2 // 2, h, w))
    return n, c2 // 2, h * w


def add(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    check_add(a, b, out)
    _gpu(a, b, out)
    if out is None:
        out = torch.empty_like(a)
    else:
        drop_split(out)
    L.check(L.load().mf_add_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), stream()), "mf_add_f32")
    return out


def nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    check_layout("nchw_to_nhwc", x, copies=True)
    _gpu(x)
    n, c, h, w = x.shape
    x = x.contiguous()
    out = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_nchw_to_nhwc_f32(x.data_ptr(), out.data_ptr(), n, c, h, w, stream()), "mf_nchw_to_nhwc_f32")
    return out


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    check_layout("nhwc_to_nchw", x, copies=False)
    _gpu(x)
    n, h, w, c = x.shape
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_nhwc_to_nchw_f32(x.data_ptr(), out.data_ptr(), n, c, h, w, stream()), "mf_nhwc_to_nchw_f32")
    return out


def avgpool2d(x: torch.Tensor, k: int, stride: int, pad: int) -> torch.Tensor:
    """nn.AvgPool2d(k, stride, pad) on NHWC (count_include_pad like torch's default)"""
    ho, wo = check_avgpool2d(x, k, stride, pad)
    _gpu(x)
    n, h, w, c = x.shape
    out = torch.empty((n, ho, wo, c), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_avgpool2d_nhwc_f32(x.contiguous().data_ptr(), out.data_ptr(), n, h, w, c, k, stride, pad, stream()), "mf_avgpool2d_nhwc_f32")
    return out


def upsample_nearest2x(x: torch.Tensor) -> torch.Tensor:
    """F.interpolate(scale 2, nearest-exact) on NHWC"""
    check_upsample_nearest2x(x)
    _gpu(x)
    n, h, w, c = x.shape
    out = torch.empty((n, 2 * h, 2 * w, c), dtype=torch.float32, device=x.device)
    L.check(L.load().mf_upsample_nearest2x_nhwc_f32(x.contiguous().data_ptr(), out.data_ptr(), n, h, w, c, stream()), "mf_upsample_nearest2x_nhwc_f32")
    return out


def pixel_unshuffle2_add(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """y [N, H/2, W/2, 4C] += nn.PixelUnshuffle(2)(x [N, H, W, C]) on NHWC, in place (BasicDown(use_res=True))"""
    check_pixel_shuffle_pair("pixel_unshuffle2_add", x, y, unshuffle=True)
    _gpu(x, y)
    n, h, w, c = x.shape
    drop_split(y)
    L.check(L.load().mf_pixel_unshuffle2_add_nhwc_f32(x.contiguous().data_ptr(), y.data_ptr(), n, h, w, c, stream()), "mf_pixel_unshuffle2_add_nhwc_f32")
    return y


def pixel_shuffle2_add(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """y [N, 2H, 2W, C/4] += nn.PixelShuffle(2)(x [N, H, W, C]) on NHWC, in place (BasicUp(use_res=True))"""
    check_pixel_shuffle_pair("pixel_shuffle2_add", x, y, unshuffle=False)
    _gpu(x, y)
    n, h, w, c = x.shape
    drop_split(y)
    L.check(L.load().mf_pixel_shuffle2_add_nhwc_f32(x.contiguous().data_ptr(), y.data_ptr(), n, h, w, c, stream()), "mf_pixel_shuffle2_add_nhwc_f32")
    return y


def diag_gaussian_sample(moments_nchw: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    """z = mean + exp(0.5 clamp(logvar, -30, 20)) noise of DiagonalGaussianDistribution (latent_embedders.py:18-27): moments [N, 2C, H, W] = mean | logvar,
    noise [N, C, H, W], both contiguous fp32 (read in place: no copy is made)"""
    n, c, hw = check_diag_gaussian("diag_gaussian_sample", moments_nchw, noise)
    _gpu(moments_nchw, noise)
    h, w = moments_nchw.shape[2:]
    z = torch.empty((n, c, h, w), dtype=torch.float32, device=moments_nchw.device)
    L.check(L.load().mf_diag_gaussian_sample_f32(moments_nchw.data_ptr(), noise.data_ptr(), z.data_ptr(), n, c, hw, stream()),
            "mf_diag_gaussian_sample_f32")
    return z


def diag_gaussian_kl(moments_nchw: torch.Tensor) -> torch.Tensor:
    """the KL term of DiagonalGaussianDistribution (latent_embedders.py:29-31) as a 0-dim device tensor"""
    n, c, hw = check_diag_gaussian("diag_gaussian_kl", moments_nchw)
    _gpu(moments_nchw)
    kl = torch.empty((1,), dtype=torch.float32, device=moments_nchw.device)
    L.check(L.load().mf_diag_gaussian_kl_f32(moments_nchw.contiguous().data_ptr(), kl.data_ptr(), n, c, hw, stream()), "mf_diag_gaussian_kl_f32")
    return kl.reshape(())


def vector_quantize(z_nchw: torch.Tensor, codebook: torch.Tensor, want_idx: bool = False, want_sqerr: bool = False):
    """VectorQuantizer.forward (latent_embedders.py:40-71) on the device: z [N,C,H,W], codebook [K,C] -> (z_q [N,C,H,W] = z + (e_idx - z),
    idx int32 [N*H*W] or None, sum of (e_idx - z)^2 as a 0-dim fp64 device tensor or None).  Nearest code by the reference's formula, lowest
    index on ties, first NaN wins (include/medfusion_hip.h)."""
    _gpu(z_nchw, codebook)
    if z_nchw.dim() != 4 or codebook.dim() != 2 or z_nchw.dtype != torch.float32 or codebook.dtype != torch.float32:
        raise RuntimeError(f"vector_quantize: z {tuple(z_nchw.shape)} {z_nchw.dtype} / codebook {tuple(codebook.shape)} {codebook.dtype}: "
                           f"expected fp32 [N,C,H,W] and [K,C]")
    n, c, h, w = z_nchw.shape
    k, ce = codebook.shape
    if ce != c:
        raise RuntimeError(f"vector_quantize: z has {c} channels, the codebook {ce}")
    z = z_nchw.contiguous()
    cb = codebook.detach().contiguous()
    zq = torch.empty_like(z)
    idx = torch.empty((n * h * w,), dtype=torch.int32, device=z.device) if want_idx else None
    sq = torch.zeros((1,), dtype=torch.float64, device=z.device) if want_sqerr else None
    lib = L.load()
    nbytes = lib.mf_vq_workspace_bytes(n * h * w)
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=z.device)
    L.check(lib.mf_vector_quantize_f32(z.data_ptr(), cb.data_ptr(), zq.data_ptr(), _ptr(idx), _ptr(sq), ws.data_ptr(), nbytes, n, c, h * w, k,
                                       stream()), "mf_vector_quantize_f32")
    return zq, idx, (sq.reshape(()) if sq is not None else None)


# ----------------------------------------------------------------------------- launch timing
_PROF_ACTIVE = [False]


def prof_active() -> bool:
    """launch timing is on (the command-list loop steps aside: replayed launches would not be timed)"""
    return _PROF_ACTIVE[0]


class prof:
    """with prof() as p: ...; p.table() -> {family: (ms, launches, algorithmic flops, bytes, executed flops)}"""

    def __enter__(self):
        lib = L.load()
        lib.mf_prof_reset()
        lib.mf_prof_enable(1)
        _PROF_ACTIVE[0] = True
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        L.load().mf_prof_enable(0)
        _PROF_ACTIVE[0] = False
        return False

    @staticmethod
    def table() -> dict:
        lib = L.load()
        out = {}
        for i, name in enumerate(L.FAMILIES):
            ms, n, fl, by, ex = C.c_double(), C.c_int64(), C.c_double(), C.c_double(), C.c_double()
            L.check(lib.mf_prof_query2(i, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by), C.byref(ex)), "mf_prof_query2")
            if n.value:
                out[name] = (ms.value, n.value, fl.value, by.value, ex.value)
        return out


def prof_rows(family: str):
    """the records of `family` (a name of lib.FAMILIES) since prof() started, grouped by kernel instantiation:
    [{kernel (as rocprofv3 prints it), variant, launches, ms, flops, bytes, exec_flops}]"""
    lib = L.load()
    fam = L.FAMILIES.index(family)
    rows = (L.MfProfRow * 64)()
    n = lib.mf_prof_rows(fam, rows, 64)
    if n < 0:
        L.check(n, "mf_prof_rows")
    out = []
    buf = C.create_string_buffer(256)
    for r in rows[:n]:
        lib.mf_prof_tag_name(fam, r.tag, buf, 256)
        out.append(dict(kernel=buf.value.decode(), tag=r.tag, variant=r.variant, launches=r.launches, ms=r.ms, flops=r.flops, bytes=r.bytes, exec_flops=r.exec_flops))
    return out


def mfma_sustained_tflops(device, data: str = "random", iters: int = 4000, reps: int = 3) -> float:
    """TFLOP/s the fp16 matrix pipe sustains on `device` with nothing but MFMAs in flight (mf_mfma_rate_probe_f16), operands "random"
    (N(0,1) as fp16) or "zeros": the measured ceiling bench.py sets next to the nominal peak."""
    wgs = torch.cuda.get_device_properties(device).multi_processor_count
    n = wgs * 512 * 8 * 8
    ops = (torch.randn((n,), device=device, generator=torch.Generator(device=device).manual_seed(1)) if data == "random"
           else torch.zeros((n,), device=device)).to(torch.float16)
    out = torch.empty((wgs * 512,), dtype=torch.float32, device=device)
    fl = C.c_double(0.0)
    lib = L.load()
    best = 0.0
    for r in range(reps + 1):   # first launch: warm-up of the same length
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(lib.mf_mfma_rate_probe_f16(ops.data_ptr(), out.data_ptr(), wgs, iters, C.byref(fl), stream()), "mf_mfma_rate_probe_f16")
        e1.record()
        e1.synchronize()
        if r:
            best = max(best, fl.value / (e0.elapsed_time(e1) * 1e-3) / 1e12)
    return best
