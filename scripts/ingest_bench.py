#!/usr/bin/env python3
"""What the data set's transform costs on the device, against PIL on the host for the same arrays (profiles/ingest_bench.txt).

  python scripts/ingest_bench.py [--reps 200] [--out profiles/ingest_bench.txt]      (on a ROCm device)
  python scripts/ingest_bench.py --plan                                             (no device: launches, workgroups, bytes)

Two batches of the reference's data sets, resize 256 (shorter side) + centre crop 256, normalised to [-1, 1]:
  * 16 x 2828 x 2320 x 1 uint8 (a chest radiograph at its native size; 11 : 1)
  * 16 x  390 x  320 x 3 uint8 (a small RGB tile; 1.2 : 1)
Device time between two events around medfusion_amd.ingest.transform of the packed batch, after a warm-up, `reps` back-to-back calls: once with the
pinned buffer going up inside the call (the one host-to-device copy included) and once with the bytes already on the device (the two launches alone).
The host figure is wall time of Image.resize(BILINEAR) + crop + the same value map in numpy, one thread, the same arrays.  DECODING (PNG / JPEG ->
array) is not in either figure: it stays on the host, is not timed here, and is expected to bound a folder run.
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

BATCHES = [("16 x 2828 x 2320 x 1", 16, (2828, 2320), 1), ("16 x 390 x 320 x 3", 16, (390, 320), 3)]
RESIZE, CROP = 256, 256


def plan_lines():
    import numpy as np

    from medfusion_amd import ingest as I
    lines = []
    for label, n, shape, c in BATCHES:
        p = I.plan([shape] * n, resize=RESIZE, crop=CROP, dtype=np.uint8, channels=c)
        lines.append(f"{label} uint8 -> {n} x {c} x {p['out_size'][0]} x {p['out_size'][1]} fp32 (resized {I.resized_size(*shape, RESIZE)}): {p['launches']} launches, "
                     f"workgroups {p['workgroups'][0]} + {p['workgroups'][1]}, source {p['source_bytes']} B, workspace {p['workspace_bytes']} B, "
                     f"tables {p['table_bytes']} B ({p['tables']} built once), descriptors {p['descriptor_bytes']} B")
    return lines


def main(a):
    import numpy as np
    import torch
    from PIL import Image

    from medfusion_amd import ingest as I
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    lines = [f"resize {RESIZE} (shorter side) + centre crop {CROP} + ((v / 255) - 0.5) / 0.5; {a.reps} back-to-back calls between two device events after a warm-up; "
             "host: PIL " + Image.__version__ + ", one thread"] + plan_lines()

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    for label, n, shape, c in BATCHES:
        arrays = [rng.integers(0, 256, shape + (c,), dtype=np.uint8) for _ in range(n)]
        p = I.plan([shape] * n, resize=RESIZE, crop=CROP, dtype=np.uint8, channels=c)
        ws = torch.empty(max(p["workspace_bytes"], 16), dtype=torch.uint8, device=dev)
        out = torch.empty((n, c) + p["out_size"], device=dev)
        packed = I.pack(arrays, resize=RESIZE, crop=CROP)
        with_copy = timed(lambda: I.transform(packed, device=dev, workspace=ws, out=out))
        packed.to(dev)
        resident = timed(lambda: I.transform(packed, device=dev, workspace=ws, out=out))
        got = I.resample_bytes(packed, device=dev, workspace=ws).cpu().numpy()
        Hr, Wr = I.resized_size(*shape, RESIZE)
        top, left, h, w = I.center_crop_box(Hr, Wr, CROP)
        t0 = time.perf_counter()
        ref = []
        for arr in arrays:
            im = Image.fromarray(arr[..., 0], "L") if c == 1 else Image.fromarray(arr, "RGB")
            r = np.asarray(im.resize((Wr, Hr), Image.BILINEAR)).reshape(Hr, Wr, c)[top:top + h, left:left + w]
            ref.append(r)
            _ = ((r.astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1)
        host = 1e3 * (time.perf_counter() - t0)
        bad = int(sum((g != r).sum() for g, r in zip(got, ref)))
        mb = p["source_bytes"] / 1e6
        lines.append(f"{label}: device, copy included {with_copy:8.3f} ms ({mb / with_copy:6.1f} GB/s of source bytes) | bytes resident {resident:8.3f} ms "
                     f"({mb / resident:6.1f} GB/s) | PIL on the host {host:8.1f} ms | pixels differing from PIL: {bad}")
    lines.append("Decoding is in neither figure: PNG / JPEG files are decoded by PIL on the host (not timed here; expected to bound a folder run).")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("The data set's transform on an AMD Instinct MI355X against PIL on the host, measured by scripts/ingest_bench.py (one process).\n\n" + text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--plan", action="store_true", help="print launches, workgroups and bytes, touch no device")
    a = ap.parse_args()
    if a.plan:
        print("\n".join(plan_lines()))
        sys.exit(0)
    main(a)
