"""bench.py's own contract: a plain run prints the headline line only, `--steps` is the number of timed steps, and `--dump-outputs DIR`
writes the images of the last timed step (a fixed, seeded choice of whole images beyond the size cap)."""
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def _bench_module():
    spec = importlib.util.spec_from_file_location("_medfusion_bench", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_caps_the_size_with_a_fixed_choice_of_images(tmp_path, monkeypatch):
    bench = _bench_module()
    img = torch.arange(10 * 3 * 4 * 4, dtype=torch.float32).reshape(10, 3, 4, 4)
    bench.dump_outputs(str(tmp_path / "all"), img)
    a = np.load(tmp_path / "all" / "images.npy")
    assert a.dtype == np.float32 and np.array_equal(a, img.numpy())
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * img[0].numel() * 4)       # room for 4 of the 10 images
    bench.dump_outputs(str(tmp_path / "a"), img)
    bench.dump_outputs(str(tmp_path / "b"), img)
    a, b = np.load(tmp_path / "a" / "images.npy"), np.load(tmp_path / "b" / "images.npy")
    assert a.shape == (4, 3, 4, 4) and np.array_equal(a, b)
    rows = a[:, 0, 0, 0] // img[0].numel()
    assert list(rows) == sorted(set(rows.tolist())) and np.array_equal(a, img.numpy()[rows.astype(int)])


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_images(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--ddim-steps", "2", "--batch", "2",
                        "--dump-outputs", str(out)], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    assert {"metric", "unit", "dtype"} <= set(line)
    assert line["roofline"] is None and line["cpu_baseline"] is None and "other_workloads" not in line   # the --full parts stay off
    img = np.load(out / "images.npy")
    assert img.dtype == np.float32 and img.shape == (2, 3, 256, 256) and np.isfinite(img).all() and np.abs(img).max() > 0
