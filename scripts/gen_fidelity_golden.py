#!/usr/bin/env python3
"""Writes tests/golden/fidelity_c0.npz and fidelity_c1.npz: the feature banks of the first two cases of tests/fidelity_cases.py and what the REAL
reference's ImprovedPrecessionRecall(feature=torch.nn.Identity(), knn=3, splits_real=1, splits_fake=1) returns with real_features / fake_features
set from them -- what the commented "Load features" block of the reference's evaluate_images.py does -- in fp32 and in fp64, plus its radii.

The reference's module imports torchmetrics and torchvision, which are not needed for this path: in-process stand-ins take their place
(torchmetrics.Metric as a torch.nn.Module with add_state, torchmetrics.utilities.imports without torch-fidelity, torchvision.models / .transforms
as empty modules), and the name `Module`, which the module's fallback branch uses without importing, is bound through builtins while it loads.
The fixtures hold data only.  Runs on the CPU; needs the reference checkout.

Run from the repository root:  python scripts/gen_fidelity_golden.py [reference root]
"""
from __future__ import annotations

import builtins
import importlib.util
import sys
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
REF = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT.parent / "reference"
sys.path.insert(0, str(ROOT))

import numpy as np
import torch

torch.set_num_threads(1)   # fixed summation order for the stored results

from tests import fidelity_cases as FC

GOLD = ROOT / "tests" / "golden"
LIMIT = 400 * 1024


def load_reference_module():
    class Metric(torch.nn.Module):
        def add_state(self, name, default, dist_reduce_fx=None):
            setattr(self, name, default)

    tm, tmu, tmi = types.ModuleType("torchmetrics"), types.ModuleType("torchmetrics.utilities"), types.ModuleType("torchmetrics.utilities.imports")
    tm.Metric, tm.utilities, tmu.imports, tmi._TORCH_FIDELITY_AVAILABLE = Metric, tmu, tmi, False
    tv, tvm, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.models"), types.ModuleType("torchvision.transforms")
    tv.models, tv.transforms = tvm, tvt
    stand_ins = {"torchmetrics": tm, "torchmetrics.utilities": tmu, "torchmetrics.utilities.imports": tmi, "torchvision": tv, "torchvision.models": tvm,
                 "torchvision.transforms": tvt}
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    builtins.Module = torch.nn.Module
    try:
        spec = importlib.util.spec_from_file_location("_reference_pr_recall", REF / "medical_diffusion" / "metrics" / "torchmetrics_pr_recall.py")
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        del builtins.Module
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


@torch.no_grad()
def run(mod, name):
    real, fake = FC.case(name)
    out = {"real": real.numpy(), "fake": fake.numpy(), "knn": np.int64(FC.KNN)}
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        metric = mod.ImprovedPrecessionRecall(feature=torch.nn.Identity(), knn=FC.KNN, splits_real=1, splits_fake=1)
        r, f = real.to(dtype), fake.to(dtype)
        metric.real_features, metric.fake_features = list(r.chunk(3)), list(f.chunk(3))
        precision, recall = metric.compute()
        out[f"precision_{tag}"], out[f"recall_{tag}"] = np.float64(float(precision)), np.float64(float(recall))
        out[f"radii_real_{tag}"] = mod._distances2radii(mod._compute_pairwise_distances(r, 1), FC.KNN).numpy()
        out[f"radii_fake_{tag}"] = mod._distances2radii(mod._compute_pairwise_distances(f, 1), FC.KNN).numpy()
        print(f"{name} {tag}: precision {float(precision):.5f} recall {float(recall):.5f}")
    np.savez_compressed(GOLD / f"fidelity_{name}.npz", **out)
    assert (GOLD / f"fidelity_{name}.npz").stat().st_size < LIMIT, name


if __name__ == "__main__":
    module = load_reference_module()
    for case_name in ("c0", "c1"):
        run(module, case_name)
