"""The ramp of the fp16-pair convolution kernels (conv_f16x2_body.inc: bounds and bias fetched at the entry, exponents carried through the
loop, the kernel argument in one burst) against the twin of the library built with -DMFC2_EXPS_EARLY=1, the form of rounds 3 - 6: the same
values are loaded, only when and where differs, so every output, bound slot and GroupNorm record is equal bit for bit.  The launches
(tests/ramp_cases.py) run once per library in a child process each; the product results are also held against an fp64 convolution."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from tests import ramp_cases as RC

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """{library: {case id: {name: tensor}}} for the product library and the MFC2_EXPS_EARLY=1 twin"""
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from medfusion_amd import build as B
    twin = B.build_variant("ramp1", conv_flags=["-DMFC2_EXPS_EARLY=1"])
    tmp = tmp_path_factory.mktemp("ramp")
    res = {}
    for name, extra in (("product", {}), ("twin", {"MEDFUSION_LIB": str(twin)})):
        env = {k: v for k, v in os.environ.items() if k != "MEDFUSION_LIB"}
        env.update(extra)
        out = tmp / f"{name}.pt"
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "ramp_cases.py"), str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (name, r.stdout[-1500:], r.stderr[-3000:])
        res[name] = torch.load(out)
    return res


@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_product_equals_the_parent_form_twin_bit_for_bit(both, case):
    a, b = both["product"][RC.case_id(case)], both["twin"][RC.case_id(case)]
    assert set(a) == set(b) and "y" in a, (case, sorted(a), sorted(b))
    for name in a:
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, (case, name)
        # (the raw bytes: a NaN or a signed zero that differs counts)
        assert torch.equal(a[name].contiguous().view(torch.uint8), b[name].contiguous().view(torch.uint8)), (case, name)
    if "y_gn" in a:
        assert torch.equal(a["y_gn"], a["y"]), case


@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_product_against_fp64(both, case):
    """per SAMPLE (their magnitudes are 2^10 apart): max |y - fp64| / max |fp64| < 1e-5, the bound of the kernel tests (test_conv_f16x2)"""
    got = both["product"][RC.case_id(case)]
    kind, n = case[0], case[1]
    x1, x2, wt, b = RC.operands(case)
    xin = x1 if x2 is None else torch.cat([x1, x2], 1)
    if kind == "conv":
        k, stride, ups = case[7:10]
        if ups:
            xin = F.interpolate(xin, scale_factor=2, mode="nearest-exact")
        want = F.conv2d(xin.double(), wt.double(), b.double(), stride=stride, padding=1 if k == 3 else 0)
    else:
        want = F.conv2d(xin.double(), wt.double(), b.double(), padding=1)
    y = got["y"].permute(0, 3, 1, 2).double()
    assert y.shape == want.shape, (case, y.shape, want.shape)
    err = (y - want).abs().amax(dim=(1, 2, 3)) / want.abs().amax(dim=(1, 2, 3))
    print(f"[measured] {RC.case_id(case)}: per-sample max-norm rel err vs fp64 {[f'{float(e):.2e}' for e in err]}")
    assert float(err.max()) < 1e-5, (case, err)
