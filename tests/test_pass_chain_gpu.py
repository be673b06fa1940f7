"""wino_tail_kernel, wino_input_kernel (csrc/winograd.h) and gn_apply_part_kernel (csrc/groupnorm.hip) in the product form (MF_PASS_CHAIN == 2,
csrc/split_f16.h: everything that depends on nothing requested at the kernel's entry, counted waits, barriers that order LDS only) against the
twin of the library built with -DMF_PASS_CHAIN=1, the form of rounds 3 - 6: the same values are loaded and the same arithmetic runs in the same
order, only when the loads are issued and waited for differs, so every output tensor, the pair mirror, out_bound, wino_bound and V are equal
bit for bit.  The launches (tests/pass_chain_cases.py) run once per library, in a child process each.

The tail cases are the four (N, H x W, C, G) that exercise its code paths.  The component GEMM in front of the fp16-pair tail needs a tile
whose rows divide a component's N (H/2)(W/2) rows, so the two 8 x 8 cases run that entry at the smallest multiple of their N the planner takes
(8 at 64 channels, 4 at 128) and their own N = 2 on mf_wino_tail_f32, which takes M as it
is (the same kernel, v_f32).  Every fp16-pair case runs with no residual, an fp32 residual with res_bound, an fp32 residual with res_slots and
a pair residual, each with embedding and gamma / beta on and off and with the output combinations kernels.py asks for (pairs; + fp32; + V)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests import pass_chain_cases as PC

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """{library: {case id: {variant: {name: tensor or (shape, dtype, SHA-256)}}}} for the product library and the MF_PASS_CHAIN=1 twin"""
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from medfusion_amd import build as B
    twin = B.build_variant("chain1", conv_flags=["-DMF_PASS_CHAIN=1"], unit_flags={"groupnorm.hip": ["-DMF_PASS_CHAIN=1"]})
    tmp = tmp_path_factory.mktemp("pass_chain")
    res = {}
    for name, extra in (("product", {}), ("twin", {"MEDFUSION_LIB": str(twin)})):
        env = {k: v for k, v in os.environ.items() if k not in ("MEDFUSION_LIB", "MF_GN_U", "MF_GN_BLOCKS_PER_CU")}
        env.update(extra)
        out = tmp / f"{name}.pt"
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "pass_chain_cases.py"), str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (name, r.stdout[-1500:], r.stderr[-3000:])
        res[name] = torch.load(out)
    return res


@pytest.mark.parametrize("case", PC.CASES, ids=PC.case_id)
def test_product_equals_the_parent_form_twin_bit_for_bit(both, case):
    a, b = both["product"][PC.case_id(case)], both["twin"][PC.case_id(case)]
    want = {str(v) for v in PC.variants(case)}
    assert set(a) == set(b) and want <= set(a), (case, sorted(a), sorted(b))
    for var in a:
        assert set(a[var]) == set(b[var]) and a[var], (case, var, sorted(a[var]), sorted(b[var]))
        for name, x in a[var].items():
            y = b[var][name]
            if isinstance(x, tuple):      # (shape, dtype, SHA-256 of the bytes)
                assert x == y, (case, var, name)
                continue
            assert x.dtype == y.dtype and x.shape == y.shape, (case, var, name)
            # (the raw bytes: a NaN or a signed zero that differs counts)
            assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (case, var, name)
            if x.dtype == torch.float32:
                assert bool(torch.isfinite(x).all()), (case, var, name)


def test_tail_outputs_are_consistent(both):
    """the launches did what the bit comparison assumes: the transform-domain bound is 4 x the output bound, per component; the bound does not
    shrink with a residual, and grows where the residual is not negligible; the fp32 output and its pair mirror agree to the 23 bits of the pair form"""
    for case in PC.TAIL_CASES:
        r = both["product"][PC.case_id(case)]
        plain, with_res = r[str(("f16", None, True, True, True, True))], r[str(("f16", "f32", True, True, True, True))]
        n = plain["out_bound"].numel()
        assert torch.equal(plain["wino_bound"].view(16, n), (4.0 * plain["out_bound"]).expand(16, n)), case
        # (bconst + bound(residual) + bound(embedding) in fp32: a residual 2^40 below the embedding row of its sample adds less than an ulp)
        assert bool((with_res["out_bound"] >= plain["out_bound"]).all()) and bool((with_res["out_bound"] > plain["out_bound"]).any()), case
        s = torch.floor(torch.log2(plain["out_bound"].double())) - 14
        raw = plain["pairs"].contiguous().view(torch.float16).double().reshape(-1, 2, 8)
        dec = (raw[:, 0] + raw[:, 1] / 2048.0).reshape(plain["y"].shape) * (2.0 ** s).view(-1, 1, 1, 1)
        assert float((dec - plain["y"].double()).abs().max() / plain["y"].abs().max()) < 2.0 ** -22, case
