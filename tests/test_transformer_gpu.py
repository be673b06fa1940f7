"""The attention kernels (csrc/attention.hip) and the linear / LayerNorm / GEGLU kernels (csrc/small_ops.hip) against fp64 at the edges of their
paths, in-process on the product entry points K.attention, K.linear, K.layernorm, K.geglu.  Cases, regimes, restatements and bounds:
tests/transformer_cases.py (checked by tests/test_transformer_cpu.py, which also asserts which path every case reaches).  Every check is per
(batch, head) or per row; the figures of a case are printed as [measured] (profiles/transformer_parity_measured.txt holds one run's).

a. attention, every table row in five input regimes: uniform (2 ulp of Sum v / Nk), onehot (v[pi(i)] bit for bit), diffuse and steep / steep-rev
   (RMS-relative error per head <= 4 x that of the fp32 CPU chain; every element inside E)
b. rows past Nq stay unwritten (mf_attention_f32 itself, on padded buffers)      c. a NaN in q or k stays where the reference's is
d. what the four wrappers refuse      e. linear within E over its variants      f. LayerNorm within E, C = 1 exact      g. GEGLU"""
import pytest
import torch

from tests import transformer_cases as TC

pytestmark = pytest.mark.gpu

REFUSED = (AssertionError, RuntimeError)
SENTINEL = -7777.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import medfusion_amd  # noqa: F401  (loads libmedfusion_hip.so; raises if missing)
    return torch.device("cuda:0")


def _place(case, t, dev):
    """the tensor on the device at the alignment the case names"""
    if case[5]:
        td = t.to(dev)
        assert td.data_ptr() % 16 == 0
        return td
    return TC.misaligned(t, dev)


def _attend(K, case, q, k, v, dev):
    """K.attention on the case's placement -> (fp32 [B, Nq, C] on the CPU, the same in head layout)"""
    H, d = case[1], case[4]
    got = K.attention(_place(case, q, dev), _place(case, k, dev), _place(case, v, dev), H, TC.attn_scale(d)).cpu()
    assert got.shape == q.shape and got.dtype == torch.float32
    return got, TC.heads(got, H)


# ---------------------------------------------------------------- a. attention against fp64

@pytest.mark.parametrize("case", TC.ATTN_CASES, ids=TC.case_id)
def test_attention_regimes_against_fp64(dev, case):
    from medfusion_amd import kernels as K
    B, H, Nq, Nk, d, _ = case
    cs = TC.attn_census(case)
    cid = f"{TC.case_id(case)} ({cs['path']})"
    for regime in TC.REGIMES:
        q, k, v = TC.attn_inputs(case, regime)
        got, gh = _attend(K, case, q, k, v, dev)
        assert bool(torch.isfinite(got).all()), (case, regime)
        if regime == "uniform":
            want = TC.uniform_expected(v, H).expand(B, H, Nq, d)
            ulps = torch.where(want == 0, torch.where(gh != 0, float("inf"), 0.0).double(), (gh.double() - want).abs() / TC.ulp32(want).clamp_min(1e-300))
            worst = ulps.amax(dim=(-1, -2))      # per (batch, head)
            print(f"[measured] attention {cid} uniform: |out - Sum v / Nk| <= {float(worst.max()):.3f} ulp")
            assert float(worst.max()) <= 2.0, (case, regime, worst.tolist())
        elif regime == "onehot":
            want = TC.onehot_expected(case, v)
            same = (got.view(torch.int32) == want.contiguous().view(torch.int32))
            wrong = TC.heads(~same, H).sum(dim=(-1, -2))      # per (batch, head)
            print(f"[measured] attention {cid} onehot: {int(wrong.sum())} of {got.numel()} elements differ from v[pi(i)] in their bits")
            assert int(wrong.sum()) == 0, (case, regime, wrong.tolist(), (~same).nonzero()[:8].tolist())
        else:
            tm = TC.attn_terms(q, k, v, H)
            E = TC.attn_bound_E(tm, cs["T"])
            rk, rc = TC.rms_rel(gh, tm["out"]), TC.rms_rel(TC.attn_chain(q, k, v, H), tm["out"])
            over_E = TC.ratio_heads(gh, tm["out"], E)
            rel = torch.where(rk == 0, torch.zeros_like(rk), rk / rc)
            print(f"[measured] attention {cid} {regime}: kernel / fp32-chain RMS ratio <= {float(rel.max()):.3f} (chain's RMS-relative error "
                  f"{float(rc.min()):.2e} to {float(rc.max()):.2e}), largest |err| / E {float(over_E.max()):.4f}")
            assert bool((rk <= 4.0 * rc).all()), (case, regime, rk.tolist(), rc.tolist())
            assert float(over_E.max()) <= 1.0, (case, regime, over_E.tolist())


# ---------------------------------------------------------------- b. the canary

@pytest.mark.parametrize("case", TC.CANARY_CASES, ids=TC.case_id)
def test_attention_leaves_rows_past_nq_alone(dev, case):
    from medfusion_amd import kernels as K, lib as L
    B, H, Nq, Nk, d, _ = case
    C = H * d
    q, k, v = (t.to(dev) for t in TC.attn_inputs(case, "diffuse"))
    want = K.attention(q, k, v, H, TC.attn_scale(d))
    qpad = torch.full((B, Nq + 3, C), SENTINEL, device=dev)
    qpad[:, :Nq] = q
    out = torch.full((B, Nq + 3, C), SENTINEL, device=dev)
    if TC.attn_census(case)["path"] == "mfma":      # (a batch of the padded buffers starts on a 16-byte boundary: the same path as K.attention)
        assert all(t[b].data_ptr() % 16 == 0 for t in (qpad, out, k, v) for b in range(B))
    for b in range(B):      # one call per batch: the entry's batch stride is Nq C, the buffers' (Nq + 3) C
        rc = L.load().mf_attention_f32(qpad[b].data_ptr(), k[b].data_ptr(), v[b].data_ptr(), out[b].data_ptr(), 1, H, Nq, Nk, d, TC.attn_scale(d), K.stream())
        L.check(rc, "mf_attention_f32")
    torch.cuda.synchronize()
    assert bool((out[:, Nq:] == SENTINEL).all()), (case, (out[:, Nq:] != SENTINEL).nonzero()[:8].tolist())
    assert torch.equal(out[:, :Nq], want), case      # (same kernel, same arithmetic: the rows that are written are those of K.attention)


# ---------------------------------------------------------------- c. NaN confinement

@pytest.mark.parametrize("case", TC.NAN_CASES, ids=TC.case_id)
def test_attention_confines_a_nan(dev, case):
    from medfusion_amd import kernels as K
    B, H, Nq, Nk, d, _ = case
    q, k, v = TC.attn_inputs(case, "diffuse")
    base, _ = _attend(K, case, q, k, v, dev)
    assert bool(torch.isfinite(base).all())
    b0, h0 = B - 1, H - 1
    # the last query (the lanes past Nq hold clamped copies of it) and the last key (alone in a ragged tile whose padding rows copy it)
    for which, row in (("q", Nq - 1), ("k", Nk - 1)):
        qn, kn = q.clone(), k.clone()
        (qn if which == "q" else kn)[b0, row, h0 * d + d // 2] = float("nan")
        ref_nan = torch.isnan(TC.attn_terms(qn, kn, v, H)["out"])
        expect = torch.zeros((B, H, Nq, d), dtype=torch.bool)
        if which == "q":
            expect[b0, h0, row] = True
        else:
            expect[b0, h0] = True
        assert torch.equal(ref_nan, expect), (case, which)
        got, gh = _attend(K, case, qn, kn, v, dev)
        assert torch.equal(torch.isnan(gh), ref_nan), (case, which, (torch.isnan(gh) != ref_nan).nonzero()[:8].tolist())
        keep = ~TC.heads(torch.isnan(got), H)
        assert torch.equal(gh.contiguous().view(torch.int32)[keep], TC.heads(base, H).contiguous().view(torch.int32)[keep]), (case, which)


# ---------------------------------------------------------------- d. refusals

def _pairs_only_tensor(K, dev, shape):
    """a tensor whose values exist only as fp16 pairs: the output of the GroupNorm-apply pass with out_fp32=False"""
    x = torch.randn(shape, device=dev)
    rec, parts = K.gn_stats_partial(x, 1)
    t = K.gn_apply(x, K.GnPartials(rec, parts, 1e-5), None, None, 1, 1, split=True, bconst=float(x[0].numel()) ** 0.5, out_fp32=False)
    assert K.pairs_only(t)
    return t


def test_wrappers_refuse_what_the_kernels_would_misread(dev):
    from medfusion_amd import kernels as K
    g = torch.Generator().manual_seed(7)
    rnd = lambda *shape: torch.randn(shape, generator=g).to(dev)
    q, k, v = rnd(2, 5, 32), rnd(2, 9, 32), rnd(2, 9, 32)
    s = TC.attn_scale(16)
    ok = K.attention(q, k, v, 2, s)
    with pytest.raises(REFUSED, match="fp32"):
        K.attention(q.double(), k, v, 2, s)
    with pytest.raises(REFUSED, match="contiguous"):
        K.attention(q, rnd(2, 32, 9).transpose(1, 2), v, 2, s)
    with pytest.raises(REFUSED, match="heads"):
        K.attention(q, k, v, 3, s)
    with pytest.raises(REFUSED, match="k .* and v"):
        K.attention(q, k, rnd(2, 8, 32), 2, s)
    with pytest.raises(REFUSED, match="k .* and v"):
        K.attention(q, rnd(2, 9, 16), rnd(2, 9, 16), 2, s)
    po = _pairs_only_tensor(K, dev, (2, 1, 5, 32))
    with pytest.raises(REFUSED, match="only as fp16 pairs"):
        K.attention(po, k, v, 2, s)
    with pytest.raises(RuntimeError, match="head dim 129"):
        K.attention(rnd(1, 4, 129), rnd(1, 8, 129), rnd(1, 8, 129), 1, TC.attn_scale(129))
    assert torch.equal(K.attention(q, k, v, 2, s), ok)      # (and what is right is still taken)

    x, ga, be = rnd(3, 4, 40), rnd(40), rnd(40)
    ok = K.layernorm(x, ga, be)
    with pytest.raises(REFUSED, match="fp32"):
        K.layernorm(x.double(), ga, be)
    with pytest.raises(REFUSED, match="fp32"):
        K.layernorm(x, ga.double(), be)
    with pytest.raises(REFUSED, match="contiguous"):
        K.layernorm(rnd(3, 40, 4).transpose(1, 2), ga, be)
    with pytest.raises(REFUSED, match="gamma"):
        K.layernorm(x, rnd(4), rnd(4))
    with pytest.raises(REFUSED, match="only as fp16 pairs"):
        K.layernorm(_pairs_only_tensor(K, dev, (1, 3, 4, 40)), ga, be)
    assert torch.equal(K.layernorm(x, ga, be), ok)

    h = rnd(3, 4, 48)
    ok = K.geglu(h)
    with pytest.raises(REFUSED, match="fp32"):
        K.geglu(h.double())
    with pytest.raises(REFUSED, match="contiguous"):
        K.geglu(rnd(3, 48, 4).transpose(1, 2))
    with pytest.raises(REFUSED, match="contiguous"):
        K.geglu(rnd(3, 4, 47))
    with pytest.raises(REFUSED, match="only as fp16 pairs"):
        K.geglu(_pairs_only_tensor(K, dev, (1, 3, 4, 48)))
    assert torch.equal(K.geglu(h), ok)

    x, w, b = rnd(3, 8), rnd(5, 8), rnd(5)
    ok = K.linear(x, w, b)
    with pytest.raises(REFUSED, match="fp32"):
        K.linear(x.double(), w, b)
    with pytest.raises(REFUSED, match="fp32"):
        K.linear(x, w.double(), b)
    with pytest.raises(REFUSED, match="fp32"):
        K.linear(x, w, b, out=torch.zeros((3, 5), dtype=torch.float64, device=dev))
    with pytest.raises(REFUSED, match="bias"):
        K.linear(x, w, rnd(4))
    with pytest.raises(REFUSED, match="out"):
        K.linear(x, w, b, out=torch.zeros((3, 6), device=dev))
    with pytest.raises(REFUSED, match="out"):
        K.linear(x, w, b, out=torch.zeros((3, 10), device=dev)[:, ::2])
    with pytest.raises(REFUSED):
        K.linear(x, rnd(8, 5).t(), b)      # a transposed weight
    with pytest.raises(REFUSED):
        K.linear(rnd(8, 3).t(), w, b)      # a transposed input
    assert torch.equal(K.linear(x, w, b), ok)


def test_linear_limits(dev):
    """In = 2048 is exactly 64 KiB of dynamic LDS and runs (test_linear_is_within_E); 2049 is refused.  The float4 loop needs a 16-byte aligned
    weight: refused 4 bytes off at In = 260, while In = 1027 (the scalar loop) runs there and stays inside E."""
    from medfusion_amd import kernels as K
    g = torch.Generator().manual_seed(11)
    with pytest.raises(RuntimeError, match="In=2049 too large"):
        K.linear(torch.randn((2, 2049), generator=g).to(dev), torch.randn((3, 2049), generator=g).to(dev), None)
    x_wide, w, bias, _ = TC.lin_inputs((17, 260, 7))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        K.linear(TC.x_of(x_wide.to(dev)), TC.misaligned(w, dev), bias.to(dev))
    x_wide, w, bias, _ = TC.lin_inputs((3, 1027, 5))
    got = K.linear(TC.x_of(x_wide.to(dev)), TC.misaligned(w, dev), bias.to(dev)).cpu()
    tm = TC.lin_terms(TC.x_of(x_wide), w, bias, False, False)
    ratios = TC.ratio_rows(got, tm["out"], TC.lin_bound_E(tm))
    print(f"[measured] linear 3-1027-5, weight 4 bytes off: largest |err| / E {max(ratios):.3f}")
    assert max(ratios) <= 1.0, ratios


# ---------------------------------------------------------------- e. linear

@pytest.mark.parametrize("case", TC.LIN_CASES, ids=TC.case_id)
def test_linear_is_within_E(dev, case):
    from medfusion_amd import kernels as K
    B, In, Out = case
    x_wide, w, bias, out_wide = TC.lin_inputs(case)
    x_cpu, out0_cpu = TC.x_of(x_wide), TC.out_of(out_wide)
    wd, bd = w.to(dev), bias.to(dev)
    worst = (0.0, None)
    for variant in TC.LIN_VARIANTS:
        act_in, act_out, has_bias, x_slice, out_slice, acc = variant
        x = TC.x_of(x_wide.to(dev)) if x_slice else x_cpu.contiguous().to(dev)
        assert B == 1 or (x.stride(0) == In + 8) == x_slice      # (one row has no row stride to speak of)
        ow = torch.cat([out_wide, torch.full((8, Out + 8), SENTINEL)]).to(dev)      # (8 more rows: a pass of linear_kernel handles 8)
        out = TC.out_of(ow[:B]) if out_slice else (out0_cpu.contiguous().to(dev) if acc else None)
        got = K.linear(x, wd, bd if has_bias else None, act_in=act_in, act_out=act_out, out=out, accumulate=acc)
        assert out is None or got is out
        tm = TC.lin_terms(x_cpu, w, bias if has_bias else None, act_in, act_out, out0_cpu if acc else None)
        ratios = TC.ratio_rows(got.cpu(), tm["out"], TC.lin_bound_E(tm))      # per row: the rows are 2^6 apart
        if max(ratios) > worst[0]:
            worst = (max(ratios), variant)
        assert max(ratios) <= 1.0, (case, variant, ratios)
        if out_slice:      # the columns around the slice and the rows below it keep their values
            owc = ow.cpu()
            assert torch.equal(owc[:B, :4], out_wide[:, :4]) and torch.equal(owc[:B, -4:], out_wide[:, -4:]), (case, variant)
            assert bool((owc[B:] == SENTINEL).all()), (case, variant, (owc[B:] != SENTINEL).nonzero()[:8].tolist())
    print(f"[measured] linear / E, case {TC.case_id(case)}: {worst[0]:.3f} at (act_in, act_out, bias, x slice, out slice, accumulate) = {worst[1]}")


# ---------------------------------------------------------------- f. LayerNorm

@pytest.mark.parametrize("case", TC.LN_CASES, ids=TC.case_id)
def test_layernorm_is_within_E(dev, case):
    from medfusion_amd import kernels as K
    rows, C = case
    for regime in TC.LN_REGIMES:
        x, gamma, beta = TC.ln_inputs(case, regime)
        got = K.layernorm(x.to(dev), gamma.to(dev), beta.to(dev), TC.LN_EPS).cpu()
        tm = TC.ln_terms(x, gamma, beta)
        ratios = TC.ratio_rows(got, tm["out"], TC.ln_bound_E(tm))
        print(f"[measured] layernorm / E, case {TC.case_id(case)} {regime}: {max(ratios):.3f}")
        assert max(ratios) <= 1.0, (case, regime, ratios)
        if C == 1:
            assert torch.equal(got, beta.expand(rows, 1)), (case, regime)


# ---------------------------------------------------------------- g. GEGLU

@pytest.mark.parametrize("case", TC.GEGLU_CASES, ids=TC.case_id)
def test_geglu_against_the_cpu_chain(dev, case):
    from medfusion_amd import kernels as K
    h = TC.geglu_inputs(case)
    tm = TC.geglu_terms(h)
    got = K.geglu(h.to(dev)).cpu()
    assert got.shape == tm["out"].shape
    rk, rc = TC.geglu_ratio(got, tm), TC.geglu_ratio(TC.geglu_chain(h), tm)
    print(f"[measured] geglu, case {TC.case_id(case)}: kernel |err| / E0 {rk:.4f}, fp32 CPU a * F.gelu(g) {rc:.4f}")
    assert rk <= 4.0 * rc, (case, rk, rc)
