"""The yardstick of tests/test_transformer_gpu.py, checked without a GPU (tests/transformer_cases.py): every row of the attention table lands on
the path and edge it is there for; the exact regimes are exact in the fp64 restatement and the one-hot gap is >= 200; a plain fp32 torch chain
of each of the four operations stays inside its bound (at most 0.95 of it) while the bound stays of the order of u times the conditioning it
claims; a restatement with the last key dropped, or with s = d^-0.5, leaves both attention criteria by a factor > 100.

Figures of the fp32 chains on the CPU (printed as [measured]): attention, largest |err| / E over the table: diffuse 0.005 to 0.07, steep and
steep-rev 0.003 to 0.16 (0 where one key carries the whole weight); the chain's own RMS-relative error 1e-7 to 4e-7 (diffuse), up to 5.7e-6
(steep); largest E / Sum w |v| 3e-6 to 2.7e-3.  linear 0.28 to 0.84 of E (the accumulating variants lead: half an ulp of a large `out` under a bound of one), LayerNorm 0.06 to 0.23,
GEGLU 0.0005 (one element) to 1.76 of E0, which leaves the error of erf out (see test_fp32_geglu_chain_against_E0)."""
import math

import pytest
import torch

from tests import transformer_cases as TC

u = TC.U24

# what every row of the attention table is there for: the census entries its comment names
ATTN_EXPECT = {
    (1, 1, 1, 8, 8, True): {"path": "mfma", "tiles": 1, "idle_waves": 3, "ragged": True, "last_tile_keys": 8, "DT": 1},
    (2, 3, 33, 7, 8, True): {"path": "valu", "mfma_dim_on_valu": True, "tiles": 1, "upper_half": False},
    (2, 2, 31, 31, 16, True): {"path": "mfma", "tiles": 1, "ragged": True, "last_tile_keys": 31, "ragged_wave": True, "idle_waves": 3},
    (1, 2, 32, 32, 16, True): {"path": "mfma", "tiles": 1, "ragged": False, "ragged_wave": False, "idle_waves": 3},
    (2, 2, 33, 33, 16, True): {"path": "mfma", "tiles": 2, "ragged": True, "last_tile_keys": 1, "idle_waves": 2},
    (1, 2, 127, 63, 32, True): {"path": "mfma", "tiles": 2, "ragged": True, "last_tile_keys": 31, "blocks": 1, "idle_waves": 0, "ragged_wave": True},
    (1, 1, 128, 64, 32, True): {"path": "mfma", "tiles": 2, "ragged": False, "blocks": 1, "idle_waves": 0, "ragged_wave": False},
    (2, 1, 129, 65, 32, True): {"path": "mfma", "tiles": 3, "ragged": True, "last_tile_keys": 1, "blocks": 2, "idle_waves": 3},
    (1, 2, 40, 47, 64, True): {"path": "mfma", "DT": 2, "tiles": 2, "ragged": True},
    (1, 1, 70, 130, 128, True): {"path": "mfma", "DT": 4, "tiles": 5, "ragged": True, "last_tile_keys": 2},
    (2, 2, 33, 47, 16, False): {"path": "valu", "mfma_dim_on_valu": True, "tiles": 1, "ragged": True},
    (1, 1, 70, 130, 128, False): {"path": "valu", "mfma_dim_on_valu": True, "upper_half": True, "upper_lanes": 64, "lds_bytes": 99840, "over_64k": True, "tiles": 3, "blocks": 2},
    (1, 2, 40, 97, 64, False): {"path": "valu", "mfma_dim_on_valu": True, "upper_half": False, "upper_lanes": 0, "over_64k": False, "tiles": 2},
    (2, 2, 40, 97, 65, True): {"path": "valu", "upper_half": True, "upper_lanes": 1, "over_64k": False, "tiles": 2},
    (1, 1, 20, 70, 84, True): {"path": "valu", "upper_half": True, "upper_lanes": 20, "over_64k": True, "lds_bytes": 66048, "tiles": 2, "last_tile_keys": 6},
    (1, 2, 17, 65, 127, True): {"path": "valu", "upper_half": True, "upper_lanes": 63, "over_64k": True, "tiles": 2, "last_tile_keys": 1},
    (2, 3, 9, 33, 12, True): {"path": "valu", "upper_half": False, "over_64k": False, "tiles": 1},
    (1, 2, 5, 64, 1, True): {"path": "valu", "upper_half": False, "tiles": 1, "ragged": False},
    (2, 4, 64, 1, 4, True): {"path": "valu", "tiles": 1, "last_tile_keys": 1},
}


def test_every_attention_row_lands_on_the_path_it_names():
    assert list(ATTN_EXPECT) == TC.ATTN_CASES
    rows = []
    for case, want in ATTN_EXPECT.items():
        cs = TC.attn_census(case)
        got = {k: cs[k] for k in want}
        assert got == want, (case, got, want)
        rows.append(cs)
    valu = [r for r in rows if r["path"] == "valu"]
    mfma = [r for r in rows if r["path"] == "mfma"]
    assert valu and mfma
    assert {r["DT"] for r in mfma} == {1, 2, 4} and {r["ragged"] for r in mfma} == {True, False} and max(r["tiles"] for r in mfma) >= 4
    # d = 83 is the last head dim under 64 KiB: 84 is the edge the table claims
    assert TC.attn_census((1, 1, 20, 70, 83, True))["lds_bytes"] <= 64 * 1024 < TC.attn_census((1, 1, 20, 70, 84, True))["lds_bytes"]
    assert max(r["lds_bytes"] for r in valu) <= 160 * 1024      # what mf_attention_f32 asks hipFuncSetAttribute for
    # every (path x regime): each case runs every regime
    assert {(r["path"], g) for r in rows for g in TC.REGIMES} == {(p, g) for p in ("mfma", "valu") for g in TC.REGIMES}
    for case in TC.CANARY_CASES + TC.NAN_CASES:
        assert case in TC.ATTN_CASES
    assert {TC.attn_census(c)["path"] for c in TC.NAN_CASES} == {"mfma", "valu"} == {TC.attn_census(c)["path"] for c in TC.CANARY_CASES}


def test_small_op_rows_land_on_the_paths_they_name():
    lc = {case: TC.lin_census(case) for case in TC.LIN_CASES}
    assert [lc[c]["passes"] for c in TC.LIN_CASES] == [1, 1, 2, 3, 1, 2]
    assert lc[(8, 3, 5)]["last_pass_rows"] == 8 and lc[(9, 4, 4)]["last_pass_rows"] == 1 and lc[(17, 260, 7)]["last_pass_rows"] == 1
    assert [lc[c]["float4"] for c in TC.LIN_CASES] == [False, False, True, True, False, True]
    assert lc[(17, 260, 7)]["float4_ragged_last_turn"] and lc[(17, 260, 7)]["float4_turns"] == 2
    assert lc[(9, 2048, 4)]["lds_at_limit"] and not lc[(9, 2048, 4)]["refused"] and TC.lin_census((1, 2049, 1))["refused"]
    assert lc[(8, 3, 5)]["idle_waves"] == 3 and lc[(8, 3, 5)]["blocks"] == 2
    for flag in range(6):      # every flag of the variants is seen on and off
        assert {v[flag] for v in TC.LIN_VARIANTS} == {True, False}
    nc = {case: TC.ln_census(case) for case in TC.LN_CASES}
    assert [nc[c]["lane_turns"] for c in TC.LN_CASES] == [1, 1, 1, 2, 5, 20]
    assert nc[(1, 1)]["idle_lanes"] == 63 and nc[(5, 63)]["idle_lanes"] == 1 and nc[(4, 64)]["idle_lanes"] == 0 and nc[(7, 65)]["last_turn_lanes"] == 1
    assert [nc[c]["idle_waves"] for c in TC.LN_CASES] == [3, 3, 0, 1, 1, 3]
    gc = [TC.geglu_census(case) for case in TC.GEGLU_CASES]
    assert [g["second_round"] for g in gc] == [False, False, True] and gc[2]["total"] == 525825 and gc[2]["blocks"] == 2048
    for case in TC.GEGLU_CASES[1:]:
        gate = TC.geglu_inputs(case)[:, case[1]:]
        assert set(TC.GEGLU_PLANTED) <= set(gate.flatten().tolist()), case


@pytest.mark.parametrize("case", TC.ATTN_CASES, ids=TC.case_id)
def test_exact_regimes_are_exact_in_the_restatement(case):
    B, H, Nq, Nk, d, _ = case
    q, k, v = TC.attn_inputs(case, "uniform")
    hs = TC.head_scales(B, H)
    units = TC.heads(v, H) / (4.0 * hs.permute(0, 2, 1, 3))
    assert torch.equal(units, units.round()) and float(units.abs().max()) <= 8 and bool((q == 0).all()) and bool((k != 0).any())
    tm = TC.attn_terms(q, k, v, H)
    assert bool((tm["score"] == 0).all())
    want = TC.uniform_expected(v, H)
    # (fp64 softmax weights are fl(1 / Nk): Sum v / Nk up to fp64 rounding, nine orders below an fp32 ulp)
    assert float(((tm["out"] - want).abs() / (4.0 * hs.permute(0, 2, 1, 3).double())).max()) <= 8 * 2.0 ** -50
    q, k, v = TC.attn_inputs(case, "onehot")
    tm = TC.attn_terms(q, k, v, H)
    assert torch.equal(tm["out"], TC.heads(TC.onehot_expected(case, v), H).double()), case
    gap = TC.onehot_gap(case)
    pi = TC.onehot_pi(Nq, Nk, d)
    if d > 1 and Nq >= Nk:
        assert set(pi) == set(range(Nk)), case      # every key slot wins for some query
    c = TC.onehot_c(d)
    assert 200.0 <= (c * TC.attn_scale(d)) ** 2 <= 203.2 and c * 2 ** 20 % 1 == 0 and math.frexp(c)[0] * 256 % 1 == 0
    print(f"[measured] one-hot gap, case {TC.case_id(case)}: {gap:.2f}; largest |score| {float(tm['score'].abs().max()):.3g}")
    assert gap >= 200.0, (case, gap)
    assert float(tm["score"].abs().max()) * 2 * u <= 1.0 or d == 1      # the fp32 rounding of a score stays below 1


@pytest.mark.parametrize("case", TC.ATTN_CASES, ids=TC.case_id)
def test_fp32_attention_chain_is_inside_E_and_the_mutations_are_outside(case):
    B, H, Nq, Nk, d, _ = case
    cs = TC.attn_census(case)
    for regime in ("diffuse", "steep", "steep-rev"):
        q, k, v = TC.attn_inputs(case, regime)
        tm = TC.attn_terms(q, k, v, H)
        E = TC.attn_bound_E(tm, cs["T"])
        chain = TC.attn_chain(q, k, v, H)
        ratio = float(TC.ratio_heads(chain, tm["out"], E).max())
        rms = TC.rms_rel(chain, tm["out"])
        # E stays of the order of u times its own conditioning: the scores' (d + 3) A, the exponent's 3 + 2 |x| (where the weights are), the chain
        live = tm["w"] > u
        cond = 2.0 * ((d + 3) * float(tm["A"][live].max()) + 3.0 + 2.0 * float(tm["x"][live].abs().max())) + min(Nk, cs["T"]) + 2 * cs["tiles"] + 3
        wv = tm["w"] @ tm["absv"]
        assert float((E / wv).max()) <= u * cond * (1 + 1e-9), (case, regime)
        print(f"[measured] fp32 chain, case {TC.case_id(case)} {regime}: max |err| / E {ratio:.4f}, RMS-relative error {float(rms.max()):.2e}, "
              f"max E / sum w|v| {float((E / wv).max()):.2e}")
        assert ratio <= 0.95, (case, regime, ratio)
        if regime == "steep-rev":      # the same problem in another key order
            fwd = TC.attn_terms(*TC.attn_inputs(case, "steep"), H)["out"]
            assert float(((fwd - tm["out"]).abs() / E).max()) < 1e-6
        if regime != "diffuse" or Nk == 1:
            continue
        muts = [("last key dropped", {"drop_last_key": True})] + ([("s = d^-0.5", {"scale": d ** -0.5})] if d > 1 else [])
        for name, kw in muts:
            bad = TC.attn_terms(q, k, v, H, **kw)["out"]
            over_E = float(TC.ratio_heads(bad, tm["out"], E).amin())      # every (batch, head) sees it
            over_rms = float((TC.rms_rel(bad, tm["out"]) / (4.0 * rms)).amin())
            print(f"[measured] mutation '{name}', case {TC.case_id(case)}: max |err| / E >= {over_E:.3g}, RMS / (4 x chain's) >= {over_rms:.3g} in every head")
            assert over_E > 100.0 and over_rms > 100.0, (case, name, over_E, over_rms)


@pytest.mark.parametrize("case", TC.LIN_CASES, ids=TC.case_id)
def test_fp32_linear_chain_is_inside_E(case):
    B, In, Out = case
    x_wide, w, bias, out_wide = TC.lin_inputs(case)
    worst = 0.0
    for act_in, act_out, has_bias, x_slice, out_slice, acc in TC.LIN_VARIANTS:
        x = TC.x_of(x_wide)
        out0 = TC.out_of(out_wide) if acc else None
        b = bias if has_bias else None
        tm = TC.lin_terms(x, w, b, act_in, act_out, out0)
        E = TC.lin_bound_E(tm)
        ratio = max(TC.ratio_rows(TC.lin_chain(x, w, b, act_in, act_out, out0), tm["out"], E))
        worst = max(worst, ratio)
        assert ratio <= 0.95, (case, act_in, act_out, ratio)
        # of the order of u (chain length) times the sum of the magnitudes
        assert bool((E <= 1.1 * (-(-In // 64) + 8 + 5 + 5 + 1) * u * (tm["S"] + tm["out"].abs()) + 2 * TC.TINY * (1 + tm["absw"])).all()), case
    print(f"[measured] fp32 linear chain / E, case {TC.case_id(case)}: {worst:.3f}")


@pytest.mark.parametrize("case", TC.LN_CASES, ids=TC.case_id)
def test_fp32_layernorm_chain_is_inside_E_and_a_one_pass_variance_is_not(case):
    rows, C = case
    n = -(-C // 64)
    for regime in TC.LN_REGIMES:
        x, gamma, beta = TC.ln_inputs(case, regime)
        tm = TC.ln_terms(x, gamma, beta)
        want = torch.nn.functional.layer_norm(x.double(), (C,), gamma.double(), beta.double(), TC.LN_EPS)
        assert float((tm["out"] - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max()))
        E = TC.ln_bound_E(tm)
        ratio = max(TC.ratio_rows(TC.ln_chain(x, gamma, beta), tm["out"], E))
        print(f"[measured] fp32 LayerNorm chain / E, case {TC.case_id(case)} {regime}: {ratio:.3f}")
        assert ratio <= 0.95, (case, regime, ratio)
        # u times the conditioning: |mean| / sigma for the mean, |z| for the rest (dm^2 / var stays below u (n + 7)^2 u |mean|^2 / var)
        k2 = ((n + 7) * u * tm["absmean"]) ** 2 / (2.0 * (tm["var"] + tm["eps"]))
        cond = tm["ga"].abs() * (tm["absmean"] * tm["rstd"] + tm["z"].abs()) + (tm["z"] * tm["ga"]).abs() + tm["t"].abs()
        assert bool((E <= ((n + 7) + (n / 2.0 + 10.0)) * u * cond + k2 * tm["ga"].abs() * tm["z"].abs() + 1e-300).all()), (case, regime)
        if C == 1:
            assert torch.equal(tm["out"], beta.double().expand(rows, 1))
    if C >= 63:      # the yardstick can see: a one-pass fp32 variance at mean = 1000 sigma
        x, gamma, beta = TC.ln_inputs(case, "offset")
        tm = TC.ln_terms(x, gamma, beta)
        over = max(TC.ratio_rows(TC.ln_one_pass(x, gamma, beta), tm["out"], TC.ln_bound_E(tm)))
        print(f"[measured] one-pass variance / E, case {TC.case_id(case)} offset: {over:.3g}")
        assert over > 100.0, (case, over)


@pytest.mark.parametrize("case", TC.GEGLU_CASES, ids=TC.case_id)
def test_fp32_geglu_chain_against_E0(case):
    """E0 leaves the error of erf itself out, so the CPU chain is not held to 0.95 of it: its figure IS the yardstick of the GPU test (4 x).  Here:
    E0 is of the order of u |a g|; an erf good to 4 u absolute (4 ulp at |erf| near 1) adds |a g| / 2 * 4 u <= 2 E0, so the chain stays below 3;
    and the tanh form of GELU in place of the erf form leaves 4 x the chain's figure by a factor > 100."""
    h = TC.geglu_inputs(case)
    tm = TC.geglu_terms(h)
    assert float((tm["one_plus_erf"] - (1.0 + tm["erf"])).abs().max()) <= 2.0 ** -52 * 2
    E0 = TC.geglu_bound_E0(tm)
    assert bool((E0 <= 5.0 * u * (tm["a"] * tm["g"]).abs()).all()) and bool((E0 >= u * (tm["a"] * tm["g"]).abs()).all())
    ratio = TC.geglu_ratio(TC.geglu_chain(h), tm)
    print(f"[measured] fp32 GEGLU chain (a * F.gelu(g)) / E0, case {TC.case_id(case)}: {ratio:.3f}")
    assert ratio <= 3.0, (case, ratio)
    if case[0] * case[1] > 1:
        a, g = h.chunk(2, dim=-1)
        over = TC.geglu_ratio(a * torch.nn.functional.gelu(g, approximate="tanh"), tm)
        print(f"[measured] tanh-form GELU / E0, case {TC.case_id(case)}: {over:.3g}")
        assert over > 100.0 * 4.0 * ratio, (case, over, ratio)
