"""What tests/test_step_gpu.py assumes, checked without a GPU (no device, no library load): the launch arithmetic of every cap shape restated from
csrc/sched_noise.hip and the cited lines held to the source, the table of extreme Philox counters against philox4x32_10, the learned-variance
bound holding for the fp32 ATen chain on every case, and the non-finite counts of every seeded case."""
import numpy as np
import pytest
import torch

import medfusion_amd as M
from oracle import restate as R
from oracle import synth as S
from tests import step_cases as SC


def _lines(path):
    return path.read_text().splitlines()


# ------------------------------------------------------------------------------------------------ 1. the caps
def test_every_cap_shape_crosses_its_cap():
    for name, n, blocks, trips, last in SC.CAP_RUNS:
        spec = SC.LAUNCHES[name]
        work = spec["work"](n)
        assert SC.launch(work, spec["cap"]) == (blocks, trips), name
        assert blocks == spec["cap"] and trips >= 2 and work - (trips - 1) * blocks * SC.WG == last and 0 < last < blocks * SC.WG, name
        print(f"[measured] {name}: {work} items on {blocks} workgroups of {SC.WG}: {trips} trips, {last} items in the last")
    n = SC.numel(SC.CAP)
    B, Cc, cells = SC.CAP
    assert n == 1_050_000 and n % 4 == 0 and n // 4 == 1024 * 256 + 356 and 356 == 256 + 100      # a whole workgroup and a partial one on the second trip
    assert cells % 4 == 0 and (Cc * cells) // 4 == 52_500 and n % (4 * B) == 0                     # the blend and Philox forms accept it
    assert SC.numel(SC.CAP_PHILOX) // 4 == 2048 * 256 + 712 and SC.CAP_PHILOX[1] * SC.CAP_PHILOX[2] % 4 == 0
    assert SC.CAP_ABSDIFF[0] * SC.CAP_ABSDIFF[2] == 2048 * 256 + 712
    assert 4 * 2 * n == 8_400_000                                                                  # the largest tensor: a [2][n] history buffer
    # the largest n of the kernel tests that were there before stays under every cap: one trip
    assert SC.launch(15360, SC.STEP_CAP)[1] == 1 and SC.launch(15360 // 4, SC.WIDE_CAP)[1] == 1


def test_the_tails_split_into_a_vector_body_and_a_scalar_tail():
    for n in SC.TAILS:
        assert n % 4 != 0 and n < SC.STEP_CAP * SC.WG
        nq = n // 4
        assert (nq > 0) == (n > 1) and 0 < n - 4 * nq < 4                       # aligned: nq vectors, then 1..3 scalars (n = 1: scalars only)
        assert SC.launch(nq if nq else n, SC.STEP_CAP)[1] == 1 and SC.launch(n, SC.STEP_CAP)[1] == 1
    assert {SC.launch(n, SC.STEP_CAP)[0] for n in SC.TAILS} == {1, 2, 4}        # one workgroup, a whole one plus one element, four with a partial last
    assert 255 in SC.TAILS and 257 in SC.TAILS and 1023 in SC.TAILS


def test_the_restated_lines_are_the_source():
    src = _lines(SC.SOURCE)
    for name, spec in SC.LAUNCHES.items():
        for line, text in spec["lines"]:
            assert text in src[line - 1], (name, line, src[line - 1])
    for name, (line, text, code, fragment) in SC.REFUSALS.items():
        assert text in src[line - 1], (name, line, src[line - 1])
        window = " ".join(src[line - 1: line + 2])
        assert ("MF_EINVAL" if code == SC.EINVAL else "MF_EUNSUPPORTED") in window, name
        frag = fragment.split(": ", 1)[-1]
        assert frag in window, (name, frag)
    for line in SC.TICKET_LINES:
        assert SC.TICKET_TEXT in src[line - 1], line
    for line, text in SC.SAMPLE_CAST_LINES:
        assert text in src[line - 1], line
    assert SC.U01_LINE[1] in _lines(SC.PHILOX_H)[SC.U01_LINE[0] - 1]
    header = (SC.SOURCE.parents[2] / "include" / "medfusion_hip.h").read_text()
    assert "enum { MF_OK = 0, MF_EINVAL = -1, MF_EUNSUPPORTED = -2" in header and (SC.EINVAL, SC.EUNSUPPORTED) == (-1, -2)
    assert "mod 2^32" in header.split("int mf_philox_normal_f32")[0].rsplit("/* ---", 1)[1]       # the wrap of the sample counter is documented


# ------------------------------------------------------------------------------------------------ 2. the Philox table
def test_the_extreme_counters_hold_the_bits_they_claim():
    kinds = set()
    for sample, quad, draw, word, top in SC.EXTREMES:
        w = SC.philox_words(sample, quad, draw)
        assert w[word] >> 8 == top, (sample, quad, draw, word, hex(w[word]))
        assert sample < SC.EXTREME_SAMPLES and quad < SC.EXTREME_PER_SAMPLE // 4
        kinds.add((word, top))
        u = float(S._u01(np.uint32(w[word])))
        assert u == (1.0 if top == SC.ONES else 2.0 ** -25)
        block = SC.spec_block(draw)
        pair = block[sample, 4 * quad + 2 * (word // 2): 4 * quad + 2 * (word // 2) + 2]
        if word in (0, 2) and top == SC.ONES:          # radius -0: both normals are zeros of either sign
            assert np.all(pair == 0.0) and not np.any(np.isnan(pair))
        elif word in (0, 2):                           # the largest radius: sqrt(-2 ln 2^-25) = sqrt(50 ln 2)
            assert abs(float(np.hypot(*pair.astype(np.float64))) - float(np.sqrt(50 * np.log(2.0)))) < 1e-5
        else:                                          # angle 2 pi u with u = 1: the pair is (r, ~0)
            assert abs(float(pair[1])) < 1e-5 and float(pair[0]) > 0
        print(f"[measured] spec at sample {sample} quad {quad} draw {draw} word {word} ({'ones' if top else 'zero'}): {pair.tolist()}")
        assert np.isfinite(block).all()
    assert kinds == {(0, SC.ONES), (2, SC.ONES), (0, SC.ZERO), (2, SC.ZERO), (1, SC.ONES), (3, SC.ONES)}
    # the two zero-radius-word entries as the spec evaluates them
    assert abs(float(SC.spec_block(1721)[0, 4 * 453:4 * 453 + 2].min()) - (-5.868124)) < 1e-5
    assert abs(float(SC.spec_block(1932)[2, 4 * 252 + 2:4 * 252 + 4].min()) - (-5.685834)) < 1e-5
    # a shape of (8, 4, 1024) reaches quad 958 of sample 0 and quad 131 of sample 4
    assert 4 * 1024 // 4 > 958 and 8 > 4


def test_the_spec_wraps_the_sample_index_mod_2_32():
    per = 8
    for off in (2 ** 31 - 2, 2 ** 32 - 2):
        rows = SC.spec_rows(SC.SEED, 3, off, 4, per)
        for b in range(4):
            one = S.philox_normal(SC.SEED, 3, np.array([(off + b) % 2 ** 32], dtype=np.uint32), per)
            assert np.array_equal(rows[b], one[0])
    assert np.array_equal(SC.spec_rows(SC.SEED, 3, 2 ** 32 - 2, 4, per)[2:], S.philox_normal(SC.SEED, 3, np.arange(2), per))


# ------------------------------------------------------------------------------------------------ 3. learned variance
def test_the_aten_chain_sits_inside_the_learned_variance_bound():
    osch = SC.oracle_scheduler()
    psch = M.GaussianNoiseScheduler(**R.published_scheduler_kwargs())
    assert SC.EXP_ULPS == max(SC.EXP_ULPS_ATEN, SC.EXP_ULPS_DEVICE) >= 1
    worst, seen = 0.0, set()
    for case in SC.variance_cases():
        x_t, pred, pv, npost = SC.variance_inputs(case)
        assert float(pv.abs().max()) <= case["amp"] and float(pv.abs().max()) > 0.9 * case["amp"]
        c = SC.chain32(osch, [case["t"]], 0, False, x_t, pred, None, 1.0, 0, False, npost, pv=pv)
        rec = psch.step_records([case["t"]], False)[0]
        assert rec.t == case["t"] and rec.mode == 0
        want, E = SC.variance_bound(c["mean"], c["hl"], npost, case["t"])
        assert all(bool(torch.isfinite(v).all()) for v in (c["x_t"], c["x0"], want, E))
        err = (c["x_t"].double() - want).abs()
        if case["t"] == 0:
            assert SC.same_bits(c["x_t"], c["mean"]) == []
            continue
        bad = (err > E).nonzero().reshape(-1)
        ratio = float((err / E).max())
        worst = max(worst, ratio)
        sn = (want - c["mean"].double()).abs()
        seen.add("dominates" if float((sn / c["mean"].double().abs()).median()) > 1e3 else "vanishes" if float((sn / c["mean"].double().abs()).median()) < 1e-3 else "mixed")
        assert bad.numel() == 0, (case["name"], [(int(i), float(c["x_t"][i]), float(want[i]), float(E[i])) for i in bad[:8]])
    print(f"[measured] learned variance, the ATen chain: largest |x_t - fp64| / E over {len(SC.variance_cases())} cases: {worst:.3f} (k = {SC.EXP_ULPS})")
    assert {"dominates", "vanishes"} <= seen
    assert 0 < worst <= 1.0


# ------------------------------------------------------------------------------------------------ 4. the non-finite counts of the seeded cases
@pytest.mark.parametrize("n", list(SC.TAILS) + [SC.numel(SC.CAP)])
def test_finite_cases_are_finite_and_planted_ones_hold_exactly_the_planted(n):
    osch = SC.oracle_scheduler()
    ts = SC.timesteps()
    assert ts == M.GaussianNoiseScheduler(**R.published_scheduler_kwargs()).loop_timesteps(SC.STEPS, True)[0]
    d = SC.step_inputs(n)
    assert all(SC.nonfinite_counts(v) == (0, 0) for v in d.values())
    if n <= 1023:      # the solver-step inputs of the same sizes ("c"), the saturated-uniform shape ("sat") and the refusals' arguments ("h")
        others = [SC.step_inputs(n, "c"), SC.step_inputs(8 * 4 * 1024, "sat"), SC.step_inputs(64, "h")]
        assert all(SC.nonfinite_counts(v) == (0, 0) for o in others for v in o.values())
    for objective, clip, cfg in SC.STEP_CONFIGS:
        for row, i in SC.STEP_ROWS.items():
            c = SC.chain32(osch, ts, i, True, d["x_t"], d["pred"], d["pu"] if cfg else None, SC.G, objective, bool(clip), d["npost"], d["nddim"])
            for k in ("x_t", "x0", "xT"):
                assert SC.nonfinite_counts(c[k]) == (0, 0), (n, objective, clip, cfg, row, k)
            if n != 1023:
                continue
            planted = SC.plant_nonfinite(d["pred"])
            assert SC.nonfinite_counts(planted) == (1, 2) and bool(torch.isnan(planted[1020])) and 1020 == 4 * (1023 // 4)      # the scalar tail
            c = SC.chain32(osch, ts, i, True, d["x_t"], planted, d["pu"] if cfg else None, SC.G, objective, True, d["npost"], d["nddim"])
            want = SC.planted_counts(objective, row)
            for k in ("x_t", "x0", "xT"):
                assert SC.nonfinite_counts(c[k]) == want[k], (objective, cfg, row, k)
                assert bool(torch.isnan(c[k][1020])) and SC.nonfinite_counts(c[k][:1020]) == (0, 0)
