"""The step and noise kernels (csrc/sched_noise.hip, csrc/philox.h) without a device: the shapes of tests/test_step_gpu.py with the launch arithmetic
that proves each crosses its grid cap, the host's refusals restated line by line, the seeded inputs (oracle.synth), the fp32 ATen chain of one
scheduler step built from oracle.restate's scheduler, the learned-variance bound, and the table of Philox counters whose uniforms sit at the two
ends of u01.  No constant here comes from a run of the kernels; tests/test_step_cpu.py holds every table to the source and to the numpy spec."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from oracle import restate as R
from oracle import synth as S

SOURCE = Path(__file__).resolve().parents[1] / "medfusion_amd" / "csrc" / "sched_noise.hip"
PHILOX_H = SOURCE.with_name("philox.h")
U = 2.0 ** -24                 # unit roundoff of fp32

# ------------------------------------------------------------------------------------------------ shapes
CAP = (5, 3, 70000)            # n = 1 050 000 = 262 500 quads = 1024 * 256 + 356: a second trip of one whole workgroup and a partial one
CAP_PHILOX = (5, 3, 140000)    # mf_philox_normal_f32: 525 000 quads = 2048 * 256 + 712
CAP_ABSDIFF = (2, 2, 262500)   # mf_absdiff_mean_c_f32: 525 000 output cells
TAILS = (1, 5, 255, 257, 1021, 1022, 1023)     # no multiple of 4: aligned, a body of n // 4 vectors plus a scalar tail; 4 bytes off, scalars only
WG = 256                       # __launch_bounds__(256), dim3(256) of every launch in the file
STEP_CAP, WIDE_CAP = 1024, 2048


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def launch(work: int, cap: int):
    """the host's grid for `work` items under `cap` workgroups, and the trips of the grid-stride loop -> (blocks, trips)"""
    blocks = min(cap, cdiv(work, WG))
    return blocks, cdiv(work, blocks * WG)


def numel(shape) -> int:
    return int(np.prod(shape))


# what each launch counts (its `work`), its cap, and the two source lines that say so: (line, text the line must hold)
LAUNCHES = {
    "sched_step": dict(work=lambda n: n, cap=STEP_CAP, lines=((438, "long blocks = (a->n + 255) / 256;"), (439, "if (blocks > 1024) blocks = 1024;"))),
    "sched_step_philox": dict(work=lambda n: n // 4, cap=STEP_CAP, lines=((462, "long blocks = (quads + 255) / 256;"), (463, "if (blocks > 1024) blocks = 1024;"))),
    "solver_step.vector": dict(work=lambda n: n // 4, cap=STEP_CAP,
                               lines=((523, "long blocks = ((nq ? nq : a->n) + 255) / 256;"), (524, "if (blocks > 1024) blocks = 1024;"))),
    "solver_step.scalar": dict(work=lambda n: n, cap=STEP_CAP, lines=((520, "const long nq = (al & 15) ? 0 : a->n / 4;"), (524, "if (blocks > 1024) blocks = 1024;"))),
    "solver_step_noise.vector": dict(work=lambda n: n // 4, cap=STEP_CAP,
                                     lines=((557, "long blocks = ((nq ? nq : a->n) + 255) / 256;"), (558, "if (blocks > 1024) blocks = 1024;"))),
    "solver_step_noise.scalar": dict(work=lambda n: n, cap=STEP_CAP, lines=((554, "const long nq = (al & 15) ? 0 : a->n / 4;"), (558, "if (blocks > 1024) blocks = 1024;"))),
    "philox_normal": dict(work=lambda n: n // 4, cap=WIDE_CAP, lines=((683, "long blocks = (total + 255) / 256;"), (684, "if (blocks > 2048) blocks = 2048;"))),
    "absdiff_mean_c": dict(work=lambda n: n, cap=WIDE_CAP, lines=((612, "long blocks = (total + 255) / 256;"), (613, "if (blocks > 2048) blocks = 2048;"))),
}
# (launch, its element count, blocks, trips, items of the last trip) as the GPU tests run them: restated by hand, held to `launch` by the CPU test
CAP_RUNS = [
    ("sched_step", numel(CAP), 1024, 5, 1424),
    ("sched_step_philox", numel(CAP), 1024, 2, 356),
    ("solver_step.vector", numel(CAP), 1024, 2, 356),
    ("solver_step.scalar", numel(CAP), 1024, 5, 1424),
    ("solver_step_noise.vector", numel(CAP), 1024, 2, 356),
    ("solver_step_noise.scalar", numel(CAP), 1024, 5, 1424),
    ("philox_normal", numel(CAP_PHILOX), 2048, 2, 712),
    ("absdiff_mean_c", CAP_ABSDIFF[0] * CAP_ABSDIFF[2], 2048, 2, 712),
]
# the ticket every workgroup takes (csrc/sched_noise.hip:203, :308, :399): the launch is over when `old + 1u == gridDim.x`
TICKET_LINES = (203, 308, 399)
TICKET_TEXT = "if (old + 1u == gridDim.x) {"

# ------------------------------------------------------------------------------------------------ what the entries refuse before any launch
EINVAL, EUNSUPPORTED = -1, -2       # include/medfusion_hip.h:34
# rule -> (line of csrc/sched_noise.hip, text the line must hold, error code, fragment of the message)
REFUSALS = {
    "sched_step.objective": (433, 'MF_REQUIRE(a->objective == 0 || a->objective == 1, MF_EINVAL, "sched_step: objective");', EINVAL, "sched_step: objective"),
    "sched_step.var_with_pair": (434, "MF_REQUIRE(!(a->pred_var && a->pred_uncond), MF_EUNSUPPORTED,", EUNSUPPORTED, "sched_step: learned variance with classifier-free guidance"),
    "blend.state": (426, 'MF_EINVAL, "%s: bad blend state", who);', EINVAL, "bad blend state"),
    "blend.samples": (427, 'MF_EINVAL, "%s: n is not a whole number of samples of channels x cells", who);', EINVAL, "n is not a whole number of samples"),
    "philox.objective": (451, 'MF_EINVAL, "sched_step_philox: objective");', EINVAL, "sched_step_philox: objective"),
    "philox.var_with_pair": (452, "MF_REQUIRE(!(a->pred_var && a->pred_uncond), MF_EUNSUPPORTED,", EUNSUPPORTED, "sched_step_philox: learned variance with classifier-free guidance"),
    "philox.noise_pointers": (454, "MF_REQUIRE(!a->noise_post && !a->noise_ddim, MF_EINVAL,", EINVAL, "noise pointers must be NULL"),
    "philox.quads": (455, "MF_REQUIRE(a->n % (4L * B) == 0, MF_EUNSUPPORTED,", EUNSUPPORTED, "sched_step_philox: elements per sample must be a multiple of 4"),
    "philox.aligned": (458, "MF_REQUIRE((al & 15) == 0, MF_EINVAL,", EINVAL, "sched_step_philox: tensors must be 16-byte aligned"),
    "philox_blend.cells": (595, "MF_REQUIRE(bl->cells % 4 == 0, MF_EUNSUPPORTED,", EUNSUPPORTED, "sched_step_philox_blend: cells per sample must be a multiple of 4"),
    "philox_blend.n": (596, "MF_REQUIRE(B > 0 && a->n == (int64_t)B * bl->cells * bl->channels, MF_EINVAL,", EINVAL, "sched_step_philox_blend: n != B x channels x cells"),
    "philox_blend.z0": (597, "MF_REQUIRE((((uintptr_t)bl->z0 | (uintptr_t)bl->eps0) & 15) == 0 && ((uintptr_t)bl->mask & 3) == 0, MF_EINVAL,", EINVAL,
                        "z0 / eps0 must be 16-byte aligned"),
    "solver.objective": (478, 'MF_EINVAL, "solver_step: objective");', EINVAL, "solver_step: objective"),
    "solver.counter_ticket": (479, "MF_REQUIRE(!a->step_counter == !a->ticket, MF_EINVAL,", EINVAL, "step_counter and ticket come together"),
    "solver.step": (480, "MF_REQUIRE(a->step_counter || a->step_dev || a->step >= 0, MF_EINVAL,", EINVAL, "solver_step: step"),
    "solver.hist_overlap": (485, "MF_REQUIRE(!h0 || !p || p + a->n <= h0 || p >= h1, MF_EINVAL,", EINVAL, "x0_hist overlaps another tensor"),
    "solver_blend.state": (620, 'MF_EINVAL, "solver_step_blend: bad blend state");', EINVAL, "solver_step_blend: bad blend state"),
    "solver_blend.samples": (621, "MF_REQUIRE(a->n % (bl->cells * (int64_t)bl->channels) == 0, MF_EINVAL,", EINVAL, "solver_step_blend: n is not a whole number of samples"),
    "noise.scale": (541, "MF_REQUIRE(nz->scale, MF_EINVAL,", EINVAL, "the table of noise scales is missing"),
    "noise.samples": (545, "MF_REQUIRE(nz->B > 0 && a->n % nz->B == 0, MF_EINVAL,", EINVAL, "n is not B whole samples"),
    "noise.stride": (551, "MF_REQUIRE(nz->noise_step_stride >= 0, MF_EINVAL,", EINVAL, "solver_step_noise: noise_step_stride"),
    "normal.per_sample": (677, "MF_REQUIRE(per_sample % 4 == 0, MF_EUNSUPPORTED,", EUNSUPPORTED, "per_sample must be a multiple of 4"),
    "normal.aligned": (678, "MF_REQUIRE(((uintptr_t)out & 15) == 0, MF_EINVAL,", EINVAL, "out must be 16-byte aligned"),
}


# ------------------------------------------------------------------------------------------------ seeded inputs
def rand(name: str, shape, scale: float = 1.0) -> torch.Tensor:
    """unit-variance input named `name` (oracle.synth's counter hash), times `scale`"""
    return S.synth_input("step." + name, shape, scale)


def uniform(name: str, n: int, amp: float) -> torch.Tensor:
    """[n] values in (-amp, amp): the same hash, not rescaled to unit variance"""
    return torch.from_numpy(S.hash_uniform("input:step." + name, n)) * amp


def plant_nonfinite(pred: torch.Tensor) -> torch.Tensor:
    """a NaN, a +Inf and a -Inf in the last three elements: at n = 1023 the partial group behind the last whole vector"""
    out = pred.clone()
    n = out.numel()
    for pos, v in ((n - 3, float("nan")), (n - 2, float("inf")), (n - 1, float("-inf"))):
        out.view(-1)[pos] = v
    return out


def nonfinite_counts(t: torch.Tensor):
    return int(torch.isnan(t).sum()), int(torch.isinf(t).sum())


# ------------------------------------------------------------------------------------------------ the scheduler-step cases
STEPS = 7                      # a 7-iteration loop on the reference's grid: linspace(0, T - 1, 7) (diffusion_pipeline.py:283-287)
G = 3.5
STEP_CONFIGS = [(0, 0, False), (0, 1, True), (1, 1, False), (1, 0, True)]      # (objective, clip_x0, guidance pair): both objectives, clip on and off
STEP_ROWS = {"ddim": 3, "final": 6}                                            # a DDIM row and the last row, which samples the posterior


def timesteps(steps: int = STEPS):
    return [int(v) for v in torch.linspace(0, 999, steps, dtype=torch.long)]


def step_inputs(n: int, tag: str = "a") -> dict:
    """-> x_t, pred, pu, npost, nddim: fp32 [n], finite"""
    d = {k: rand(f"{tag}.{n}.{k}", (n,), 1.3) for k in ("x_t", "pred", "pu")}
    d.update({k: rand(f"{tag}.{n}.{k}", (n,)) for k in ("npost", "nddim")})
    return d


def planted_counts(objective: int, row: str) -> dict:
    """(NaNs, Infs) of each output when `pred` holds plant_nonfinite's three values and clip_x0 is on: the clamp keeps the NaN and takes +-Inf to
    +-1, so x_0 holds the NaN alone; x_T is the prediction itself under the 'x_T' objective (the NaN and both Infs) and is computed from the
    clamped x_0 under 'x_0'; the DDIM update adds c x_T, the posterior mean reads x_0 only"""
    xT = (1, 2) if objective == 0 else (1, 0)
    return dict(x0=(1, 0), xT=xT, x_t=xT if row == "ddim" else (1, 0))


# ------------------------------------------------------------------------------------------------ the fp32 chain of one scheduler step
def oracle_scheduler():
    return R.GaussianNoiseScheduler(**R.published_scheduler_kwargs())


def chain32(osch, ts, i: int, use_ddim: bool, x_t, pred, pu, g: float, objective: int, clip: bool, npost, nddim=None, pv=None) -> dict:
    """Iteration i of the loop over reversed(ts), as the reference runs it, in fp32 ATen operators on the CPU, each rounded on its own -- what
    tests/test_kernels_gpu.py::test_sched_step_bit_exact composes, on flat tensors: the guidance combine (diffusion_pipeline.py:244), the estimates
    (gaussian_scheduler.py:119-131), the posterior sample (:95-116), the DDIM update (diffusion_pipeline.py:297-304) on every iteration but the
    last.  pv: the learned-variance channel, var_scale = pv / 2 + 0.5 (diffusion_pipeline.py:256).
    -> x_t, x0, xT (fp32 [n]) and, for the learned variance, mean and hl = 0.5 * log-variance (the argument of exp)"""
    rev = list(reversed(ts))
    t = torch.full((1,), rev[i], dtype=torch.long)
    x = x_t.reshape(1, -1)
    p = pred if pu is None else pu + g * (pred - pu)
    p = p.reshape(1, -1)
    if objective == 0:
        x0 = osch.estimate_x_0(x, p, t, clip_x0=clip)
        xT = p
    else:
        x0 = p.clamp(-1, 1) if clip else p
        xT = osch.estimate_x_T(x, x_0=p, t=t, clip_x0=clip)
    mean = osch.estimate_mean_t(x, x0, t)
    var_scale = 0 if pv is None else pv.reshape(1, -1) / 2 + 0.5
    hl = 0.5 * osch.estimate_variance_t(t, x.ndim, True, var_scale)
    std = torch.exp(hl)
    std[t == 0] = 0.0
    out = mean + std * npost.reshape(1, -1)
    if use_ddim and i < len(rev) - 1:
        alpha, alpha_next = osch.alphas_cumprod[rev[i]], osch.alphas_cumprod[rev[i + 1]]
        sigma = 1 * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
        c = (1 - alpha_next - sigma ** 2).sqrt()
        out = x0 * alpha_next.sqrt() + c * xT + sigma * nddim.reshape(1, -1)
    flat = lambda v: v.reshape(-1)
    return dict(x_t=flat(out), x0=flat(x0), xT=flat(xT), mean=flat(mean), hl=flat(hl.expand_as(mean)) if pv is not None else None)


def same_bits(got: torch.Tensor, want: torch.Tensor):
    """-> the indices (at most 8) where the two fp32 tensors differ in their bits; a NaN equals a NaN whatever its payload"""
    got, want = got.detach().cpu().contiguous().reshape(-1), want.detach().cpu().contiguous().reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = (got.view(torch.int32) != want.view(torch.int32)) & ~(torch.isnan(got) & torch.isnan(want))
    return bad.nonzero().reshape(-1)[:8].tolist()


# ------------------------------------------------------------------------------------------------ learned variance, element by element
# ulps of the two exp implementations, as published:
#   torch's CPU exp on fp32 is SLEEF's Sleef_expf8_u10 (ATen/cpu/vec/vec256/vec256_float.h: Vectorized<float>::exp); the _u10 suffix is SLEEF's
#   statement of a maximum error of 1.0 ULP (sleef.org, "Single precision functions": Sleef_expf*_u10, error bound 1.0 ULP).  The scalar
#   remainder of a vector loop goes through the same Vectorized code, and glibc's expf, where a build falls back to it, is documented under 1 ULP
#   (the GNU C Library manual, "Known Maximum Errors in Math Functions": expf 1).
#   the device library's expf: the HIP programming guide's table of single-precision device functions ("HIP math API", expf) gives 1 ULP, which
#   is also what ROCm's OCML documents for exp on fp32 without -ffast-math; the library is built with -O3 and no fast-math flag (build.py CFLAGS).
EXP_ULPS_ATEN, EXP_ULPS_DEVICE = 1, 1
EXP_ULPS = max(EXP_ULPS_ATEN, EXP_ULPS_DEVICE)

VAR_T = (0, 1, 5, 999)
VAR_N = (255, 1023)
VAR_PV_AMP = (1.0, 3.0)                          # inside the interpolation range of var_scale = pv / 2 + 0.5, and outside it
VAR_NPOST_SCALE = (2.0 ** -20, 1.0, 2.0 ** 20)   # |sd npost| vanishes against |mean|, is of its order (t = 999), dominates it


def variance_cases():
    return [dict(t=t, n=n, amp=amp, ns=ns, name=f"t{t}-n{n}-pv{amp:g}-npost{ns:g}") for t in VAR_T for n in VAR_N for amp in VAR_PV_AMP for ns in VAR_NPOST_SCALE]


def variance_inputs(case):
    """-> x_t, pred, pv, npost (fp32 [n])"""
    n, tag = case["n"], f"var.{case['n']}"
    return rand(tag + ".xt", (n,)), rand(tag + ".pred", (n,)), uniform(tag + ".pv", n, case["amp"]), rand(tag + ".npost", (n,)) * case["ns"]


def variance_bound(mean32, hl32, npost, t: int):
    """-> (want64, E): want64 = mean32 + exp(hl32) npost in fp64 from the chain's own fp32 mean and exponent (sd = 0 at t = 0, gaussian_scheduler.py
    std[t == 0] = 0); E = 2^-24 (|mean| + (2 + 2k) |sd npost|): one rounding of the product, one of the sum, k ulps (2k half-ulps) of exp"""
    sn = torch.zeros_like(mean32, dtype=torch.float64) if t == 0 else torch.exp(hl32.double()) * npost.double()
    return mean32.double() + sn, U * (mean32.double().abs() + (2 + 2 * EXP_ULPS) * sn.abs())


# ------------------------------------------------------------------------------------------------ Philox at the ends of its uniforms
SEED = (7 << 32) | 123
ONES, ZERO = 0xFFFFFF, 0
# (sample, quad, draw, word, top 24 bits): word 0 / 2 feed the radius of the first / second pair of the quad's normals, word 1 / 3 their angle.
# Top 24 bits all ones: u01 = fl32((2^24 - 1 + 0.5) 2^-24) = 1.0 exactly (philox.h:19), radius sqrt(-2 log 1) = -0; zero: u = 2^-25, the largest
# radius the generator can make, sqrt(50 ln 2) = 5.887.  Found by `search_extremes` below; held to philox4x32_10 by tests/test_step_cpu.py.
EXTREMES = [
    (0, 958, 880, 0, ONES),
    (4, 131, 2528, 2, ONES),
    (0, 453, 1721, 0, ZERO),
    (2, 252, 1932, 2, ZERO),
    (2, 256, 335, 1, ONES),
    (2, 537, 2554, 3, ONES),
]
EXTREME_SAMPLES, EXTREME_PER_SAMPLE = 8, 4096      # the block a GPU test generates per entry: samples 0..7, quads 0..1023 of the entry's draw
PHILOX_TOL = 2e-6                                  # the absolute tolerance of tests/test_kernels_gpu.py::test_philox_normal_matches_spec
U01_LINE = (19, "return ((float)(x >> 8) + 0.5f) * 5.9604644775390625e-08f; }  // 2^-24")
SAMPLE_CAST_LINES = ((158, "(uint32_t)(sample_offset + b)"), (181, "(uint32_t)(ph.sample_offset + b)"), (359, "(uint32_t)(nz.sample_offset + b)"))


def philox_words(sample: int, quad: int, draw: int, seed: int = SEED):
    """the four output words of the counter (quad, sample, draw, 0) under `seed` -> tuple of 4 ints"""
    w = S.philox4x32_10(np.uint32(quad), np.uint32(sample), np.uint32(draw), np.uint32(0), np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))
    return tuple(int(v) for v in w)


def spec_block(draw: int, seed: int = SEED) -> np.ndarray:
    """the numpy spec's [EXTREME_SAMPLES, EXTREME_PER_SAMPLE] block of one draw"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return S.philox_normal(seed, draw, np.arange(EXTREME_SAMPLES), EXTREME_PER_SAMPLE)


def spec_rows(seed: int, draw: int, sample_offset: int, B: int, per_sample: int) -> np.ndarray:
    """the spec with the sample index taken mod 2^32, as the 32-bit counter word holds it"""
    idx = np.array([(sample_offset + b) % (1 << 32) for b in range(B)], dtype=np.uint64).astype(np.uint32)
    return S.philox_normal(seed, draw, idx, per_sample)


def search_extremes(seed: int = SEED, samples: int = 8, quads: int = 1024, draws: int = 8192):
    """Every counter of the searched box one of whose words has its top 24 bits all ones or all zero -> list of (sample, quad, draw, word, top 24
    bits).  About 20 s of numpy; nothing calls it by default (EXTREMES is its output, filtered to one entry per kind)."""
    found = []
    s = np.arange(samples, dtype=np.uint32)[:, None]
    q = np.arange(quads, dtype=np.uint32)[None, :]
    for d in range(draws):
        w = S.philox4x32_10(q, s, np.uint32(d), np.uint32(0), np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))
        for k, x in enumerate(w):
            top = x >> np.uint32(8)
            for val in (ONES, ZERO):
                for si, qi in zip(*np.nonzero(top == np.uint32(val))):
                    found.append((int(si), int(qi), d, k, val))
    return found
