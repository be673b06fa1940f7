// sched_noise.hip -- fused scheduler step (CFG combine + x0/xT algebra + posterior sample + DDIM update) and
// counter-based Gaussian noise.  Pure streaming kernels over [B, C, h, w] latents (8192 floats per sample).
#include "common.h"
#include "philox.h"

using namespace mf;

namespace {

// Every product/sum is rounded on its own so that, given identical inputs, the result is bit-identical to
// ATen's chain of elementwise ops on CPU.  The library is built with -ffp-contract=off (on AMD the __f*_rn
// intrinsics are plain operators and would otherwise be fused into FMAs); the pragma restates it locally.
struct SchedOut { float xn, x0, xT; };

// the front half of a step, shared by the stochastic step (sched_elem) and the deterministic solver step (solver_elem): classifier-free
// guidance combine, then the x_0 / x_T estimates by objective
struct Estimate { float x0, xT; };
__device__ __forceinline__ Estimate estimate_elem(bool cfg, float g, int objective, int clip_x0, float sqrt_recip_ac, float sqrt_recipm1_ac, float xt, float pred,
                                                  float pu) {
#pragma clang fp contract(off)
  if (cfg) {  // diffusion_pipeline.py:244  pred_uncond + g * (pred_cond - pred_uncond)
    const float dlt = pred - pu;
    const float sc = g * dlt;
    pred = pu + sc;
  }
  float x0, xT;
  if (objective == 0) {  // 'x_T': gaussian_scheduler.py:119-124
    const float p1 = sqrt_recip_ac * xt;
    const float p2 = sqrt_recipm1_ac * pred;
    x0 = p1 - p2;
    if (clip_x0) x0 = clamp_keep_nan(x0, -1.0f, 1.0f);
    xT = pred;
  } else {  // 'x_0': diffusion_pipeline.py:264-267, gaussian_scheduler.py:127-131
    x0 = clip_x0 ? clamp_keep_nan(pred, -1.0f, 1.0f) : pred;
    const float p1 = sqrt_recip_ac * xt;
    const float df = p1 - x0;
    xT = df / sqrt_recipm1_ac;
  }
  return Estimate{x0, xT};
}

// one element of the step: every product / sum rounded on its own (see above)
__device__ __forceinline__ SchedOut sched_elem(const MfSchedArgs& a, const MfSchedStep& S, float xt, float pred, float pu, float pv, float npost, float nddim) {
#pragma clang fp contract(off)
  const Estimate e = estimate_elem(a.pred_uncond != nullptr, a.guidance_scale, a.objective, a.clip_x0, S.sqrt_recip_ac, S.sqrt_recipm1_ac, xt, pred, pu);
  const float x0 = e.x0, xT = e.xT;
  // posterior mean / std: gaussian_scheduler.py:95-100
  const float m1 = S.coef1 * x0;
  const float m2 = S.coef2 * xt;
  const float mean = m1 + m2;
  float sd = S.std_fixed;
  if (a.pred_var) {  // learned variance: var_scale = pred_var/2 + 0.5 (diffusion_pipeline.py:256), :110-116
    const float hv = pv / 2.0f;
    const float vs = hv + 0.5f;
    const float l1 = vs * S.log_var_max;
    const float om = 1.0f - vs;
    const float l2 = om * S.log_var_min;
    const float lv = l1 + l2;
    const float hl = 0.5f * lv;
    sd = S.t == 0 ? 0.0f : expf(hl);
  }
  const float sn = sd * npost;
  const float prior = mean + sn;
  float xn = prior;
  if (S.mode == 1) {  // DDIM: x_0*sqrt(a_next) + c*x_T + sigma*noise  (diffusion_pipeline.py:304)
    const float d1 = x0 * S.ddim_sqrt_an;
    const float d2 = S.ddim_c * xT;
    const float d3 = S.ddim_sigma * nddim;
    const float d12 = d1 + d2;
    xn = d12 + d3;
  }
  return SchedOut{xn, x0, xT};
}

// Inpainting (MfSchedBlend): the kept cells of the next latent take the known latent at the next timestep, a * z0 + c * eps0 with the two
// products rounded separately (rows_axpby_kernel's chain), (a, c) = coef[step].  BL == false compiles the select away.
struct BlendCoef { float a, c; };
__device__ __forceinline__ BlendCoef blend_coef(const MfSchedBlend& bl, int step) { return BlendCoef{bl.coef[2 * step], bl.coef[2 * step + 1]}; }
__device__ __forceinline__ float blend_elem(float xn, float z0, float e0, bool regen, BlendCoef k) {
#pragma clang fp contract(off)
  const float p1 = k.a * z0;
  const float p2 = k.c * e0;
  const float kn = p1 + p2;
  return regen ? xn : kn;
}

template <bool BL>
__global__ __launch_bounds__(256) void sched_step_kernel(const MfSchedArgs a, const MfSchedBlend bl) {
#pragma clang fp contract(off)
  const int step = a.step_dev ? *a.step_dev : a.step;
  const MfSchedStep S = a.table[step];
  const float* npost = a.noise_post ? a.noise_post + (long)step * a.noise_step_stride : nullptr;
  const float* nddim = a.noise_ddim ? a.noise_ddim + (long)step * a.noise_step_stride : nullptr;
  const BlendCoef k = BL ? blend_coef(bl, step) : BlendCoef{0.f, 0.f};
  const long per = BL ? bl.cells * bl.channels : 1;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    SchedOut o = sched_elem(a, S, a.x_t[i], a.pred[i], a.pred_uncond ? a.pred_uncond[i] : 0.f, a.pred_var ? a.pred_var[i] : 0.f, npost ? npost[i] : 0.0f,
                            nddim ? nddim[i] : 0.0f);
    if (BL) {
      const long b = i / per;
      const long cell = (i - b * per) % bl.cells;
      o.xn = blend_elem(o.xn, bl.z0[i], bl.eps0[i], bl.mask[b * bl.cells + cell] != 0, k);
    }
    a.x_t_out[i] = o.xn;
    if (a.x0_out) a.x0_out[i] = o.x0;
    if (a.xT_out) a.xT_out[i] = o.xT;
  }
}

// out[b][0..row_len) = table[(step * ncol + cols[b]) * row_len ...): the rows of loop iteration `step` (device counter or host value) of a
// [S][ncol][row_len] table, one table column per batch row.  float4 when row_len % 4 == 0.
__global__ __launch_bounds__(256) void gather_step_rows_kernel(const float* __restrict__ table, const long* __restrict__ cols,
                                                               const int* __restrict__ step_dev, int step, int ncol, long row_len,
                                                               float* __restrict__ out, long total) {
  const long st = step_dev ? (long)*step_dev : (long)step;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / row_len, k = i - b * row_len;
    out[i] = table[((st * ncol) + cols[b]) * row_len + k];
  }
}

__global__ void broadcast_from_table_kernel(const float* __restrict__ table, const int32_t* __restrict__ step_dev, int step, float* __restrict__ out, int n) {
  const int st = step_dev ? *step_dev : step;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = table[st];
}

__global__ void counter_add_kernel(int32_t* c, int32_t inc) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *c += inc;
}

// out[n][cell] = (1 / C) * sum_c |a[n][c][cell] - b[n][c][cell]|, channels summed in index order: the change map of an edit
__global__ __launch_bounds__(256) void absdiff_mean_c_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, long total, int C,
                                                             long cells) {
#pragma clang fp contract(off)
  const float inv = 1.0f / (float)C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long n = i / cells, cell = i - n * cells;
    const float* pa = a + n * C * cells + cell;
    const float* pb = b + n * C * cells + cell;
    float s = 0.f;
    for (int c = 0; c < C; ++c) s = s + fabsf(pa[c * cells] - pb[c * cells]);
    out[i] = inv * s;
  }
}

// one thread per quad of 4 consecutive elements of one sample
__global__ __launch_bounds__(256) void philox_normal_kernel(float* __restrict__ out, uint32_t seed_lo, uint32_t seed_hi, int draw_base, int draw_stride,
                                                             const int32_t* step_dev, int step, long sample_offset, int B, long quads_per_sample) {
  const int st = step_dev ? *step_dev : step;
  const uint32_t draw = (uint32_t)(draw_base + draw_stride * st);
  const long total = (long)B * quads_per_sample;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long b = i / quads_per_sample;
    const long q = i - b * quads_per_sample;
    *reinterpret_cast<float4*>(out + i * 4) = philox_quad((uint32_t)q, (uint32_t)(sample_offset + b), draw, seed_lo, seed_hi);
  }
}

// The tail of a denoise iteration in ONE launch (round 4): both noise draws generated in registers (the Philox quads of
// philox_normal_kernel: draw_base + draw_stride * step is the posterior draw, + 1 the DDIM draw), the scheduler step of sched_step_kernel
// on them (sched_elem: the same arithmetic, bit for bit), and the step counter advanced by whichever workgroup finishes LAST (a ticket:
// every workgroup has read the counter before it takes its ticket) -- four launches of the loop body become one.
struct PhiloxP { uint32_t seed_lo, seed_hi; int draw_base, draw_stride; long sample_offset, quads_per_sample; int32_t* step_rw; uint32_t* ticket; };

template <bool BL>
__global__ __launch_bounds__(256) void sched_step_philox_kernel(const MfSchedArgs a, const PhiloxP ph, const MfSchedBlend bl) {
#pragma clang fp contract(off)
  const int step = *ph.step_rw;
  const MfSchedStep S = a.table[step];
  const BlendCoef k = BL ? blend_coef(bl, step) : BlendCoef{0.f, 0.f};
  const uint32_t draw = (uint32_t)(ph.draw_base + ph.draw_stride * step);
  const bool ddim = S.mode == 1;
  const long total = a.n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long b = i / ph.quads_per_sample;
    const long q = i - b * ph.quads_per_sample;
    const float4 np = philox_quad((uint32_t)q, (uint32_t)(ph.sample_offset + b), draw, ph.seed_lo, ph.seed_hi);
    const float4 nd = ddim ? philox_quad((uint32_t)q, (uint32_t)(ph.sample_offset + b), draw + 1u, ph.seed_lo, ph.seed_hi) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 xt = *reinterpret_cast<const float4*>(a.x_t + i * 4), pr = *reinterpret_cast<const float4*>(a.pred + i * 4);
    const float4 pu = a.pred_uncond ? *reinterpret_cast<const float4*>(a.pred_uncond + i * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 pv = a.pred_var ? *reinterpret_cast<const float4*>(a.pred_var + i * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    const SchedOut o0 = sched_elem(a, S, xt.x, pr.x, pu.x, pv.x, np.x, nd.x), o1 = sched_elem(a, S, xt.y, pr.y, pu.y, pv.y, np.y, nd.y);
    const SchedOut o2 = sched_elem(a, S, xt.z, pr.z, pu.z, pv.z, np.z, nd.z), o3 = sched_elem(a, S, xt.w, pr.w, pu.w, pv.w, np.w, nd.w);
    float4 xn = make_float4(o0.xn, o1.xn, o2.xn, o3.xn);
    if (BL) {   // (cells % 4 == 0: a quad lies inside one channel plane, its four cells are consecutive mask bytes)
      const float4 z = *reinterpret_cast<const float4*>(bl.z0 + i * 4), e = *reinterpret_cast<const float4*>(bl.eps0 + i * 4);
      const long cell = (q * 4) % bl.cells;
      const uchar4 m = *reinterpret_cast<const uchar4*>(bl.mask + b * bl.cells + cell);
      xn = make_float4(blend_elem(xn.x, z.x, e.x, m.x != 0, k), blend_elem(xn.y, z.y, e.y, m.y != 0, k), blend_elem(xn.z, z.z, e.z, m.z != 0, k),
                       blend_elem(xn.w, z.w, e.w, m.w != 0, k));
    }
    *reinterpret_cast<float4*>(a.x_t_out + i * 4) = xn;
    if (a.x0_out) *reinterpret_cast<float4*>(a.x0_out + i * 4) = make_float4(o0.x0, o1.x0, o2.x0, o3.x0);
    if (a.xT_out) *reinterpret_cast<float4*>(a.xT_out + i * 4) = make_float4(o0.xT, o1.xT, o2.xT, o3.xT);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned old = __hip_atomic_fetch_add(ph.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old + 1u == gridDim.x) {   // the last workgroup: every other one has read *step_rw (before its own ticket)
      __hip_atomic_store(ph.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ph.step_rw, step + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The deterministic solver step (DDIM eta = 0, DPM-Solver++(2M)): estimate_elem's front half, then one row of MfSolverStep.  No noise, so no
// Philox; the x_0 history of the second-order rows lives in a caller-owned [2][n] buffer whose slots alternate with the step's parity.  One
// pass of 16-byte vectors over the first `nq` quads, the remaining n - 4 nq elements one by one (nq = 0: unaligned tensors, or a blend whose
// cells are not a multiple of 4).  a.step_counter != NULL: the counter is the step and is advanced by the workgroup that finishes last
// (sched_step_philox_kernel's ticket).
__device__ __forceinline__ float solver_elem(const MfSolverStep& S, float xt, Estimate e, float x0_prev) {
#pragma clang fp contract(off)
  if (S.mode == MF_SOLVER_DDIM0) {  // diffusion_pipeline.py:304 with sigma = 0: x_0 * sqrt(a_next) + c * x_T
    const float d1 = e.x0 * S.B;
    const float d2 = S.A * e.xT;
    return d1 + d2;
  }
  if (S.mode == MF_SOLVER_FINAL) return e.x0;
  const float p1 = S.A * xt;
  const float p2 = S.B * e.x0;
  const float s12 = p1 + p2;
  if (S.mode == MF_SOLVER_ORDER1) return s12;
  const float p3 = S.C * x0_prev;
  return s12 + p3;
}

// The trajectory of an inversion (MfSolverTraj): slot = slot0 + slot_stride * step of a caller-owned [slots][n] buffer.  TR == MF_TRAJ_RECORD + 1:
// the slot receives what x_t_out receives; TR == MF_TRAJ_KEEP + 1: the kept cells of x_t_out take the slot's values.  A slot outside [0, slots)
// (only a device-resolved step can get here: the host refuses one it knows) is never touched: nothing is recorded, the kept cells say so (NaN).
// TR == 0 compiles all of it away.
template <bool BL, int TR>
__global__ __launch_bounds__(256) void solver_step_kernel(const MfSolverArgs a, const MfSchedBlend bl, const MfSolverTraj tr, const long nq) {
#pragma clang fp contract(off)
  const int step = a.step_counter ? *a.step_counter : a.step_dev ? *a.step_dev : a.step;
  const MfSolverStep S = a.table[step];
  const long slot = TR ? (long)tr.slot0 + (long)tr.slot_stride * step : 0;
  float* const tj = (TR && slot >= 0 && slot < tr.slots) ? tr.traj + slot * a.n : nullptr;
  const long tper = TR == 2 ? tr.cells * tr.channels : 1;
  const float lost = __builtin_nanf("");
  const BlendCoef k = BL ? blend_coef(bl, step) : BlendCoef{0.f, 0.f};
  const bool cfg = a.pred_uncond != nullptr;
  // a second-order row without a history buffer cannot be computed: the output says so (NaN) instead of reading through a null pointer
  const bool hist = S.mode == MF_SOLVER_ORDER2 && a.x0_hist;
  const float missing = (S.mode == MF_SOLVER_ORDER2 && !a.x0_hist) ? __builtin_nanf("") : 0.f;
  const float* hprev = a.x0_hist ? a.x0_hist + (long)((step + 1) & 1) * a.n : nullptr;
  float* hcur = a.x0_hist ? a.x0_hist + (long)(step & 1) * a.n : nullptr;
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = BL ? bl.cells * bl.channels : 1;
  for (long i = tid; i < nq; i += stride) {
    const float4 xt = *reinterpret_cast<const float4*>(a.x_t + i * 4), pr = *reinterpret_cast<const float4*>(a.pred + i * 4);
    const float4 pu = cfg ? *reinterpret_cast<const float4*>(a.pred_uncond + i * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 hp = hist ? *reinterpret_cast<const float4*>(hprev + i * 4) : make_float4(missing, missing, missing, missing);
    const Estimate e0 = estimate_elem(cfg, a.guidance_scale, a.objective, a.clip_x0, S.sqrt_recip_ac, S.sqrt_recipm1_ac, xt.x, pr.x, pu.x);
    const Estimate e1 = estimate_elem(cfg, a.guidance_scale, a.objective, a.clip_x0, S.sqrt_recip_ac, S.sqrt_recipm1_ac, xt.y, pr.y, pu.y);
    const Estimate e2 = estimate_elem(cfg, a.guidance_scale, a.objective, a.clip_x0, S.sqrt_recip_ac, S.sqrt_recipm1_ac, xt.z, pr.z, pu.z);
    const Estimate e3 = estimate_elem(cfg, a.guidance_scale, a.objective, a.clip_x0, S.sqrt_recip_ac, S.sqrt_recipm1_ac, xt.w, pr.w, pu.w);
    float4 xn = make_float4(solver_elem(S, xt.x, e0, hp.x), solver_elem(S, xt.y, e1, hp.y), solver_elem(S, xt.z, e2, hp.z), solver_elem(S, xt.w, e3, hp.w));
    if (BL) {   // (cells % 4 == 0 here: a quad lies inside one channel plane, its four cells are consecutive mask bytes)
      const float4 z = *reinterpret_cast<const float4*>(bl.z0 + i * 4), e = *reinterpret_cast<const float4*>(bl.eps0 + i * 4);
      const long b = (i * 4) / per;
      const long cell = (i * 4 - b * per) % bl.cells;
      const uchar4 m = *reinterpret_cast<const uchar4*>(bl.mask + b * bl.cells + cell);
      xn = make_float4(blend_elem(xn.x, z.x, e.x, m.x != 0, k), blend_elem(xn.y, z.y, e.y, m.y != 0, k), blend_elem(xn.z, z.z, e.z, m.z != 0, k),
                       blend_elem(xn.w, z.w, e.w, m.w != 0, k));
    }
    if (TR == 2) {   // (cells % 4 == 0 here, as for the blend)
      const float4 kp = tj ? *reinterpret_cast<const float4*>(tj + i * 4) : make_float4(lost, lost, lost, lost);
      const long b = (i * 4) / tper;
      const long cell = (i * 4 - b * tper) % tr.cells;
      const uchar4 m = *reinterpret_cast<const uchar4*>(tr.mask + b * tr.cells + cell);
      xn = make_float4(m.x ? xn.x : kp.x, m.y ? xn.y : kp.y, m.z ? xn.z : kp.z, m.w ? xn.w : kp.w);
    }
    const float4 x0v = make_float4(e0.x0, e1.x0, e2.x0, e3.x0);
    *reinterpret_cast<float4*>(a.x_t_out + i * 4) = xn;
    if (TR == 1 && tj) *reinterpret_cast<float4*>(tj + i * 4) = xn;
    if (hcur) *reinterpret_cast<float4*>(hcur + i * 4) = x0v;
    if (a.x0_out) *reinterpret_cast<float4*>(a.x0_out + i * 4) = x0v;
    if (a.xT_out) *reinterpret_cast<float4*>(a.xT_out + i * 4) = make_float4(e0.xT, e1.xT, e2.xT, e3.xT);
  }
  for (long i = nq * 4 + tid; i < a.n; i += stride) {
    const Estimate e = estimate_elem(cfg, a.guidance_scale, a.objective, a.clip_x0, S.sqrt_recip_ac, S.sqrt_recipm1_ac, a.x_t[i], a.pred[i], cfg ? a.pred_uncond[i] : 0.f);
    float xn = solver_elem(S, a.x_t[i], e, hist ? hprev[i] : missing);
    if (BL) {
      const long b = i / per;
      const long cell = (i - b * per) % bl.cells;
      xn = blend_elem(xn, bl.z0[i], bl.eps0[i], bl.mask[b * bl.cells + cell] != 0, k);
    }
    if (TR == 2) {
      const long b = i / tper;
      const long cell = (i - b * tper) % tr.cells;
      if (tr.mask[b * tr.cells + cell] == 0) xn = tj ? tj[i] : lost;
    }
    a.x_t_out[i] = xn;
    if (TR == 1 && tj) tj[i] = xn;
    if (hcur) hcur[i] = e.x0;
    if (a.x0_out) a.x0_out[i] = e.x0;
    if (a.xT_out) a.xT_out[i] = e.xT;
  }
  if (a.step_counter) {
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned old = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old + 1u == gridDim.x) {   // the last workgroup: every other one has read *step_counter (before its own ticket)
        __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.step_counter, step + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// The stochastic solver step (DDIM eta = 1 on any grid, SDE-DPM-Solver++(2M)): solver_step_kernel's front half and deterministic back half, then
// x_t_out = det + scale[step] * eps with the product rounded on its own.  eps is a caller-supplied draw (slot step * eps_step_stride of a bank) or,
// PH, the Philox quad of philox_normal_kernel for draw = draw_base + draw_stride * step, generated in registers (then nq == n / 4: the host refuses
// anything else).  An MF_SOLVER_FINAL row draws nothing and adds nothing.  No trajectory.
struct SolverNoiseP { const float* scale; const float* eps; long eps_step_stride; uint32_t seed_lo, seed_hi; int draw_base, draw_stride; long sample_offset, quads_per_sample; };

__device__ __forceinline__ float noise_elem(float det, float sc, float eps) {
#pragma clang fp contract(off)
  const float p = sc * eps;
  return det + p;
}

template <bool BL, bool PH>
__global__ __launch_bounds__(256) void solver_step_noise_kernel(const MfSolverArgs a, const MfSchedBlend bl, const SolverNoiseP nz, const long nq) {
#pragma clang fp contract(off)
  const int step = a.step_counter ? *a.step_counter : a.step_dev ? *a.step_dev : a.step;
  const MfSolverStep S = a.table[step];
  const bool draws = S.mode != MF_SOLVER_FINAL;
  const float sc = draws ? nz.scale[step] : 0.f;
  const uint32_t draw = (uint32_t)(nz.draw_base + nz.draw_stride * step);
  const float* eps = (!PH && draws) ? nz.eps + (long)step * nz.eps_step_stride : nullptr;
  const BlendCoef k = BL ? blend_coef(bl, step) : BlendCoef{0.f, 0.f};
  const bool cfg = a.pred_uncond != nullptr;
  const bool hist = S.mode == MF_SOLVER_ORDER2 && a.x0_hist;
  const float missing = (S.mode == MF_SOLVER_ORDER2 && !a.x0_hist) ? __builtin_nanf("") : 0.f;
  const float* hprev = a.x0_hist ? a.x0_hist + (long)((step + 1) & 1) * a.n : nullptr;
  float* hcur = a.x0_hist ? a.x0_hist + (long)(step & 1) * a.n : nullptr;
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = BL ? bl.cells * bl.channels : 1;
  for (long i = tid; i < nq; i += stride) {
    const float4 xt = *reinterpret_cast<const float4*>(a.x_t + i * 4), pr = *reinterpret_cast<const float4*>(a.pred + i * 4);
    const float4 pu = cfg ? *reinterpret_cast<const float4*>(a.pred_uncond + i * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 hp = hist ? *reinterpret_cast<const float4*>(hprev + i * 4) : make_float4(missing, missing, missing, missing);
    const Estimate e0 = estimate_elem(cfg, a.guidance_scale, a.objective, a.clip_x0, S.sqrt_recip_ac, S.sqrt_recipm1_ac, xt.x, pr.x, pu.x);
    const Estimate e1 = estimate_elem(cfg, a.guidance_scale, a.objective, a.clip_x0, S.sqrt_recip_ac, S.sqrt_recipm1_ac, xt.y, pr.y, pu.y);
    const Estimate e2 = estimate_elem(cfg, a.guidance_scale, a.objective, a.clip_x0, S.sqrt_recip_ac, S.sqrt_recipm1_ac, xt.z, pr.z, pu.z);
    const Estimate e3 = estimate_elem(cfg, a.guidance_scale, a.objective, a.clip_x0, S.sqrt_recip_ac, S.sqrt_recipm1_ac, xt.w, pr.w, pu.w);
    float4 xn = make_float4(solver_elem(S, xt.x, e0, hp.x), solver_elem(S, xt.y, e1, hp.y), solver_elem(S, xt.z, e2, hp.z), solver_elem(S, xt.w, e3, hp.w));
    if (draws) {
      float4 ep;
      if (PH) {
        const long b = i / nz.quads_per_sample;
        ep = philox_quad((uint32_t)(i - b * nz.quads_per_sample), (uint32_t)(nz.sample_offset + b), draw, nz.seed_lo, nz.seed_hi);
      } else {
        ep = *reinterpret_cast<const float4*>(eps + i * 4);
      }
      xn = make_float4(noise_elem(xn.x, sc, ep.x), noise_elem(xn.y, sc, ep.y), noise_elem(xn.z, sc, ep.z), noise_elem(xn.w, sc, ep.w));
    }
    if (BL) {   // (cells % 4 == 0 here: a quad lies inside one channel plane, its four cells are consecutive mask bytes)
      const float4 z = *reinterpret_cast<const float4*>(bl.z0 + i * 4), e = *reinterpret_cast<const float4*>(bl.eps0 + i * 4);
      const long b = (i * 4) / per;
      const long cell = (i * 4 - b * per) % bl.cells;
      const uchar4 m = *reinterpret_cast<const uchar4*>(bl.mask + b * bl.cells + cell);
      xn = make_float4(blend_elem(xn.x, z.x, e.x, m.x != 0, k), blend_elem(xn.y, z.y, e.y, m.y != 0, k), blend_elem(xn.z, z.z, e.z, m.z != 0, k),
                       blend_elem(xn.w, z.w, e.w, m.w != 0, k));
    }
    const float4 x0v = make_float4(e0.x0, e1.x0, e2.x0, e3.x0);
    *reinterpret_cast<float4*>(a.x_t_out + i * 4) = xn;
    if (hcur) *reinterpret_cast<float4*>(hcur + i * 4) = x0v;
    if (a.x0_out) *reinterpret_cast<float4*>(a.x0_out + i * 4) = x0v;
    if (a.xT_out) *reinterpret_cast<float4*>(a.xT_out + i * 4) = make_float4(e0.xT, e1.xT, e2.xT, e3.xT);
  }
  if (!PH) {   // (the Philox form runs on whole quads only)
    for (long i = nq * 4 + tid; i < a.n; i += stride) {
      const Estimate e = estimate_elem(cfg, a.guidance_scale, a.objective, a.clip_x0, S.sqrt_recip_ac, S.sqrt_recipm1_ac, a.x_t[i], a.pred[i], cfg ? a.pred_uncond[i] : 0.f);
      float xn = solver_elem(S, a.x_t[i], e, hist ? hprev[i] : missing);
      if (draws) xn = noise_elem(xn, sc, eps[i]);
      if (BL) {
        const long b = i / per;
        const long cell = (i - b * per) % bl.cells;
        xn = blend_elem(xn, bl.z0[i], bl.eps0[i], bl.mask[b * bl.cells + cell] != 0, k);
      }
      a.x_t_out[i] = xn;
      if (hcur) hcur[i] = e.x0;
      if (a.x0_out) a.x0_out[i] = e.x0;
      if (a.xT_out) a.xT_out[i] = e.xT;
    }
  }
  if (a.step_counter) {
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned old = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old + 1u == gridDim.x) {   // the last workgroup: every other one has read *step_counter (before its own ticket)
        __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.step_counter, step + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// up to three gathers of the rows of loop iteration `step` in one launch (blockIdx.y = which): gather_step_rows_kernel's work for the
// embedding rows, the local-embedder rows and their bounds, which share `cols` and the step
struct GatherSeg { const float* table; float* out; long row_len; };
__global__ __launch_bounds__(256) void gather_step_rows3_kernel(const GatherSeg g0, const GatherSeg g1, const GatherSeg g2, const long* __restrict__ cols,
                                                                const int* __restrict__ step_dev, int step, int ncol, int B) {
  const GatherSeg g = blockIdx.y == 0 ? g0 : blockIdx.y == 1 ? g1 : g2;
  const long st = step_dev ? (long)*step_dev : (long)step;
  const long total = (long)B * g.row_len;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / g.row_len, k = i - b * g.row_len;
    g.out[i] = g.table[((st * ncol) + cols[b]) * g.row_len + k];
  }
}

// ---- host side of the two step launches: one body each for the plain and the blended entry point
const MfSchedBlend kNoBlend = {nullptr, nullptr, nullptr, nullptr, 0, 0, 0};

// the blend state against the step's element count: every sample is `channels` planes of `cells` values
int check_blend(const MfSchedArgs* a, const MfSchedBlend* bl, const char* who) {
  MF_REQUIRE(bl && bl->z0 && bl->eps0 && bl->mask && bl->coef && bl->cells > 0 && bl->channels > 0, MF_EINVAL, "%s: bad blend state", who);
  MF_REQUIRE(a->n % (bl->cells * (int64_t)bl->channels) == 0, MF_EINVAL, "%s: n is not a whole number of samples of channels x cells", who);
  return MF_OK;
}

int sched_step_launch(const MfSchedArgs* a, const MfSchedBlend* bl, void* stream) {
  MF_REQUIRE(a && a->x_t && a->pred && a->x_t_out && a->table && a->n > 0, MF_EINVAL, "sched_step: bad args");
  MF_REQUIRE(a->objective == 0 || a->objective == 1, MF_EINVAL, "sched_step: objective");
  MF_REQUIRE(!(a->pred_var && a->pred_uncond), MF_EUNSUPPORTED,
             "sched_step: learned variance with classifier-free guidance is unreachable in the reference (it raises)");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_SCHED, s, (bl ? 15.0 : 12.0) * a->n, 4.0 * a->n * (bl ? 8 : 6));
  long blocks = (a->n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  if (bl) {
    MF_LAUNCH(sched_step_kernel<true>, dim3((int)blocks), dim3(256), 0, s, *a, *bl);
  } else {
    MF_LAUNCH(sched_step_kernel<false>, dim3((int)blocks), dim3(256), 0, s, *a, kNoBlend);
  }
  return check_launch("sched_step");
}

int sched_step_philox_launch(const MfSchedArgs* a, uint64_t seed, int32_t draw_base, int32_t draw_stride, int64_t sample_offset, int B, int32_t* step_counter,
                             uint32_t* ticket, const MfSchedBlend* bl, void* stream) {
  MF_REQUIRE(a && a->x_t && a->pred && a->x_t_out && a->table && a->n > 0 && step_counter && ticket && B > 0, MF_EINVAL, "sched_step_philox: bad args");
  MF_REQUIRE(a->objective == 0 || a->objective == 1, MF_EINVAL, "sched_step_philox: objective");
  MF_REQUIRE(!(a->pred_var && a->pred_uncond), MF_EUNSUPPORTED,
             "sched_step_philox: learned variance with classifier-free guidance is unreachable in the reference (it raises)");
  MF_REQUIRE(!a->noise_post && !a->noise_ddim, MF_EINVAL, "sched_step_philox: the noise is generated inside the launch (noise pointers must be NULL)");
  MF_REQUIRE(a->n % (4L * B) == 0, MF_EUNSUPPORTED, "sched_step_philox: elements per sample must be a multiple of 4");
  const uintptr_t al = (uintptr_t)a->x_t | (uintptr_t)a->pred | (uintptr_t)a->x_t_out | (uintptr_t)a->pred_uncond | (uintptr_t)a->pred_var | (uintptr_t)a->x0_out |
                       (uintptr_t)a->xT_out;
  MF_REQUIRE((al & 15) == 0, MF_EINVAL, "sched_step_philox: tensors must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const long quads = a->n / 4;
  ProfScope ps(MF_FAM_SCHED, s, (bl ? 15.0 : 12.0) * a->n + 200.0 * quads, 4.0 * a->n * (bl ? 6 : 4));
  long blocks = (quads + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  const PhiloxP ph{(uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), draw_base, draw_stride, (long)sample_offset, quads / B, step_counter, ticket};
  if (bl) {
    MF_LAUNCH(sched_step_philox_kernel<true>, dim3((int)blocks), dim3(256), 0, s, *a, ph, *bl);
  } else {
    MF_LAUNCH(sched_step_philox_kernel<false>, dim3((int)blocks), dim3(256), 0, s, *a, ph, kNoBlend);
  }
  return check_launch("sched_step_philox");
}

const MfSolverTraj kNoTraj = {nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0};

// the argument rules every solver step shares; *al_out: the OR of everything that must be 16-byte aligned for the vector path
int solver_args_check(const MfSolverArgs* a, const MfSchedBlend* bl, uintptr_t* al_out) {
  MF_REQUIRE(a && a->x_t && a->pred && a->x_t_out && a->table && a->n > 0, MF_EINVAL, "solver_step: bad args");
  MF_REQUIRE(a->objective == 0 || a->objective == 1, MF_EINVAL, "solver_step: objective");
  MF_REQUIRE(!a->step_counter == !a->ticket, MF_EINVAL, "solver_step: step_counter and ticket come together");
  MF_REQUIRE(a->step_counter || a->step_dev || a->step >= 0, MF_EINVAL, "solver_step: step");
  // the history slots must not overlap what the same launch reads or writes elsewhere
  const float* const h0 = a->x0_hist;
  const float* const h1 = h0 ? h0 + 2 * a->n : nullptr;
  const float* const others[] = {a->x_t, a->pred, a->pred_uncond, a->x_t_out, a->x0_out, a->xT_out};
  for (const float* p : others) MF_REQUIRE(!h0 || !p || p + a->n <= h0 || p >= h1, MF_EINVAL, "solver_step: x0_hist overlaps another tensor");
  uintptr_t al = (uintptr_t)a->x_t | (uintptr_t)a->pred | (uintptr_t)a->x_t_out | (uintptr_t)a->pred_uncond | (uintptr_t)a->x0_out | (uintptr_t)a->xT_out |
                 (uintptr_t)a->x0_hist;
  if (a->x0_hist && (a->n & 3)) al |= 4;   // (the second history slot starts n floats in)
  if (bl) al |= (uintptr_t)bl->z0 | (uintptr_t)bl->eps0 | ((uintptr_t)bl->mask & 3 ? 4 : 0) | (bl->cells & 3 ? 4 : 0);
  *al_out = al;
  return MF_OK;
}

int solver_step_launch(const MfSolverArgs* a, const MfSchedBlend* bl, const MfSolverTraj* tr, void* stream) {
  uintptr_t al = 0;
  const int rc = solver_args_check(a, bl, &al);
  if (rc) return rc;
  const float* const h0 = a->x0_hist;
  const float* const h1 = h0 ? h0 + 2 * a->n : nullptr;
  const float* const others[] = {a->x_t, a->pred, a->pred_uncond, a->x_t_out, a->x0_out, a->xT_out};
  if (tr) {
    MF_REQUIRE(!bl, MF_EINVAL, "solver_step_traj: the trajectory and the blend do not combine");
    MF_REQUIRE(tr->traj && tr->slots > 0 && (tr->mode == MF_TRAJ_RECORD || tr->mode == MF_TRAJ_KEEP), MF_EINVAL, "solver_step_traj: bad trajectory state");
    if (tr->mode == MF_TRAJ_KEEP) {
      MF_REQUIRE(tr->mask && tr->cells > 0 && tr->channels > 0, MF_EINVAL, "solver_step_traj: MF_TRAJ_KEEP needs mask, cells and channels");
      MF_REQUIRE(a->n % (tr->cells * (int64_t)tr->channels) == 0, MF_EINVAL, "solver_step_traj: n is not a whole number of samples of channels x cells");
      al |= ((uintptr_t)tr->mask & 3 ? 4 : 0) | (tr->cells & 3 ? 4 : 0);
    }
    if (!a->step_counter && !a->step_dev) {   // a host-known step: its slot is checked here (a device-resolved one inside the launch)
      const int64_t slot = (int64_t)tr->slot0 + (int64_t)tr->slot_stride * a->step;
      MF_REQUIRE(slot >= 0 && slot < tr->slots, MF_EINVAL, "solver_step_traj: slot %lld outside [0, %d)", (long long)slot, tr->slots);
    }
    // the trajectory must not overlap what the same launch reads or writes elsewhere
    const float* const t0 = tr->traj;
    const float* const t1 = t0 + (int64_t)tr->slots * a->n;
    for (const float* p : others) MF_REQUIRE(!p || p + a->n <= t0 || p >= t1, MF_EINVAL, "solver_step_traj: traj overlaps another tensor");
    MF_REQUIRE(!h0 || h1 <= t0 || h0 >= t1, MF_EINVAL, "solver_step_traj: traj overlaps x0_hist");
    al |= (uintptr_t)tr->traj | ((a->n & 3) ? 4 : 0);   // (slot s starts s * n floats in)
  }
  const long nq = (al & 15) ? 0 : a->n / 4;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_SCHED, s, (bl ? 12.0 : 9.0) * a->n, 4.0 * a->n * (bl ? 8 : 6));
  long blocks = ((nq ? nq : a->n) + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  if (tr && tr->mode == MF_TRAJ_RECORD) {
    MF_LAUNCH((solver_step_kernel<false, 1>), dim3((int)blocks), dim3(256), 0, s, *a, kNoBlend, *tr, nq);
  } else if (tr) {
    MF_LAUNCH((solver_step_kernel<false, 2>), dim3((int)blocks), dim3(256), 0, s, *a, kNoBlend, *tr, nq);
  } else if (bl) {
    MF_LAUNCH((solver_step_kernel<true, 0>), dim3((int)blocks), dim3(256), 0, s, *a, *bl, kNoTraj, nq);
  } else {
    MF_LAUNCH((solver_step_kernel<false, 0>), dim3((int)blocks), dim3(256), 0, s, *a, kNoBlend, kNoTraj, nq);
  }
  return check_launch(tr ? "solver_step_traj" : "solver_step");
}

int solver_step_noise_launch(const MfSolverArgs* a, const MfSolverNoise* nz, const MfSchedBlend* bl, void* stream) {
  uintptr_t al = 0;
  const int rc = solver_args_check(a, bl, &al);
  if (rc) return rc;
  MF_REQUIRE(nz->scale, MF_EINVAL, "solver_step_noise: the table of noise scales is missing");
  const bool philox = nz->noise == nullptr;
  long qps = 0;
  if (philox) {
    MF_REQUIRE(nz->B > 0 && a->n % nz->B == 0, MF_EINVAL, "solver_step_noise: n is not B whole samples");
    MF_REQUIRE(a->n % (4L * nz->B) == 0, MF_EUNSUPPORTED, "solver_step_noise: elements per sample must be a multiple of 4 for the draw inside the launch");
    MF_REQUIRE((al & 15) == 0, MF_EUNSUPPORTED,
               "solver_step_noise: the draw inside the launch needs 16-byte aligned tensors (with a blend: cells a multiple of 4, a 4-byte aligned mask)");
    qps = a->n / 4 / nz->B;
  } else {
    MF_REQUIRE(nz->noise_step_stride >= 0, MF_EINVAL, "solver_step_noise: noise_step_stride");
    al |= (uintptr_t)nz->noise | (nz->noise_step_stride & 3 ? 4 : 0);
  }
  const long nq = (al & 15) ? 0 : a->n / 4;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_SCHED, s, (bl ? 14.0 : 11.0) * a->n + (philox ? 50.0 * a->n : 0.0), 4.0 * a->n * ((bl ? 8 : 6) + (philox ? 0 : 1)));
  long blocks = ((nq ? nq : a->n) + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  const SolverNoiseP p{nz->scale, nz->noise, (long)nz->noise_step_stride, (uint32_t)(nz->seed & 0xFFFFFFFFu), (uint32_t)(nz->seed >> 32), nz->draw_base, nz->draw_stride,
                       (long)nz->sample_offset, qps};
  if (philox && bl) {
    MF_LAUNCH((solver_step_noise_kernel<true, true>), dim3((int)blocks), dim3(256), 0, s, *a, *bl, p, nq);
  } else if (philox) {
    MF_LAUNCH((solver_step_noise_kernel<false, true>), dim3((int)blocks), dim3(256), 0, s, *a, kNoBlend, p, nq);
  } else if (bl) {
    MF_LAUNCH((solver_step_noise_kernel<true, false>), dim3((int)blocks), dim3(256), 0, s, *a, *bl, p, nq);
  } else {
    MF_LAUNCH((solver_step_noise_kernel<false, false>), dim3((int)blocks), dim3(256), 0, s, *a, kNoBlend, p, nq);
  }
  return check_launch("solver_step_noise");
}

}  // namespace

extern "C" {

int mf_sched_step_f32(const MfSchedArgs* a, void* stream) { return sched_step_launch(a, nullptr, stream); }

int mf_sched_step_blend_f32(const MfSchedArgs* a, const MfSchedBlend* bl, void* stream) {
  MF_REQUIRE(a, MF_EINVAL, "sched_step_blend: bad args");
  const int rc = check_blend(a, bl, "sched_step_blend");
  return rc ? rc : sched_step_launch(a, bl, stream);
}

int mf_sched_step_philox_f32(const MfSchedArgs* a, uint64_t seed, int32_t draw_base, int32_t draw_stride, int64_t sample_offset, int B, int32_t* step_counter,
                             uint32_t* ticket, void* stream) {
  return sched_step_philox_launch(a, seed, draw_base, draw_stride, sample_offset, B, step_counter, ticket, nullptr, stream);
}

int mf_sched_step_philox_blend_f32(const MfSchedArgs* a, uint64_t seed, int32_t draw_base, int32_t draw_stride, int64_t sample_offset, int B,
                                   int32_t* step_counter, uint32_t* ticket, const MfSchedBlend* bl, void* stream) {
  MF_REQUIRE(a, MF_EINVAL, "sched_step_philox_blend: bad args");
  const int rc = check_blend(a, bl, "sched_step_philox_blend");
  if (rc) return rc;
  MF_REQUIRE(bl->cells % 4 == 0, MF_EUNSUPPORTED, "sched_step_philox_blend: cells per sample must be a multiple of 4");
  MF_REQUIRE(B > 0 && a->n == (int64_t)B * bl->cells * bl->channels, MF_EINVAL, "sched_step_philox_blend: n != B x channels x cells");
  MF_REQUIRE((((uintptr_t)bl->z0 | (uintptr_t)bl->eps0) & 15) == 0 && ((uintptr_t)bl->mask & 3) == 0, MF_EINVAL,
             "sched_step_philox_blend: z0 / eps0 must be 16-byte aligned, mask 4-byte aligned");
  return sched_step_philox_launch(a, seed, draw_base, draw_stride, sample_offset, B, step_counter, ticket, bl, stream);
}

int mf_solver_step_f32(const MfSolverArgs* a, void* stream) { return solver_step_launch(a, nullptr, nullptr, stream); }

int mf_solver_step_traj_f32(const MfSolverArgs* a, const MfSolverTraj* tr, void* stream) {
  MF_REQUIRE(a && tr, MF_EINVAL, "solver_step_traj: bad args");
  return solver_step_launch(a, nullptr, tr, stream);
}

int mf_absdiff_mean_c_f32(const float* a, const float* b, float* out, int N, int C, int64_t cells, void* stream) {
  MF_REQUIRE(a && b && out && N > 0 && C > 0 && cells > 0, MF_EINVAL, "absdiff_mean_c: bad args");
  const long total = (long)N * cells;
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  MF_LAUNCH(absdiff_mean_c_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, a, b, out, total, C, (long)cells);
  return check_launch("absdiff_mean_c");
}

int mf_solver_step_blend_f32(const MfSolverArgs* a, const MfSchedBlend* bl, void* stream) {
  MF_REQUIRE(a, MF_EINVAL, "solver_step_blend: bad args");
  MF_REQUIRE(bl && bl->z0 && bl->eps0 && bl->mask && bl->coef && bl->cells > 0 && bl->channels > 0, MF_EINVAL, "solver_step_blend: bad blend state");
  MF_REQUIRE(a->n % (bl->cells * (int64_t)bl->channels) == 0, MF_EINVAL, "solver_step_blend: n is not a whole number of samples of channels x cells");
  return solver_step_launch(a, bl, nullptr, stream);
}

int mf_solver_step_noise_f32(const MfSolverArgs* a, const MfSolverNoise* nz, const MfSchedBlend* bl, void* stream) {
  MF_REQUIRE(a && nz, MF_EINVAL, "solver_step_noise: bad args");
  if (bl) {
    MF_REQUIRE(bl->z0 && bl->eps0 && bl->mask && bl->coef && bl->cells > 0 && bl->channels > 0, MF_EINVAL, "solver_step_noise: bad blend state");
    MF_REQUIRE(a->n % (bl->cells * (int64_t)bl->channels) == 0, MF_EINVAL, "solver_step_noise: n is not a whole number of samples of channels x cells");
  }
  return solver_step_noise_launch(a, nz, bl, stream);
}

int mf_gather_step_rows3_f32(const float* const* tables, const int64_t* row_lens, float* const* outs, int n_tables, const int64_t* cols, const int32_t* step_dev,
                             int32_t step, int ncol, int B, void* stream) {
  MF_REQUIRE(tables && row_lens && outs && cols && n_tables >= 1 && n_tables <= 3 && ncol > 0 && B > 0, MF_EINVAL, "gather_step_rows3: bad args");
  GatherSeg g[3] = {{nullptr, nullptr, 0}, {nullptr, nullptr, 0}, {nullptr, nullptr, 0}};
  long mx = 0;
  for (int i = 0; i < n_tables; ++i) {
    MF_REQUIRE(tables[i] && outs[i] && row_lens[i] > 0, MF_EINVAL, "gather_step_rows3: table %d", i);
    g[i] = GatherSeg{tables[i], outs[i], (long)row_lens[i]};
    if ((long)B * row_lens[i] > mx) mx = (long)B * row_lens[i];
  }
  long blocks = (mx + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  MF_LAUNCH(gather_step_rows3_kernel, dim3((int)blocks, n_tables), dim3(256), 0, (hipStream_t)stream, g[0], g[1], g[2], reinterpret_cast<const long*>(cols), step_dev, step,
            ncol, B);
  return check_launch("gather_step_rows3");
}

int mf_broadcast_from_table_f32(const float* table, const int32_t* step_dev, int32_t step, float* out, int n, void* stream) {
  MF_REQUIRE(table && out && n > 0, MF_EINVAL, "broadcast_from_table: bad args");
  MF_LAUNCH(broadcast_from_table_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, table, step_dev, step, out, n);
  return check_launch("broadcast_from_table");
}

int mf_gather_step_rows_f32(const float* table, const int64_t* cols, const int32_t* step_dev, int32_t step, int ncol, int64_t row_len, float* out,
                            int B, void* stream) {
  MF_REQUIRE(table && cols && out && ncol > 0 && row_len > 0 && B > 0, MF_EINVAL, "gather_step_rows: bad args");
  const long total = (long)B * row_len;
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  MF_LAUNCH(gather_step_rows_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, table, reinterpret_cast<const long*>(cols), step_dev,
                     step, ncol, (long)row_len, out, total);
  return check_launch("gather_step_rows");
}

int mf_counter_add_i32(int32_t* counter, int32_t inc, void* stream) {
  MF_REQUIRE(counter, MF_EINVAL, "counter_add: null");
  MF_LAUNCH(counter_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counter, inc);
  return check_launch("counter_add");
}

int mf_philox_normal_f32(float* out, uint64_t seed, int32_t draw_base, int32_t draw_stride, const int32_t* step_dev, int32_t step,
                         int64_t sample_offset, int B, int64_t per_sample, void* stream) {
  MF_REQUIRE(out && B > 0 && per_sample > 0, MF_EINVAL, "philox_normal: bad args");
  MF_REQUIRE(per_sample % 4 == 0, MF_EUNSUPPORTED, "philox_normal: per_sample must be a multiple of 4");
  MF_REQUIRE(((uintptr_t)out & 15) == 0, MF_EINVAL, "philox_normal: out must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const long quads = per_sample / 4;
  const long total = (long)B * quads;
  ProfScope ps(MF_FAM_NOISE, s, 100.0 * total, 16.0 * total);
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  MF_LAUNCH(philox_normal_kernel, dim3((int)blocks), dim3(256), 0, s, out, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), draw_base,
                     draw_stride, step_dev, step, (long)sample_offset, B, quads);
  return check_launch("philox_normal");
}

}  // extern "C"
