// loss.hip -- the held-out denoising loss on the device (include/medfusion_hip.h, "Held-out denoising loss"): the forward process with a timestep
// per row, and per-row error sums of a prediction against a target that is read, or regenerated from Philox in registers, and average-pooled on the
// fly.  Streaming reductions: every byte is read once, nothing but a few doubles per workgroup is written.  fp64 partial sums in a fixed order, no
// atomics: a row's bits depend on that row's data only -- not on the batch, the row's place in it or the load path (metrics.hip's rule).
#include "common.h"
#include "philox.h"

#include <math.h>

using namespace mf;

namespace {

constexpr int LANES = 256;
constexpr long QUAD_SPAN = 4L * LANES;      // elements the lanes of a workgroup take per pass: lane l the quad l of the pass
constexpr long CHUNK_MIN = 8192;            // elements per partial, at least
constexpr int PARTS_MAX = 256;              // partials per row, at most

// elements one workgroup reduces: 8192, or -- from 2 Mi elements per row on -- what keeps a row at PARTS_MAX partials (a multiple of QUAD_SPAN)
long loss_chunk(long per) {
  if ((per + CHUNK_MIN - 1) / CHUNK_MIN <= PARTS_MAX) return CHUNK_MIN;
  const long c = (per + PARTS_MAX - 1) / PARTS_MAX;
  return (c + QUAD_SPAN - 1) / QUAD_SPAN * QUAD_SPAN;
}
int loss_parts(long per) { const long c = loss_chunk(per); return (int)((per + c - 1) / c); }

// NV running sums of the 256 lanes -> lane 0, through LDS by a fixed tree (lane l += lane l + s, s = 128, 64, ... 1)
template <int NV>
__device__ __forceinline__ void block_tree(double (&v)[NV], double* red) {
  const int l = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NV; ++k) red[k * LANES + l] = v[k];
  __syncthreads();
  for (int s = LANES / 2; s > 0; s >>= 1) {
    if (l < s) {
#pragma unroll
      for (int k = 0; k < NV; ++k) red[k * LANES + l] += red[k * LANES + l + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = red[k * LANES];
}

// one thread per row: its partials in ascending order
__global__ __launch_bounds__(64) void loss_finish_kernel(const double* __restrict__ part, double* __restrict__ out, int B, int parts, int nv) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* q = part + (long)b * parts * nv;
  for (int k = 0; k < nv; ++k) {
    double s = 0.0;
    for (int i = 0; i < parts; ++i) s += q[(long)i * nv + k];
    out[(long)b * nv + k] = s;
  }
}

// ---------------------------------------------------------------------------------------------- the forward process, t per row
__device__ __forceinline__ float diffuse_elem(int t, int T, float a, float c, float x, float e) {
#pragma clang fp contract(off)
  if (t < 0) return x;
  if (t >= T) return e;
  const float p1 = a * x;
  const float p2 = c * e;
  return p1 + p2;
}

// nq: quads the 16-byte pass takes (all of them, or 0); the rest element by element (never with PH: the host refuses)
template <bool PH>
__global__ __launch_bounds__(256) void diffuse_rows_kernel(const MfDiffuseArgs a, const long nq) {
#pragma clang fp contract(off)
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long qps = a.per_row >> 2;
  const uint32_t seed_lo = (uint32_t)(a.seed & 0xFFFFFFFFu), seed_hi = (uint32_t)(a.seed >> 32);
  for (long i = tid; i < nq; i += stride) {
    const long b = i / qps, q = i - b * qps;
    const int t = a.t[b];
    const bool in = t >= 0 && t < a.T;
    const float ca = in ? a.sqrt_ac[t] : 0.f, cc = in ? a.sqrt_1m_ac[t] : 0.f;
    const float4 x = *reinterpret_cast<const float4*>(a.x_0 + i * 4);
    const float4 e = PH ? philox_quad((uint32_t)q, (uint32_t)(a.sample_offset + b), (uint32_t)a.draw, seed_lo, seed_hi) : *reinterpret_cast<const float4*>(a.eps + i * 4);
    *reinterpret_cast<float4*>(a.x_t + i * 4) =
        make_float4(diffuse_elem(t, a.T, ca, cc, x.x, e.x), diffuse_elem(t, a.T, ca, cc, x.y, e.y), diffuse_elem(t, a.T, ca, cc, x.z, e.z), diffuse_elem(t, a.T, ca, cc, x.w, e.w));
    if (PH && a.eps_out) *reinterpret_cast<float4*>(a.eps_out + i * 4) = e;
  }
  if (!PH) {
    const long n = (long)a.B * a.per_row;
    for (long i = nq * 4 + tid; i < n; i += stride) {
      const long b = i / a.per_row;
      const int t = a.t[b];
      const bool in = t >= 0 && t < a.T;
      a.x_t[i] = diffuse_elem(t, a.T, in ? a.sqrt_ac[t] : 0.f, in ? a.sqrt_1m_ac[t] : 0.f, a.x_0[i], a.eps[i]);
    }
  }
}

// ---------------------------------------------------------------------------------------------- |d| and d^2 of a prediction against its target
struct LossGeom {
  long per, tper, chunk;          // elements per row of pred and of the target, elements per partial
  int D, H, W, f, fz, parts;      // pred's extents, the pooling factor (fz: along depth; 1 in 2-D)
  uint32_t seed_lo, seed_hi, draw;
  long sample_offset;
};

// the target under pred element i of a row, pooled: the f^dims block summed in (depth, row, column) order in fp32, then divided.  PH: the block's
// values come from the Philox quads that hold them (a quad is recomputed only when the index leaves it)
template <bool PH>
__device__ __forceinline__ float pooled_target(const float* __restrict__ trow, const LossGeom& g, uint32_t sample, long i) {
#pragma clang fp contract(off)
  const int x = (int)(i % g.W);
  long r = i / g.W;
  const int y = (int)(r % g.H);
  r /= g.H;
  const int z = (int)(r % g.D);
  const long c = r / g.D;
  const long TH = (long)g.H * g.f, TW = (long)g.W * g.f, TD = (long)g.D * g.fz;
  float s = 0.f;
  long have = -1;
  float4 qv = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int dz = 0; dz < g.fz; ++dz)
    for (int dy = 0; dy < g.f; ++dy) {
      const long base = ((c * TD + (long)z * g.fz + dz) * TH + (long)y * g.f + dy) * TW + (long)x * g.f;
      for (int dx = 0; dx < g.f; ++dx) {
        const long e = base + dx;
        float v;
        if (PH) {
          if ((e >> 2) != have) {
            have = e >> 2;
            qv = philox_quad((uint32_t)have, sample, g.draw, g.seed_lo, g.seed_hi);
          }
          const int k = (int)(e & 3);
          v = k == 0 ? qv.x : k == 1 ? qv.y : k == 2 ? qv.z : qv.w;
        } else {
          v = trow[e];
        }
        s = s + v;
      }
    }
  return s / (float)(g.fz * g.f * g.f);
}

// grid (parts, B): workgroup (p, b) reduces elements [p chunk, (p + 1) chunk) of row b; lane l takes the quads l, l + 256, ... of that span.
// V: 16-byte loads of pred and of an un-pooled stored target; else element by element -- the same elements in the same lanes in the same order.
template <bool V, bool PH>
__global__ __launch_bounds__(LANES) void denoise_loss_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, double* __restrict__ part, const LossGeom g) {
#pragma clang fp contract(off)
  __shared__ double red[2 * LANES];
  const int b = blockIdx.y, p = blockIdx.x;
  const float* __restrict__ prow = pred + (long)b * g.per;
  const float* __restrict__ trow = PH ? nullptr : tgt + (long)b * g.tper;
  const uint32_t sample = (uint32_t)(g.sample_offset + b);
  const long start = (long)p * g.chunk;
  const long end = start + g.chunk < g.per ? start + g.chunk : g.per;
  double acc[2] = {0.0, 0.0};
  for (long e = start + 4L * threadIdx.x; e < end; e += QUAD_SPAN) {
    const int n = end - e < 4 ? (int)(end - e) : 4;
    float pv[4] = {0.f, 0.f, 0.f, 0.f}, tv[4] = {0.f, 0.f, 0.f, 0.f};
    if (V) {
      const float4 v = *reinterpret_cast<const float4*>(prow + e);
      pv[0] = v.x, pv[1] = v.y, pv[2] = v.z, pv[3] = v.w;
    } else {
      for (int j = 0; j < n; ++j) pv[j] = prow[e + j];
    }
    if (g.f == 1) {
      if (PH) {   // (per % 4 == 0 here: n == 4)
        const float4 v = philox_quad((uint32_t)(e >> 2), sample, g.draw, g.seed_lo, g.seed_hi);
        tv[0] = v.x, tv[1] = v.y, tv[2] = v.z, tv[3] = v.w;
      } else if (V) {
        const float4 v = *reinterpret_cast<const float4*>(trow + e);
        tv[0] = v.x, tv[1] = v.y, tv[2] = v.z, tv[3] = v.w;
      } else {
        for (int j = 0; j < n; ++j) tv[j] = trow[e + j];
      }
    } else {
      for (int j = 0; j < n; ++j) tv[j] = pooled_target<PH>(trow, g, sample, e + j);
    }
    for (int j = 0; j < n; ++j) {
      const float d = pv[j] - tv[j];
      acc[0] += (double)fabsf(d);
      acc[1] += (double)d * (double)d;
    }
  }
  block_tree<2>(acc, red);
  if (threadIdx.x == 0) {
    double* out = part + ((long)b * g.parts + p) * 2;
    out[0] = acc[0];
    out[1] = acc[1];
  }
}

// ---------------------------------------------------------------------------------------------- the learned-variance terms
// The terms are evaluated in fp64 on the fp32 data -- the inputs, the tables and the two clamp constants as the reference's fp32 run holds them (1e-20f,
// 1e-6f) -- not in the reference's fp32 chain: at t = 0 exp(-pred_logvar) reaches e^46 and log(v) + (x - mu)^2 / v cancels, so one fp32 evaluation
// of an element is only good to ~2e-6 of it, and a row's sum would be one sample of that noise.  The kernel streams 20 bytes per element; the fp64
// exp / log do not show next to them.
struct VarRow { double lmax, lmin, c1, c2, sr, srm1; };

__device__ __forceinline__ void variance_elem(const VarRow& R, int objective, int clip_x0, float x0f, float xtf, float xTf, float predf, float pvf, double (&acc)[3]) {
  const double x0 = x0f, xt = xtf, xT = xTf, pred = predf, pv = pvf;
  const double vs = (pv + 1.0) / 2.0;                                  // (pred_var + 1) / 2
  const double plv = vs * R.lmax + (1.0 - vs) * R.lmin;                // estimate_variance_t(log=True, var_scale)
  const double tlv = R.lmin;                                           // 0 * lmax + (1 - 0) * lmin
  double px0;
  if (objective == 0) {                                                // estimate_x_0(x_t, x_T, t, clip_x0) with the TRUE x_T
    px0 = R.sr * xt - R.srm1 * xT;
    if (clip_x0) px0 = px0 != px0 ? px0 : fmin(fmax(px0, -1.0), 1.0);  // (torch.clamp keeps a NaN)
  } else {
    px0 = pred;
  }
  const double m2 = R.c2 * xt;
  const double pmean = R.c1 * px0 + m2, tmean = R.c1 * x0 + m2;
  // kl_gaussians(true_mean, true_logvar, pred_mean, pred_logvar): 0.5 * (lv2 - lv1 + exp(lv1 - lv2) + (m1 - m2)^2 * exp(-lv2) - 1.0)
  const double dm = tmean - pmean;
  const double kl = 0.5 * (plv - tlv + exp(tlv - plv) + dm * dm * exp(-plv) - 1.0);
  // F.gaussian_nll_loss(pred_x_0, x_0, exp(pred_logvar), reduction='none'): 0.5 * (log(v) + (input - target)^2 / v), v clamped at 1e-6 (as fp32 holds it)
  const double var = fmax(exp(plv), (double)1e-6f);
  const double dx = px0 - x0;
  const double nll = 0.5 * (log(var) + dx * dx / var);
  acc[0] += kl;
  acc[1] += nll;
  acc[2] += vs;
}

template <bool V>
__global__ __launch_bounds__(LANES) void variance_loss_kernel(const MfVarianceLossArgs a, double* __restrict__ part, const long chunk, const int parts) {
#pragma clang fp contract(off)
  __shared__ double red[3 * LANES];
  const int b = blockIdx.y, p = blockIdx.x;
  double* out = part + ((long)b * parts + p) * 3;
  const int t = a.t[b];
  if (t < 0 || t >= a.T) {   // no table row: the row's sums say so, nothing is read
    if (threadIdx.x == 0) out[0] = out[1] = out[2] = (double)NAN;
    return;
  }
  const VarRow R{log((double)fmaxf(a.betas[t], 1e-20f)), log((double)fmaxf(a.posterior_variance[t], 1e-20f)), a.coef1[t], a.coef2[t], a.sqrt_recip_ac[t], a.sqrt_recipm1_ac[t]};
  const long off = (long)b * a.per_row;
  const long start = (long)p * chunk;
  const long end = start + chunk < a.per_row ? start + chunk : a.per_row;
  double acc[3] = {0.0, 0.0, 0.0};
  for (long e = start + 4L * threadIdx.x; e < end; e += QUAD_SPAN) {
    const int n = end - e < 4 ? (int)(end - e) : 4;
    const long i = off + e;
    if (V) {
      const float4 x0 = *reinterpret_cast<const float4*>(a.x_0 + i), xt = *reinterpret_cast<const float4*>(a.x_t + i), xT = *reinterpret_cast<const float4*>(a.x_T + i);
      const float4 pr = *reinterpret_cast<const float4*>(a.pred + i), pv = *reinterpret_cast<const float4*>(a.pred_var + i);
      variance_elem(R, a.objective, a.clip_x0, x0.x, xt.x, xT.x, pr.x, pv.x, acc);
      variance_elem(R, a.objective, a.clip_x0, x0.y, xt.y, xT.y, pr.y, pv.y, acc);
      variance_elem(R, a.objective, a.clip_x0, x0.z, xt.z, xT.z, pr.z, pv.z, acc);
      variance_elem(R, a.objective, a.clip_x0, x0.w, xt.w, xT.w, pr.w, pv.w, acc);
    } else {
      for (int j = 0; j < n; ++j) variance_elem(R, a.objective, a.clip_x0, a.x_0[i + j], a.x_t[i + j], a.x_T[i + j], a.pred[i + j], a.pred_var[i + j], acc);
    }
  }
  block_tree<3>(acc, red);
  if (threadIdx.x == 0) {
    out[0] = acc[0];
    out[1] = acc[1];
    out[2] = acc[2];
  }
}

int finish_launch(const void* workspace, double* out, int B, int64_t per_row, int nv, const char* who, void* stream) {
  MF_REQUIRE(workspace && out && B > 0 && B <= 65535 && per_row > 0, MF_EINVAL, "%s: bad args", who);
  MF_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & 7) == 0, MF_EINVAL, "%s: workspace and out must be 8-byte aligned", who);
  MF_LAUNCH(loss_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const double*>(workspace), out, B, loss_parts((long)per_row), nv);
  return check_launch(who);
}

}  // namespace

extern "C" {

int mf_loss_parts(int64_t per_row) { return per_row > 0 ? loss_parts((long)per_row) : 0; }

size_t mf_loss_workspace_bytes(int B, int64_t per_row, int values) {
  if (B <= 0 || per_row <= 0 || values <= 0) return 0;
  return (size_t)B * (size_t)loss_parts((long)per_row) * (size_t)values * sizeof(double);
}

int mf_diffuse_rows_f32(const MfDiffuseArgs* a, void* stream) {
  MF_REQUIRE(a && a->x_0 && a->x_t && a->t && a->sqrt_ac && a->sqrt_1m_ac && a->B > 0 && a->per_row > 0 && a->T > 0, MF_EINVAL, "diffuse_rows: bad args");
  MF_REQUIRE(a->reserved == 0, MF_EINVAL, "diffuse_rows: reserved must be 0");
  MF_REQUIRE(a->eps || a->sample_offset >= 0, MF_EINVAL, "diffuse_rows: sample_offset");
  MF_REQUIRE(!(a->eps && a->eps_out), MF_EINVAL, "diffuse_rows: eps_out goes with the draw inside the launch (eps must be NULL)");
  const bool philox = a->eps == nullptr;
  const uintptr_t al = (uintptr_t)a->x_0 | (uintptr_t)a->x_t | (uintptr_t)a->eps | (uintptr_t)a->eps_out;
  const bool vec = (al & 15) == 0 && a->per_row % 4 == 0;
  if (philox) {
    MF_REQUIRE(a->per_row % 4 == 0, MF_EUNSUPPORTED, "diffuse_rows: elements per sample must be a multiple of 4 for the draw inside the launch");
    MF_REQUIRE(vec, MF_EUNSUPPORTED, "diffuse_rows: the draw inside the launch needs 16-byte aligned tensors");
    MF_REQUIRE(a->per_row / 4 <= 0xFFFFFFFFL, MF_EUNSUPPORTED, "diffuse_rows: more than 2^32 quads per sample");
  }
  const long n = (long)a->B * a->per_row;
  const long nq = vec ? n / 4 : 0;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_SCHED, s, 3.0 * n + (philox ? 50.0 * n : 0.0), 4.0 * n * (philox ? (a->eps_out ? 3 : 2) : 3));
  long blocks = ((nq ? nq : n) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (philox) {
    MF_LAUNCH(diffuse_rows_kernel<true>, dim3((int)blocks), dim3(256), 0, s, *a, nq);
  } else {
    MF_LAUNCH(diffuse_rows_kernel<false>, dim3((int)blocks), dim3(256), 0, s, *a, nq);
  }
  return check_launch("diffuse_rows");
}

int mf_denoise_loss_f32(const float* pred, const float* target, const MfLossDesc* d, void* workspace, size_t workspace_bytes, void* stream) {
  MF_REQUIRE(pred && d && workspace, MF_EINVAL, "denoise_loss: bad args");
  MF_REQUIRE(d->B > 0 && d->B <= 65535 && d->C > 0 && (d->dims == 2 || d->dims == 3) && d->size[0] > 0 && d->size[1] > 0 && d->size[2] > 0, MF_EINVAL,
             "denoise_loss: bad descriptor");
  MF_REQUIRE(d->dims == 3 || d->size[0] == 1, MF_EINVAL, "denoise_loss: D must be 1 in 2-D");
  MF_REQUIRE(d->f >= 1, MF_EUNSUPPORTED, "denoise_loss: the pooling factor is an integer >= 1");
  const long fz = d->dims == 3 ? d->f : 1;
  const long per = (long)d->C * d->size[0] * d->size[1] * d->size[2];
  const long tper = per * fz * d->f * d->f;
  MF_REQUIRE(((uintptr_t)workspace & 7) == 0, MF_EINVAL, "denoise_loss: workspace must be 8-byte aligned");
  MF_REQUIRE(workspace_bytes >= mf_loss_workspace_bytes(d->B, per, 2), MF_EWORKSPACE, "denoise_loss: workspace of %zu bytes, %zu needed", workspace_bytes,
             mf_loss_workspace_bytes(d->B, per, 2));
  const bool philox = target == nullptr;
  if (philox) {
    MF_REQUIRE(tper % 4 == 0, MF_EUNSUPPORTED, "denoise_loss: the target's elements per sample must be a multiple of 4 to regenerate it");
    MF_REQUIRE(tper / 4 <= 0xFFFFFFFFL && d->sample_offset >= 0, MF_EUNSUPPORTED, "denoise_loss: more than 2^32 quads per sample, or a negative sample_offset");
  }
  const uintptr_t al = (uintptr_t)pred | (d->f == 1 ? (uintptr_t)target : 0);
  const bool vec = (al & 15) == 0 && per % 4 == 0;
  LossGeom g;
  g.per = per, g.tper = tper, g.chunk = loss_chunk(per);
  g.D = d->size[0], g.H = d->size[1], g.W = d->size[2], g.f = d->f, g.fz = (int)fz, g.parts = loss_parts(per);
  g.seed_lo = (uint32_t)(d->seed & 0xFFFFFFFFu), g.seed_hi = (uint32_t)(d->seed >> 32), g.draw = (uint32_t)d->draw;
  g.sample_offset = (long)d->sample_offset;
  hipStream_t s = (hipStream_t)stream;
  const double n = (double)d->B * per, tn = (double)d->B * tper;
  ProfScope ps(MF_FAM_MISC, s, 4.0 * n + tn + (philox ? 50.0 * tn : 0.0), 4.0 * n + (philox ? 0.0 : 4.0 * tn));
  double* part = reinterpret_cast<double*>(workspace);
  const dim3 grid(g.parts, d->B);
  if (philox && vec) {
    MF_LAUNCH((denoise_loss_kernel<true, true>), grid, dim3(LANES), 0, s, pred, target, part, g);
  } else if (philox) {
    MF_LAUNCH((denoise_loss_kernel<false, true>), grid, dim3(LANES), 0, s, pred, target, part, g);
  } else if (vec) {
    MF_LAUNCH((denoise_loss_kernel<true, false>), grid, dim3(LANES), 0, s, pred, target, part, g);
  } else {
    MF_LAUNCH((denoise_loss_kernel<false, false>), grid, dim3(LANES), 0, s, pred, target, part, g);
  }
  return check_launch("denoise_loss");
}

int mf_denoise_loss_finish_f32(const void* workspace, double* out, int B, int64_t per_row, void* stream) {
  return finish_launch(workspace, out, B, per_row, 2, "denoise_loss_finish", stream);
}

int mf_variance_loss_f32(const MfVarianceLossArgs* a, void* workspace, size_t workspace_bytes, void* stream) {
  MF_REQUIRE(a && workspace && a->x_0 && a->x_t && a->x_T && a->pred && a->pred_var && a->t, MF_EINVAL, "variance_loss: bad args");
  MF_REQUIRE(a->betas && a->posterior_variance && a->coef1 && a->coef2 && a->sqrt_recip_ac && a->sqrt_recipm1_ac, MF_EINVAL, "variance_loss: a scheduler table is missing");
  MF_REQUIRE(a->B > 0 && a->B <= 65535 && a->per_row > 0 && a->T > 0, MF_EINVAL, "variance_loss: bad sizes");
  MF_REQUIRE(a->objective == 0 || a->objective == 1, MF_EINVAL, "variance_loss: objective");
  MF_REQUIRE(((uintptr_t)workspace & 7) == 0, MF_EINVAL, "variance_loss: workspace must be 8-byte aligned");
  MF_REQUIRE(workspace_bytes >= mf_loss_workspace_bytes(a->B, a->per_row, 3), MF_EWORKSPACE, "variance_loss: workspace of %zu bytes, %zu needed", workspace_bytes,
             mf_loss_workspace_bytes(a->B, a->per_row, 3));
  const uintptr_t al = (uintptr_t)a->x_0 | (uintptr_t)a->x_t | (uintptr_t)a->x_T | (uintptr_t)a->pred | (uintptr_t)a->pred_var;
  const bool vec = (al & 15) == 0 && a->per_row % 4 == 0;
  hipStream_t s = (hipStream_t)stream;
  const double n = (double)a->B * a->per_row;
  ProfScope ps(MF_FAM_MISC, s, 60.0 * n, 20.0 * n);
  const long chunk = loss_chunk((long)a->per_row);
  const int parts = loss_parts((long)a->per_row);
  double* part = reinterpret_cast<double*>(workspace);
  const dim3 grid(parts, a->B);
  if (vec) {
    MF_LAUNCH(variance_loss_kernel<true>, grid, dim3(LANES), 0, s, *a, part, chunk, parts);
  } else {
    MF_LAUNCH(variance_loss_kernel<false>, grid, dim3(LANES), 0, s, *a, part, chunk, parts);
  }
  return check_launch("variance_loss");
}

int mf_variance_loss_finish_f32(const void* workspace, double* out, int B, int64_t per_row, void* stream) {
  return finish_launch(workspace, out, B, per_row, 3, "variance_loss_finish", stream);
}

}  // extern "C"
