// guide.hip -- the guidance stage of a denoise iteration (include/medfusion_hip.h, "Guidance stage"): the classifier-free combine with a scale per
// executed iteration, guidance rescale (two per-row variances) and dynamic thresholding (an exact per-row order statistic of |x_0|), between the
// estimator and the scheduler / solver step.  Per-row reductions with no host sync: fp64 sums in a fixed order, integer histograms through LDS atomics
// (integer sums do not depend on their order), no floating-point atomics, no global atomics.  A row's bits depend on that row's data and its table
// row only -- not on B, the row's place, the load path or the launch (metrics.hip's rule).
#include "common.h"

#include <math.h>

using namespace mf;

namespace {

constexpr int LANES = 256;
constexpr long QUAD_SPAN = 4L * LANES;                      // elements the lanes of a workgroup take per pass: lane l the quad l of the pass
constexpr int QPL = MF_GUIDE_ROW_ONE_WG / (4 * LANES);      // quads a lane holds in registers on the one-workgroup path
constexpr int PARTS_MAX = 64;                               // workgroups per row on the multi-workgroup path, at most
static_assert(MF_GUIDE_ROW_ONE_WG % (4 * LANES) == 0, "a one-workgroup row is a whole number of passes");

// elements one workgroup of the multi-workgroup path takes: MF_GUIDE_ROW_ONE_WG, or what keeps a row at PARTS_MAX workgroups (a multiple of QUAD_SPAN)
long guide_chunk(long n) {
  if ((n + MF_GUIDE_ROW_ONE_WG - 1) / MF_GUIDE_ROW_ONE_WG <= PARTS_MAX) return MF_GUIDE_ROW_ONE_WG;
  const long c = (n + PARTS_MAX - 1) / PARTS_MAX;
  return (c + QUAD_SPAN - 1) / QUAD_SPAN * QUAD_SPAN;
}
int guide_parts(long n) { const long c = guide_chunk(n); return (int)((n + c - 1) / c); }

// the workspace of the multi-workgroup path: [B][parts][6] fp64 partial sums and their pivots | [2][B][parts][2][256] digit counts | [3][B][4] select state
struct GuideGeom {
  long chunk;
  int parts;
  double* sums;
  unsigned* hist;
  unsigned* state;
};
size_t sums_bytes(int B, int parts) { return (size_t)B * parts * 6 * sizeof(double); }
size_t hist_bytes(int B, int parts) { return (size_t)2 * B * parts * 2 * 256 * sizeof(unsigned); }
size_t state_bytes(int B) { return (size_t)3 * B * 4 * sizeof(unsigned); }

// ---------------------------------------------------------------------------------------------- the arithmetic of one element
// every product / sum rounded on its own: estimate_elem's chains (sched_noise.hip)
__device__ __forceinline__ float combine_elem(bool cfg, float g, float pc, float pu) {
#pragma clang fp contract(off)
  if (!cfg) return pc;
  const float dlt = pc - pu;
  const float sc = g * dlt;
  return pu + sc;
}
__device__ __forceinline__ float x0_elem(int objective, float ra, float rb, float xt, float p) {
#pragma clang fp contract(off)
  if (objective != 0) return p;
  const float p1 = ra * xt;
  const float p2 = rb * p;
  return p1 - p2;
}
// the prediction consistent with a thresholded x_0 estimate
__device__ __forceinline__ float back_elem(int objective, float ra, float rb, float xt, float x0n) {
#pragma clang fp contract(off)
  if (objective != 0) return x0n;
  const float p1 = ra * xt;
  const float df = p1 - x0n;
  return df / rb;
}
__device__ __forceinline__ float threshold_elem(float x0, float s) {
#pragma clang fp contract(off)
  const float c = clamp_keep_nan(x0, -s, s);
  return c / s;
}
__device__ __forceinline__ unsigned abs_key(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }

// acc = (sum dc, sum dc^2, sum dp, sum dp^2) about the row's pivots -> k = fl32(phi sigma_pos / sigma_cfg + (1 - phi)) in fp64
__device__ __forceinline__ float rescale_k(float phi, const double (&acc)[4], long n) {
#pragma clang fp contract(off)
  if (n < 2) return 1.0f;
  const double nn = (double)n;
  double vc = acc[1] - acc[0] * acc[0] / nn;
  double vp = acc[3] - acc[2] * acc[2] / nn;
  if (vc < 0.0) vc = 0.0;
  if (vp < 0.0) vp = 0.0;
  if (vp == 0.0) return 1.0f;
  const double ratio = sqrt(vc) / sqrt(vp);   // (the n - 1 of the two unbiased estimates cancels)
  const double ph = (double)phi;
  return (float)(ph * ratio + (1.0 - ph));
}

// the position of the quantile among the n sorted magnitudes
struct QuantPos { double pos; unsigned lo, hi; };
__device__ __forceinline__ QuantPos quant_pos(float q, long n) {
#pragma clang fp contract(off)
  QuantPos r;
  r.pos = (double)q * (double)(n - 1);
  if (!(r.pos >= 0.0)) r.pos = 0.0;
  if (r.pos > (double)(n - 1)) r.pos = (double)(n - 1);
  r.lo = (unsigned)floor(r.pos);
  r.hi = (unsigned)ceil(r.pos);
  return r;
}
__device__ __forceinline__ float limit_of(const QuantPos& qp, unsigned klo, unsigned khi, float s_max) {
#pragma clang fp contract(off)
  const double vlo = (double)__uint_as_float(klo), vhi = (double)__uint_as_float(khi);
  const double w = qp.pos - (double)qp.lo;
  const double sd = qp.hi == qp.lo ? vlo : vlo + (vhi - vlo) * w;   // torch.quantile's 'linear' rule
  float s = (float)sd;
  s = fmaxf(s, 1.0f);
  if (s_max > 0.0f) s = fminf(s, s_max);
  return s;
}

__device__ __forceinline__ void load4(const float* p, long e, int nv, bool vec, float (&v)[4]) {
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(p + e);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[e + j] : 0.f;
  }
}
__device__ __forceinline__ void store4(float* p, long e, int nv, bool vec, const float (&v)[4]) {
  if (vec) {
    *reinterpret_cast<float4*>(p + e) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nv) p[e + j] = v[j];
  }
}

// NV running sums of the 256 lanes -> every lane, through LDS by a fixed tree (lane l += lane l + s, s = 128, 64, ... 1)
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
  __syncthreads();
}

// One digit of the most-significant-digit-first radix select, for the two ranks (lo, hi) at once.  Lane l holds the counts (h0, h1) of digit l among
// the keys that match the prefix of rank lo / rank hi; an inclusive scan over the 256 digits finds the digit each rank falls into; pre[w] takes the
// digit, r[w] becomes the rank among the keys of that digit.  Integer arithmetic only.
struct SelectLds { uint2 scan[2][LANES]; unsigned sel[4]; };
__device__ __forceinline__ void select_digit(unsigned h0, unsigned h1, int shift, unsigned (&pre)[2], unsigned (&r)[2], SelectLds& S) {
  const int l = threadIdx.x;
  int cur = 0;
  S.scan[0][l] = make_uint2(h0, h1);
  __syncthreads();
  for (int off = 1; off < LANES; off <<= 1) {
    uint2 v = S.scan[cur][l];
    if (l >= off) {
      const uint2 u = S.scan[cur][l - off];
      v.x += u.x, v.y += u.y;
    }
    S.scan[cur ^ 1][l] = v;
    __syncthreads();
    cur ^= 1;
  }
  const uint2 incl = S.scan[cur][l];
  if (incl.x - h0 <= r[0] && r[0] < incl.x) S.sel[0] = (unsigned)l, S.sel[1] = r[0] - (incl.x - h0);
  if (incl.y - h1 <= r[1] && r[1] < incl.y) S.sel[2] = (unsigned)l, S.sel[3] = r[1] - (incl.y - h1);
  __syncthreads();
  pre[0] |= S.sel[0] << shift, r[0] = S.sel[1];
  pre[1] |= S.sel[2] << shift, r[1] = S.sel[3];
  __syncthreads();
}
__device__ __forceinline__ void count_key(unsigned key, int pass, const unsigned (&pre)[2], unsigned (*hist)[LANES]) {
  const int shift = 24 - 8 * pass;
  const unsigned d = (key >> shift) & 255u;
  // (pass 0 counts every key: the top digit has no prefix above it)
  if (pass == 0 || (key >> (shift + 8)) == (pre[0] >> (shift + 8))) atomicAdd(&hist[0][d], 1u);
  if (pass == 0 || (key >> (shift + 8)) == (pre[1] >> (shift + 8))) atomicAdd(&hist[1][d], 1u);
}

// ---------------------------------------------------------------------------------------------- a row that fits one workgroup: ONE launch
// grid (B): lane l holds the quads l, l + 256, ... of the row in registers (QPL of them); combine, the two variances, k, x_0, the select and the
// apply never leave the workgroup.  vec: 16-byte loads and stores; else element by element -- the same elements in the same lanes.
__global__ __launch_bounds__(LANES) void guide_row_kernel(const MfGuideArgs a, const bool vec) {
#pragma clang fp contract(off)
  __shared__ double red[4 * LANES];
  __shared__ unsigned hist[2][LANES];
  __shared__ SelectLds sl;
  const int b = blockIdx.x, l = threadIdx.x;
  const int step = a.step_dev ? *a.step_dev : a.step;
  const MfGuideStep S = a.table[step];
  const long n = a.n, off = (long)b * n;
  const bool cfg = a.pred_uncond != nullptr, rescale = (a.stages & MF_GUIDE_RESCALE) != 0, thr = (a.stages & MF_GUIDE_THRESHOLD) != 0;
  const float* pcr = a.pred + off;                                      // (pred_out may be pred: no __restrict__ on the two)
  const float* __restrict__ pur = cfg ? a.pred_uncond + off : nullptr;
  float p[QPL * 4];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const float piv_c = pcr[0];                                           // the pivots of the two variances: the row's first element
  const float piv_p = combine_elem(cfg, S.g, piv_c, cfg ? pur[0] : 0.f);
#pragma unroll
  for (int j = 0; j < QPL; ++j) {
    const long e = 4L * ((long)j * LANES + l);
    float pc[4] = {0.f, 0.f, 0.f, 0.f}, pu[4] = {0.f, 0.f, 0.f, 0.f};
    const int nv = e >= n ? 0 : (n - e < 4 ? (int)(n - e) : 4);
    if (nv > 0) {
      load4(pcr, e, nv, vec, pc);
      if (cfg) load4(pur, e, nv, vec, pu);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      p[j * 4 + c] = combine_elem(cfg, S.g, pc[c], pu[c]);
      if (rescale && c < nv) {
        const double dc = (double)pc[c] - (double)piv_c, dp = (double)p[j * 4 + c] - (double)piv_p;
        acc[0] += dc, acc[1] += dc * dc, acc[2] += dp, acc[3] += dp * dp;
      }
    }
  }
  float kf = 1.0f;
  if (rescale) {
    block_tree<4>(acc, red);
    kf = rescale_k(S.phi, acc, n);
#pragma unroll
    for (int i = 0; i < QPL * 4; ++i) p[i] = kf * p[i];
  }
  float s = 0.0f;
  if (thr) {
    const float* __restrict__ xtr = a.x_t + off;
    float xt[QPL * 4];
#pragma unroll
    for (int j = 0; j < QPL; ++j) {
      const long e = 4L * ((long)j * LANES + l);
      const int nv = e >= n ? 0 : (n - e < 4 ? (int)(n - e) : 4);
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (nv > 0 && a.objective == 0) load4(xtr, e, nv, vec, v);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        xt[j * 4 + c] = v[c];
        p[j * 4 + c] = x0_elem(a.objective, S.sqrt_recip_ac, S.sqrt_recipm1_ac, v[c], p[j * 4 + c]);   // (p holds the x_0 estimate from here on)
      }
    }
    const QuantPos qp = quant_pos(S.q, n);
    unsigned pre[2] = {0u, 0u}, r[2] = {qp.lo, qp.hi};
    for (int pass = 0; pass < 4; ++pass) {
      hist[0][l] = 0u, hist[1][l] = 0u;
      __syncthreads();
#pragma unroll
      for (int j = 0; j < QPL; ++j) {
        const long e = 4L * ((long)j * LANES + l);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (e + c < n) count_key(abs_key(p[j * 4 + c]), pass, pre, hist);
      }
      __syncthreads();
      select_digit(hist[0][l], hist[1][l], 24 - 8 * pass, pre, r, sl);
    }
    s = limit_of(qp, pre[0], pre[1], S.s_max);
#pragma unroll
    for (int i = 0; i < QPL * 4; ++i) p[i] = back_elem(a.objective, S.sqrt_recip_ac, S.sqrt_recipm1_ac, xt[i], threshold_elem(p[i], s));
  }
  float* outr = a.pred_out + off;
#pragma unroll
  for (int j = 0; j < QPL; ++j) {
    const long e = 4L * ((long)j * LANES + l);
    const int nv = e >= n ? 0 : (n - e < 4 ? (int)(n - e) : 4);
    if (nv > 0) {
      const float v[4] = {p[j * 4], p[j * 4 + 1], p[j * 4 + 2], p[j * 4 + 3]};
      store4(outr, e, nv, vec, v);
    }
  }
  if (l == 0) {
    if (a.scale_out) a.scale_out[b] = kf;
    if (a.limit_out) a.limit_out[b] = s;
  }
}

// ---------------------------------------------------------------------------------------------- longer rows: a fixed sequence of launches
// grid (parts, B) each; workgroup (p, b) takes elements [p chunk, (p + 1) chunk) of row b, lane l the quads l, l + 256, ... of that span.
//   combine:     pred_out = the combined prediction; four fp64 partial sums per workgroup about its own pivots (with rescale);
//   pass 0 .. 3: every workgroup adds the row's partial sums in ascending order (k), resolves the digit the launch before counted, and counts the
//                next digit of |x_0| among the keys that still match: [2][256] counts per workgroup;
//   pass 4:      resolves the last digit -> the limit s, and applies k and s.
// Nothing is zeroed between launches: every word read was written by the launch before, whole.
__global__ __launch_bounds__(LANES) void guide_combine_kernel(const MfGuideArgs a, const GuideGeom g, const bool vec) {
#pragma clang fp contract(off)
  __shared__ double red[4 * LANES];
  const int b = blockIdx.y, part = blockIdx.x;
  const int step = a.step_dev ? *a.step_dev : a.step;
  const MfGuideStep S = a.table[step];
  const long n = a.n, off = (long)b * n;
  const bool cfg = a.pred_uncond != nullptr, rescale = (a.stages & MF_GUIDE_RESCALE) != 0;
  const float* pcr = a.pred + off;                                      // (pred_out may be pred: no __restrict__ on the two)
  const float* __restrict__ pur = cfg ? a.pred_uncond + off : nullptr;
  float* outr = a.pred_out + off;
  const long start = (long)part * g.chunk;
  const long end = start + g.chunk < n ? start + g.chunk : n;
  // the pivots of this workgroup's sums: the first element of its own span (pred_out may be pred: no other workgroup's element is read)
  const float piv_c = pcr[start];
  const float piv_p = combine_elem(cfg, S.g, piv_c, cfg ? pur[start] : 0.f);
  __syncthreads();   // (every lane has the pivots before the element is overwritten)
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (long e = start + 4L * threadIdx.x; e < end; e += QUAD_SPAN) {
    const int nv = end - e < 4 ? (int)(end - e) : 4;
    float pc[4], pu[4] = {0.f, 0.f, 0.f, 0.f}, p[4];
    load4(pcr, e, nv, vec, pc);
    if (cfg) load4(pur, e, nv, vec, pu);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      p[c] = combine_elem(cfg, S.g, pc[c], pu[c]);
      if (rescale && c < nv) {
        const double dc = (double)pc[c] - (double)piv_c, dp = (double)p[c] - (double)piv_p;
        acc[0] += dc, acc[1] += dc * dc, acc[2] += dp, acc[3] += dp * dp;
      }
    }
    store4(outr, e, nv, vec, p);
  }
  if (rescale) {
    block_tree<4>(acc, red);
    if (threadIdx.x == 0) {
      double* o = g.sums + ((long)b * g.parts + part) * 6;
      o[0] = acc[0], o[1] = acc[1], o[2] = acc[2], o[3] = acc[3], o[4] = (double)piv_c, o[5] = (double)piv_p;
    }
  }
  if (threadIdx.x == 0 && part == 0 && a.stages == 0) {
    if (a.scale_out) a.scale_out[b] = 1.0f;
    if (a.limit_out) a.limit_out[b] = 0.0f;
  }
}

__global__ __launch_bounds__(LANES) void guide_pass_kernel(const MfGuideArgs a, const GuideGeom g, const bool vec, const int pass) {
#pragma clang fp contract(off)
  __shared__ unsigned hist[2][LANES];
  __shared__ SelectLds sl;
  __shared__ float k_lds;
  const int b = blockIdx.y, part = blockIdx.x, l = threadIdx.x;
  const int B = gridDim.y;
  const int step = a.step_dev ? *a.step_dev : a.step;
  const MfGuideStep S = a.table[step];
  const long n = a.n, off = (long)b * n;
  const bool rescale = (a.stages & MF_GUIDE_RESCALE) != 0, thr = (a.stages & MF_GUIDE_THRESHOLD) != 0;
  if (l == 0) {
    float kf = 1.0f;
    if (rescale) {   // the row's partial sums, moved to the pivots of workgroup 0, in ascending order
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      const double* q = g.sums + (long)b * g.parts * 6;
      const double c0 = q[4], p0 = q[5];
      for (int i = 0; i < g.parts; ++i) {
        const double* w = q + (long)i * 6;
        const long lo = (long)i * g.chunk, hi = lo + g.chunk < n ? lo + g.chunk : n;
        const double m = (double)(hi - lo), dc = w[4] - c0, dp = w[5] - p0;
        acc[0] += w[0] + m * dc;
        acc[1] += w[1] + 2.0 * dc * w[0] + m * dc * dc;
        acc[2] += w[2] + m * dp;
        acc[3] += w[3] + 2.0 * dp * w[2] + m * dp * dp;
      }
      kf = rescale_k(S.phi, acc, n);
    }
    k_lds = kf;
  }
  __syncthreads();
  const float kf = k_lds;
  const QuantPos qp = quant_pos(S.q, n);
  unsigned pre[2] = {0u, 0u}, r[2] = {qp.lo, qp.hi};
  float s = 0.0f;
  if (thr && pass > 0) {
    if (pass > 1) {   // the select after digit pass - 2, as the launch before left it
      const unsigned* st = g.state + ((long)(pass - 2) * B + b) * 4;
      pre[0] = st[0], r[0] = st[1], pre[1] = st[2], r[1] = st[3];
    }
    // the counts of digit pass - 1: lane l adds digit l over the row's workgroups
    const unsigned* hp = g.hist + ((long)((pass - 1) & 1) * B + b) * g.parts * 2 * LANES;
    unsigned h0 = 0u, h1 = 0u;
    for (int i = 0; i < g.parts; ++i) {
      h0 += hp[((long)i * 2) * LANES + l];
      h1 += hp[((long)i * 2 + 1) * LANES + l];
    }
    select_digit(h0, h1, 24 - 8 * (pass - 1), pre, r, sl);
    if (pass < 4) {
      if (part == 0 && l == 0) {
        unsigned* st = g.state + ((long)(pass - 1) * B + b) * 4;
        st[0] = pre[0], st[1] = r[0], st[2] = pre[1], st[3] = r[1];
      }
    } else {
      s = limit_of(qp, pre[0], pre[1], S.s_max);
    }
  }
  if (pass < 4) {
    hist[0][l] = 0u, hist[1][l] = 0u;
    __syncthreads();
  }
  const float* __restrict__ xtr = (thr && a.objective == 0) ? a.x_t + off : nullptr;
  float* __restrict__ outr = a.pred_out + off;
  const long start = (long)part * g.chunk;
  const long end = start + g.chunk < n ? start + g.chunk : n;
  for (long e = start + 4L * l; e < end; e += QUAD_SPAN) {
    const int nv = end - e < 4 ? (int)(end - e) : 4;
    float p[4], xt[4] = {0.f, 0.f, 0.f, 0.f};
    load4(outr, e, nv, vec, p);
    if (xtr) load4(xtr, e, nv, vec, xt);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (rescale) p[c] = kf * p[c];
      if (thr) {
        const float x0 = x0_elem(a.objective, S.sqrt_recip_ac, S.sqrt_recipm1_ac, xt[c], p[c]);
        if (pass < 4) {
          if (c < nv) count_key(abs_key(x0), pass, pre, hist);
        } else {
          p[c] = back_elem(a.objective, S.sqrt_recip_ac, S.sqrt_recipm1_ac, xt[c], threshold_elem(x0, s));
        }
      }
    }
    if (pass == 4) store4(outr, e, nv, vec, p);
  }
  if (pass < 4) {
    __syncthreads();
    unsigned* ho = g.hist + (((long)(pass & 1) * B + b) * g.parts + part) * 2 * LANES;
    ho[l] = hist[0][l];
    ho[LANES + l] = hist[1][l];
  } else if (part == 0 && l == 0) {
    if (a.scale_out) a.scale_out[b] = kf;
    if (a.limit_out) a.limit_out[b] = s;
  }
}

}  // namespace

extern "C" {

size_t mf_guide_workspace_bytes(int B, int64_t n) {
  if (B <= 0 || n <= MF_GUIDE_ROW_ONE_WG) return 0;
  const int parts = guide_parts((long)n);
  return sums_bytes(B, parts) + hist_bytes(B, parts) + state_bytes(B);
}

int mf_guide_f32(const MfGuideArgs* a, void* stream) {
  MF_REQUIRE(a && a->pred && a->pred_out && a->table && a->B > 0 && a->B <= 65535 && a->n > 0 && a->n <= 0x7FFFFFFFL, MF_EINVAL, "guide: bad args");
  MF_REQUIRE(a->objective == 0 || a->objective == 1, MF_EINVAL, "guide: objective");
  MF_REQUIRE((a->stages & ~(MF_GUIDE_RESCALE | MF_GUIDE_THRESHOLD)) == 0 && a->reserved == 0 && a->reserved2 == 0, MF_EINVAL, "guide: stages / reserved");
  MF_REQUIRE(a->step_dev || a->step >= 0, MF_EINVAL, "guide: step");
  const bool rescale = (a->stages & MF_GUIDE_RESCALE) != 0, thr = (a->stages & MF_GUIDE_THRESHOLD) != 0;
  MF_REQUIRE(!rescale || a->pred_uncond, MF_EINVAL, "guide: guidance rescale needs the guidance pair (pred_uncond)");
  MF_REQUIRE(!(thr && a->objective == 0) || a->x_t, MF_EINVAL, "guide: thresholding with objective 'x_T' reads x_t");
  MF_REQUIRE(a->pred_out != a->pred_uncond && a->pred_out != a->x_t, MF_EINVAL, "guide: pred_out may alias pred only");
  const uintptr_t al = (uintptr_t)a->pred | (uintptr_t)a->pred_out | (uintptr_t)a->pred_uncond | ((thr && a->objective == 0) ? (uintptr_t)a->x_t : 0);
  const bool vec = (al & 15) == 0 && a->n % 4 == 0;
  hipStream_t s = (hipStream_t)stream;
  const double tot = (double)a->B * (double)a->n;
  ProfScope ps(MF_FAM_SCHED, s, 12.0 * tot, 4.0 * tot * (a->pred_uncond ? 4 : 3));
  if (a->n <= MF_GUIDE_ROW_ONE_WG) {
    MF_LAUNCH(guide_row_kernel, dim3(a->B), dim3(LANES), 0, s, *a, vec);
    return check_launch("guide");
  }
  GuideGeom g;
  g.chunk = guide_chunk((long)a->n), g.parts = guide_parts((long)a->n);
  g.sums = nullptr, g.hist = nullptr, g.state = nullptr;
  if (a->stages) {
    const size_t need = mf_guide_workspace_bytes(a->B, a->n);
    MF_REQUIRE(a->workspace && ((uintptr_t)a->workspace & 7) == 0, MF_EINVAL, "guide: workspace must be given, 8-byte aligned");
    MF_REQUIRE(a->workspace_bytes >= need, MF_EWORKSPACE, "guide: workspace of %zu bytes, %zu needed", (size_t)a->workspace_bytes, need);
    char* w = reinterpret_cast<char*>(a->workspace);
    g.sums = reinterpret_cast<double*>(w);
    g.hist = reinterpret_cast<unsigned*>(w + sums_bytes(a->B, g.parts));
    g.state = reinterpret_cast<unsigned*>(w + sums_bytes(a->B, g.parts) + hist_bytes(a->B, g.parts));
  }
  const dim3 grid(g.parts, a->B);
  MF_LAUNCH(guide_combine_kernel, grid, dim3(LANES), 0, s, *a, g, vec);
  if (thr) {
    for (int pass = 0; pass < 4; ++pass) MF_LAUNCH(guide_pass_kernel, grid, dim3(LANES), 0, s, *a, g, vec, pass);
  }
  if (a->stages) MF_LAUNCH(guide_pass_kernel, grid, dim3(LANES), 0, s, *a, g, vec, 4);
  return check_launch("guide");
}

}  // extern "C"
