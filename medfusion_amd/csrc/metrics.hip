// metrics.hip -- image-quality metrics on the device: SSIM / MS-SSIM / MSE of image PAIRS drawn from two image banks (include/medfusion_hip.h,
// MfSsimDesc), the 2x2 pooling of the banks' pyramids and the per-image min / max of data_range=None.  One launch per scale for ALL pairs:
// every input plane is read once per scale (plus the tile halos) and nothing but three partial sums per workgroup is written; a second small
// launch adds each pair's partials in ascending tile order in fp64.  No floating-point atomics anywhere: the same bits on every launch, and a
// pair's result does not depend on how many pairs the launch holds or where the pair sits among them.
// Built without packed fp32 like vq.hip (medfusion_amd/build.py): the filters and the SSIM arithmetic are plain fp32 VALU work that hipcc would pack.
#include "common.h"

#include <math.h>

using namespace mf;

namespace {

constexpr int TILE = 32;                          // window origins per workgroup and axis
constexpr int MAXK = MF_SSIM_MAX_K;               // 11
constexpr int HALO = TILE + MAXK - 1;             // 42 rows / columns of pixels under a tile's windows
constexpr int HSTRIDE = 44;                       // a staged row: 11 sixteen-byte groups

// geometry and taps by value in the kernarg segment: no device table to upload
struct SsimGeom {
  int P, C, H, W, OH, OW, tiles_x, tiles_y, Nx, Ny, want_mse;
  float taps[MAXK];
  float k1, k2, data_range;
  float wsum, wdef;   // W = (sum of the taps)^2 and 1 - W, formed in fp64 on the host: the rounded taps miss 1 by a few 1e-9
};

// L of a pair: the fixed data_range, or (data_range=None) the larger of the two images' max - min from the banks' [N][2] min / max rows
__device__ __forceinline__ float pair_range(const float* __restrict__ mmx, const float* __restrict__ mmy, int a, int b, float fixed) {
  if (mmx == nullptr) return fixed;
  return fmaxf(mmx[2 * a + 1] - mmx[2 * a], mmy[2 * b + 1] - mmy[2 * b]);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// One workgroup: the TILE x TILE window origins at (ty * TILE, tx * TILE) of channel c of pair p.
//   1. stage the (TILE + K - 1)^2 pixels under them of x and of y in LDS, minus a per-tile PIVOT (the tile's first pixel of x, of y): variances
//      and the covariance are shift-invariant, and E[x^2] - mu^2 of a near-constant region no longer cancels four digits away.  (Invariant for
//      weights of sum W = 1; for the W the rounded taps have, the definition's moments about 0 are the pivoted ones plus (1 - W) times a
//      known term, added in step 3: E[x^2] - mu^2 = (E'[u^2] - E'[u]^2) + (1 - W)(2 p E'[u] + p^2 W) with u = x - p, and alike for xy.)
//   2. horizontal pass: the five fields sum_j g[j] {x, y, x^2, y^2, x y} into LDS;
//   3. vertical pass in registers, four outputs (consecutive rows of one column) per thread, then ssim / cs, masked to the valid origins;
//   4. sum over the wave (shuffles, a fixed tree), over the four waves through LDS in wave order; three doubles out.
// (x - y)^2 is summed while staging, over the pixels the tile OWNS (its TILE x TILE block; the last tile of an axis also the K - 1 trailing ones).
// V = 4: sixteen-byte global loads (W % 4 == 0, 16-byte aligned banks); V = 1: element by element.  Both stage the same values and give every
// thread the same pixels in the same order: the same bits in sim, cs AND mse.
template <int K, int V>
__global__ __launch_bounds__(256) void ssim_pairs_kernel(const float* __restrict__ xbank, const float* __restrict__ ybank, const int* __restrict__ ix,
                                                         const int* __restrict__ iy, const float* __restrict__ mmx, const float* __restrict__ mmy,
                                                         double* __restrict__ part, const SsimGeom g) {
  constexpr int HR = TILE + K - 1;
  __shared__ float sx[HALO * HSTRIDE], sy[HALO * HSTRIDE];
  __shared__ float sh[5][HALO * TILE];
  __shared__ double red[4][3];
  const int t = threadIdx.x, tile = blockIdx.x, c = blockIdx.y, p = blockIdx.z;
  const int a = ix ? ix[p] : p, b = iy ? iy[p] : p;
  double* out = part + (((long)p * g.C + c) * ((long)g.tiles_x * g.tiles_y) + tile) * 3;
  if ((unsigned)a >= (unsigned)g.Nx || (unsigned)b >= (unsigned)g.Ny) {   // an index outside its bank: the pair's result is NaN, nothing is read
    if (t == 0) out[0] = out[1] = out[2] = (double)NAN;
    return;
  }
  const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
  const int r0 = ty * TILE, c0 = tx * TILE;
  const float* __restrict__ x = xbank + ((long)a * g.C + c) * g.H * g.W;
  const float* __restrict__ y = ybank + ((long)b * g.C + c) * g.H * g.W;
  const int nOy = min(TILE, g.OH - r0), nOx = min(TILE, g.OW - c0);             // valid origins of this tile (>= 1)
  const int ownR = ty == g.tiles_y - 1 ? nOy + K - 1 : TILE, ownC = tx == g.tiles_x - 1 ? nOx + K - 1 : TILE;
  const float px = x[(long)r0 * g.W + c0], py = y[(long)r0 * g.W + c0];
  float se = 0.f;
  // ---- 1. stage: ONE assignment of pixels to threads for both load widths -- a thread takes groups of four consecutive pixels of a row, in the
  // same order, so its fp32 sum of (x - y)^2 rounds the same way whether the four came in one 16-byte load or in four
  for (int idx = t; idx < HR * (HSTRIDE / 4); idx += 256) {
    const int r = idx / (HSTRIDE / 4), q = (idx - r * (HSTRIDE / 4)) * 4;
    const int gr = r0 + r, gc = c0 + q;
    float xs[4], ys[4];
    bool in[4];
    if (V == 4) {
      float4 xv = make_float4(px, px, px, px), yv = make_float4(py, py, py, py);
      const bool all = gr < g.H && gc < g.W;                                     // W % 4 == 0: a group is inside or outside as a whole
      if (all) {
        xv = *reinterpret_cast<const float4*>(x + (long)gr * g.W + gc);
        yv = *reinterpret_cast<const float4*>(y + (long)gr * g.W + gc);
      }
      xs[0] = xv.x, xs[1] = xv.y, xs[2] = xv.z, xs[3] = xv.w;
      ys[0] = yv.x, ys[1] = yv.y, ys[2] = yv.z, ys[3] = yv.w;
      in[0] = in[1] = in[2] = in[3] = all;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        in[j] = gr < g.H && gc + j < g.W;
        xs[j] = in[j] ? x[(long)gr * g.W + gc + j] : px;
        ys[j] = in[j] ? y[(long)gr * g.W + gc + j] : py;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sx[r * HSTRIDE + q + j] = xs[j] - px;
      sy[r * HSTRIDE + q + j] = ys[j] - py;
      if (g.want_mse && in[j] && r < ownR && q + j < ownC) {
        const float d = xs[j] - ys[j];
        se = fmaf(d, d, se);
      }
    }
  }
  __syncthreads();
  // ---- 2. horizontal pass
  for (int idx = t; idx < HR * TILE; idx += 256) {
    const int r = idx / TILE, cc = idx - r * TILE;
    const float* rx = sx + r * HSTRIDE + cc;
    const float* ry = sy + r * HSTRIDE + cc;
    float hx = 0.f, hy = 0.f, hxx = 0.f, hyy = 0.f, hxy = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const float w = g.taps[j], xv = rx[j], yv = ry[j];
      const float wx = w * xv, wy = w * yv;
      hx += wx;
      hy += wy;
      hxx = fmaf(wx, xv, hxx);
      hyy = fmaf(wy, yv, hyy);
      hxy = fmaf(wx, yv, hxy);
    }
    sh[0][idx] = hx;
    sh[1][idx] = hy;
    sh[2][idx] = hxx;
    sh[3][idx] = hyy;
    sh[4][idx] = hxy;
  }
  __syncthreads();
  // ---- 3. vertical pass, ssim / cs
  const int cc = t & (TILE - 1), rg = t / TILE;                                  // column, group of four rows
  float e[5][4];
#pragma unroll
  for (int f = 0; f < 5; ++f) {
    float v[4 + K - 1];
#pragma unroll
    for (int i = 0; i < 4 + K - 1; ++i) v[i] = sh[f][(rg * 4 + i) * TILE + cc];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < K; ++j) s = fmaf(g.taps[j], v[o + j], s);
      e[f][o] = s;
    }
  }
  const float L = pair_range(mmx, mmy, a, b, g.data_range);
  const float c1 = (g.k1 * L) * (g.k1 * L), c2 = (g.k2 * L) * (g.k2 * L);
  float s_ssim = 0.f, s_cs = 0.f;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const float ex = e[0][o], ey = e[1][o];
    const float vx = (e[2][o] - ex * ex) + g.wdef * (2.f * px * ex + px * px * g.wsum);
    const float vy = (e[3][o] - ey * ey) + g.wdef * (2.f * py * ey + py * py * g.wsum);
    const float vxy = (e[4][o] - ex * ey) + g.wdef * (py * ex + px * ey + px * py * g.wsum);
    const float mux = ex + px * g.wsum, muy = ey + py * g.wsum;                  // the pivot restored in the means
    const float cs = (2.f * vxy + c2) / (vx + vy + c2);
    const float lum = (2.f * mux * muy + c1) / (mux * mux + muy * muy + c1);
    const bool valid = rg * 4 + o < nOy && cc < nOx;
    s_cs += valid ? cs : 0.f;
    s_ssim += valid ? lum * cs : 0.f;
  }
  // ---- 4. reduce
  const double w0 = wave_sum((double)s_ssim), w1 = wave_sum((double)s_cs), w2 = wave_sum((double)se);
  if ((t & 63) == 0) {
    red[t >> 6][0] = w0;
    red[t >> 6][1] = w1;
    red[t >> 6][2] = w2;
  }
  __syncthreads();
  if (t < 3) out[t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

struct SsimFinish {
  int P, parts, out_stride;      // partial triples per pair (C * tiles), distance in floats between two pairs' outputs
  double windows, pixels;        // C * OH * OW, C * H * W
};

// one thread per pair: its partials in ascending (channel, tile) order, in fp64
__global__ __launch_bounds__(64) void ssim_finish_kernel(const double* __restrict__ part, float* __restrict__ sim, float* __restrict__ cs,
                                                         float* __restrict__ mse, const SsimFinish f) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= f.P) return;
  const double* q = part + (long)p * f.parts * 3;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < f.parts; ++i) {
    s0 += q[3 * i];
    s1 += q[3 * i + 1];
    s2 += q[3 * i + 2];
  }
  if (sim) sim[(long)p * f.out_stride] = (float)(s0 / f.windows);
  if (cs) cs[(long)p * f.out_stride] = (float)(s1 / f.windows);
  if (mse) mse[p] = (float)(s2 / f.pixels);
}

// out[n][c][oy][ox] = the mean of the 2 x 2 block at (2 oy, 2 ox); an odd trailing row or column is dropped
__global__ __launch_bounds__(256) void avgpool2_planes_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int OH, int OW, long total) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
    const int ox = (int)(q % OW);
    const long r = q / OW;
    const int oy = (int)(r % OH);
    const long pl = r / OH;
    const float* s = x + (pl * H + 2 * oy) * (long)W + 2 * ox;
    y[q] = ((s[0] + s[1]) + (s[W] + s[W + 1])) * 0.25f;
  }
}

// out[row] = {min, max} of x[row][0 .. n), both NaN when the row holds one (as torch's amin / amax): one workgroup per row
__global__ __launch_bounds__(256) void rows_minmax_kernel(const float* __restrict__ x, float* __restrict__ out, long n) {
  __shared__ float red[4][2];
  __shared__ int red_nan[4];
  const float* row = x + (long)blockIdx.x * n;
  float lo = INFINITY, hi = -INFINITY;
  int nan = 0;                                                                   // fminf / fmaxf drop a NaN: torch's amin / amax return it
  for (long i = threadIdx.x; i < n; i += 256) {
    const float v = row[i];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
    nan |= v != v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_down(lo, o, 64));
    hi = fmaxf(hi, __shfl_down(hi, o, 64));
    nan |= __shfl_down(nan, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = lo;
    red[threadIdx.x >> 6][1] = hi;
    red_nan[threadIdx.x >> 6] = nan;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool bad = (red_nan[0] | red_nan[1] | red_nan[2] | red_nan[3]) != 0;
    out[2 * (long)blockIdx.x] = bad ? NAN : fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0]));
    out[2 * (long)blockIdx.x + 1] = bad ? NAN : fmaxf(fmaxf(red[0][1], red[1][1]), fmaxf(red[2][1], red[3][1]));
  }
}

// the descriptor's rules, checked on the host before any launch; fills the kernel's geometry
int ssim_geometry(const MfSsimDesc* d, const char* what, SsimGeom* g) {
  MF_REQUIRE(d != nullptr, MF_EINVAL, "%s: no descriptor", what);
  MF_REQUIRE(d->k >= 3 && d->k <= MF_SSIM_MAX_K && (d->k & 1), MF_EINVAL, "%s: k=%d (odd, 3 .. %d)", what, d->k, MF_SSIM_MAX_K);
  MF_REQUIRE(d->P > 0 && d->C > 0 && d->P <= 65535 && d->C <= 65535, MF_EINVAL, "%s: P=%d C=%d (1 .. 65535)", what, d->P, d->C);
  MF_REQUIRE(d->H >= d->k && d->W >= d->k, MF_EINVAL, "%s: extents %d x %d under the window of %d", what, d->H, d->W, d->k);
  MF_REQUIRE(d->Nx > 0 && d->Ny > 0, MF_EINVAL, "%s: banks Nx=%d Ny=%d", what, d->Nx, d->Ny);
  MF_REQUIRE((d->indexed & ~3) == 0, MF_EINVAL, "%s: indexed=%d (bit 0: ix, bit 1: iy)", what, d->indexed);
  MF_REQUIRE((d->indexed & 1) || d->P <= d->Nx, MF_EINVAL, "%s: P=%d pairs without ix over a bank of Nx=%d", what, d->P, d->Nx);
  MF_REQUIRE((d->indexed & 2) || d->P <= d->Ny, MF_EINVAL, "%s: P=%d pairs without iy over a bank of Ny=%d", what, d->P, d->Ny);
  MF_REQUIRE((d->want_mse & ~1) == 0 && (d->range_on_device & ~1) == 0, MF_EINVAL, "%s: want_mse / range_on_device are 0 or 1", what);
  MF_REQUIRE((long)d->H * d->W <= (1L << 31) - 1, MF_EINVAL, "%s: a plane of %d x %d", what, d->H, d->W);
  g->P = d->P, g->C = d->C, g->H = d->H, g->W = d->W;
  g->OH = d->H - d->k + 1, g->OW = d->W - d->k + 1;
  g->tiles_x = cdiv(g->OW, TILE), g->tiles_y = cdiv(g->OH, TILE);
  g->Nx = d->Nx, g->Ny = d->Ny, g->want_mse = d->want_mse;
  double w1 = 0.0;
  for (int j = 0; j < MAXK; ++j) {
    g->taps[j] = j < d->k ? d->taps[j] : 0.f;
    w1 += (double)g->taps[j];
  }
  g->wsum = (float)(w1 * w1), g->wdef = (float)(1.0 - w1 * w1);
  g->k1 = d->k1, g->k2 = d->k2, g->data_range = d->data_range;
  return MF_OK;
}

inline size_t ssim_bytes(const SsimGeom& g) { return (size_t)g.P * g.C * g.tiles_x * g.tiles_y * 3 * sizeof(double); }

template <int K>
void launch_pairs(bool by4, dim3 grid, hipStream_t s, const float* xb, const float* yb, const int* ix, const int* iy, const float* mmx, const float* mmy,
                  double* part, const SsimGeom& g) {
  if (by4) MF_LAUNCH((ssim_pairs_kernel<K, 4>), grid, dim3(256), 0, s, xb, yb, ix, iy, mmx, mmy, part, g);
  else MF_LAUNCH((ssim_pairs_kernel<K, 1>), grid, dim3(256), 0, s, xb, yb, ix, iy, mmx, mmy, part, g);
}

}  // namespace

extern "C" {

int mf_ssim_ok(const MfSsimDesc* desc) {
  SsimGeom g;
  return ssim_geometry(desc, "ssim_ok", &g) == MF_OK ? 1 : 0;
}

size_t mf_ssim_workspace_bytes(const MfSsimDesc* desc) {
  SsimGeom g;
  return ssim_geometry(desc, "ssim_workspace_bytes", &g) == MF_OK ? ssim_bytes(g) : 0;
}

int mf_ssim_pairs_f32(const float* xbank, const float* ybank, const int32_t* ix, const int32_t* iy, const float* minmax_x, const float* minmax_y,
                      void* workspace, size_t workspace_bytes, const MfSsimDesc* desc, void* stream) {
  SsimGeom g;
  const int rc = ssim_geometry(desc, "ssim_pairs", &g);
  if (rc != MF_OK) return rc;
  MF_REQUIRE(xbank && ybank && workspace, MF_EINVAL, "ssim_pairs: bad args");
  MF_REQUIRE((ix != nullptr) == ((desc->indexed & 1) != 0) && (iy != nullptr) == ((desc->indexed & 2) != 0), MF_EINVAL,
             "ssim_pairs: indexed=%d against ix %s, iy %s", desc->indexed, ix ? "given" : "null", iy ? "given" : "null");
  MF_REQUIRE((minmax_x != nullptr) == (desc->range_on_device != 0) && (minmax_y != nullptr) == (desc->range_on_device != 0), MF_EINVAL,
             "ssim_pairs: range_on_device=%d against the min / max rows", desc->range_on_device);
  MF_REQUIRE(((uintptr_t)workspace & 7) == 0, MF_EINVAL, "ssim_pairs: an 8-byte aligned workspace");
  MF_REQUIRE(workspace_bytes >= ssim_bytes(g), MF_EWORKSPACE, "ssim_pairs: workspace of %zu bytes, %zu needed", workspace_bytes, ssim_bytes(g));
  hipStream_t s = (hipStream_t)stream;
  const bool by4 = g.W % 4 == 0 && ((((uintptr_t)xbank | (uintptr_t)ybank) & 15) == 0);
  const dim3 grid(g.tiles_x * g.tiles_y, g.C, g.P);
  const double px = (double)g.P * g.C * g.H * g.W;
  ProfScope ps(MF_FAM_MISC, s, px * (10.0 * desc->k + 30.0), 8.0 * px);
  double* part = (double*)workspace;
  switch (desc->k) {
    case 3: launch_pairs<3>(by4, grid, s, xbank, ybank, ix, iy, minmax_x, minmax_y, part, g); break;
    case 5: launch_pairs<5>(by4, grid, s, xbank, ybank, ix, iy, minmax_x, minmax_y, part, g); break;
    case 7: launch_pairs<7>(by4, grid, s, xbank, ybank, ix, iy, minmax_x, minmax_y, part, g); break;
    case 9: launch_pairs<9>(by4, grid, s, xbank, ybank, ix, iy, minmax_x, minmax_y, part, g); break;
    default: launch_pairs<11>(by4, grid, s, xbank, ybank, ix, iy, minmax_x, minmax_y, part, g); break;
  }
  return check_launch("ssim_pairs");
}

int mf_ssim_finish_f32(const void* workspace, float* sim, float* cs, float* mse, int out_stride, const MfSsimDesc* desc, void* stream) {
  SsimGeom g;
  const int rc = ssim_geometry(desc, "ssim_finish", &g);
  if (rc != MF_OK) return rc;
  MF_REQUIRE(workspace && (sim || cs || mse) && out_stride >= 1, MF_EINVAL, "ssim_finish: bad args");
  MF_REQUIRE(mse == nullptr || desc->want_mse, MF_EINVAL, "ssim_finish: mse asked of a launch without want_mse");
  hipStream_t s = (hipStream_t)stream;
  SsimFinish f;
  f.P = g.P, f.parts = g.C * g.tiles_x * g.tiles_y, f.out_stride = out_stride;
  f.windows = (double)g.C * g.OH * g.OW, f.pixels = (double)g.C * g.H * g.W;
  ProfScope ps(MF_FAM_MISC, s, 0, 24.0 * g.P * f.parts);
  MF_LAUNCH(ssim_finish_kernel, dim3(cdiv(g.P, 64)), dim3(64), 0, s, (const double*)workspace, sim, cs, mse, f);
  return check_launch("ssim_finish");
}

int mf_avgpool2_planes_f32(const float* x, float* y, int64_t planes, int H, int W, void* stream) {
  MF_REQUIRE(x && y && planes > 0 && H >= 2 && W >= 2, MF_EINVAL, "avgpool2_planes: planes=%lld H=%d W=%d", (long long)planes, H, W);
  hipStream_t s = (hipStream_t)stream;
  const int OH = H / 2, OW = W / 2;
  const long total = (long)planes * OH * OW;
  ProfScope ps(MF_FAM_MISC, s, 4.0 * total, 20.0 * total);
  const long blocks = (total + 255) / 256;
  MF_LAUNCH(avgpool2_planes_kernel, dim3((int)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, x, y, H, W, OH, OW, total);
  return check_launch("avgpool2_planes");
}

int mf_rows_minmax_f32(const float* x, float* out, int N, int64_t n, void* stream) {
  MF_REQUIRE(x && out && N > 0 && n > 0, MF_EINVAL, "rows_minmax: N=%d n=%lld", N, (long long)n);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 0, 4.0 * N * (double)n);
  MF_LAUNCH(rows_minmax_kernel, dim3(N), dim3(256), 0, s, x, out, (long)n);
  return check_launch("rows_minmax");
}

}  // extern "C"
