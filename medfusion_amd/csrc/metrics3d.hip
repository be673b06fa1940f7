// metrics3d.hip -- the volume (NCDHW) half of the image-quality metrics: SSIM / MS-SSIM / MSE of volume PAIRS drawn from two banks
// (include/medfusion_hip.h, MfSsim3dDesc) and the 2 x 2 x 2 pooling of the banks' pyramids.  The window is g (x) g (x) g, VALID positions only.
// One launch per scale for ALL pairs, no intermediate field in global memory: the only global stores of the main launch are three fp64 partial
// sums per workgroup; a second small launch adds each pair's partials in ascending (channel, tile) order in fp64.  No floating-point atomics:
// the same bits on every launch, and a pair's result depends neither on how many pairs the launch holds nor on where the pair sits among them.
//
// The workgroup (256 threads) owns TILE x TILE = 16 x 16 in-plane window origins -- ONE per thread -- for a chunk of DCHUNK = 16 origins in depth,
// and marches over the nOz + K - 1 input planes under them:
//   * a plane's (TILE + K - 1)^2 voxels of x and of y are staged in LDS minus the workgroup's PIVOT (its first voxel of x, of y), filtered along W
//     (five fields x, y, x^2, y^2, xy -> LDS) and along H (registers): the 2-D kernel's two passes, per plane;
//   * the depth pass keeps, per field, a ring of K partial sums in registers, one per window origin in flight along depth: plane z adds
//     g[j] * v into the sum of origin z - j.  Every sum is an fmaf chain in ascending depth = ascending tap index.  The plane loop is unrolled
//     K times, so that every ring slot is a register with a static name; the origin that completes (z - K + 1) gives its ssim / cs at once.
// Budget: the ring is 5 K = 55 VGPRs at K = 11, the kernels take 63 (K = 3) to 121 VGPRs in all, no scratch: 4 waves per SIMD or more, four workgroups per CU
// (LDS: 18 KiB per workgroup, not the limit).  Two origins per thread (110 VGPRs of ring) would halve the in-plane halo but leave 2 - 3 waves.
// Halo re-read factors at K = 11: (16 + 10) / 16 = 1.63 along H and along W (1.38 at K = 7, 1.13 at K = 3), and the same (nOz + K - 1) / nOz
// along depth for a full chunk; the re-reads are neighbours' planes and come from L2.
// Parallelism does not lean on P: the grid is (tiles_x tiles_y chunks, C, P), and ONE pair of 1 x 64 x 128 x 128 at K = 11 (54 x 118 x 118
// origins) is 8 x 8 x 4 = 256 workgroups -- one per CU; four such pairs fill every CU's four slots.
// A full-halo 3-D stage would not fit: a 32 x 32 tile of five fields over 18 planes is over 200 KiB against 160 KiB of LDS.
// Built without packed fp32 like metrics.hip (medfusion_amd/build.py): the filters and the SSIM arithmetic are plain fp32 VALU work that hipcc would pack.
#include "common.h"

#include <math.h>

using namespace mf;

namespace {

constexpr int TILE = 16;                          // window origins per workgroup along H and along W: one origin per thread
constexpr int DCHUNK = 16;                        // window origins per workgroup along depth
constexpr int MAXK = MF_SSIM_MAX_K;               // 11
constexpr int HALO = TILE + MAXK - 1;             // 26 rows / columns of voxels under a tile's windows
constexpr int HGROUPS = 7;                        // a staged row: seven sixteen-byte groups (28 >= 26 voxels) ...
constexpr int HSTRIDE = 48;                       // ... at a stride of 48 floats: rows r and r + 1 of the horizontal pass (16 lanes each) fall on disjoint banks
static_assert(HALO * HGROUPS <= 256, "one staged group of four voxels per thread and plane at the most");
static_assert(HGROUPS * 4 >= HALO && TILE * TILE == 256, "tile geometry");

struct Ssim3dGeom {
  int P, C, D, H, W, OD, OH, OW, tiles_x, tiles_y, tiles_z, Nx, Ny, want_mse;
  float taps[MAXK];
  float k1, k2, data_range;
  float wsum, wdef;   // W = (sum of the taps)^3 and 1 - W, formed in fp64 on the host: the rounded taps miss 1 by a few 1e-9
};

__device__ __forceinline__ float pair_range(const float* __restrict__ mmx, const float* __restrict__ mmy, int a, int b, float fixed) {
  if (mmx == nullptr) return fixed;
  return fmaxf(mmx[2 * a + 1] - mmx[2 * a], mmy[2 * b + 1] - mmy[2 * b]);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// the four voxels of x and of y a thread stages per plane
struct Group {
  float xs[4], ys[4];
  bool in[4];
};

// V = 4: one sixteen-byte load each (W % 4 == 0, 16-byte aligned banks: a group is inside or outside as a whole); V = 1: element by element.
// Both give every thread the same voxels in the same order; a voxel outside the volume reads as the pivot (0 once staged).
template <int V>
__device__ __forceinline__ void load_group(Group& q, const float* __restrict__ x, const float* __restrict__ y, long plane, int gr, int gc, int H, int W,
                                           float px, float py, bool active) {
  if (V == 4) {
    float4 xv = make_float4(px, px, px, px), yv = make_float4(py, py, py, py);
    const bool all = active && gr < H && gc < W;
    if (all) {
      xv = *reinterpret_cast<const float4*>(x + plane + (long)gr * W + gc);
      yv = *reinterpret_cast<const float4*>(y + plane + (long)gr * W + gc);
    }
    q.xs[0] = xv.x, q.xs[1] = xv.y, q.xs[2] = xv.z, q.xs[3] = xv.w;
    q.ys[0] = yv.x, q.ys[1] = yv.y, q.ys[2] = yv.z, q.ys[3] = yv.w;
    q.in[0] = q.in[1] = q.in[2] = q.in[3] = all;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      q.in[j] = active && gr < H && gc + j < W;
      q.xs[j] = q.in[j] ? x[plane + (long)gr * W + gc + j] : px;
      q.ys[j] = q.in[j] ? y[plane + (long)gr * W + gc + j] : py;
    }
  }
}

// One workgroup: the TILE x TILE x nOz window origins at (tz * DCHUNK, ty * TILE, tx * TILE) of channel c of pair p.  Per input plane z:
//   1. stage: the group of four voxels loaded one plane ahead goes to LDS minus the pivot; (x - y)^2 of the voxels the workgroup OWNS (its
//      DCHUNK x TILE x TILE block; the last tile of an axis also the K - 1 trailing ones) is summed, at most four squares in fp32, then fp64;
//   2. horizontal pass: sum_j g[j] {x, y, x^2, y^2, x y} into LDS;
//   3. vertical pass in registers: the five in-plane moments v[f] of the thread's origin;
//   4. depth pass: ring slot (z - j) mod K takes g[j] * v[f]; the slot of origin z - K + 1 is complete: ssim / cs, masked to the valid origins,
//      added in fp64 (the correction for taps of sum W != 1 is the 2-D kernel's with W = (sum g)^3);
// then the sums over the wave (shuffles, a fixed tree) and over the four waves through LDS in wave order; three doubles out.
template <int K, int V>
__global__ __launch_bounds__(256) void ssim3d_pairs_kernel(const float* __restrict__ xbank, const float* __restrict__ ybank, const int* __restrict__ ix,
                                                           const int* __restrict__ iy, const float* __restrict__ mmx, const float* __restrict__ mmy,
                                                           double* __restrict__ part, const Ssim3dGeom g) {
  constexpr int HR = TILE + K - 1;
  __shared__ float sx[HALO * HSTRIDE], sy[HALO * HSTRIDE];
  __shared__ float sh[5][HALO * TILE];
  __shared__ double red[4][3];
  const int t = threadIdx.x, tile = blockIdx.x, c = blockIdx.y, p = blockIdx.z;
  const int a = ix ? ix[p] : p, b = iy ? iy[p] : p;
  const int tiles = g.tiles_x * g.tiles_y * g.tiles_z;
  double* out = part + (((long)p * g.C + c) * tiles + tile) * 3;
  if ((unsigned)a >= (unsigned)g.Nx || (unsigned)b >= (unsigned)g.Ny) {   // an index outside its bank: the pair's result is NaN, nothing is read
    if (t == 0) out[0] = out[1] = out[2] = (double)NAN;
    return;
  }
  const int tz = tile / (g.tiles_x * g.tiles_y), rem = tile - tz * (g.tiles_x * g.tiles_y);
  const int ty = rem / g.tiles_x, tx = rem - ty * g.tiles_x;
  const int d0 = tz * DCHUNK, r0 = ty * TILE, c0 = tx * TILE;
  const long HW = (long)g.H * g.W;
  const float* __restrict__ x = xbank + (((long)a * g.C + c) * g.D + d0) * HW;
  const float* __restrict__ y = ybank + (((long)b * g.C + c) * g.D + d0) * HW;
  const int nOz = min(DCHUNK, g.OD - d0), nOy = min(TILE, g.OH - r0), nOx = min(TILE, g.OW - c0);     // valid origins of this workgroup (>= 1 each)
  const int ownZ = tz == g.tiles_z - 1 ? nOz + K - 1 : DCHUNK;
  const int ownR = ty == g.tiles_y - 1 ? nOy + K - 1 : TILE, ownC = tx == g.tiles_x - 1 ? nOx + K - 1 : TILE;
  const int nplanes = nOz + K - 1;                                               // d0 + nplanes <= D
  const float px = x[(long)r0 * g.W + c0], py = y[(long)r0 * g.W + c0];
  const float L = pair_range(mmx, mmy, a, b, g.data_range);
  const float c1 = (g.k1 * L) * (g.k1 * L), c2 = (g.k2 * L) * (g.k2 * L);
  // the thread's staged group: row sr, columns sq .. sq + 3 of the halo
  const bool stager = t < HR * HGROUPS;
  const int sr = t / HGROUPS, sq = (t - sr * HGROUPS) * 4;
  const bool own_rc[4] = {sr < ownR && sq < ownC, sr < ownR && sq + 1 < ownC, sr < ownR && sq + 2 < ownC, sr < ownR && sq + 3 < ownC};
  const int oc = t & (TILE - 1), orow = t / TILE;                                // the thread's window origin
  const bool valid_rc = orow < nOy && oc < nOx;
  float ring[5][K];
#pragma unroll
  for (int f = 0; f < 5; ++f)
#pragma unroll
    for (int s = 0; s < K; ++s) ring[f][s] = 0.f;
  double s_ssim = 0.0, s_cs = 0.0, s_se = 0.0;
  Group q;
  load_group<V>(q, x, y, 0, r0 + sr, c0 + sq, g.H, g.W, px, py, stager);
  for (int zb = 0; zb < nplanes; zb += K) {
#pragma unroll
    for (int r = 0; r < K; ++r) {
      const int z = zb + r;
      if (z < nplanes) {                                                         // uniform over the workgroup
        // ---- 1. stage
        if (stager) {
          float se = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            sx[sr * HSTRIDE + sq + j] = q.xs[j] - px;
            sy[sr * HSTRIDE + sq + j] = q.ys[j] - py;
            if (g.want_mse && q.in[j] && own_rc[j] && z < ownZ) {
              const float d = q.xs[j] - q.ys[j];
              se = fmaf(d, d, se);
            }
          }
          s_se += (double)se;
        }
        __syncthreads();
        if (z + 1 < nplanes) load_group<V>(q, x, y, (long)(z + 1) * HW, r0 + sr, c0 + sq, g.H, g.W, px, py, stager);   // in flight under this plane's arithmetic
        // ---- 2. horizontal pass
        for (int idx = t; idx < HR * TILE; idx += 256) {
          const int rr = idx / TILE, cc = idx - rr * TILE;
          const float* rx = sx + rr * HSTRIDE + cc;
          const float* ry = sy + rr * HSTRIDE + cc;
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
        // ---- 3. vertical pass, 4. depth pass
#pragma unroll
        for (int f = 0; f < 5; ++f) {
          float v = 0.f;
#pragma unroll
          for (int j = 0; j < K; ++j) v = fmaf(g.taps[j], sh[f][(orow + j) * TILE + oc], v);
          ring[f][r] = g.taps[0] * v;                                            // origin z begins (its slot finished K planes ago)
#pragma unroll
          for (int j = 1; j < K; ++j) ring[f][(r - j + K) % K] = fmaf(g.taps[j], v, ring[f][(r - j + K) % K]);
        }
        if (z >= K - 1) {                                                        // origin z - K + 1 (< nOz) is complete, in slot (r + 1) mod K
          const int DONE = (r + 1) % K;
          const float ex = ring[0][DONE], ey = ring[1][DONE];
          const float vx = (ring[2][DONE] - ex * ex) + g.wdef * (2.f * px * ex + px * px * g.wsum);
          const float vy = (ring[3][DONE] - ey * ey) + g.wdef * (2.f * py * ey + py * py * g.wsum);
          const float vxy = (ring[4][DONE] - ex * ey) + g.wdef * (py * ex + px * ey + px * py * g.wsum);
          const float mux = ex + px * g.wsum, muy = ey + py * g.wsum;            // the pivot restored in the means
          const float cs = (2.f * vxy + c2) / (vx + vy + c2);
          const float lum = (2.f * mux * muy + c1) / (mux * mux + muy * muy + c1);
          s_cs += valid_rc ? (double)cs : 0.0;
          s_ssim += valid_rc ? (double)(lum * cs) : 0.0;
        }
      }
    }
  }
  // ---- reduce
  const double w0 = wave_sum(s_ssim), w1 = wave_sum(s_cs), w2 = wave_sum(s_se);
  if ((t & 63) == 0) {
    red[t >> 6][0] = w0;
    red[t >> 6][1] = w1;
    red[t >> 6][2] = w2;
  }
  __syncthreads();
  if (t < 3) out[t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

struct Ssim3dFinish {
  int P, parts, out_stride;      // partial triples per pair (C * tiles), distance in floats between two pairs' outputs
  double windows, voxels;        // C * OD * OH * OW, C * D * H * W
};

// one thread per pair: its partials in ascending (channel, tile) order, in fp64
__global__ __launch_bounds__(64) void ssim3d_finish_kernel(const double* __restrict__ part, float* __restrict__ sim, float* __restrict__ cs,
                                                           float* __restrict__ mse, const Ssim3dFinish f) {
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
  if (mse) mse[p] = (float)(s2 / f.voxels);
}

// out[pl][oz][oy][ox] = the mean of the 2 x 2 x 2 block at (2 oz, 2 oy, 2 ox); an odd trailing plane, row or column is dropped.  The eight are
// added one after the other in (depth, row, column) order from 0 -- ((((((v000 + v001) + v010) + v011) + v100) + v101) + v110) + v111 -- and the
// sum is multiplied by 1/8 (exact): the order of a plain triple loop
__global__ __launch_bounds__(256) void avgpool2_volumes_kernel(const float* __restrict__ x, float* __restrict__ y, int D, int H, int W, int OD, int OH, int OW,
                                                               long total) {
  const long stride = (long)gridDim.x * blockDim.x;
  const long HW = (long)H * W;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
    const int ox = (int)(q % OW);
    long r = q / OW;
    const int oy = (int)(r % OH);
    r /= OH;
    const int oz = (int)(r % OD);
    const long pl = r / OD;
    const float* s = x + ((pl * D + 2 * oz) * H + 2 * oy) * (long)W + 2 * ox;
    float v = s[0] + s[1];
    v += s[W];
    v += s[W + 1];
    v += s[HW];
    v += s[HW + 1];
    v += s[HW + W];
    v += s[HW + W + 1];
    y[q] = v * 0.125f;
  }
}

// the descriptor's rules, checked on the host before any launch; fills the kernel's geometry
int ssim3d_geometry(const MfSsim3dDesc* d, const char* what, Ssim3dGeom* g) {
  MF_REQUIRE(d != nullptr, MF_EINVAL, "%s: no descriptor", what);
  MF_REQUIRE(d->k >= 3 && d->k <= MF_SSIM_MAX_K && (d->k & 1), MF_EINVAL, "%s: k=%d (odd, 3 .. %d)", what, d->k, MF_SSIM_MAX_K);
  MF_REQUIRE(d->P > 0 && d->C > 0 && d->P <= 65535 && d->C <= 65535, MF_EINVAL, "%s: P=%d C=%d (1 .. 65535)", what, d->P, d->C);
  MF_REQUIRE(d->D >= d->k && d->H >= d->k && d->W >= d->k, MF_EINVAL, "%s: extents %d x %d x %d under the window of %d", what, d->D, d->H, d->W, d->k);
  MF_REQUIRE(d->Nx > 0 && d->Ny > 0, MF_EINVAL, "%s: banks Nx=%d Ny=%d", what, d->Nx, d->Ny);
  MF_REQUIRE((d->indexed & ~3) == 0, MF_EINVAL, "%s: indexed=%d (bit 0: ix, bit 1: iy)", what, d->indexed);
  MF_REQUIRE((d->indexed & 1) || d->P <= d->Nx, MF_EINVAL, "%s: P=%d pairs without ix over a bank of Nx=%d", what, d->P, d->Nx);
  MF_REQUIRE((d->indexed & 2) || d->P <= d->Ny, MF_EINVAL, "%s: P=%d pairs without iy over a bank of Ny=%d", what, d->P, d->Ny);
  MF_REQUIRE((d->want_mse & ~1) == 0 && (d->range_on_device & ~1) == 0, MF_EINVAL, "%s: want_mse / range_on_device are 0 or 1", what);
  MF_REQUIRE((long)d->D * d->H * d->W <= (1L << 31) - 1, MF_EINVAL, "%s: a volume of %d x %d x %d", what, d->D, d->H, d->W);
  g->P = d->P, g->C = d->C, g->D = d->D, g->H = d->H, g->W = d->W;
  g->OD = d->D - d->k + 1, g->OH = d->H - d->k + 1, g->OW = d->W - d->k + 1;
  g->tiles_x = cdiv(g->OW, TILE), g->tiles_y = cdiv(g->OH, TILE), g->tiles_z = cdiv(g->OD, DCHUNK);
  g->Nx = d->Nx, g->Ny = d->Ny, g->want_mse = d->want_mse;
  double w1 = 0.0;
  for (int j = 0; j < MAXK; ++j) {
    g->taps[j] = j < d->k ? d->taps[j] : 0.f;
    w1 += (double)g->taps[j];
  }
  g->wsum = (float)(w1 * w1 * w1), g->wdef = (float)(1.0 - w1 * w1 * w1);
  g->k1 = d->k1, g->k2 = d->k2, g->data_range = d->data_range;
  MF_REQUIRE((long)g->tiles_x * g->tiles_y * g->tiles_z <= (1L << 31) - 1, MF_EINVAL, "%s: too many tiles", what);
  return MF_OK;
}

inline size_t ssim3d_bytes(const Ssim3dGeom& g) { return (size_t)g.P * g.C * g.tiles_x * g.tiles_y * g.tiles_z * 3 * sizeof(double); }

template <int K>
void launch_pairs(bool by4, dim3 grid, hipStream_t s, const float* xb, const float* yb, const int* ix, const int* iy, const float* mmx, const float* mmy,
                  double* part, const Ssim3dGeom& g) {
  if (by4) MF_LAUNCH((ssim3d_pairs_kernel<K, 4>), grid, dim3(256), 0, s, xb, yb, ix, iy, mmx, mmy, part, g);
  else MF_LAUNCH((ssim3d_pairs_kernel<K, 1>), grid, dim3(256), 0, s, xb, yb, ix, iy, mmx, mmy, part, g);
}

}  // namespace

extern "C" {

int mf_ssim3d_ok(const MfSsim3dDesc* desc) {
  Ssim3dGeom g;
  return ssim3d_geometry(desc, "ssim3d_ok", &g) == MF_OK ? 1 : 0;
}

size_t mf_ssim3d_workspace_bytes(const MfSsim3dDesc* desc) {
  Ssim3dGeom g;
  return ssim3d_geometry(desc, "ssim3d_workspace_bytes", &g) == MF_OK ? ssim3d_bytes(g) : 0;
}

int mf_ssim3d_pairs_f32(const float* xbank, const float* ybank, const int32_t* ix, const int32_t* iy, const float* minmax_x, const float* minmax_y,
                        void* workspace, size_t workspace_bytes, const MfSsim3dDesc* desc, void* stream) {
  Ssim3dGeom g;
  const int rc = ssim3d_geometry(desc, "ssim3d_pairs", &g);
  if (rc != MF_OK) return rc;
  MF_REQUIRE(xbank && ybank && workspace, MF_EINVAL, "ssim3d_pairs: bad args");
  MF_REQUIRE((ix != nullptr) == ((desc->indexed & 1) != 0) && (iy != nullptr) == ((desc->indexed & 2) != 0), MF_EINVAL,
             "ssim3d_pairs: indexed=%d against ix %s, iy %s", desc->indexed, ix ? "given" : "null", iy ? "given" : "null");
  MF_REQUIRE((minmax_x != nullptr) == (desc->range_on_device != 0) && (minmax_y != nullptr) == (desc->range_on_device != 0), MF_EINVAL,
             "ssim3d_pairs: range_on_device=%d against the min / max rows", desc->range_on_device);
  MF_REQUIRE(((uintptr_t)workspace & 7) == 0, MF_EINVAL, "ssim3d_pairs: an 8-byte aligned workspace");
  MF_REQUIRE(workspace_bytes >= ssim3d_bytes(g), MF_EWORKSPACE, "ssim3d_pairs: workspace of %zu bytes, %zu needed", workspace_bytes, ssim3d_bytes(g));
  hipStream_t s = (hipStream_t)stream;
  const bool by4 = g.W % 4 == 0 && ((((uintptr_t)xbank | (uintptr_t)ybank) & 15) == 0);
  const dim3 grid(g.tiles_x * g.tiles_y * g.tiles_z, g.C, g.P);
  const double vox = (double)g.P * g.C * g.D * g.H * g.W;
  ProfScope ps(MF_FAM_MISC, s, vox * (15.0 * desc->k + 30.0), 8.0 * vox);
  double* part = (double*)workspace;
  switch (desc->k) {
    case 3: launch_pairs<3>(by4, grid, s, xbank, ybank, ix, iy, minmax_x, minmax_y, part, g); break;
    case 5: launch_pairs<5>(by4, grid, s, xbank, ybank, ix, iy, minmax_x, minmax_y, part, g); break;
    case 7: launch_pairs<7>(by4, grid, s, xbank, ybank, ix, iy, minmax_x, minmax_y, part, g); break;
    case 9: launch_pairs<9>(by4, grid, s, xbank, ybank, ix, iy, minmax_x, minmax_y, part, g); break;
    default: launch_pairs<11>(by4, grid, s, xbank, ybank, ix, iy, minmax_x, minmax_y, part, g); break;
  }
  return check_launch("ssim3d_pairs");
}

int mf_ssim3d_finish_f32(const void* workspace, float* sim, float* cs, float* mse, int out_stride, const MfSsim3dDesc* desc, void* stream) {
  Ssim3dGeom g;
  const int rc = ssim3d_geometry(desc, "ssim3d_finish", &g);
  if (rc != MF_OK) return rc;
  MF_REQUIRE(workspace && (sim || cs || mse) && out_stride >= 1, MF_EINVAL, "ssim3d_finish: bad args");
  MF_REQUIRE(mse == nullptr || desc->want_mse, MF_EINVAL, "ssim3d_finish: mse asked of a launch without want_mse");
  hipStream_t s = (hipStream_t)stream;
  Ssim3dFinish f;
  f.P = g.P, f.parts = g.C * g.tiles_x * g.tiles_y * g.tiles_z, f.out_stride = out_stride;
  f.windows = (double)g.C * g.OD * g.OH * g.OW, f.voxels = (double)g.C * g.D * g.H * g.W;
  ProfScope ps(MF_FAM_MISC, s, 0, 24.0 * g.P * f.parts);
  MF_LAUNCH(ssim3d_finish_kernel, dim3(cdiv(g.P, 64)), dim3(64), 0, s, (const double*)workspace, sim, cs, mse, f);
  return check_launch("ssim3d_finish");
}

int mf_avgpool2_volumes_f32(const float* x, float* y, int64_t planes, int D, int H, int W, void* stream) {
  MF_REQUIRE(x && y && planes > 0 && D >= 2 && H >= 2 && W >= 2, MF_EINVAL, "avgpool2_volumes: planes=%lld D=%d H=%d W=%d", (long long)planes, D, H, W);
  hipStream_t s = (hipStream_t)stream;
  const int OD = D / 2, OH = H / 2, OW = W / 2;
  const long total = (long)planes * OD * OH * OW;
  ProfScope ps(MF_FAM_MISC, s, 8.0 * total, 36.0 * total);
  const long blocks = (total + 255) / 256;
  MF_LAUNCH(avgpool2_volumes_kernel, dim3((int)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, x, y, D, H, W, OD, OH, OW, total);
  return check_launch("avgpool2_volumes");
}

}  // extern "C"
