// conv3d.hip -- the 3-D convolution of the spatial_dims=3 models (MONAI Convolution with Conv[CONV, 3], conv_blocks.py:48,169,229 at
// spatial_dims=3) on the fp16-pair arithmetic MF_CONV_FP32_F16X2 (conv_f16x2.h has the arithmetic: x ~ hi + lo'/2048, three matrix terms per
// product, fp32 accumulate, per-sample power-of-two operand scales).
//
// Implicit GEMM: M = N Do Ho Wo output voxels, N = Cout, K = taps x Cin with a tap = (kd, kh, kw) walked in 32-channel chunks, chunk-major
// (all taps of a chunk, then the next chunk) so that the K loop meets the second source of a fused concat exactly once and re-scales its
// accumulators there, as the 2-D kernel does.  Every input voxel is an NDHWC row of fp16 pairs, [C/8][hi x 8 | lo' x 8] -- what
// mf_split_f16x2 / the GroupNorm apply pass / mf_pack_nchw_pairs_f32 write for the [N, D*H, W, C] view of the tensor -- and a chunk of one
// row is 128 contiguous bytes, as in 2-D.  Nearest x2 upsampling per axis is folded into the gather: the tap reads voxel u >> 1 of the source
// for coordinate u of the upsampled grid.  Out-of-range taps and rows past M / Cout load zeros.
//
// Data movement: register-staged (one 16-byte global load per thread and 32 rows), written to a two-stage LDS tile whose 16-byte slots are
// XOR-permuted by (row >> 1) & 7 (the 2-D kernel's permutation, conflict-free for the ds_read_b128 fragment reads), one barrier per chunk;
// the loads of chunk it + 1 are in flight while the matrix cores work on chunk it.  Four waves in 2 x 2, each 32 TM voxels x 32 TN channels.
// Split-K: slice kz takes a contiguous range of (chunk, tap) iterations and writes its partial tile to its own slab; a second launch sums
// the slabs in slice order and adds the bias -- deterministic, bit-identical from run to run.
#include <string.h>

#include "common.h"
#include "split_f16.h"

using namespace mf;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kRowBytes = 128;   // one 32-channel chunk of one row: [4 groups][hi | lo'][8 fp16]
constexpr int kMaxSplit = 16;

struct Conv3dP {
  const u32x4* x1;        // [N][D][H][W][C1/8][2][8] fp16 pairs (16-byte units)
  const u32x4* x2;        // second source of the fused concat, or null
  const u32x4* w;         // [Cout][taps][Cin][pairs]
  const float* bias;
  float* y;               // fp32 [M][Cout], or the split-K slabs [splitk][M][Cout]
  const float* bound1;    // [N] bounds the sources were scaled with, or null (unscaled)
  const float* bound2;
  int wexp;               // the weights were split as w 2^-wexp
  int D, H, W, C1, C2, Cin, Cout, k, taps;
  int sd, sh, sw, pd, ph, pw, ud, uh, uw;
  int Ho, Wo, DHWo, HWo, M;
  int nit, it_per_split;
  int tiles_m, tiles_n;
  long slab;              // M * Cout
};

template <int TM, int TN>
__global__ __launch_bounds__(256) void conv3d_f16x2_kernel(const Conv3dP p) {
  constexpr int BM = 64 * TM, BN = 64 * TN, FM = 32 * TM, FN = 32 * TN;
  constexpr int RA = BM / 32, RW = BN / 32;          // rows per thread and chunk (a thread moves slot `tid & 7` of rows (tid >> 3) + 32 i)
  constexpr int STAGE = (BM + BN) * kRowBytes;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int tile_m = blockIdx.x % p.tiles_m;
  const int r1 = blockIdx.x / p.tiles_m;
  const int tile_n = r1 % p.tiles_n, kz = r1 / p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int it0 = kz * p.it_per_split, it1 = min(p.nit, it0 + p.it_per_split);

  // ---- gather geometry of this thread's rows: sample base, first tap coordinate on the (upsampled) grid per axis
  const int lrow = tid >> 3, slot = tid & 7;
  int a_n[RA], a_z[RA], a_y[RA], a_x[RA];
#pragma unroll
  for (int i = 0; i < RA; ++i) {
    const int m = m0 + lrow + 32 * i;
    a_n[i] = 0; a_z[i] = -(1 << 28); a_y[i] = 0; a_x[i] = 0;   // rows past M: every tap outside
    if (m < p.M) {
      const int n = m / p.DHWo, r = m - n * p.DHWo;
      const int od = r / p.HWo, r2 = r - od * p.HWo;
      const int oh = r2 / p.Wo, ow = r2 - oh * p.Wo;
      a_n[i] = n * p.D;
      a_z[i] = od * p.sd - p.pd;
      a_y[i] = oh * p.sh - p.ph;
      a_x[i] = ow * p.sw - p.pw;
    }
  }
  const int De = p.D << p.ud, He = p.H << p.uh, We = p.W << p.uw;
  const int wst = (lrow * kRowBytes) + ((slot ^ ((lrow >> 1) & 7)) << 4);   // LDS byte offset of this thread's slot in row lrow (+32 rows per i)

  u32x4 ra[RA], rw[RW];
  auto load = [&](int it) {
    const int cc = it / p.taps, t = it - cc * p.taps;
    const int kd = t / (p.k * p.k), t2 = t - kd * p.k * p.k;
    const int kh = t2 / p.k, kw = t2 - kh * p.k;
    const bool first = cc * 32 < p.C1;
    const u32x4* src = first ? p.x1 : p.x2;
    const long cs4 = (first ? p.C1 : p.C2) >> 2;                    // 16-byte units per voxel
    const int cb = ((first ? cc * 32 : cc * 32 - p.C1) >> 2) + slot;
#pragma unroll
    for (int i = 0; i < RA; ++i) {
      const int uz = a_z[i] + kd, uy = a_y[i] + kh, ux = a_x[i] + kw;
      u32x4 v = {0u, 0u, 0u, 0u};
      if ((unsigned)uz < (unsigned)De && (unsigned)uy < (unsigned)He && (unsigned)ux < (unsigned)We) {
        const long vox = ((long)(a_n[i] + (uz >> p.ud)) * p.H + (uy >> p.uh)) * p.W + (ux >> p.uw);
        v = src[vox * cs4 + cb];
      }
      ra[i] = v;
    }
    const long wrow = (long)t * (p.Cin >> 2) + cc * 8 + slot;
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      const int co = n0 + lrow + 32 * j;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (co < p.Cout) v = p.w[(long)co * p.taps * (p.Cin >> 2) + wrow];
      rw[j] = v;
    }
  };
  auto stage_store = [&](int st) {
    char* s = smem + st * STAGE + wst;
#pragma unroll
    for (int i = 0; i < RA; ++i) *reinterpret_cast<u32x4*>(s + i * 32 * kRowBytes) = ra[i];
#pragma unroll
    for (int j = 0; j < RW; ++j) *reinterpret_cast<u32x4*>(s + (BM + j * 32) * kRowBytes) = rw[j];
  };

  f32x16 accm[TM][TN], accx[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) { accm[i][j][r] = 0.f; accx[i][j][r] = 0.f; }

  // per-voxel (= per-lane column) operand scales of the sample the lane's output voxel belongs to
  int e1[TM], e2[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int pm = min(m0 + wm * FM + i * 32 + (lane & 31), p.M - 1);
    const int pn = pm / p.DHWo;
    const bool has2 = p.bound2 && p.C2 > 0;
    source_exps(p.bound1 ? p.bound1[pn] : 0.f, p.bound1 != nullptr, has2 ? p.bound2[pn] : 0.f, has2, e1[i], e2[i]);   // (a zero bound: split_f16.h)
  }
  const int it_sw = p.C2 > 0 ? (p.C1 / 32) * p.taps : p.nit;   // first iteration that reads the second source

  // fragment reads: lane reads row (lane & 31) (+ 32 per sub-tile), slot (4 step + 2 (lane >> 5) + piece) ^ key
  const int fkey = (lane >> 1) & 7, fh = lane >> 5;
  const int xrow0 = (wm * FM + (lane & 31)) * kRowBytes, wrow0 = (BM + wn * FN + (lane & 31)) * kRowBytes;

  if (it0 < it1) {
    load(it0);
    stage_store(0);
    __syncthreads();
    for (int it = it0; it < it1; ++it) {
      const int st = (it - it0) & 1;
      if (it + 1 < it1) load(it + 1);   // in flight under this chunk's matrix work
      if (it == it_sw && it != it0) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const float f = exp2i(e1[i]) * exp2i(-e2[i]);   // (in range for e1 - e2 <= 97 - log2(C1 taps); 1 for an all-zero source: source_exps)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { accm[i][j][r] *= f; accx[i][j][r] *= f; }
        }
      }
      const char* sb = smem + st * STAGE;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        f16x8 fx[TM][2], fw[TN][2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int so = ((4 * s + 2 * fh + c) ^ fkey) << 4;
#pragma unroll
          for (int i = 0; i < TM; ++i) fx[i][c] = *reinterpret_cast<const f16x8*>(sb + xrow0 + i * 32 * kRowBytes + so);
#pragma unroll
          for (int j = 0; j < TN; ++j) fw[j][c] = *reinterpret_cast<const f16x8*>(sb + wrow0 + j * 32 * kRowBytes + so);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            accm[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw[j][0], fx[i][0], accm[i][j], 0, 0, 0);
            accx[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw[j][0], fx[i][1], accx[i][j], 0, 0, 0);
            accx[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw[j][1], fx[i][0], accx[i][j], 0, 0, 0);
          }
      }
      if (it + 1 < it1) stage_store(st ^ 1);   // (stage st ^ 1 was last read in iteration it - 1, before its barrier)
      __syncthreads();
    }
  }

  // ---- epilogue: register r of a 32 x 32 accumulator holds output channel (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of voxel (lane & 31)
  const bool split = p.it_per_split < p.nit;
  float* yb = p.y + (split ? (long)kz * p.slab : 0L);
  const bool last_src2 = p.C2 > 0 && it1 - 1 >= it_sw;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int pm = m0 + wm * FM + i * 32 + (lane & 31);
    const float f = exp2i(last_src2 ? e2[i] : e1[i]) * exp2i(p.wexp);
    if (pm >= p.M) continue;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = n0 + wn * FN + j * 32 + 8 * q + 4 * fh;
        if (co >= p.Cout) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = (accm[i][j][4 * q + e] + accx[i][j][4 * q + e] * kLoInv) * f;
          if (!split && p.bias && co + e < p.Cout) v[e] += p.bias[co + e];
        }
        float* dst = yb + (long)pm * p.Cout + co;
        if ((p.Cout & 3) == 0) {
          *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (co + e < p.Cout) dst[e] = v[e];
        }
      }
  }
}

// y = sum of the split-K slabs in slice order + bias
__global__ __launch_bounds__(256) void conv3d_splitk_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ bias, float* __restrict__ y,
                                                                  long total, int Cout, int splitk) {
  const long stride = (long)gridDim.x * 256;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    float v = ws[e];
    for (int k = 1; k < splitk; ++k) v += ws[(long)k * total + e];
    if (bias) v += bias[e % Cout];
    y[e] = v;
  }
}

// OIDHW fp32 -> [Cout][kd][kh][kw][cin_pad] fp32, input channels Cin.. zero
__global__ __launch_bounds__(256) void pack_conv3d_weight_kernel(const float* __restrict__ w, float* __restrict__ out, int Cout, int Cin, int taps,
                                                                int cin_pad) {
  const long total = (long)Cout * taps * cin_pad;
  const long stride = (long)gridDim.x * 256;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    const int ci = (int)(e % cin_pad);
    const long r = e / cin_pad;
    const int t = (int)(r % taps), co = (int)(r / taps);
    out[e] = ci < Cin ? w[((long)co * Cin + ci) * taps + t] : 0.f;
  }
}

int host_scale_exp(float bound) {   // the host-side twin of scale_exp_of (split_f16.h), as in conv_f16x2.hip
  if (!(bound > 0.f)) return 0;
  uint32_t u;
  memcpy(&u, &bound, 4);
  const int s = (int)((u >> 23) & 0xffu) - 127 - 14;
  return s < -100 ? -100 : (s > 100 ? 100 : s);
}

struct Geo {
  int Do, Ho, Wo;
  long M;
};

bool geometry(const MfConv3dDesc* d, Geo* g) {
  const int in[3] = {d->D, d->H, d->W};
  int out[3];
  for (int a = 0; a < 3; ++a) {
    if (d->stride[a] != 1 && d->stride[a] != 2) return false;
    if (d->upsample[a] != 0 && d->upsample[a] != 1) return false;
    if (d->pad[a] < 0 || d->pad[a] >= d->k) return false;
    const int e = in[a] << d->upsample[a];
    const int o = (e + 2 * d->pad[a] - d->k) / d->stride[a] + 1;
    if (in[a] < 1 || e + 2 * d->pad[a] < d->k || o < 1) return false;
    out[a] = o;
  }
  g->Do = out[0]; g->Ho = out[1]; g->Wo = out[2];
  g->M = (long)d->N * out[0] * out[1] * out[2];
  return true;
}

// the checks that make a launch valid (mf_conv3d_ok's contract): returns a message, or null
const char* invalid(const MfConv3dDesc* d, Geo* g) {
  if (!d) return "null descriptor";
  if (d->precision != MF_CONV_FP32_F16X2) return "precision: only MF_CONV_FP32_F16X2 is built in 3-D";
  if (d->N < 1 || d->Cout < 1) return "N and Cout must be >= 1";
  if (d->k != 1 && d->k != 3) return "kernel size must be 1 or 3";
  if (d->C1 < 32 || d->C1 % 32 || d->C2 < 0 || d->C2 % 32) return "C1 >= 32 and C2 >= 0 must be whole 32-channel chunks (zero-pad the operand)";
  if (!geometry(d, g)) return "stride / pad / upsample / size out of range";
  if (g->M >= (1L << 31)) return "too many output voxels";
  if ((long)d->N * d->D * d->H * d->W >= (1L << 31)) return "too many input voxels";
  if (d->tile_hint < 0 || d->tile_hint > 4 || d->splitk_hint < 0 || d->splitk_hint > kMaxSplit) return "tile / split-K hint out of range";
  return nullptr;
}

// tile ids: 1 (64 x 64), 2 (128 x 64), 3 (64 x 128), 4 (128 x 128) voxels x channels; split-K in {1, 2, 4, 8, 16}, at most one slice per
// 8 iterations.  Auto: the widest channel tile Cout fills, the taller voxel tile while there are >= 256 workgroups, then split-K up to ~512.
void plan(const MfConv3dDesc* d, const Geo& g, int* tile, int* splitk) {
  const int nit = (d->C1 + d->C2) / 32 * d->k * d->k * d->k;
  const int tn = d->Cout > 64 ? 2 : 1;
  int tm = 2;
  const long tiles_n = (d->Cout + 64 * tn - 1) / (64 * tn);
  if ((g.M + 127) / 128 * tiles_n < 256) tm = 1;
  int t = d->tile_hint ? d->tile_hint : (tm == 1 ? (tn == 1 ? 1 : 3) : (tn == 1 ? 2 : 4));
  const int bm = (t == 2 || t == 4) ? 128 : 64, bn = (t >= 3) ? 128 : 64;
  const long tiles = (g.M + bm - 1) / bm * ((d->Cout + bn - 1) / bn);
  int s = 1;
  if (d->splitk_hint) {
    s = d->splitk_hint;
  } else {
    while (s < kMaxSplit && tiles * s < 512 && nit / (2 * s) >= 8) s *= 2;
  }
  if (s > nit) s = nit;
  *tile = t;
  *splitk = s;
}

template <int TM, int TN>
void launch_tile(const Conv3dP& p, int grid, hipStream_t s) {
  constexpr size_t lds = 2 * (64 * TM + 64 * TN) * kRowBytes;
  MF_LAUNCH(conv3d_f16x2_kernel<TM, TN>, dim3(grid), dim3(256), lds, s, p);
}

}  // namespace

extern "C" {

int mf_conv3d_ok(const MfConv3dDesc* d) {
  Geo g;
  return invalid(d, &g) == nullptr ? 1 : 0;
}

int mf_conv3d_out_dims(const MfConv3dDesc* d, int32_t* out3) {
  Geo g;
  MF_REQUIRE(d && out3 && geometry(d, &g), MF_EINVAL, "conv3d_out_dims: invalid geometry");
  out3[0] = g.Do; out3[1] = g.Ho; out3[2] = g.Wo;
  return MF_OK;
}

int mf_conv3d_plan_query(const MfConv3dDesc* d, int32_t* tile, int32_t* splitk) {
  Geo g;
  const char* why = invalid(d, &g);
  MF_REQUIRE(!why, MF_EUNSUPPORTED, "conv3d: unsupported descriptor: %s", why);
  int t, s;
  plan(d, g, &t, &s);
  if (tile) *tile = t;
  if (splitk) *splitk = s;
  return MF_OK;
}

size_t mf_conv3d_workspace_bytes(const MfConv3dDesc* d) {
  Geo g;
  if (invalid(d, &g)) return 0;
  int t, s;
  plan(d, g, &t, &s);
  const int nit = (d->C1 + d->C2) / 32 * d->k * d->k * d->k;
  const int per = (nit + s - 1) / s;
  s = (nit + per - 1) / per;
  return s > 1 ? (size_t)s * (size_t)g.M * (size_t)d->Cout * sizeof(float) : 0;
}

int mf_pack_conv3d_weight_f32(const float* w_oidhw, float* out, int Cout, int Cin, int k, int cin_pad, void* stream) {
  MF_REQUIRE(w_oidhw && out && Cout > 0 && Cin > 0 && (k == 1 || k == 3) && cin_pad >= Cin, MF_EINVAL,
             "pack_conv3d_weight: bad arguments Cout=%d Cin=%d k=%d cin_pad=%d", Cout, Cin, k, cin_pad);
  hipStream_t s = (hipStream_t)stream;
  const int taps = k * k * k;
  const long total = (long)Cout * taps * cin_pad;
  const int grid = (int)(total < 256L * 4096 ? (total + 255) / 256 : 4096);
  MF_LAUNCH(pack_conv3d_weight_kernel, dim3(grid), dim3(256), 0, s, w_oidhw, out, Cout, Cin, taps, cin_pad);
  return check_launch("pack_conv3d_weight");
}

int mf_conv3d_f16x2(const void* x1, const void* x2, const void* w, const float* bias, float* y, const float* x1_bound, const float* x2_bound,
                    float w_bound, void* workspace, size_t workspace_bytes, const MfConv3dDesc* d, void* stream) {
  Geo g;
  const char* why = invalid(d, &g);
  MF_REQUIRE(!why, MF_EUNSUPPORTED, "conv3d_f16x2: unsupported descriptor: %s", why);
  MF_REQUIRE(x1 && w && y && (d->C2 == 0 || x2), MF_EINVAL, "conv3d_f16x2: null pointer");
  int tile, s;
  plan(d, g, &tile, &s);
  const int taps = d->k * d->k * d->k;
  Conv3dP p;
  p.x1 = static_cast<const u32x4*>(x1);
  p.x2 = static_cast<const u32x4*>(x2);
  p.w = static_cast<const u32x4*>(w);
  p.bias = bias;
  p.bound1 = x1_bound;
  p.bound2 = x2_bound;
  p.wexp = host_scale_exp(w_bound);
  p.D = d->D; p.H = d->H; p.W = d->W; p.C1 = d->C1; p.C2 = d->C2; p.Cin = d->C1 + d->C2; p.Cout = d->Cout; p.k = d->k; p.taps = taps;
  p.sd = d->stride[0]; p.sh = d->stride[1]; p.sw = d->stride[2];
  p.pd = d->pad[0]; p.ph = d->pad[1]; p.pw = d->pad[2];
  p.ud = d->upsample[0]; p.uh = d->upsample[1]; p.uw = d->upsample[2];
  p.Ho = g.Ho; p.Wo = g.Wo; p.HWo = g.Ho * g.Wo; p.DHWo = g.Do * g.Ho * g.Wo; p.M = (int)g.M;
  p.nit = p.Cin / 32 * taps;
  p.it_per_split = (p.nit + s - 1) / s;
  s = (p.nit + p.it_per_split - 1) / p.it_per_split;   // (no empty slice)
  p.slab = g.M * (long)d->Cout;
  const size_t need = s > 1 ? (size_t)s * (size_t)p.slab * sizeof(float) : 0;
  MF_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), MF_EWORKSPACE, "conv3d_f16x2: workspace %zu < %zu bytes", workspace_bytes, need);
  p.y = s > 1 ? static_cast<float*>(workspace) : y;
  const int bm = (tile == 2 || tile == 4) ? 128 : 64, bn = tile >= 3 ? 128 : 64;
  p.tiles_m = (int)((g.M + bm - 1) / bm);
  p.tiles_n = (d->Cout + bn - 1) / bn;
  const long grid = (long)p.tiles_m * p.tiles_n * s;
  MF_REQUIRE(grid < (1L << 31), MF_EUNSUPPORTED, "conv3d_f16x2: grid too large");
  hipStream_t st = (hipStream_t)stream;
  const double macs = (double)g.M * d->Cout * taps * p.Cin;
  ProfScope ps(MF_FAM_CONV_IGEMM, st, 2.0 * macs, 4.0 * ((double)d->N * d->D * d->H * d->W * p.Cin + (double)d->Cout * taps * p.Cin + (double)p.slab),
               6.0 * macs);
  ps.set_tag(100 + tile, s);
  switch (tile) {
    case 1: launch_tile<1, 1>(p, (int)grid, st); break;
    case 2: launch_tile<2, 1>(p, (int)grid, st); break;
    case 3: launch_tile<1, 2>(p, (int)grid, st); break;
    default: launch_tile<2, 2>(p, (int)grid, st); break;
  }
  if (s > 1) {
    const long total = p.slab;
    const int rg = (int)(total < 256L * 8192 ? (total + 255) / 256 : 8192);
    MF_LAUNCH(conv3d_splitk_reduce_kernel, dim3(rg), dim3(256), 0, st, static_cast<const float*>(workspace), bias, y, total, d->Cout, s);
  }
  return check_launch("conv3d_f16x2");
}

}  // extern "C"
