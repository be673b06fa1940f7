// cnn_layers.hip -- the plain layers of a CNN trunk on the device, NHWC fp32, shared by LPIPS and Inception (include/medfusion_hip.h, "LPIPS" and
// "Inception"): ONE general tiled implicit-GEMM convolution on the fp32 matrix cores (mf_conv2d_gemm_f32; mf_conv2d_direct_f32 is the same kernel with
// one padding and one chain), ONE pool (window 2 or 3: mf_pool2d_nhwc_f32, mf_maxpool_nhwc_f32) and the ReLU in place.
// The convolution: C[M][N] = A[M][K] B[K][N] with M the output pixels of the whole batch, N = Cout and K = (kh, kw, cin) flattened -- which is the
// row index of the [KH][KW][Cin][Cout] weights as they lie in memory.  A workgroup of four waves owns a TM x TN tile of C and walks ALL of K in chunks
// of 32 through LDS (two buffers, one barrier per chunk, the next chunk's global loads in flight while this one is multiplied): K is never split
// across workgroups, so an output value is one fmaf chain over k ascending (v_mfma_f32_32x32x2_f32 is that chain: tests/test_fidelity_gpu.py) whatever
// the tile, the grid, the batch or the load path.  Padding taps, k >= K, pixels >= M and channels >= Cout are staged as zeros -- fmaf(0, 0, acc) = acc,
// and an accumulator that starts at +0 never becomes -0, so on finite data the zeros leave no trace in the bits (a non-finite weight under a padding
// tap makes a NaN).
#include "common.h"

#include <math.h>

using namespace mf;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int BK = 32;                       // k per staged chunk; a chain piece is a whole number of chunks
constexpr int CUS = 256;                     // the planner's picture of the device: 256 compute units, two workgroups resident on each

struct GemmP {
  const float* x; const float* w; const float* bias; float* y;
  int Hin, Win, Cin, Cout, KW, stride, pad_h, pad_w, Hout, Wout, relu, ldy, y_offset;
  int K, chunks, piece;                      // KH KW Cin; ceil(K / BK); chunks per chain piece (0: one chain)
  long M;                                    // N Hout Wout
};

// Staged images: As [BK][TM] and Bs [BK][TN], k-major, so that the 32 lanes of a half wave read 32 consecutive floats of one k row -- lane (i, h) of
// the wave takes A[i][2 s + h] and B[2 s + h][i] for matrix instruction s of the chunk: k ascending.  Thread t stages ONE pixel (t % TM) of A and ONE
// group of V output channels (t % (TN / V)) of B in every chunk: the pixel's coordinates are decoded once.  V = 4: sixteen-byte loads (Cin % 4 == 0:
// a group of four k lies inside one tap; Cout % 4 == 0: a group of channels is inside or outside as a whole); V = 1: element by element -- the same
// values either way.  Every load is issued unconditionally from an address clamped into the tensor and masked afterwards by a select.
template <int WM, int WN, int V>
__global__ __launch_bounds__(THREADS) void conv_gemm_kernel(const GemmP p) {
  constexpr int TM = 64 * WM, TN = 64 * WN;
  constexpr int GA = TM * BK / V / THREADS, GB = TN * BK / V / THREADS;      // groups per thread and chunk
  constexpr int SA = THREADS / TM, CG = TN / V, SB = THREADS / CG;           // k groups (A) / k rows (B) between a thread's consecutive groups
  constexpr int BUF = BK * (TM + TN);
  __shared__ __attribute__((aligned(16))) float smem[2 * BUF];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave >> 1, wc = wave & 1, j = lane & 31, h = lane >> 5;

  // A: this thread's pixel
  const int arow = t % TM, akg = t / TM;
  const long m = (long)blockIdx.x * TM + arow;
  const bool row_in = m < p.M;
  const long mm = row_in ? m : 0;
  const int wo = (int)(mm % p.Wout);
  const long mr = mm / p.Wout;
  const int ho = (int)(mr % p.Hout);
  const long n_img = mr / p.Hout;
  const int hi0 = ho * p.stride - p.pad_h, wi0 = wo * p.stride - p.pad_w;
  const float* __restrict__ xn = p.x + n_img * p.Hin * p.Win * p.Cin;
  // B: this thread's output channels
  const int bcg = t % CG, bkr = t / CG;
  const int co0 = blockIdx.y * TN + bcg * V;
  const bool co_in = co0 < p.Cout;

  float ra[GA][V], rb[GB][V];
  auto load_chunk = [&](int k0) {
#pragma unroll
    for (int q = 0; q < GA; ++q) {
      const int k = k0 + (akg + SA * q) * V;
      const int kc = min(k, p.K - V);
      const int tap = kc / p.Cin, ci = kc - tap * p.Cin;
      const int kh = tap / p.KW, kw = tap - kh * p.KW;
      const int hi = hi0 + kh, wi = wi0 + kw;
      const bool in = row_in && k < p.K && hi >= 0 && hi < p.Hin && wi >= 0 && wi < p.Win;
      const float* __restrict__ src = xn + (in ? ((long)hi * p.Win + wi) * p.Cin + ci : 0L);
      if constexpr (V == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
        for (int e = 0; e < V; ++e) ra[q][e] = in ? v[e] : 0.f;
      } else {
        const float v = *src;
        ra[q][0] = in ? v : 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < GB; ++q) {
      const int k = k0 + bkr + SB * q;
      const bool in = co_in && k < p.K;
      const float* __restrict__ src = p.w + (in ? (long)k * p.Cout + co0 : 0L);
      if constexpr (V == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
        for (int e = 0; e < V; ++e) rb[q][e] = in ? v[e] : 0.f;
      } else {
        const float v = *src;
        rb[q][0] = in ? v : 0.f;
      }
    }
  };
  auto store_chunk = [&](float* __restrict__ dst) {
#pragma unroll
    for (int q = 0; q < GA; ++q)
#pragma unroll
      for (int e = 0; e < V; ++e) dst[((akg + SA * q) * V + e) * TM + arow] = ra[q][e];
    float* __restrict__ db = dst + BK * TM;
#pragma unroll
    for (int q = 0; q < GB; ++q) {
      float* d = db + (bkr + SB * q) * TN + bcg * V;
      if constexpr (V == 4) {
        *reinterpret_cast<f32x4*>(d) = f32x4{rb[q][0], rb[q][1], rb[q][2], rb[q][3]};
      } else {
        d[0] = rb[q][0];
      }
    }
  };

  f32x16 acc[WM][WN], tot[WM][WN];
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int b = 0; b < WN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f, tot[a][b][r] = 0.f;

  load_chunk(0);
  store_chunk(smem);
  __syncthreads();
  int in_piece = 0;
  for (int c = 0; c < p.chunks; ++c) {
    const float* cur = smem + (c & 1) * BUF;
    const bool more = c + 1 < p.chunks;
    if (more) load_chunk((c + 1) * BK);
    const float* As = cur + wr * (32 * WM) + j;
    const float* Bs = cur + BK * TM + wc * (32 * WN) + j;
#pragma unroll
    for (int s = 0; s < BK / 2; ++s) {
      const int kk = 2 * s + h;
      float fa[WM], fb[WN];
#pragma unroll
      for (int a = 0; a < WM; ++a) fa[a] = As[kk * TM + 32 * a];
#pragma unroll
      for (int b = 0; b < WN; ++b) fb[b] = Bs[kk * TN + 32 * b];
#pragma unroll
      for (int a = 0; a < WM; ++a)
#pragma unroll
        for (int b = 0; b < WN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    // a chain piece ends here: it joins the sum of the pieces before it, and the next piece starts from +0
    if (p.piece && ++in_piece == p.piece && more) {
      in_piece = 0;
#pragma unroll
      for (int a = 0; a < WM; ++a)
#pragma unroll
        for (int b = 0; b < WN; ++b) {
          tot[a][b] = tot[a][b] + acc[a][b];
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
        }
    }
    if (more) store_chunk(smem + ((c + 1) & 1) * BUF);
    __syncthreads();
  }

  // the lane's column is lane & 31, register r is row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int b = 0; b < WN; ++b) {
    const int co = blockIdx.y * TN + wc * (32 * WN) + 32 * b + j;
    const float bv = (p.bias && co < p.Cout) ? p.bias[co] : 0.f;
#pragma unroll
    for (int a = 0; a < WM; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long gm = (long)blockIdx.x * TM + wr * (32 * WM) + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * h;
        float v = p.piece ? tot[a][b][r] + acc[a][b][r] : acc[a][b][r];
        if (p.bias) v = v + bv;
        if (p.relu) v = v < 0.f ? 0.f : v;
        if (gm < p.M && co < p.Cout) p.y[gm * p.ldy + p.y_offset + co] = v;
      }
  }
}

constexpr int TILES = 3;
constexpr int TILE_M[TILES + 1] = {0, 128, 128, 64}, TILE_N[TILES + 1] = {0, 128, 64, 64};

// The tile of a layer: the one whose launch takes the fewest rounds of the device times its area (two workgroups per compute unit make a round); a
// smaller tile pays for its poorer operand reuse with an eighth of its time.  Host arithmetic on (M, Cout) only; no output bit depends on it.
int pick_tile(long M, int Cout) {
  int best = 1;
  double best_cost = 0.0;
  for (int id = 1; id <= TILES; ++id) {
    const double wg = (double)((M + TILE_M[id] - 1) / TILE_M[id]) * ((Cout + TILE_N[id] - 1) / TILE_N[id]);
    const double rounds = ceil(wg / (2.0 * CUS));
    const double cost = rounds * TILE_M[id] * TILE_N[id] * (1.0 + 0.125 * (id - 1) / 2.0);
    if (id == 1 || cost < best_cost) best = id, best_cost = cost;
  }
  return best;
}

int gemm_check(const MfGemmConvDesc* d, int32_t* hw) {
  MF_REQUIRE(d, MF_EINVAL, "conv2d_gemm: null descriptor");
  MF_REQUIRE(d->N > 0 && d->Hin > 0 && d->Win > 0 && d->Cin > 0 && d->Cout > 0, MF_EINVAL, "conv2d_gemm: bad dims");
  MF_REQUIRE(d->KH >= 1 && d->KH <= 11 && d->KW >= 1 && d->KW <= 11, MF_EINVAL, "conv2d_gemm: kernel %dx%d (1 .. 11)", d->KH, d->KW);
  MF_REQUIRE(d->stride >= 1 && d->stride <= 4 && d->pad_h >= 0 && d->pad_w >= 0, MF_EINVAL, "conv2d_gemm: stride %d (1 .. 4), pad %d, %d", d->stride, d->pad_h, d->pad_w);
  MF_REQUIRE(d->chain >= 0 && d->tile >= 0 && d->tile <= TILES && d->reserved == 0, MF_EINVAL, "conv2d_gemm: chain %d (>= 0), tile %d (0 .. %d), reserved must be 0", d->chain,
             d->tile, TILES);
  MF_REQUIRE(d->y_offset >= 0 && (d->ldy == 0 ? d->y_offset == 0 : (long)d->ldy >= (long)d->y_offset + d->Cout), MF_EINVAL,
             "conv2d_gemm: ldy %d, y_offset %d: the slice [y_offset, y_offset + Cout) must lie inside a pixel's ldy channels (ldy 0: dense)", d->ldy, d->y_offset);
  const long ho = ((long)d->Hin + 2L * d->pad_h - d->KH) / d->stride + 1, wo = ((long)d->Win + 2L * d->pad_w - d->KW) / d->stride + 1;
  MF_REQUIRE((long)d->Hin + 2L * d->pad_h >= d->KH && (long)d->Win + 2L * d->pad_w >= d->KW && ho > 0 && wo > 0 && ho < (1L << 30) && wo < (1L << 30), MF_EINVAL,
             "conv2d_gemm: empty output");
  hw[0] = (int32_t)ho, hw[1] = (int32_t)wo;
  return MF_OK;
}

template <int WM, int WN>
void gemm_launch(const GemmP& p, bool vec, dim3 grid, hipStream_t s) {
  if (vec) {
    MF_LAUNCH((conv_gemm_kernel<WM, WN, 4>), grid, dim3(THREADS), 0, s, p);
  } else {
    MF_LAUNCH((conv_gemm_kernel<WM, WN, 1>), grid, dim3(THREADS), 0, s, p);
  }
}

// ---------------------------------------------------------------------------------------------- the pools, NHWC, window KS x KS (2 or 3)
// one thread per output value (pixel, c), c fastest.  max: the largest valid tap, a NaN wins; avg: the fp32 sum of the valid taps in ascending (kh, kw)
// order, divided once by their number
template <int KS>
__global__ __launch_bounds__(THREADS) void pool_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C, int Ho, int Wo, int stride, int pad, int mode,
                                                            int ldy, int y_offset, long total) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  long r = idx / C;
  const long pix = r;
  const int wo = (int)(r % Wo);
  r /= Wo;
  const int ho = (int)(r % Ho);
  const long n = r / Ho;
  float mx = -INFINITY, sum = 0.f;
  int cnt = 0;
  for (int kh = 0; kh < KS; ++kh) {
    const int hi = ho * stride - pad + kh;
    if (hi < 0 || hi >= H) continue;
    for (int kw = 0; kw < KS; ++kw) {
      const int wi = wo * stride - pad + kw;
      if (wi < 0 || wi >= W) continue;
      const float v = x[((n * H + hi) * W + wi) * C + c];
      if (v > mx || v != v) mx = v;
      sum = sum + v;
      ++cnt;
    }
  }
  y[pix * ldy + y_offset + c] = mode == MF_POOL_MAX ? mx : sum / (float)cnt;
}

// ---------------------------------------------------------------------------------------------- ReLU in place
__global__ __launch_bounds__(THREADS) void relu_kernel(float* __restrict__ x, long n, long nq) {
  const long stride = (long)gridDim.x * THREADS;
  const long tid = (long)blockIdx.x * THREADS + threadIdx.x;
  for (long i = tid; i < nq; i += stride) {
    float4 v = *reinterpret_cast<float4*>(x + i * 4);
    v.x = v.x < 0.f ? 0.f : v.x, v.y = v.y < 0.f ? 0.f : v.y, v.z = v.z < 0.f ? 0.f : v.z, v.w = v.w < 0.f ? 0.f : v.w;
    *reinterpret_cast<float4*>(x + i * 4) = v;
  }
  for (long i = nq * 4 + tid; i < n; i += stride) x[i] = x[i] < 0.f ? 0.f : x[i];
}

}  // namespace

extern "C" {

int mf_conv2d_gemm_out_dims(const MfGemmConvDesc* d, int32_t* out2) {
  MF_REQUIRE(out2, MF_EINVAL, "conv2d_gemm: null pointer");
  return gemm_check(d, out2);
}

int mf_conv2d_gemm_plan(const MfGemmConvDesc* d, int32_t* out2) {
  MF_REQUIRE(out2, MF_EINVAL, "conv2d_gemm: null pointer");
  int32_t hw[2];
  const int rc = gemm_check(d, hw);
  if (rc) return rc;
  const long M = (long)d->N * hw[0] * hw[1];
  const int tile = d->tile ? d->tile : pick_tile(M, d->Cout);
  const long wg = ((M + TILE_M[tile] - 1) / TILE_M[tile]) * ((d->Cout + TILE_N[tile] - 1) / TILE_N[tile]);
  MF_REQUIRE(wg < (1L << 31), MF_EUNSUPPORTED, "conv2d_gemm: problem too large");
  out2[0] = tile, out2[1] = (int32_t)wg;
  return MF_OK;
}

int mf_conv2d_gemm_f32(const float* x, const float* w_hwio, const float* bias, float* y, const MfGemmConvDesc* d, void* stream) {
  int32_t hw[2];
  const int rc = gemm_check(d, hw);
  if (rc) return rc;
  MF_REQUIRE(x && w_hwio && y, MF_EINVAL, "conv2d_gemm: null pointer");
  GemmP p;
  p.x = x, p.w = w_hwio, p.bias = bias, p.y = y;
  p.Hin = d->Hin, p.Win = d->Win, p.Cin = d->Cin, p.Cout = d->Cout, p.KW = d->KW, p.stride = d->stride, p.pad_h = d->pad_h, p.pad_w = d->pad_w;
  p.Hout = hw[0], p.Wout = hw[1], p.relu = d->relu ? 1 : 0;
  p.ldy = d->ldy ? d->ldy : d->Cout, p.y_offset = d->y_offset;
  const long K = (long)d->KH * d->KW * d->Cin;
  p.M = (long)d->N * hw[0] * hw[1];
  MF_REQUIRE(K < (1L << 30) && (long)d->N * d->Hin * d->Win * d->Cin < (1L << 40) && p.M * p.ldy < (1L << 40) && K * d->Cout < (1L << 40), MF_EUNSUPPORTED,
             "conv2d_gemm: problem too large");
  p.K = (int)K, p.chunks = (int)((K + BK - 1) / BK);
  p.piece = d->chain ? (int)(((long)d->chain + BK - 1) / BK) : 0;
  const int tile = d->tile ? d->tile : pick_tile(p.M, d->Cout);
  const long gx = (p.M + TILE_M[tile] - 1) / TILE_M[tile], gy = (d->Cout + TILE_N[tile] - 1) / TILE_N[tile];
  MF_REQUIRE(gx < (1L << 31) && gy < 65536, MF_EUNSUPPORTED, "conv2d_gemm: problem too large");
  const bool vec = d->Cin % 4 == 0 && d->Cout % 4 == 0 && (((uintptr_t)x | (uintptr_t)w_hwio) & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  ProfScope ps(MF_FAM_CONV_IGEMM, s, 2.0 * p.M * d->Cout * (double)K, 4.0 * ((double)d->N * d->Hin * d->Win * d->Cin + (double)K * d->Cout + (double)p.M * d->Cout),
               2.0 * (double)gx * TILE_M[tile] * (double)gy * TILE_N[tile] * (double)p.chunks * BK);
  if (tile == 1) gemm_launch<2, 2>(p, vec, grid, s);
  else if (tile == 2) gemm_launch<2, 1>(p, vec, grid, s);
  else gemm_launch<1, 1>(p, vec, grid, s);
  return check_launch("conv2d_gemm");
}

int mf_conv2d_direct_out_dims(const MfDirectConvDesc* d, int32_t* out2) {
  MF_REQUIRE(d && out2, MF_EINVAL, "conv2d_direct: null pointer");
  MF_REQUIRE(d->N > 0 && d->Hin > 0 && d->Win > 0 && d->Cin > 0 && d->Cout > 0, MF_EINVAL, "conv2d_direct: bad dims");
  MF_REQUIRE(d->KH >= 1 && d->KH <= 11 && d->KW >= 1 && d->KW <= 11, MF_EINVAL, "conv2d_direct: kernel %dx%d (1 .. 11)", d->KH, d->KW);
  MF_REQUIRE(d->stride >= 1 && d->stride <= 4 && d->pad >= 0, MF_EINVAL, "conv2d_direct: stride %d (1 .. 4), pad %d", d->stride, d->pad);
  MF_REQUIRE(d->reserved == 0, MF_EINVAL, "conv2d_direct: reserved must be 0");
  const long ho = ((long)d->Hin + 2L * d->pad - d->KH) / d->stride + 1, wo = ((long)d->Win + 2L * d->pad - d->KW) / d->stride + 1;
  MF_REQUIRE((long)d->Hin + 2L * d->pad >= d->KH && (long)d->Win + 2L * d->pad >= d->KW && ho > 0 && wo > 0 && ho < (1L << 30) && wo < (1L << 30), MF_EINVAL,
             "conv2d_direct: empty output");
  out2[0] = (int32_t)ho, out2[1] = (int32_t)wo;
  return MF_OK;
}

// the general convolution with one padding for both axes, one chain, the planner's tile and a dense output
int mf_conv2d_direct_f32(const float* x, const float* w_hwio, const float* bias, float* y, const MfDirectConvDesc* d, void* stream) {
  int32_t hw[2];
  const int rc = mf_conv2d_direct_out_dims(d, hw);
  if (rc) return rc;
  MF_REQUIRE(x && w_hwio && y, MF_EINVAL, "conv2d_direct: null pointer");
  MF_REQUIRE(((long)d->N * hw[0] * hw[1] * d->Cout + THREADS - 1) / THREADS < (1L << 31) && (long)d->N * d->Hin * d->Win * d->Cin < (1L << 40), MF_EUNSUPPORTED,
             "conv2d_direct: problem too large");
  MfGemmConvDesc g = {};
  g.N = d->N, g.Hin = d->Hin, g.Win = d->Win, g.Cin = d->Cin, g.Cout = d->Cout, g.KH = d->KH, g.KW = d->KW, g.stride = d->stride;
  g.pad_h = g.pad_w = d->pad, g.relu = d->relu;
  return mf_conv2d_gemm_f32(x, w_hwio, bias, y, &g, stream);
}

int mf_pool2d_nhwc_f32(const float* x, float* y, int N, int H, int W, int C, int stride, int pad, int mode, int ldy, int y_offset, void* stream) {
  MF_REQUIRE(x && y, MF_EINVAL, "pool2d: null pointer");
  MF_REQUIRE((stride == 1 || stride == 2) && (pad == 0 || pad == 1), MF_EINVAL, "pool2d: stride %d (1 or 2), pad %d (0 or 1)", stride, pad);
  MF_REQUIRE(mode == MF_POOL_MAX || mode == MF_POOL_AVG_VALID, MF_EINVAL, "pool2d: mode %d", mode);
  MF_REQUIRE(N > 0 && C > 0 && H + 2 * pad >= 3 && W + 2 * pad >= 3 && H > 0 && W > 0, MF_EINVAL, "pool2d: bad dims (padded sides of at least the window of 3)");
  MF_REQUIRE(y_offset >= 0 && (ldy == 0 ? y_offset == 0 : (long)ldy >= (long)y_offset + C), MF_EINVAL, "pool2d: ldy %d, y_offset %d: the slice must lie inside a pixel's ldy channels", ldy,
             y_offset);
  const int Ho = (H + 2 * pad - 3) / stride + 1, Wo = (W + 2 * pad - 3) / stride + 1;
  const long total = (long)N * Ho * Wo * C;
  const long blocks = (total + THREADS - 1) / THREADS;
  MF_REQUIRE(blocks < (1L << 31), MF_EUNSUPPORTED, "pool2d: problem too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 9.0 * total, 4.0 * ((double)N * H * W * C + (double)total));
  MF_LAUNCH(pool_nhwc_kernel<3>, dim3((unsigned)blocks), dim3(THREADS), 0, s, x, y, H, W, C, Ho, Wo, stride, pad, mode, ldy ? ldy : C, y_offset, total);
  return check_launch("pool2d");
}

// the pool above without padding, max, dense output (floor mode: every window lies inside the image)
int mf_maxpool_nhwc_f32(const float* x, float* y, int N, int H, int W, int C, int k, int stride, void* stream) {
  MF_REQUIRE(x && y, MF_EINVAL, "maxpool: null pointer");
  MF_REQUIRE((k == 2 && stride == 2) || (k == 3 && stride == 2), MF_EINVAL, "maxpool: window %d stride %d ((2, 2) or (3, 2))", k, stride);
  MF_REQUIRE(N > 0 && C > 0 && H >= k && W >= k, MF_EINVAL, "maxpool: bad dims (sides of at least the window)");
  const int Ho = (H - k) / stride + 1, Wo = (W - k) / stride + 1;
  const long total = (long)N * Ho * Wo * C;
  const long blocks = (total + THREADS - 1) / THREADS;
  MF_REQUIRE(blocks < (1L << 31), MF_EUNSUPPORTED, "maxpool: problem too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, (double)total * k * k, 4.0 * ((double)N * H * W * C + (double)total));
  if (k == 2) {
    MF_LAUNCH(pool_nhwc_kernel<2>, dim3((unsigned)blocks), dim3(THREADS), 0, s, x, y, H, W, C, Ho, Wo, stride, 0, MF_POOL_MAX, C, 0, total);
  } else {
    MF_LAUNCH(pool_nhwc_kernel<3>, dim3((unsigned)blocks), dim3(THREADS), 0, s, x, y, H, W, C, Ho, Wo, stride, 0, MF_POOL_MAX, C, 0, total);
  }
  return check_launch("maxpool");
}

int mf_relu_f32(float* x, int64_t n, void* stream) {
  MF_REQUIRE(x && n > 0, MF_EINVAL, "relu: bad args");
  const long nq = ((uintptr_t)x & 15) == 0 ? (long)n / 4 : 0;
  long blocks = ((nq ? nq : (long)n) + THREADS - 1) / THREADS;
  if (blocks > 4096) blocks = 4096;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, (double)n, 8.0 * n);
  MF_LAUNCH(relu_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, x, (long)n, nq);
  return check_launch("relu");
}

}  // extern "C"
