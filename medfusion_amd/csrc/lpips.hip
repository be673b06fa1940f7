// lpips.hip -- LPIPS v0.1 on the device (include/medfusion_hip.h, "LPIPS"): the scaling layer, the plain layers of a pretrained-CNN trunk the
// implicit-GEMM convolution does not take (a direct convolution, ReLU, max-pool) and the distance of two feature maps of a tap.
// The direct convolution is deliberately simple: one thread per output value, one fp32 fma chain in (kh, kw, cin) order.  The distance is evaluated in
// fp64 on the fp32 features: channel sums and pixel sums in a fixed order, per-workgroup partials in a caller-supplied workspace, no atomics -- a pair's
// bits depend on that pair's feature values only, not on the batch, the pair's place in it or the load path (metrics.hip's rule).
#include "common.h"

#include <math.h>

using namespace mf;

namespace {

constexpr int LANES = 256;
constexpr int GROUP = 16;                    // lanes that share a pixel in the distance kernel: lane g owns the channel quads g, g + 16, ...
constexpr int GROUPS = LANES / GROUP;        // pixels a workgroup has in flight
constexpr long PIX_MIN = 64;                 // pixels per partial, at least
constexpr int PARTS_MAX = 1024;              // partials per pair, at most

int layer_parts(long P) { const long n = (P + PIX_MIN - 1) / PIX_MIN; return (int)(n < PARTS_MAX ? n : PARTS_MAX); }
long layer_chunk(long P) { const int parts = layer_parts(P); return (P + parts - 1) / parts; }

// ---------------------------------------------------------------------------------------------- the scaling layer
// out [2B][H][W][3]: rows [0, B) from x, rows [B, 2B) from y; h_c = fl(fl(v - shift_c) / scale_c), v = fl(2 x - 1) first where asked
__global__ __launch_bounds__(LANES) void lpips_prepare_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out, int B, int C, long HW,
                                                              int normalize, long total) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * LANES + threadIdx.x;      // (row, pixel)
  if (i >= total) return;
  const long row = i / HW, pix = i - row * HW;
  const float* __restrict__ src = row < B ? x + row * C * HW : y + (row - B) * C * HW;
  const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = src[(C == 3 ? c : 0) * HW + pix];
    if (normalize) v = 2.0f * v - 1.0f;
    const float d = v - shift[c];
    out[i * 3 + c] = d / scale[c];
  }
}

// ---------------------------------------------------------------------------------------------- direct convolution, NHWC
struct DirectP {
  const float* x; const float* w; const float* bias; float* y;
  int N, Hin, Win, Cin, Cout, KH, KW, stride, pad, Hout, Wout, relu;
  long total;
};

// one thread per output value (pixel, cout), cout fastest: the lanes of a wave read one input value and consecutive weights ([KH][KW][Cin][Cout])
__global__ __launch_bounds__(LANES) void conv_direct_nhwc_kernel(const DirectP p) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * LANES + threadIdx.x;
  if (idx >= p.total) return;
  const int co = (int)(idx % p.Cout);
  long r = idx / p.Cout;
  const int wo = (int)(r % p.Wout);
  r /= p.Wout;
  const int ho = (int)(r % p.Hout);
  const long n = r / p.Hout;
  float acc = 0.f;
  for (int kh = 0; kh < p.KH; ++kh) {
    const int hi = ho * p.stride - p.pad + kh;
    if (hi < 0 || hi >= p.Hin) continue;
    for (int kw = 0; kw < p.KW; ++kw) {
      const int wi = wo * p.stride - p.pad + kw;
      if (wi < 0 || wi >= p.Win) continue;
      const float* __restrict__ xp = p.x + ((n * p.Hin + hi) * p.Win + wi) * p.Cin;
      const float* __restrict__ wp = p.w + (long)(kh * p.KW + kw) * p.Cin * p.Cout + co;
      for (int ci = 0; ci < p.Cin; ++ci) acc = __builtin_fmaf(xp[ci], wp[(long)ci * p.Cout], acc);
    }
  }
  if (p.bias) acc = acc + p.bias[co];
  if (p.relu) acc = acc < 0.f ? 0.f : acc;
  p.y[idx] = acc;
}

// ---------------------------------------------------------------------------------------------- ReLU in place, max-pool (floor mode, no padding)
__global__ __launch_bounds__(LANES) void relu_kernel(float* __restrict__ x, long n, long nq) {
  const long stride = (long)gridDim.x * LANES;
  const long tid = (long)blockIdx.x * LANES + threadIdx.x;
  for (long i = tid; i < nq; i += stride) {
    float4 v = *reinterpret_cast<float4*>(x + i * 4);
    v.x = v.x < 0.f ? 0.f : v.x, v.y = v.y < 0.f ? 0.f : v.y, v.z = v.z < 0.f ? 0.f : v.z, v.w = v.w < 0.f ? 0.f : v.w;
    *reinterpret_cast<float4*>(x + i * 4) = v;
  }
  for (long i = nq * 4 + tid; i < n; i += stride) x[i] = x[i] < 0.f ? 0.f : x[i];
}

__global__ __launch_bounds__(LANES) void maxpool_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C, int Ho, int Wo, int k, int s, long total) {
  const long idx = (long)blockIdx.x * LANES + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  long r = idx / C;
  const int wo = (int)(r % Wo);
  r /= Wo;
  const int ho = (int)(r % Ho);
  const long n = r / Ho;
  float m = -INFINITY;
  for (int dy = 0; dy < k; ++dy)
    for (int dx = 0; dx < k; ++dx) {     // (floor mode: every window lies inside the image)
      const float v = x[((n * H + ho * s + dy) * W + wo * s + dx) * C + c];
      if (v > m || v != v) m = v;         // a NaN wins, as in F.max_pool2d
    }
  y[idx] = m;
}

// ---------------------------------------------------------------------------------------------- the distance of two feature maps of a tap
__device__ __forceinline__ double group_sum(double v) {      // the 16 lanes of a pixel: a butterfly (a + b == b + a: every lane ends with the same bits)
#pragma unroll
  for (int s = GROUP / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, GROUP);
  return v;
}

template <bool V>
__device__ __forceinline__ void load_quad(const float* __restrict__ p, int c, int C, float (&v)[4]) {
  if (V) {
    const float4 q = *reinterpret_cast<const float4*>(p + c);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = c + j < C ? p[c + j] : 0.f;
  }
}

// grid (parts, B): workgroup (p, b) takes pixels [p chunk, (p + 1) chunk) of pair b; the 16 lanes of group k take the pixels k, k + 16, ... of that span.
// V: 16-byte loads; else element by element -- the same channels in the same lanes in the same order.
template <bool V>
__global__ __launch_bounds__(LANES) void lpips_layer_kernel(const float* __restrict__ fx, const float* __restrict__ fy, const float* __restrict__ w, double* __restrict__ part,
                                                            long P, int C, long chunk, int parts) {
  __shared__ double red[GROUPS];
  const int b = blockIdx.y, p = blockIdx.x;
  const int grp = threadIdx.x / GROUP, g = threadIdx.x % GROUP;
  const long start = (long)p * chunk;
  const long end = start + chunk < P ? start + chunk : P;
  const float* __restrict__ xa = fx + (long)b * P * C;
  const float* __restrict__ xb = fy + (long)b * P * C;
  double acc = 0.0;
  for (long base = start; base < end; base += GROUPS) {      // (uniform trip count: the butterfly runs with every lane of the wave)
    const long pix = base + grp;
    const bool live = pix < end;
    const float* __restrict__ pa = xa + (live ? pix : start) * C;
    const float* __restrict__ pb = xb + (live ? pix : start) * C;
    double sa = 0.0, sb = 0.0;
    for (int c = 4 * g; c < C; c += 4 * GROUP) {
      float a[4], bb[4];
      load_quad<V>(pa, c, C, a);
      load_quad<V>(pb, c, C, bb);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sa += (double)a[j] * (double)a[j];
        sb += (double)bb[j] * (double)bb[j];
      }
    }
    const double ra = 1.0 / (sqrt(group_sum(sa)) + 1e-10), rb = 1.0 / (sqrt(group_sum(sb)) + 1e-10);
    double d = 0.0;
    for (int c = 4 * g; c < C; c += 4 * GROUP) {
      float a[4], bb[4], ww[4];
      load_quad<V>(pa, c, C, a);
      load_quad<V>(pb, c, C, bb);
      load_quad<false>(w, c, C, ww);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double e = (double)a[j] * ra - (double)bb[j] * rb;
        d += (double)ww[j] * (e * e);
      }
    }
    d = group_sum(d);
    if (live) acc += d;
  }
  if (g == 0) red[grp] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < GROUPS; ++k) s += red[k];
    part[(long)b * parts + p] = s;
  }
}

// one thread per pair: its partials in ascending order, the mean over the pixels; with `total` the sum of the pair's terms in ascending order
__global__ __launch_bounds__(64) void lpips_finish_kernel(const double* __restrict__ part, double* __restrict__ terms, float* __restrict__ total, int B, int parts, long P, int layer,
                                                          int layers) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int i = 0; i < parts; ++i) s += part[(long)b * parts + i];
  terms[(long)b * layers + layer] = s / (double)P;
  if (total) {
    double t = 0.0;
    for (int l = 0; l < layers; ++l) t += terms[(long)b * layers + l];
    total[b] = (float)t;
  }
}

}  // namespace

extern "C" {

int mf_lpips_min_side(int net) { return net == MF_LPIPS_VGG ? 16 : net == MF_LPIPS_ALEX ? 31 : 0; }

int mf_lpips_prepare_f32(const float* x, const float* y, float* out, int B, int C, int H, int W, int normalize, int net, void* stream) {
  MF_REQUIRE(x && y && out, MF_EINVAL, "lpips_prepare: null pointer");
  MF_REQUIRE(net == MF_LPIPS_VGG || net == MF_LPIPS_ALEX, MF_EINVAL, "lpips_prepare: net %d", net);
  MF_REQUIRE(C == 1 || C == 3, MF_EINVAL, "lpips_prepare: C = %d, 1 or 3 channels", C);
  MF_REQUIRE(B > 0 && H >= mf_lpips_min_side(net) && W >= mf_lpips_min_side(net), MF_EINVAL, "lpips_prepare: B = %d, sides %d x %d (at least %d)", B, H, W,
             mf_lpips_min_side(net));
  const long HW = (long)H * W, total = 2L * B * HW;
  MF_REQUIRE((total + LANES - 1) / LANES < (1L << 31), MF_EUNSUPPORTED, "lpips_prepare: problem too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 6.0 * total, 4.0 * total * (C + 3));
  MF_LAUNCH(lpips_prepare_kernel, dim3((unsigned)((total + LANES - 1) / LANES)), dim3(LANES), 0, s, x, y, out, B, C, HW, normalize ? 1 : 0, total);
  return check_launch("lpips_prepare");
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

int mf_conv2d_direct_f32(const float* x, const float* w_hwio, const float* bias, float* y, const MfDirectConvDesc* d, void* stream) {
  int32_t hw[2];
  const int rc = mf_conv2d_direct_out_dims(d, hw);
  if (rc) return rc;
  MF_REQUIRE(x && w_hwio && y, MF_EINVAL, "conv2d_direct: null pointer");
  DirectP p;
  p.x = x, p.w = w_hwio, p.bias = bias, p.y = y;
  p.N = d->N, p.Hin = d->Hin, p.Win = d->Win, p.Cin = d->Cin, p.Cout = d->Cout, p.KH = d->KH, p.KW = d->KW, p.stride = d->stride, p.pad = d->pad;
  p.Hout = hw[0], p.Wout = hw[1], p.relu = d->relu ? 1 : 0;
  p.total = (long)d->N * hw[0] * hw[1] * d->Cout;
  const long blocks = (p.total + LANES - 1) / LANES;
  MF_REQUIRE(blocks < (1L << 31) && (long)d->N * d->Hin * d->Win * d->Cin < (1L << 40), MF_EUNSUPPORTED, "conv2d_direct: problem too large");
  hipStream_t s = (hipStream_t)stream;
  const double K = (double)d->KH * d->KW * d->Cin;
  ProfScope ps(MF_FAM_CONV_DIRECT, s, 2.0 * p.total * K, 4.0 * ((double)d->N * d->Hin * d->Win * d->Cin + K * d->Cout + (double)p.total));
  MF_LAUNCH(conv_direct_nhwc_kernel, dim3((unsigned)blocks), dim3(LANES), 0, s, p);
  return check_launch("conv2d_direct");
}

int mf_relu_f32(float* x, int64_t n, void* stream) {
  MF_REQUIRE(x && n > 0, MF_EINVAL, "relu: bad args");
  const long nq = ((uintptr_t)x & 15) == 0 ? (long)n / 4 : 0;
  long blocks = ((nq ? nq : (long)n) + LANES - 1) / LANES;
  if (blocks > 4096) blocks = 4096;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, (double)n, 8.0 * n);
  MF_LAUNCH(relu_kernel, dim3((unsigned)blocks), dim3(LANES), 0, s, x, (long)n, nq);
  return check_launch("relu");
}

int mf_maxpool_nhwc_f32(const float* x, float* y, int N, int H, int W, int C, int k, int stride, void* stream) {
  MF_REQUIRE(x && y, MF_EINVAL, "maxpool: null pointer");
  MF_REQUIRE((k == 2 && stride == 2) || (k == 3 && stride == 2), MF_EINVAL, "maxpool: window %d stride %d ((2, 2) or (3, 2))", k, stride);
  MF_REQUIRE(N > 0 && C > 0 && H >= k && W >= k, MF_EINVAL, "maxpool: bad dims (sides of at least the window)");
  const int Ho = (H - k) / stride + 1, Wo = (W - k) / stride + 1;
  const long total = (long)N * Ho * Wo * C;
  const long blocks = (total + LANES - 1) / LANES;
  MF_REQUIRE(blocks < (1L << 31), MF_EUNSUPPORTED, "maxpool: problem too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, (double)total * k * k, 4.0 * ((double)N * H * W * C + (double)total));
  MF_LAUNCH(maxpool_nhwc_kernel, dim3((unsigned)blocks), dim3(LANES), 0, s, x, y, H, W, C, Ho, Wo, k, stride, total);
  return check_launch("maxpool");
}

int mf_lpips_layer_parts(int64_t P) { return P > 0 ? layer_parts((long)P) : 0; }

size_t mf_lpips_workspace_bytes(int B, int64_t P) {
  if (B <= 0 || P <= 0) return 0;
  return (size_t)B * (size_t)layer_parts((long)P) * sizeof(double);
}

int mf_lpips_layer_f32(const float* fx, const float* fy, const float* w, void* workspace, size_t workspace_bytes, int B, int64_t P, int C, void* stream) {
  MF_REQUIRE(fx && fy && w && workspace, MF_EINVAL, "lpips_layer: null pointer");
  MF_REQUIRE(B > 0 && B <= 65535 && P > 0 && C > 0, MF_EINVAL, "lpips_layer: bad sizes (1 .. 65535 pairs)");
  MF_REQUIRE(((uintptr_t)workspace & 7) == 0, MF_EINVAL, "lpips_layer: workspace must be 8-byte aligned");
  MF_REQUIRE(workspace_bytes >= mf_lpips_workspace_bytes(B, P), MF_EWORKSPACE, "lpips_layer: workspace of %zu bytes, %zu needed", workspace_bytes,
             mf_lpips_workspace_bytes(B, P));
  const bool vec = (((uintptr_t)fx | (uintptr_t)fy) & 15) == 0 && C % 4 == 0;
  const int parts = layer_parts((long)P);
  const long chunk = layer_chunk((long)P);
  hipStream_t s = (hipStream_t)stream;
  const double n = (double)B * P * C;
  ProfScope ps(MF_FAM_MISC, s, 10.0 * n, 8.0 * n);
  double* part = reinterpret_cast<double*>(workspace);
  if (vec) {
    MF_LAUNCH(lpips_layer_kernel<true>, dim3(parts, B), dim3(LANES), 0, s, fx, fy, w, part, (long)P, C, chunk, parts);
  } else {
    MF_LAUNCH(lpips_layer_kernel<false>, dim3(parts, B), dim3(LANES), 0, s, fx, fy, w, part, (long)P, C, chunk, parts);
  }
  return check_launch("lpips_layer");
}

int mf_lpips_finish_f32(const void* workspace, double* terms, float* total, int B, int64_t P, int layer, int layers, void* stream) {
  MF_REQUIRE(workspace && terms && B > 0 && B <= 65535 && P > 0, MF_EINVAL, "lpips_finish: bad args");
  MF_REQUIRE(layers > 0 && layer >= 0 && layer < layers, MF_EINVAL, "lpips_finish: layer %d of %d", layer, layers);
  MF_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)terms & 7) == 0, MF_EINVAL, "lpips_finish: workspace and terms must be 8-byte aligned");
  MF_LAUNCH(lpips_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const double*>(workspace), terms, total, B,
            layer_parts((long)P), (long)P, layer, layers);
  return check_launch("lpips_finish");
}

}  // extern "C"
