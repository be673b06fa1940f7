// lpips.hip -- LPIPS v0.1 on the device (include/medfusion_hip.h, "LPIPS"): the scaling layer and the distance of two feature maps of a tap.  The
// trunk's plain layers (mf_conv2d_direct_f32, mf_relu_f32, mf_maxpool_nhwc_f32) are the general layers of cnn_layers.hip.  The distance is evaluated in
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
