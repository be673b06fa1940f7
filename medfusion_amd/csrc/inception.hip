// inception.hip -- the FID variant of Inception-v3 on the device (include/medfusion_hip.h, "Inception"): the TF1-style resize of byte images and the mean
// over the pixels.  The trunk's convolutions and pools are the general layers of cnn_layers.hip.
#include "common.h"

#include <math.h>

using namespace mf;

namespace {

constexpr int THREADS = 256;

// ---------------------------------------------------------------------------------------------- resize + value map, NCHW bytes -> NHWC fp32
// one thread per output pixel; the three channels from channel c (C == 3) or channel 0 (C == 1)
__global__ __launch_bounds__(THREADS) void inception_prepare_kernel(const uint8_t* __restrict__ x, float* __restrict__ out, int C, int H, int W, int S, long total) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % S);
  long r = i / S;
  const int oy = (int)(r % S);
  const long b = r / S;
  const float sy = (float)H / (float)S, sx = (float)W / (float)S;
  const float gy = (float)oy * sy, gx = (float)ox * sx;
  const int y0 = min((int)gy, H - 1), x0 = min((int)gx, W - 1);
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
  const float dy = gy - (float)y0, dx = gx - (float)x0;
  const long HW = (long)H * W;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint8_t* __restrict__ src = x + (b * C + (C == 3 ? c : 0)) * HW;
    const float a00 = (float)src[(long)y0 * W + x0], a01 = (float)src[(long)y0 * W + x1];
    const float a10 = (float)src[(long)y1 * W + x0], a11 = (float)src[(long)y1 * W + x1];
    const float top = a00 + (a01 - a00) * dx;
    const float bottom = a10 + (a11 - a10) * dx;
    const float v = top + (bottom - top) * dy;
    out[i * 3 + c] = (v - 128.f) / 128.f;
  }
}

// ---------------------------------------------------------------------------------------------- the mean over the pixels
// one thread per (b, c): the fp64 sum over the pixels in ascending order, divided by their number, rounded once to fp32
__global__ __launch_bounds__(THREADS) void mean_pixels_kernel(const float* __restrict__ x, float* __restrict__ out, long P, int C, long total) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= total) return;
  const long b = i / C;
  const int c = (int)(i - b * C);
  const float* __restrict__ src = x + b * P * C + c;
  double s = 0.0;
  for (long q = 0; q < P; ++q) s += (double)src[q * C];
  out[i] = (float)(s / (double)P);
}

}  // namespace

extern "C" {

int mf_inception_prepare_u8(const uint8_t* x, float* out, int B, int C, int H, int W, int S, void* stream) {
  MF_REQUIRE(x && out, MF_EINVAL, "inception_prepare: null pointer");
  MF_REQUIRE(C == 1 || C == 3, MF_EINVAL, "inception_prepare: C = %d, 1 or 3 channels", C);
  MF_REQUIRE(B > 0 && H > 0 && W > 0 && H <= 16384 && W <= 16384, MF_EINVAL, "inception_prepare: B = %d, sides %d x %d (1 .. 16384)", B, H, W);
  MF_REQUIRE(S >= MF_INCEPTION_MIN_SIZE && S <= 4096, MF_EINVAL, "inception_prepare: size %d (%d .. 4096)", S, MF_INCEPTION_MIN_SIZE);
  const long total = (long)B * S * S;
  MF_REQUIRE((total + THREADS - 1) / THREADS < (1L << 31), MF_EUNSUPPORTED, "inception_prepare: problem too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 30.0 * total, (double)B * C * H * W + 12.0 * total);
  MF_LAUNCH(inception_prepare_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, x, out, C, H, W, S, total);
  return check_launch("inception_prepare");
}

int mf_mean_pixels_f32(const float* x, float* out, int B, int64_t P, int C, void* stream) {
  MF_REQUIRE(x && out, MF_EINVAL, "mean_pixels: null pointer");
  MF_REQUIRE(B > 0 && P > 0 && C > 0, MF_EINVAL, "mean_pixels: bad sizes");
  const long total = (long)B * C;
  MF_REQUIRE((total + THREADS - 1) / THREADS < (1L << 31), MF_EUNSUPPORTED, "mean_pixels: problem too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, (double)total * P, 4.0 * ((double)total * P + (double)total));
  MF_LAUNCH(mean_pixels_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, x, out, (long)P, C, total);
  return check_launch("mean_pixels");
}

}  // extern "C"
