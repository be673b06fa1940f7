// ingest.hip -- the data set's transform on the device (include/medfusion_hip.h, "Dataset transform"): PIL's bilinear resampler (ImagingResample:
// antialiased when reducing, horizontal pass first, the intermediate rounded to the element type), a crop and the value map, for a ragged batch --
// images of any sizes back to back in one byte buffer -- in one pair of launches.  Every output sample is a fixed chain over its source pixels and
// its own table row: 32-bit integers for uint8, separately rounded fp64 products and sums for uint16 / float32.  No atomics, no reductions: a
// sample's bits depend on its source pixels and its two table rows only -- not on N, the image's place, the alignment of its bytes or the grid.
#include "common.h"

#include <math.h>

using namespace mf;

namespace {

constexpr int LANES = 256;
constexpr int PRECISION_BITS = 32 - 8 - 2;   // PIL's fixed point of the 8-bit resampler: coefficients times 2^22

int elem_bytes(int dtype) { return dtype == MF_INGEST_U8 ? 1 : dtype == MF_INGEST_U16 ? 2 : 4; }

// ksize of PIL's precompute_coeffs for the triangle filter (support 1)
int axis_ksize(int in, int out) {
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(fs) * 2 + 1;
}

// ---------------------------------------------------------------------------------------------- the arithmetic of one sample
// n taps `stride` elements apart, C interleaved channels.  uint8: clamp((2^21 + sum pix k) >> 22, 0, 255) in 32-bit integers; float32 / uint16:
// ss = ss + double(pix) w with the product and the sum rounded separately, taps ascending; uint16 rounds half up and clamps.
template <typename T, int C>
__device__ __forceinline__ void resample_taps(const T* __restrict__ p, long stride, int n, const double* __restrict__ wf, const int32_t* __restrict__ wi,
                                              T (&r)[C]) {
#pragma clang fp contract(off)
  if constexpr (std::is_same<T, uint8_t>::value) {
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
    for (int k = 0; k < n; ++k) {
      const int kw = wi[k];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += (int)p[(long)k * stride + c] * kw;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int v = acc[c] >> PRECISION_BITS;
      r[c] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
  } else {
    double ss[C];
#pragma unroll
    for (int c = 0; c < C; ++c) ss[c] = 0.0;
    for (int k = 0; k < n; ++k) {
      const double w = wf[k];
#pragma unroll
      for (int c = 0; c < C; ++c) ss[c] = __dadd_rn(ss[c], __dmul_rn((double)p[(long)k * stride + c], w));
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if constexpr (std::is_same<T, float>::value) {
        r[c] = (float)ss[c];
      } else {
        double v = floor(__dadd_rn(ss[c], 0.5));
        v = v < 0.0 ? 0.0 : v > 65535.0 ? 65535.0 : v;
        r[c] = (uint16_t)v;
      }
    }
  }
}

// image_ingress_kernel's chain (edge_ops.hip): tF.normalize(v / full, 0.5, 0.5), every step rounded
__device__ __forceinline__ float centered_elem(float v, float full) {
#pragma clang fp contract(off)
  v = v / full;
  v = v - 0.5f;
  v = v / 0.5f;
  return v;
}

// ---------------------------------------------------------------------------------------------- horizontal pass
// One lane per (needed source row, surviving output column) of an image that changes width; a workgroup finds its image as the last one whose first
// workgroup (wg_h, a prefix over the batch) is not beyond it.  Writes the rounded intermediate [rows][w][C] at the image's workspace offset.
template <typename T, int C>
__global__ __launch_bounds__(LANES) void resample_h_kernel(const uint8_t* __restrict__ src, const MfResampleImage* __restrict__ images, int N,
                                                           const double* __restrict__ wf, const int32_t* __restrict__ wi,
                                                           const int32_t* __restrict__ bounds, T* __restrict__ ws, int w) {
  int lo = 0, hi = N - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (images[mid].wg_h <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const MfResampleImage im = images[lo];
  const long item = (long)((int)blockIdx.x - im.wg_h) * LANES + threadIdx.x;
  if (item >= (long)im.rows * w) return;
  const int r = (int)(item / w), x = (int)(item % w);
  const int ox = im.left + x;
  const int xmin = bounds[2 * (im.tb_h + ox)], n = bounds[2 * (im.tb_h + ox) + 1];
  const T* row = reinterpret_cast<const T*>(src + im.src_off) + ((long)(im.row0 + r) * im.W + xmin) * C;
  const long t = im.tw_h + (long)ox * im.ksize_h;
  T v[C];
  resample_taps<T, C>(row, C, n, wf ? wf + t : nullptr, wi ? wi + t : nullptr, v);
  T* o = ws + im.ws_off + ((long)r * w + x) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) o[c] = v[c];
}

// ---------------------------------------------------------------------------------------------- vertical pass + value map
// One lane per output pixel of every image (h w of them per image, the same for all: image = workgroup / workgroups per image).  Reads the
// intermediate of an image that changed width, else the source itself; an image that keeps its height passes the element through, so that a skipped
// axis rounds nothing twice and a same-size image takes image_ingress_kernel's chain on its own bytes.
template <typename T, int C>
__global__ __launch_bounds__(LANES) void resample_v_kernel(const uint8_t* __restrict__ src, const MfResampleImage* __restrict__ images,
                                                           const double* __restrict__ wf, const int32_t* __restrict__ wi,
                                                           const int32_t* __restrict__ bounds, const T* __restrict__ ws, void* __restrict__ out, int h, int w,
                                                           int wg_per_image, int mode) {
  const int i = (int)blockIdx.x / wg_per_image;
  const long item = (long)((int)blockIdx.x % wg_per_image) * LANES + threadIdx.x;
  if (item >= (long)h * w) return;
  const MfResampleImage im = images[i];
  const int y = (int)(item / w), x = (int)(item % w);
  const T* base;      // the element (row0, output column x, channel 0)
  long rstride;
  if (im.Wr != im.W) {
    base = ws + im.ws_off + (long)x * C;
    rstride = (long)w * C;
  } else {
    base = reinterpret_cast<const T*>(src + im.src_off) + ((long)im.row0 * im.W + im.left + x) * C;
    rstride = (long)im.W * C;
  }
  const int oy = im.top + y;
  T v[C];
  if (im.Hr != im.H) {
    const int ymin = bounds[2 * (im.tb_v + oy)], n = bounds[2 * (im.tb_v + oy) + 1];
    const long t = im.tw_v + (long)oy * im.ksize_v;
    resample_taps<T, C>(base + (long)(ymin - im.row0) * rstride, rstride, n, wf ? wf + t : nullptr, wi ? wi + t : nullptr, v);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = base[(long)(oy - im.row0) * rstride + c];
  }
  if constexpr (std::is_same<T, uint8_t>::value) {
    if (mode == MF_INGEST_BYTES) {
      uint8_t* o = reinterpret_cast<uint8_t*>(out) + (((long)i * h + y) * w + x) * C;
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = v[c];
      return;
    }
  }
  const float full = std::is_same<T, uint8_t>::value ? 255.0f : 65535.0f;
  float* o = reinterpret_cast<float*>(out) + (((long)i * C) * h + y) * w + x;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float f = (float)v[c];
    o[(long)c * h * w] = mode == MF_INGEST_CENTERED ? centered_elem(f, full) : f;
  }
}

// the reference's Normalize, (v - min) / (max - min) per image in fp32, then the centring: x [N][n] in place, mm [N][2] from mf_rows_minmax_f32
__global__ __launch_bounds__(LANES) void minmax_apply_kernel(float* __restrict__ x, const float* __restrict__ mm, long n, int center) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const float mn = mm[2 * b], mx = mm[2 * b + 1];
  const float span = mx - mn;
  float* row = x + (long)b * n;
  for (long i = (long)blockIdx.x * LANES + threadIdx.x; i < n; i += (long)gridDim.x * LANES) {
    float v = row[i] - mn;
    v = v / span;
    if (center) {
      v = v - 0.5f;
      v = v / 0.5f;
    }
    row[i] = v;
  }
}

// ---------------------------------------------------------------------------------------------- host: one image's rules and derived fields
struct Derived { int row0, rows, wgs; long ws_elems; };

// checks the table rows [first, first + count) of one axis against the host copy of the bounds; -> the source range they reach
int check_axis(const char* axis, int idx, int in, int out, int ksize, int64_t tw, int64_t tb, int first, int count, const int32_t* bh, int64_t bcount,
               int64_t wcount, int* lo, int* hi) {
  MF_REQUIRE(ksize == axis_ksize(in, out), MF_EINVAL, "resample: image %d: %s ksize %d, %d -> %d has %d", idx, axis, ksize, in, out, axis_ksize(in, out));
  MF_REQUIRE(tb >= 0 && tb + out <= bcount && tw >= 0 && tw + (int64_t)out * ksize <= wcount, MF_EINVAL, "resample: image %d: %s table outside the tables given",
             idx, axis);
  int mn = in, mx = 0;
  for (int o = first; o < first + count; ++o) {
    const int xmin = bh[2 * (tb + o)], n = bh[2 * (tb + o) + 1];
    MF_REQUIRE(xmin >= 0 && n >= 0 && n <= ksize && xmin + n <= in, MF_EINVAL, "resample: image %d: %s bounds (%d, %d) of sample %d outside %d", idx, axis, xmin,
               n, o, in);
    mn = xmin < mn ? xmin : mn;
    mx = xmin + n > mx ? xmin + n : mx;
  }
  if (mx < mn) mn = mx = 0;
  *lo = mn, *hi = mx;
  return MF_OK;
}

int derive(const MfResampleImage& im, int idx, int C, int dtype, int h, int w, const int32_t* bh, int64_t bcount, int64_t wcount, int64_t src_bytes,
           Derived* d) {
  const int esz = elem_bytes(dtype);
  MF_REQUIRE(im.H >= 1 && im.W >= 1 && im.Hr >= 1 && im.Wr >= 1, MF_EINVAL, "resample: image %d: a side below 1 (%d x %d -> %d x %d)", idx, im.H, im.W, im.Hr,
             im.Wr);
  MF_REQUIRE(im.top >= 0 && im.left >= 0 && (long)im.top + h <= im.Hr && (long)im.left + w <= im.Wr, MF_EINVAL,
             "resample: image %d: crop (%d, %d, %d, %d) outside the resized image %d x %d", idx, im.top, im.left, h, w, im.Hr, im.Wr);
  MF_REQUIRE(im.src_off >= 0 && im.src_off % esz == 0 && im.src_off + (int64_t)im.H * im.W * C * esz <= src_bytes, MF_EINVAL,
             "resample: image %d: bytes [%lld, +%lld) outside the buffer of %lld", idx, (long long)im.src_off, (long long)im.H * im.W * C * esz,
             (long long)src_bytes);
  MF_REQUIRE(im.reserved == 0, MF_EINVAL, "resample: image %d: reserved", idx);
  const bool hp = im.Wr != im.W, vp = im.Hr != im.H;
  int lo = 0, hi = 0;
  if (hp) {
    const int rc = check_axis("horizontal", idx, im.W, im.Wr, im.ksize_h, im.tw_h, im.tb_h, im.left, w, bh, bcount, wcount, &lo, &hi);
    if (rc) return rc;
  }
  d->row0 = im.top, d->rows = h;
  if (vp) {
    const int rc = check_axis("vertical", idx, im.H, im.Hr, im.ksize_v, im.tw_v, im.tb_v, im.top, h, bh, bcount, wcount, &lo, &hi);
    if (rc) return rc;
    d->row0 = lo, d->rows = hi - lo;
  }
  d->ws_elems = hp ? (long)d->rows * w * C : 0;
  d->wgs = hp ? cdiv((long)d->rows * w, LANES) : 0;
  return MF_OK;
}

int check_batch(int N, int C, int dtype, int h, int w) {
  MF_REQUIRE(N >= 1 && h >= 1 && w >= 1 && (long)h * w <= (1L << 30), MF_EINVAL, "resample: N=%d, output %d x %d", N, h, w);
  MF_REQUIRE(dtype == MF_INGEST_U8 || dtype == MF_INGEST_U16 || dtype == MF_INGEST_F32, MF_EINVAL, "resample: dtype %d", dtype);
  MF_REQUIRE(C == 1 || C == 3, MF_EINVAL, "resample: C=%d, 1 or 3 channels", C);
  MF_REQUIRE(C == 1 || dtype == MF_INGEST_U8, MF_EUNSUPPORTED, "resample: 3 channels are read as uint8 only");
  return MF_OK;
}

template <typename T, int C>
void launch_passes(const MfResampleArgs& a, int wg_h, int wg_per_image, hipStream_t s) {
  const uint8_t* src = reinterpret_cast<const uint8_t*>(a.src);
  if (wg_h > 0)
    MF_LAUNCH((resample_h_kernel<T, C>), dim3(wg_h), dim3(LANES), 0, s, src, a.images, a.N, a.weights_f64, a.weights_i32, a.bounds,
              reinterpret_cast<T*>(a.workspace), a.w);
  MF_LAUNCH((resample_v_kernel<T, C>), dim3((unsigned)a.N * wg_per_image), dim3(LANES), 0, s, src, a.images, a.weights_f64, a.weights_i32, a.bounds,
            reinterpret_cast<const T*>(a.workspace), a.out, a.h, a.w, wg_per_image, a.out_mode);
}

}  // namespace

extern "C" {

int mf_resample_table(int in, int out, double* weights, int32_t* fixed, int32_t* bounds) {
  MF_REQUIRE(in >= 1 && out >= 1, MF_EINVAL, "resample_table: %d -> %d", in, out);
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * fs;
  const int ksize = (int)ceil(support) * 2 + 1;
  if (!weights && !fixed && !bounds) return ksize;
  const double ss = 1.0 / fs;
  double kk[4096];
  double* k = kk;
  double* heap = nullptr;
  if (ksize > 4096) k = heap = new double[ksize];
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      double t = (x + xmin - center + 0.5) * ss;
      if (t < 0.0) t = -t;
      const double w = t < 1.0 ? 1.0 - t : 0.0;
      k[x] = w;
      ww += w;
    }
    for (int x = 0; x < n; ++x)
      if (ww != 0.0) k[x] /= ww;
    for (int x = n; x < ksize; ++x) k[x] = 0.0;
    for (int x = 0; x < ksize; ++x) {
      if (weights) weights[(long)xx * ksize + x] = k[x];
      if (fixed) fixed[(long)xx * ksize + x] = k[x] < 0.0 ? (int)(-0.5 + k[x] * (1 << PRECISION_BITS)) : (int)(0.5 + k[x] * (1 << PRECISION_BITS));
    }
    if (bounds) bounds[2 * xx] = xmin, bounds[2 * xx + 1] = n;
  }
  delete[] heap;
  return ksize;
}

int mf_resample_plan(MfResampleImage* images, int N, int C, int dtype, int h, int w, const int32_t* bounds_host, int64_t bounds_count,
                     int64_t weights_count, int64_t src_bytes, MfResamplePlan* plan) {
  MF_REQUIRE(images && plan, MF_EINVAL, "resample_plan: null images / plan");
  int rc = check_batch(N, C, dtype, h, w);
  if (rc) return rc;
  long ws = 0, wg = 0;
  bool any_table = false;
  for (int i = 0; i < N; ++i) any_table |= images[i].Wr != images[i].W || images[i].Hr != images[i].H;
  MF_REQUIRE(!any_table || bounds_host, MF_EINVAL, "resample_plan: null bounds_host");
  for (int i = 0; i < N; ++i) {
    Derived d;
    rc = derive(images[i], i, C, dtype, h, w, bounds_host, bounds_count, weights_count, src_bytes, &d);
    if (rc) return rc;
    images[i].row0 = d.row0, images[i].rows = d.rows, images[i].ws_off = ws, images[i].wg_h = (int32_t)wg;
    ws += d.ws_elems, wg += d.wgs;
    MF_REQUIRE(wg <= 0x7FFFFFFFL, MF_EUNSUPPORTED, "resample_plan: more than 2^31 workgroups");
  }
  const int per = cdiv((long)h * w, LANES);
  MF_REQUIRE((long)N * per <= 0x7FFFFFFFL, MF_EUNSUPPORTED, "resample_plan: more than 2^31 workgroups");
  plan->workspace_bytes = ws * elem_bytes(dtype);
  plan->wg_h = (int32_t)wg, plan->wg_v = (int32_t)((long)N * per);
  plan->launches = wg > 0 ? 2 : 1, plan->reserved = 0;
  return MF_OK;
}

int mf_image_resample(const MfResampleArgs* a, void* stream) {
  MF_REQUIRE(a && a->src && a->images && a->images_host && a->out, MF_EINVAL, "resample: null src / images / images_host / out");
  int rc = check_batch(a->N, a->C, a->dtype, a->h, a->w);
  if (rc) return rc;
  MF_REQUIRE(a->out_mode == MF_INGEST_RAW || (a->out_mode == MF_INGEST_CENTERED && a->dtype != MF_INGEST_F32) ||
                 (a->out_mode == MF_INGEST_BYTES && a->dtype == MF_INGEST_U8),
             MF_EINVAL, "resample: out_mode %d with dtype %d", a->out_mode, a->dtype);
  MF_REQUIRE(a->reserved == 0, MF_EINVAL, "resample: reserved");
  // every derived field is recomputed from the host copies and compared: a descriptor that mf_resample_plan did not fill is refused here
  long ws = 0, wg = 0;
  bool any_table = false;
  for (int i = 0; i < a->N; ++i) any_table |= a->images_host[i].Wr != a->images_host[i].W || a->images_host[i].Hr != a->images_host[i].H;
  if (any_table) {
    MF_REQUIRE(a->bounds && a->bounds_host, MF_EINVAL, "resample: null bounds / bounds_host");
    MF_REQUIRE(a->dtype == MF_INGEST_U8 ? a->weights_i32 != nullptr : a->weights_f64 != nullptr, MF_EINVAL, "resample: null weights");
  }
  for (int i = 0; i < a->N; ++i) {
    const MfResampleImage& im = a->images_host[i];
    Derived d;
    rc = derive(im, i, a->C, a->dtype, a->h, a->w, a->bounds_host, a->bounds_count, a->weights_count, a->src_bytes, &d);
    if (rc) return rc;
    MF_REQUIRE(im.row0 == d.row0 && im.rows == d.rows && im.ws_off == ws && im.wg_h == (int32_t)wg, MF_EINVAL,
               "resample: image %d: derived fields are not mf_resample_plan's", i);
    ws += d.ws_elems, wg += d.wgs;
  }
  const size_t need = (size_t)ws * elem_bytes(a->dtype);
  if (need) {
    MF_REQUIRE(a->workspace && ((uintptr_t)a->workspace & 15) == 0, MF_EINVAL, "resample: workspace must be given, 16-byte aligned");
    MF_REQUIRE(a->workspace_bytes >= need, MF_EWORKSPACE, "resample: workspace of %zu bytes, %zu needed", (size_t)a->workspace_bytes, need);
  }
  MF_REQUIRE(a->dtype == MF_INGEST_U8 || ((uintptr_t)a->src & 3) == 0, MF_EINVAL, "resample: uint16 / float32 sources start 4-byte aligned");
  const int per = cdiv((long)a->h * a->w, LANES);
  MF_REQUIRE(wg <= 0x7FFFFFFFL && (long)a->N * per <= 0x7FFFFFFFL, MF_EUNSUPPORTED, "resample: more than 2^31 workgroups");
  hipStream_t s = (hipStream_t)stream;
  const double outs = (double)a->N * a->C * a->h * a->w;
  ProfScope ps(MF_FAM_MISC, s, 2.0 * outs, (double)a->src_bytes + 4.0 * outs);
  if (a->dtype == MF_INGEST_U8 && a->C == 1) launch_passes<uint8_t, 1>(*a, (int)wg, per, s);
  else if (a->dtype == MF_INGEST_U8) launch_passes<uint8_t, 3>(*a, (int)wg, per, s);
  else if (a->dtype == MF_INGEST_U16) launch_passes<uint16_t, 1>(*a, (int)wg, per, s);
  else launch_passes<float, 1>(*a, (int)wg, per, s);
  return check_launch("image_resample");
}

int mf_minmax_apply_f32(float* x, const float* minmax, int N, int64_t n, int center, void* stream) {
  MF_REQUIRE(x && minmax && N > 0 && N <= 65535 && n > 0, MF_EINVAL, "minmax_apply: N=%d n=%lld", N, (long long)n);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(MF_FAM_MISC, s, 2.0 * N * (double)n, 8.0 * N * (double)n);
  const long per = (n + LANES - 1) / LANES;
  MF_LAUNCH(minmax_apply_kernel, dim3((unsigned)(per < 1024 ? per : 1024), N), dim3(LANES), 0, s, x, minmax, (long)n, center);
  return check_launch("minmax_apply");
}

}  // extern "C"
