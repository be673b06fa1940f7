// window_ops.hip -- windowed denoising (MultiDiffusion): the crop of a canvas into overlapping windows of the trained size and the weighted
// merge of the per-window predictions back onto the canvas (include/medfusion_hip.h, MfWindowDesc).  Both are launch-latency-bound copies that
// exist as library launches so that the recorded iteration of the denoise loop holds them (a torch op inside it would end the replay).
// Built without packed fp32 like vq.hip (medfusion_amd/build.py): the merge is plain fp32 VALU arithmetic that hipcc would pack.
#include "common.h"

using namespace mf;

namespace {

// the geometry by value in the kernarg segment: no device table to upload, nothing for a replay to keep alive
struct WinGeom {
  int canvas[3], window[3], count[3];
  int origin[3][MF_WINDOW_MAX_PER_AXIS];
  int weight, C, M;
};

// windows[b * M + m][c][z][y][x] = canvas[b][c][o0 + z][o1 + y][o2 + x]; V = 4: four cells of a row per thread (16-byte loads and stores)
template <int V>
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ canvas, float* __restrict__ windows, const WinGeom g, long total) {
  const int wv = g.window[2] / V, h = g.window[1], d = g.window[0];
  const long stride = (long)gridDim.x * blockDim.x;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
    long r = q;
    const int x = (int)(r % wv) * V;
    r /= wv;
    const int y = (int)(r % h);
    r /= h;
    const int z = (int)(r % d);
    r /= d;
    const int c = (int)(r % g.C);
    r /= g.C;
    const int m = (int)(r % g.M);
    const long b = r / g.M;
    const int k2 = m % g.count[2], k1 = (m / g.count[2]) % g.count[1], k0 = m / (g.count[2] * g.count[1]);
    const long src = ((((b * g.C + c) * g.canvas[0] + g.origin[0][k0] + z) * g.canvas[1] + g.origin[1][k1] + y) * g.canvas[2]) + g.origin[2][k2] + x;
    if (V == 4) *reinterpret_cast<float4*>(windows + q * 4) = *reinterpret_cast<const float4*>(canvas + src);
    else windows[q] = canvas[src];
  }
}

// the origins [lo, hi] of one axis whose window holds position p (ascending origins without a gap: a contiguous, non-empty range)
__device__ __forceinline__ void covering(const int* org, int n, int ext, int p, int& lo, int& hi) {
  lo = n;
  hi = -1;
  for (int k = 0; k < n; ++k) {
    const int o = org[k];
    if (o <= p && p < o + ext) {
      lo = min(lo, k);
      hi = k;
    }
  }
}

__device__ __forceinline__ float profile(int weight, int i, int ext) { return weight == MF_WINDOW_TENT ? (float)min(i + 1, ext - i) : 1.0f; }

// canvas_out[b][c][Z][Y][X] = sum_m w_m p_m / sum_m w_m over the covering windows in ascending m; one covering window: its value, untouched.
// V = 4: four cells of a row per thread -- with the last axis' extents and origins multiples of 4 they share their covering windows.
template <int V>
__global__ __launch_bounds__(256) void window_merge_kernel(const float* __restrict__ windows, float* __restrict__ out, const WinGeom g, long total) {
#pragma clang fp contract(off)
  const int Wv = g.canvas[2] / V, H = g.canvas[1], D = g.canvas[0];
  const int d = g.window[0], h = g.window[1], w = g.window[2];
  const long stride = (long)gridDim.x * blockDim.x;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
    long r = q;
    const int X = (int)(r % Wv) * V;
    r /= Wv;
    const int Y = (int)(r % H);
    r /= H;
    const int Z = (int)(r % D);
    r /= D;
    const int c = (int)(r % g.C);
    const long b = r / g.C;
    int lo0, hi0, lo1, hi1, lo2, hi2;
    covering(g.origin[0], g.count[0], d, Z, lo0, hi0);
    covering(g.origin[1], g.count[1], h, Y, lo1, hi1);
    covering(g.origin[2], g.count[2], w, X, lo2, hi2);
    const bool single = lo0 == hi0 && lo1 == hi1 && lo2 == hi2;
    float acc[V], den = 0.f, den_v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f, den_v[j] = 0.f;
    for (int k0 = lo0; k0 <= hi0; ++k0) {
      const int z = Z - g.origin[0][k0];
      const float w0 = profile(g.weight, z, d);
      for (int k1 = lo1; k1 <= hi1; ++k1) {
        const int y = Y - g.origin[1][k1];
        const float w01 = w0 * profile(g.weight, y, h);
        for (int k2 = lo2; k2 <= hi2; ++k2) {
          const int x = X - g.origin[2][k2];
          const int m = (k0 * g.count[1] + k1) * g.count[2] + k2;
          const long src = ((((b * g.M + m) * g.C + c) * d + z) * h + y) * (long)w + x;
          if (V == 4) {
            const float4 p = *reinterpret_cast<const float4*>(windows + src);
            if (single) {
              *reinterpret_cast<float4*>(out + q * 4) = p;
            } else {
              const float pv[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const float wm = w01 * profile(g.weight, x + j, w);
                acc[j] = fmaf(wm, pv[j], acc[j]);
                den_v[j] += wm;
              }
            }
          } else {
            const float p = windows[src];
            if (single) {
              out[q] = p;
            } else {
              const float wm = w01 * profile(g.weight, x, w);
              acc[0] = fmaf(wm, p, acc[0]);
              den += wm;
            }
          }
        }
      }
    }
    if (!single) {
      if (V == 4) *reinterpret_cast<float4*>(out + q * 4) = make_float4(acc[0] / den_v[0], acc[1] / den_v[1], acc[2] / den_v[2], acc[3] / den_v[3]);
      else out[q] = acc[0] / den;
    }
  }
}

// the descriptor's rules, checked on the host before any launch; fills the kernels' geometry
int window_geometry(const MfWindowDesc* d, const char* what, WinGeom* g, bool* by4) {
  MF_REQUIRE(d != nullptr, MF_EINVAL, "%s: no descriptor", what);
  MF_REQUIRE(d->dims == 2 || d->dims == 3, MF_EINVAL, "%s: dims=%d (2 or 3)", what, d->dims);
  MF_REQUIRE(d->B > 0 && d->C > 0, MF_EINVAL, "%s: B=%d C=%d", what, d->B, d->C);
  MF_REQUIRE(d->weight == MF_WINDOW_UNIFORM || d->weight == MF_WINDOW_TENT, MF_EINVAL, "%s: weight kind %d", what, d->weight);
  MF_REQUIRE(d->dims == 3 || (d->canvas[0] == 1 && d->window[0] == 1 && d->count[0] == 1), MF_EINVAL, "%s: a 2-D descriptor has a leading extent of 1", what);
  *by4 = true;
  for (int a = 0; a < 3; ++a) {
    const int L = d->canvas[a], h = d->window[a], n = d->count[a];
    MF_REQUIRE(h >= 1 && L >= h, MF_EINVAL, "%s: axis %d: canvas %d, window %d", what, a, L, h);
    MF_REQUIRE(n >= 1 && n <= MF_WINDOW_MAX_PER_AXIS, MF_EINVAL, "%s: axis %d: %d origins (1 .. %d)", what, a, n, MF_WINDOW_MAX_PER_AXIS);
    MF_REQUIRE(d->origin[a][0] == 0 && d->origin[a][n - 1] == L - h, MF_EINVAL, "%s: axis %d: the origins run from 0 to canvas - window", what, a);
    for (int k = 1; k < n; ++k)
      MF_REQUIRE(d->origin[a][k] > d->origin[a][k - 1] && d->origin[a][k] - d->origin[a][k - 1] <= h, MF_EINVAL,
                 "%s: axis %d: origins ascend strictly and leave no gap", what, a);
    g->canvas[a] = L;
    g->window[a] = h;
    g->count[a] = n;
    for (int k = 0; k < MF_WINDOW_MAX_PER_AXIS; ++k) g->origin[a][k] = k < n ? d->origin[a][k] : 0;
    if (a == 2) {
      *by4 = (L % 4 == 0) && (h % 4 == 0);
      for (int k = 0; k < n; ++k) *by4 = *by4 && (d->origin[a][k] % 4 == 0);
    }
  }
  g->weight = d->weight;
  g->C = d->C;
  g->M = d->count[0] * d->count[1] * d->count[2];
  return MF_OK;
}

inline int blocks_for(long work) {
  long blocks = (work + 255) / 256;
  return (int)(blocks > 2048 ? 2048 : blocks);
}

}  // namespace

extern "C" {

int mf_window_gather_f32(const float* canvas, float* windows, const MfWindowDesc* desc, void* stream) {
  WinGeom g;
  bool by4;
  const int rc = window_geometry(desc, "window_gather", &g, &by4);
  if (rc != MF_OK) return rc;
  MF_REQUIRE(canvas && windows, MF_EINVAL, "window_gather: bad args");
  hipStream_t s = (hipStream_t)stream;
  const long total = (long)desc->B * g.M * g.C * g.window[0] * g.window[1] * g.window[2];
  ProfScope ps(MF_FAM_MISC, s, 0, 8.0 * total);
  if (by4 && ((((uintptr_t)canvas | (uintptr_t)windows) & 15) == 0)) {
    MF_LAUNCH(window_gather_kernel<4>, dim3(blocks_for(total / 4)), dim3(256), 0, s, canvas, windows, g, total / 4);
  } else {
    MF_LAUNCH(window_gather_kernel<1>, dim3(blocks_for(total)), dim3(256), 0, s, canvas, windows, g, total);
  }
  return check_launch("window_gather");
}

int mf_window_merge_f32(const float* windows, float* canvas_out, const MfWindowDesc* desc, void* stream) {
  WinGeom g;
  bool by4;
  const int rc = window_geometry(desc, "window_merge", &g, &by4);
  if (rc != MF_OK) return rc;
  MF_REQUIRE(windows && canvas_out, MF_EINVAL, "window_merge: bad args");
  hipStream_t s = (hipStream_t)stream;
  const long total = (long)desc->B * g.C * g.canvas[0] * g.canvas[1] * g.canvas[2];
  const double read = (double)desc->B * g.M * g.C * g.window[0] * g.window[1] * g.window[2];
  ProfScope ps(MF_FAM_MISC, s, 3.0 * read, 4.0 * (read + (double)total));
  if (by4 && ((((uintptr_t)canvas_out | (uintptr_t)windows) & 15) == 0)) {
    MF_LAUNCH(window_merge_kernel<4>, dim3(blocks_for(total / 4)), dim3(256), 0, s, windows, canvas_out, g, total / 4);
  } else {
    MF_LAUNCH(window_merge_kernel<1>, dim3(blocks_for(total)), dim3(256), 0, s, windows, canvas_out, g, total);
  }
  return check_launch("window_merge");
}

}  // extern "C"
