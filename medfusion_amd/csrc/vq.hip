// vq.hip -- nearest-codebook vector quantizer of VQVAE / VQGAN (latent_embedders.py:40-71: VectorQuantizer.forward).
//
// The distance follows the reference's formula, not the exact one: d = (sum z^2 + sum e^2) - 2 * sum z*e, every sum in fp32 in index order,
// no contraction (-ffp-contract=off, build.CFLAGS) -- identical latents must pick the reference's code, and the cancelling formula is what picks it.
// Ties go to the lowest index and the first NaN distance wins, like torch.argmin.
//
// Launches: (1) fill the per-pixel keys with ~0; (2) search: grid (pixel tiles, codebook slices), each workgroup stages its slice of the codebook
// in LDS chunk by chunk together with sum e^2 of every code, each thread scans it for one pixel and folds its best (key(d) << 32 | index) into
// the pixel's key with a 64-bit atomicMin -- commutative, so the result does not depend on the order in which slices arrive, and equal keys
// resolve to the lower index by themselves; (3) gather: z_q = z + (e_idx - z), the index, and per-tile fp64 partial sums of (e_idx - z)^2;
// (4) only for the squared error: one workgroup sums the partials in a fixed order.
#include "common.h"

using namespace mf;

namespace {

constexpr int kTile = 256;      // pixels per workgroup (one per thread)
constexpr int kChunk = 512;     // codes staged in LDS at a time: 512 * (16 + 1) * 4 B = 34 KB at C = 16
constexpr int kMaxSlices = 16;  // codebook slices per pixel tile (the split that fills the chip at small batches)
constexpr int kFinal = 1024;    // threads of the partial-sum reduction

// order-preserving map fp32 -> u32: negatives flip every bit, non-negatives set the sign bit; -0 and +0 coincide; NaN maps to 0, below
// everything, so that the first NaN distance wins like torch.argmin
__device__ __forceinline__ unsigned order_key(float d) {
  const unsigned b = __float_as_uint(d);
  if (d != d) return 0u;
  if (b == 0x80000000u) return 0x80000000u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(256) void vq_fill_kernel(unsigned long long* __restrict__ keys, long P) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p < P) keys[p] = ~0ull;
}

template <int C>
__global__ __launch_bounds__(kTile) void vq_search_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                          unsigned long long* __restrict__ keys, long P, int HW, int K, int S) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [kChunk][C] codes, then [kChunk] sum e^2
  float* es = lds;
  float* ees = lds + kChunk * C;
  const int tid = threadIdx.x;
  const long p = (long)blockIdx.x * kTile + tid;
  const bool live = p < P;
  float zr[C];
  float zz = 0.f;
  if (live) {
    const long n = p / HW, hw = p - n * HW;
    const float* zp = z + n * (long)C * HW + hw;
#pragma unroll
    for (int c = 0; c < C; ++c) zr[c] = zp[(long)c * HW];
    zz = zr[0] * zr[0];
#pragma unroll
    for (int c = 1; c < C; ++c) zz = zz + zr[c] * zr[c];
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) zr[c] = 0.f;
  }
  const int k0 = blockIdx.y * S;
  const int k1 = min(K, k0 + S);
  unsigned best = 0xFFFFFFFFu;   // above every real key (+inf maps to 0xFF800000): the slice's first code always replaces it
  int bi = k0;
  for (int c0 = k0; c0 < k1; c0 += kChunk) {
    const int n = min(kChunk, k1 - c0);
    __syncthreads();   // the previous chunk has been read by every thread
    for (int j = tid; j < n; j += kTile) {
      const float* er = cb + (long)(c0 + j) * C;
      float e = er[0];
      es[j * C] = e;
      float ee = e * e;
#pragma unroll
      for (int c = 1; c < C; ++c) {
        e = er[c];
        es[j * C + c] = e;
        ee = ee + e * e;
      }
      ees[j] = ee;
    }
    __syncthreads();
    if (live) {
#pragma unroll 4
      for (int j = 0; j < n; ++j) {
        const float* e = es + j * C;
        float ze = zr[0] * e[0];
#pragma unroll
        for (int c = 1; c < C; ++c) ze = ze + zr[c] * e[c];
        const float d = (zz + ees[j]) - 2.0f * ze;
        const unsigned kd = order_key(d);
        if (kd < best) {
          best = kd;
          bi = c0 + j;
        }
      }
    }
  }
  if (live) atomicMin(keys + p, ((unsigned long long)best << 32) | (unsigned)bi);
}

__global__ __launch_bounds__(kTile) void vq_gather_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                          const unsigned long long* __restrict__ keys, float* __restrict__ zq,
                                                          int* __restrict__ idx_out, double* __restrict__ part, long P, int C, int HW, int K) {
  __shared__ double red[kTile / 64];
  const int tid = threadIdx.x;
  const long p = (long)blockIdx.x * kTile + tid;
  double acc = 0.0;
  if (p < P) {
    int k = (int)(unsigned)(keys[p] & 0xFFFFFFFFull);
    if (k < 0 || k >= K) k = 0;   // (cannot happen: every slice folds a real index into every live pixel; never read outside the codebook)
    const long n = p / HW, hw = p - n * HW;
    const long base = n * (long)C * HW + hw;
    const float* er = cb + (long)k * C;
    for (int c = 0; c < C; ++c) {
      const float zc = z[base + (long)c * HW];
      const float diff = er[c] - zc;
      zq[base + (long)c * HW] = zc + diff;   // the reference's straight-through value z + (z_q - z)
      acc += (double)(diff * diff);
    }
    if (idx_out) idx_out[p] = k;
  }
  if (!part) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < kTile / 64; ++w) s += red[w];
    part[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kFinal) void vq_sum_kernel(const double* __restrict__ part, double* __restrict__ out, int nparts) {
  __shared__ double red[kFinal / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kFinal) acc += part[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < kFinal / 64; ++w) s += red[w];
    out[0] = s;
  }
}

template <int C>
void launch_search(const float* z, const float* cb, unsigned long long* keys, long P, int HW, int K, int S, int tiles, int slices, hipStream_t s) {
  MF_LAUNCH(vq_search_kernel<C>, dim3(tiles, slices), dim3(kTile), (size_t)kChunk * (C + 1) * sizeof(float), s, z, cb, keys, P, HW, K, S);
}

// codebook slice per workgroup: enough slices that pixel tiles x slices reaches ~1024 workgroups (4 per CU), at most kMaxSlices, a multiple of
// 64 codes
void plan_slices(long P, int K, int* S, int* slices) {
  const long tiles = (P + kTile - 1) / kTile;
  long want = (1024 + tiles - 1) / tiles;
  if (want > kMaxSlices) want = kMaxSlices;
  if (want < 1) want = 1;
  long s = (K + want - 1) / want;
  s = (s + 63) / 64 * 64;
  *S = (int)s;
  *slices = (int)((K + s - 1) / s);
}

}  // namespace

extern "C" {

size_t mf_vq_workspace_bytes(int64_t P) {
  if (P <= 0) return 0;
  const int64_t tiles = (P + kTile - 1) / kTile;
  return (size_t)(P * 8 + tiles * 8);
}

int mf_vector_quantize_f32(const float* z, const float* codebook, float* z_q, int32_t* idx, double* sqerr, void* workspace, size_t workspace_bytes,
                           int N, int C, int HW, int K, void* stream) {
  MF_REQUIRE(N >= 0 && C > 0 && HW > 0 && K > 0, MF_EINVAL, "vector_quantize: bad sizes N=%d C=%d HW=%d K=%d", N, C, HW, K);
  MF_REQUIRE(C <= 16, MF_EUNSUPPORTED, "vector_quantize: C=%d channels (at most 16)", C);
  if (N == 0) return MF_OK;
  MF_REQUIRE(z && codebook && z_q && workspace, MF_EINVAL, "vector_quantize: null pointer");
  const long P = (long)N * HW;
  MF_REQUIRE(P < (1L << 31) && (long)K * C < (1L << 31), MF_EINVAL, "vector_quantize: %ld pixels x %d codes too large", P, K);
  MF_REQUIRE(workspace_bytes >= mf_vq_workspace_bytes(P), MF_EWORKSPACE, "vector_quantize: workspace %zu < %zu bytes", workspace_bytes,
             mf_vq_workspace_bytes(P));
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (int)((P + kTile - 1) / kTile);
  unsigned long long* keys = static_cast<unsigned long long*>(workspace);
  double* part = reinterpret_cast<double*>(keys + P);
  int S = 0, slices = 0;
  plan_slices(P, K, &S, &slices);
  ProfScope ps(MF_FAM_MISC, s, (3.0 * C + 3.0) * (double)P * K, 8.0 * C * P + 4.0 * C * K * slices);
  MF_LAUNCH(vq_fill_kernel, dim3(cdiv(P, 256)), dim3(256), 0, s, keys, P);
  switch (C) {
#define MF_VQ_CASE(c) \
  case c: launch_search<c>(z, codebook, keys, P, HW, K, S, tiles, slices, s); break;
    MF_VQ_CASE(1) MF_VQ_CASE(2) MF_VQ_CASE(3) MF_VQ_CASE(4) MF_VQ_CASE(5) MF_VQ_CASE(6) MF_VQ_CASE(7) MF_VQ_CASE(8)
    MF_VQ_CASE(9) MF_VQ_CASE(10) MF_VQ_CASE(11) MF_VQ_CASE(12) MF_VQ_CASE(13) MF_VQ_CASE(14) MF_VQ_CASE(15) MF_VQ_CASE(16)
#undef MF_VQ_CASE
  }
  MF_LAUNCH(vq_gather_kernel, dim3(tiles), dim3(kTile), 0, s, z, codebook, keys, z_q, idx, sqerr ? part : nullptr, P, C, HW, K);
  if (sqerr) MF_LAUNCH(vq_sum_kernel, dim3(1), dim3(kFinal), 0, s, part, sqerr, tiles);
  return check_launch("vector_quantize");
}

}  // extern "C"
