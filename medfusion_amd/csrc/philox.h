// philox.h -- the counter-based Gaussian draw every unit generates in registers: Philox-4x32-10 keyed by the 64-bit seed, counter = (quad of 4
// consecutive elements of a sample, sample, draw, 0), Box-Muller on the four outputs (oracle/synth.py: philox_normal is the spec).  One definition:
// mf_philox_normal_f32 (sched_noise.hip) writes these values, the step kernels and the loss kernels (loss.hip) regenerate them bit for bit.
#pragma once
#include "common.h"

namespace mf {

__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
  const uint32_t n1 = (uint32_t)p1;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
  const uint32_t n3 = (uint32_t)p0;
  c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * 5.9604644775390625e-08f; }  // 2^-24

// the 4 standard normals of element quad q of sample `sample` in draw `draw`
__device__ __forceinline__ float4 philox_quad(uint32_t q, uint32_t sample, uint32_t draw, uint32_t seed_lo, uint32_t seed_hi) {
  uint32_t c0 = q, c1 = sample, c2 = draw, c3 = 0u;
  uint32_t k0 = seed_lo, k1 = seed_hi;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const float r0 = sqrtf(-2.0f * logf(u01(c0))), t0 = 6.283185307179586f * u01(c1);
  const float r1 = sqrtf(-2.0f * logf(u01(c2))), t1 = 6.283185307179586f * u01(c3);
  float s0, cs0, s1, cs1;
  sincosf(t0, &s0, &cs0);
  sincosf(t1, &s1, &cs1);
  return make_float4(r0 * cs0, r0 * s0, r1 * cs1, r1 * s1);
}

}  // namespace mf
