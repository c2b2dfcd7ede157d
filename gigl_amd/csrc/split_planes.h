// split_planes.h — the exact-sum split of an fp32 operand into three bf16 planes and the swizzled LDS tile the MFMA fragments
// are read from, shared by the projection kernels (agg.hip, which describes the scheme at linear_split_kernel) and the
// pairwise kernels (pairwise.hip).  Device code only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float float4_t __attribute__((ext_vector_type(4)));
typedef float float16_t __attribute__((ext_vector_type(16)));
typedef short bf16x8_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split3(float x, uint32_t& b1, uint32_t& b2, uint32_t& b3) {
  b1 = __float_as_uint(x) & 0xFFFF0000u;
  const float r1 = x - __uint_as_float(b1);
  b2 = __float_as_uint(r1) & 0xFFFF0000u;
  const float r2 = r1 - __uint_as_float(b2);
  b3 = __float_as_uint(r2) & 0xFFFF0000u;
}

// offset (in bf16 elements) of element k (0..31) of tile row `row` in a swizzled plane
__device__ __forceinline__ int split_lds_off(int row, int k) {
  return row * 32 + ((((k >> 3) ^ (row >> 2)) & 3) << 3) + (k & 7);
}

// four consecutive k of one row -> four bf16 of each plane, stored as 8 bytes per plane
__device__ __forceinline__ void split_store(const float4_t v, short* p1, short* p2, short* p3) {
  uint32_t a1[4], a2[4], a3[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) split3(v[t], a1[t], a2[t], a3[t]);
  *reinterpret_cast<uint2*>(p1) = make_uint2((a1[0] >> 16) | a1[1], (a1[2] >> 16) | a1[3]);
  *reinterpret_cast<uint2*>(p2) = make_uint2((a2[0] >> 16) | a2[1], (a2[2] >> 16) | a2[3]);
  *reinterpret_cast<uint2*>(p3) = make_uint2((a3[0] >> 16) | a3[1], (a3[2] >> 16) | a3[3]);
}
