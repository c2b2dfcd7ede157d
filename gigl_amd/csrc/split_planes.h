// split_planes.h — the exact-sum split of an fp32 operand into three bf16 planes, the packing of a plane's bf16 values and the
// swizzled LDS tile the MFMA fragments are read from, shared by the projection and weight-gradient kernels (agg.hip, which
// describes the scheme at linear_split_kernel) and, through gram_tile.h, the pairwise kernels (pairwise.hip) and the
// contrastive kernels (contrast.hip).  Device code only.
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

// eight plane values (each a float's bits with the low 16 cleared, split3's b) -> their bf16 halves, in order, as 16 bytes
__device__ __forceinline__ uint4 pack8(const uint32_t (&b)[8]) {
  return make_uint4((b[0] >> 16) | b[1], (b[2] >> 16) | b[3], (b[4] >> 16) | b[5], (b[6] >> 16) | b[7]);
}

// eight floats -> the three bf16 planes of a fragment (or of 16 bytes of a plane in LDS)
__device__ __forceinline__ void split8(const float (&x)[8], bf16x8_t& f1, bf16x8_t& f2, bf16x8_t& f3) {
  uint32_t b1[8], b2[8], b3[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) split3(x[u], b1[u], b2[u], b3[u]);
  f1 = __builtin_bit_cast(bf16x8_t, pack8(b1));
  f2 = __builtin_bit_cast(bf16x8_t, pack8(b2));
  f3 = __builtin_bit_cast(bf16x8_t, pack8(b3));
}
