// gram_tile.h — one 64 x 64 tile of a Gram-shaped product A B^T at fp32 accuracy on the bf16 matrix cores, shared by the
// pairwise kernels (pairwise.hip: both panels from one matrix) and the contrastive kernels (contrast.hip: the panels of two
// matrices).  Device code only.
#pragma once

#include "split_planes.h"

constexpr int PT = 64;            // rows per tile
constexpr int PBK = 32;           // k per LDS chunk
constexpr int PPLANE = PT * PBK;  // bf16 elements of one plane of one panel

template <bool VEC>  // VEC: d % 4 == 0 and x 16-byte aligned
__device__ __forceinline__ float4_t pair_load4(const float* __restrict__ x, int n, int d, int row, int k) {
  float4_t v = {0.f, 0.f, 0.f, 0.f};
  if (row < n) {
    const float* p = x + (int64_t)row * d + k;
    if constexpr (VEC) {
      if (k < d) v = *reinterpret_cast<const float4_t*>(p);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (k + t < d) v[t] = p[t];
    }
  }
  return v;
}

// D[a][b] = <xa[a0 + a], xb[b0 + b]> over the 64 x 64 tile, by all 256 threads (xa, xb: [n][d] contiguous; the same matrix or
// two): wave wv holds the 32 x 32 block (wv >> 1, wv & 1) in the D layout (register v of lane (r, g): row 8 (v / 4) + 4 g +
// v % 4, column r).  The panels pass through LDS in K chunks of 32, split on the way in into three bf16 planes (x = b1 + b2 +
// b3 exactly), six v_mfma_f32_32x32x16_bf16 per 16 k, two accumulators so that dependent MFMAs alternate.  Rows >= n and
// k >= d enter as zeros.  s: six planes (three of each panel).  Starts with a barrier: the caller's earlier reads of s are
// done before it is refilled.
template <bool VEC>
__device__ __forceinline__ float16_t gram_tile(const float* __restrict__ xa, const float* __restrict__ xb, int n, int d, int a0,
                                               int b0, short (*s)[PPLANE]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, g = lane >> 5;
  const int wa = wv >> 1, wb = wv & 1;
  const int lr = tid >> 3, lc = (tid & 7) * 4;  // loader: rows lr, lr + 32; k segment lc .. lc + 3
  float16_t acc0, acc1;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc0[v] = acc1[v] = 0.f;
  float4_t ra[2], rb[2];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ra[i] = pair_load4<VEC>(xa, n, d, a0 + lr + 32 * i, k0 + lc);
      rb[i] = pair_load4<VEC>(xb, n, d, b0 + lr + 32 * i, k0 + lc);
    }
  };
  gload(0);
  for (int k0 = 0; k0 < d; k0 += PBK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int o = split_lds_off(lr + 32 * i, lc);
      split_store(ra[i], &s[0][o], &s[1][o], &s[2][o]);
      split_store(rb[i], &s[3][o], &s[4][o], &s[5][o]);
    }
    __syncthreads();
    if (k0 + PBK < d) gload(k0 + PBK);  // lands during this chunk's MFMAs
    bf16x8_t fa0[3], fb0[3], fa1[3], fb1[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      fa0[p] = *reinterpret_cast<const bf16x8_t*>(&s[p][split_lds_off(wa * 32 + r, 8 * g)]);
      fb0[p] = *reinterpret_cast<const bf16x8_t*>(&s[3 + p][split_lds_off(wb * 32 + r, 8 * g)]);
      fa1[p] = *reinterpret_cast<const bf16x8_t*>(&s[p][split_lds_off(wa * 32 + r, 16 + 8 * g)]);
      fb1[p] = *reinterpret_cast<const bf16x8_t*>(&s[3 + p][split_lds_off(wb * 32 + r, 16 + 8 * g)]);
    }
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};  // smallest terms first
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa0[PA[t]], fb0[PB[t]], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa1[PA[t]], fb1[PB[t]], acc1, 0, 0, 0);
    }
  }
#pragma unroll
  for (int v = 0; v < 16; ++v) acc0[v] += acc1[v];
  return acc0;
}

// position kpos of a second product's k order -> row j of the 32-row half, when the first product was taken transposed and its
// accumulator is the second one's A operand: register v = 8 s + t of the D layout holds row 16 s + 8 (t / 4) + 4 g + t % 4, and
// an operand lane (., g) supplies k = 16 s + 8 g + t
__device__ __forceinline__ int pair_kperm(int kpos) {
  return (kpos & 0x13) | ((kpos & 4) << 1) | ((kpos & 8) >> 1);
}
