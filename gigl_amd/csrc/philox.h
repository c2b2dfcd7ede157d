// philox.h — the counter-based generator behind the training plans' dropout masks (include/gigl_hip.h:
// gigl_sage_train_plan_set_dropout): Philox4x32-10 with the Random123 constants.  One block = four 32-bit words from a
// 128-bit counter and a 64-bit key; host and device compute the same words.  Internal, nothing exported.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

// what a dropout launch is handed: the key (the seed's halves), the keep threshold T = floor(p 2^32), the kept elements'
// scale 1 / (1 - p) and counter word 3 = (encode << 8) | layer
struct DropoutMask {
  uint32_t key0, key1, thresh, tag;
  float scale;
};

inline DropoutMask gigl_dropout_mask_args(uint64_t seed, float p, int32_t encode, int32_t layer) {
  DropoutMask m;
  m.key0 = (uint32_t)seed;
  m.key1 = (uint32_t)(seed >> 32);
  m.thresh = (uint32_t)((double)p * 4294967296.0);  // (p < 1 as a float: below 2^32)
  m.tag = ((uint32_t)encode << 8) | (uint32_t)layer;
  m.scale = 1.0f / (1.0f - p);
  return m;
}

__host__ __device__ __forceinline__ void gigl_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                            uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// the four words of columns 4 g .. 4 g + 3 of `row`: element (row, col) is kept iff word col & 3 >= m.thresh
__host__ __device__ __forceinline__ void gigl_dropout_words(const DropoutMask& m, uint32_t row, uint32_t g, uint32_t step,
                                                            uint32_t out[4]) {
  gigl_philox4x32_10(row, g, step, m.tag, m.key0, m.key1, out);
}
