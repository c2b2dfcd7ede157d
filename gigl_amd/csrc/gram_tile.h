// gram_tile.h — one 64 x 64 tile of a Gram-shaped product A B^T at fp32 accuracy on the bf16 matrix cores, shared by the
// pairwise kernels (pairwise.hip: both panels from one matrix) and the contrastive kernels (contrast.hip: the panels of two
// matrices) — and, for their backward kernels, the second product of a function of that tile with one of the panels' matrices
// (gram2_*, below).  Device code only.
#pragma once

#include "split_planes.h"

constexpr int PT = 64;            // rows per tile
constexpr int PBK = 32;           // k per LDS chunk
constexpr int PPLANE = PT * PBK;  // bf16 elements of one plane of one panel

template <bool VEC>  // VEC: d % 4 == 0, ld % 4 == 0 and x 16-byte aligned; rows ld floats apart
__device__ __forceinline__ float4_t pair_load4(const float* __restrict__ x, int n, int64_t ld, int d, int row, int k) {
  float4_t v = {0.f, 0.f, 0.f, 0.f};
  if (row < n) {
    const float* p = x + (int64_t)row * ld + k;
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
// The general form: panel a has na rows lda floats apart, panel b nb rows ldb apart (an activation tile against a weight
// matrix: bootstrap.hip); either may lie in LDS, outside s.
template <bool VEC>
__device__ __forceinline__ float16_t gram_tile(const float* __restrict__ xa, int na, int64_t lda, const float* __restrict__ xb,
                                               int nb, int64_t ldb, int d, int a0, int b0, short (*s)[PPLANE]) {
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
      ra[i] = pair_load4<VEC>(xa, na, lda, d, a0 + lr + 32 * i, k0 + lc);
      rb[i] = pair_load4<VEC>(xb, nb, ldb, d, b0 + lr + 32 * i, k0 + lc);
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

// both panels [n][d] contiguous
template <bool VEC>
__device__ __forceinline__ float16_t gram_tile(const float* __restrict__ xa, const float* __restrict__ xb, int n, int d, int a0,
                                               int b0, short (*s)[PPLANE]) {
  return gram_tile<VEC>(xa, n, d, xb, n, d, d, a0, b0, s);
}

// row (of the 32 x 32 block) that register v of a lane of group g = lane / 32 holds in the D layout; the column is lane % 32
__device__ __forceinline__ constexpr int gram_row(int v, int g) { return 8 * (v >> 2) + 4 * g + (v & 3); }

// The row sums a kernel folds from its accumulators (NS sums, sixteen rows per lane in the D layout) meet: over the 32 lanes
// (., g) of a row by butterfly, then over the two column halves (waves wb = 0, 1) through s_row, [half][sum][row]; afterwards
// thread t < 64 reads row t's totals as s_row[0][j][t] + s_row[1][j][t].  Ends with a barrier.  By all 256 threads.
template <int NS>
__device__ __forceinline__ void gram_rows_meet(float (&rs)[NS][16], float (*s_row)[NS][PT]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, g = lane >> 5;
#pragma unroll
  for (int j = 0; j < NS; ++j)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      float t = rs[j][v];
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
      if (r == 0) s_row[wv & 1][j][(wv >> 1) * 32 + gram_row(v, g)] = t;
    }
  __syncthreads();
}

// ---- the second product ---------------------------------------------------------------------------------------------------
// acc[i][c] += W[i][j] X[j][c] for weights W that are a function of the Gram tile (the backward kernels of pairwise.hip and
// contrast.hip), without W ever leaving the registers.  The first product is taken TRANSPOSED, gram_tile(x, own, .., J0, I0):
// rows j, columns i.  In the D layout a lane then holds one i and sixteen j — which is, up to a fixed permutation of k, the
// A-operand layout of the second product: register v = 8 s2 + t holds row 16 s2 + 8 (t / 4) + 4 g + t % 4 of the 32-row half
// of j, and an operand lane (., g) supplies k = 16 s2 + 8 g + t.  So the kernel computes its weights where the Gram tile lies
// and splits them into planes there (fa[s2][plane], eight registers each), and the permutation (bits 2 and 3 of k swapped,
// pair_kperm) is applied to the OTHER operand, which has to be staged anyway: X_J enters LDS transposed ([column][32 kpos], a
// thread carrying eight j of one column, as the weight-gradient kernel of agg.hip stages its operands), 64 columns at a time.
// A wave owns one 32-row block of i (wi = wave & 1) and one 32-row half of j (wj = wave >> 1): NACC accumulators of 32 x 32
// per 32 columns, CH / 32 of those for the workgroup's CH columns from c0; the two halves of j meet in the epilogue through
// LDS (gram2_meet), in a fixed order.

// position kpos of the second product's k order -> row j of the 32-row half
__device__ __forceinline__ int pair_kperm(int kpos) {
  return (kpos & 0x13) | ((kpos & 4) << 1) | ((kpos & 8) >> 1);
}

// the MFMAs of one 16 k of the second product: plane of the weights, plane of the staged operand, accumulator (< NACC)
struct gram2_sched {
  int pa[6], pb[6], pc[6];
};

// columns [cs, cs + 64) of rows J0 .. J0 + 63 of x ([n][d] contiguous) -> s, transposed: planes 3 h + p hold half h of j as
// [column][32 kpos] under pair_kperm.  split(x, b1, b2, b3): one element -> its three planes (as split3).  Rows >= n and
// columns >= d enter as zeros.  Starts with a barrier (the fragments of the Gram tile / of the previous 64 columns have been
// read) and ends with one.  By all 256 threads.
template <typename Split>
__device__ __forceinline__ void gram2_stage(const float* __restrict__ x, int n, int d, int J0, int cs, short (*s)[PPLANE],
                                            Split split) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  const int col = cs + lane, h = wv >> 1;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int kb = (2 * (wv & 1) + q) * 8;  // this thread: kpos kb .. kb + 7 of column `col`, half h
    float xv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = J0 + 32 * h + pair_kperm(kb + u);
      xv[u] = (j < n && col < d) ? x[(int64_t)j * d + col] : 0.f;
    }
    uint32_t b1[8], b2[8], b3[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) split(xv[u], b1[u], b2[u], b3[u]);
    const int o = split_lds_off(lane, kb);
    *reinterpret_cast<uint4*>(&s[3 * h + 0][o]) = pack8(b1);
    *reinterpret_cast<uint4*>(&s[3 * h + 1][o]) = pack8(b2);
    *reinterpret_cast<uint4*>(&s[3 * h + 2][o]) = pack8(b3);
  }
  __syncthreads();
}

// the staged 64 columns times this wave's weights: acc[cb][SCH.pc[u]] += fa[s2][SCH.pa[u]] x (plane SCH.pb[u] of columns
// 32 cb + ., kpos 16 s2 + .), the six MFMAs of a 16 k in the schedule's order, the two column blocks alternating
template <int NACC, const gram2_sched& SCH>
__device__ __forceinline__ void gram2_mfma(const bf16x8_t (&fa)[2][3], short (*s)[PPLANE], float16_t (*acc)[NACC]) {
  const int lane = threadIdx.x & 63, r = lane & 31, g = lane >> 5, wj = threadIdx.x >> 7;
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    bf16x8_t fb[2][3];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        fb[cb][p] = *reinterpret_cast<const bf16x8_t*>(&s[3 * wj + p][split_lds_off(cb * 32 + r, 16 * s2 + 8 * g)]);
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
        acc[cb][SCH.pc[u]] =
            __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s2][SCH.pa[u]], fb[cb][SCH.pb[u]], acc[cb][SCH.pc[u]], 0, 0, 0);
  }
}

// acc[.][.] += W (fa: this wave's weights of tile J, split) times rows J0 .. J0 + 63 of x, columns [c0, c0 + CH) below d
template <int CH, int NACC, const gram2_sched& SCH, typename Split>
__device__ __forceinline__ void gram2_tile(const bf16x8_t (&fa)[2][3], const float* __restrict__ x, int n, int d, int J0,
                                           int c0, short (*s)[PPLANE], float16_t (&acc)[CH / 32][NACC], Split split) {
#pragma unroll
  for (int sub = 0; sub < CH / 64; ++sub) {
    if (c0 + 64 * sub < d) {  // (the whole workgroup)
      gram2_stage(x, n, d, J0, c0 + 64 * sub, s, split);
      gram2_mfma<NACC, SCH>(fa, s, acc + 2 * sub);
    }
  }
}

// The two halves of j meet, 32 columns at a time: the waves of half 1 put their accumulators into `strip` (LDS: this wave's
// i block's [NACC][32 rows][32 columns] floats, the same for both halves, another for the other i block), the waves of half 0
// then call f(i, c, own, other) — row i0 + local row < n, column < d, this wave's NACC accumulator values of that element and
// half 1's — for every element they hold.  Starts with a barrier: the strips may lie in s.  By all 256 threads.
template <int CH, int NACC, typename F>
__device__ __forceinline__ void gram2_meet(const float16_t (&acc)[CH / 32][NACC], float* strip, int i0, int c0, int n, int d,
                                           F f) {
  const int lane = threadIdx.x & 63, r = lane & 31, g = lane >> 5, wj = threadIdx.x >> 7;
#pragma unroll
  for (int b = 0; b < CH / 32; ++b) {
    if (c0 + 32 * b < d) {  // (the whole workgroup)
      __syncthreads();
      if (wj == 1) {
#pragma unroll
        for (int v = 0; v < 16; ++v)
#pragma unroll
          for (int a = 0; a < NACC; ++a) strip[a * 1024 + gram_row(v, g) * 32 + r] = acc[b][a][v];
      }
      __syncthreads();
      if (wj == 0) {
        const int c = c0 + 32 * b + r;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int il = gram_row(v, g);
          if (i0 + il < n && c < d) {
            float own[NACC], other[NACC];
#pragma unroll
            for (int a = 0; a < NACC; ++a) {
              own[a] = acc[b][a][v];
              other[a] = strip[a * 1024 + il * 32 + r];
            }
            f(i0 + il, c, own, other);
          }
        }
      }
    }
  }
}
