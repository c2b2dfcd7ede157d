// hadamard.hip — the hadamard_MLP link decoder with one hidden layer (python/gigl/src/common/models/layers/decoder.py:64-70 with
// decoder_channel_list [D, h, 1]), scores of all Q x C pairs and their gradient, without a per-pair tensor in HBM:
//     pre[q,c,j] = sum_k W0[j,k] q[q,k] c[c,k] + b0[j],  hid = relu(pre),  s = sum_j w1[j] hid[q,c,j] + b1,
//     scores[q,c] = s (plain_last) or relu(s)
// The first layer is a GEMM whose M axis is pairs and whose A panel, q (.) c, exists only on the way into LDS.
//   tiles     A workgroup's 64 pair-rows are ONE query against 64 consecutive candidates; it walks tq queries (a query block)
//             over the same candidate tile.  The loader (had_tile, gram_tile's loop with another A loader) reads the candidate
//             rows and one 16-byte segment of the query row, multiplies in fp32 and splits the product into the three bf16
//             planes; W0 is the other panel, 64 hidden units at a time.  A query's 64 scores are one contiguous segment of its
//             row of the output; with a fixed query the sums over candidates (dq) are column sums of the tile and the sums over
//             queries (dc) stay in the accumulators while the workgroup walks its query block.
//   forward   had_forward_kernel: per query and block of 64 hidden units the tile [pair][hidden]; bias, ReLU and the product
//             with w1 are folded from the accumulators, the rows meet (gram_rows_meet), 64 threads write the scores.
//   backward  Nothing is kept from the forward: both kernels rebuild pre per tile.  Without plain_last the clamp needs the WHOLE
//             score before any dpre = dS' w1[j] [pre > 0] is formed: h <= 64 gets it from the tile it has, beyond that a first
//             walk over the blocks of h computes it.
//             had_rowgrad_kernel (dq, dc): the tile TRANSPOSED, [hidden][pair], so that dpre lies in the A layout of the
//             second product dP[pair][k] = sum_j dpre W0[j][k] (gram2_tile with W0 as the staged operand, 64 columns of k per
//             workgroup: dP's and dc's accumulators both stay in registers).  Per query: dc's accumulators += dP q[k]; the column sums of dP (.) c are the tile's part of dq[q].
//             had_wgrad_kernel (dW0, db0, dw1, db1): the tile [pair][hidden], dpre the A operand of dW0[j][k] = sum_pairs dpre
//             (q (.) c)[k], the staged operand again the implicit panel (had2_stage: gram2_stage with the query's scale); db0,
//             dw1 (column sums) and db1 come out of the same walk.  One workgroup per (query block, candidate tile, block of
//             h, 128 columns of k).
//             No float atomics: the parts go to the ctx's arena — dq [candidate tiles][Q][D], dc [query blocks][C][D], dW0
//             [workgroups][h][D], db0 / dw1 [workgroups][h], db1 [workgroups] — and had_fold_kernel adds them in index order
//             (fp64 accumulators).  The same inputs give the same bits.
#include "common.h"
#include "dispatch.h"
#include "gram_tile.h"
#include "wave_reduce.h"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int HAD_MAX = 512;  // D and h
constexpr int HCH = 128;      // columns of k per workgroup in the weight gradient's second product
constexpr int RCH = 64;       // ... in the row gradients', which keep two sets of accumulators (dP and dc)
constexpr gram2_sched HAD_SCHED = {{2, 0, 1, 1, 0, 0}, {0, 2, 1, 0, 1, 0}, {0, 0, 0, 0, 0, 0}};  // smallest terms first

struct had_args {
  const float *q, *c;
  int64_t ldq, ldc;
  const float *w0, *b0, *w1, *b1;  // W0 [h][d] contiguous; b0, b1 may be NULL
  int nq, nc, d, h, tq, plain_last;
};

// One 64 x 64 tile of the first layer before its bias, gram_tile's loop: the pairs (qrow, candidate c0 + .) against the hidden
// units h0 + ..  PAIR_ROWS: rows are pairs and columns hidden units; otherwise the transpose.  Candidates >= nc, hidden units
// >= h and k >= d enter as zeros.  Starts with a barrier.
template <bool VEC, bool PAIR_ROWS>
__device__ __forceinline__ float16_t had_tile(const had_args& a, const float* __restrict__ qrow, int c0, int h0,
                                              short (*s)[PPLANE]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, g = lane >> 5;
  const int wa = wv >> 1, wb = wv & 1;
  const int lr = tid >> 3, lc = (tid & 7) * 4;
  constexpr int SP = PAIR_ROWS ? 0 : 3, SW = PAIR_ROWS ? 3 : 0;  // planes of the pair panel and of W0's
  float16_t acc0, acc1;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc0[v] = acc1[v] = 0.f;
  float4_t rp[2], rw[2];
  auto gload = [&](int k0) {
    const float4_t qv = pair_load4<VEC>(qrow, 1, 0, a.d, 0, k0 + lc);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      rp[i] = pair_load4<VEC>(a.c, a.nc, a.ldc, a.d, c0 + lr + 32 * i, k0 + lc) * qv;  // q (.) c, rounded once as in fp32 torch
      rw[i] = pair_load4<VEC>(a.w0, a.h, a.d, a.d, h0 + lr + 32 * i, k0 + lc);
    }
  };
  gload(0);
  for (int k0 = 0; k0 < a.d; k0 += PBK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int o = split_lds_off(lr + 32 * i, lc);
      split_store(rp[i], &s[SP][o], &s[SP + 1][o], &s[SP + 2][o]);
      split_store(rw[i], &s[SW][o], &s[SW + 1][o], &s[SW + 2][o]);
    }
    __syncthreads();
    if (k0 + PBK < a.d) gload(k0 + PBK);
    bf16x8_t fa0[3], fb0[3], fa1[3], fb1[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      fa0[p] = *reinterpret_cast<const bf16x8_t*>(&s[p][split_lds_off(wa * 32 + r, 8 * g)]);
      fb0[p] = *reinterpret_cast<const bf16x8_t*>(&s[3 + p][split_lds_off(wb * 32 + r, 8 * g)]);
      fa1[p] = *reinterpret_cast<const bf16x8_t*>(&s[p][split_lds_off(wa * 32 + r, 16 + 8 * g)]);
      fb1[p] = *reinterpret_cast<const bf16x8_t*>(&s[3 + p][split_lds_off(wb * 32 + r, 16 + 8 * g)]);
    }
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
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

// gram2_stage for the implicit panel: columns [cs, cs + 64) of the pairs (qrow, candidate c0 + j), j = 0 .. 63, transposed into
// the planes as gram2_stage does.  Starts and ends with a barrier.
__device__ __forceinline__ void had2_stage(const had_args& a, const float* __restrict__ qrow, int c0, int cs, short (*s)[PPLANE]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  const int col = cs + lane, h = wv >> 1;
  const float qk = col < a.d ? qrow[col] : 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int kb = (2 * (wv & 1) + q) * 8;
    float xv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = c0 + 32 * h + pair_kperm(kb + u);
      xv[u] = (j < a.nc && col < a.d) ? a.c[(int64_t)j * a.ldc + col] * qk : 0.f;
    }
    uint32_t b1[8], b2[8], b3[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) split3(xv[u], b1[u], b2[u], b3[u]);
    const int o = split_lds_off(lane, kb);
    *reinterpret_cast<uint4*>(&s[3 * h + 0][o]) = pack8(b1);
    *reinterpret_cast<uint4*>(&s[3 * h + 1][o]) = pack8(b2);
    *reinterpret_cast<uint4*>(&s[3 * h + 2][o]) = pack8(b3);
  }
  __syncthreads();
}

// w1 and b0 padded with zeros to 512 entries: a hidden unit >= h contributes nothing anywhere
__device__ __forceinline__ void had_load_head(const had_args& a, float* s_w1, float* s_b0) {
  for (int t = threadIdx.x; t < HAD_MAX; t += 256) {
    s_w1[t] = t < a.h ? a.w1[t] : 0.f;
    s_b0[t] = (a.b0 && t < a.h) ? a.b0[t] : 0.f;
  }
  __syncthreads();
}

// the [pair][hidden] tile's part of the rows' scores: rs[v] += w1[j] relu(acc[v] + b0[j]), j this lane's column
__device__ __forceinline__ void had_fold_rows(const float16_t& acc, float w1v, float b0v, float (&rs)[16]) {
#pragma unroll
  for (int v = 0; v < 16; ++v) rs[v] += w1v * fmaxf(acc[v] + b0v, 0.f);
}

// grid: (candidate tiles, query blocks of tq)
template <bool VEC>
__global__ __launch_bounds__(256) void had_forward_kernel(const had_args a, float* __restrict__ scores, int64_t lds) {
  __shared__ __attribute__((aligned(16))) short s[6][PPLANE];
  __shared__ float s_row[2][1][PT];
  __shared__ float s_w1[HAD_MAX], s_b0[HAD_MAX];
  const int tid = threadIdx.x, wv = tid >> 6, r = tid & 31, wb = wv & 1;
  const int c0 = blockIdx.x * PT, q0 = blockIdx.y * a.tq, q1 = min(q0 + a.tq, a.nq);
  const float b1 = a.b1 ? *a.b1 : 0.f;
  had_load_head(a, s_w1, s_b0);
  for (int qi = q0; qi < q1; ++qi) {
    const float* qrow = a.q + (int64_t)qi * a.ldq;
    float rs[1][16];
#pragma unroll
    for (int v = 0; v < 16; ++v) rs[0][v] = 0.f;
    for (int h0 = 0; h0 < a.h; h0 += PT) {
      const float16_t acc = had_tile<VEC, true>(a, qrow, c0, h0, s);
      const int hj = h0 + wb * 32 + r;
      had_fold_rows(acc, s_w1[hj], s_b0[hj], rs[0]);
    }
    gram_rows_meet<1>(rs, s_row);
    if (tid < PT && c0 + tid < a.nc) {
      const float sc = s_row[0][0][tid] + s_row[1][0][tid] + b1;
      scores[(int64_t)qi * lds + c0 + tid] = (a.plain_last || !(sc < 0.f)) ? sc : 0.f;
    }
  }
}

// s_ds[p] = dS'[qi][c0 + p]: the score's gradient where the pair exists and (without plain_last) its score is positive; sc: the
// two halves of the row's score, valid for tid < 64 when the clamp applies.  Ends with a barrier.  -> dS' of row tid (tid < 64)
__device__ __forceinline__ float had_row_grads(const had_args& a, const float* __restrict__ ds, int64_t ldds, int qi, int c0,
                                               const float* sc0, const float* sc1, float b1, float* s_ds) {
  const int tid = threadIdx.x;
  float dv = 0.f;
  if (tid < PT) {
    if (c0 + tid < a.nc) dv = ds[(int64_t)qi * ldds + c0 + tid];
    if (!a.plain_last && !(sc0[tid] + sc1[tid] + b1 > 0.f)) dv = 0.f;
    s_ds[tid] = dv;
  }
  __syncthreads();
  return dv;
}

// grid: (candidate tiles, query blocks, 64-column chunks of d).  part_q [candidate tiles][nq][d], part_c [query blocks][nc][d]
template <bool VEC>
__global__ __launch_bounds__(256) void had_rowgrad_kernel(const had_args a, const float* __restrict__ ds, int64_t ldds,
                                                          float* __restrict__ part_q, float* __restrict__ part_c) {
  __shared__ __attribute__((aligned(16))) short s[6][PPLANE];
  __shared__ float s_col[2][PT], s_ds[PT], s_cs[4][RCH];
  __shared__ float s_w1[HAD_MAX], s_b0[HAD_MAX];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, g = lane >> 5;
  const int wj = wv >> 1, wi = wv & 1;  // the tile is [hidden][pair]: this lane's pair is wi * 32 + r
  const int c0 = blockIdx.x * PT, q0 = blockIdx.y * a.tq, q1 = min(q0 + a.tq, a.nq), kc0 = blockIdx.z * RCH;
  const bool need_s = !a.plain_last, one_block = a.h <= PT;
  const float b1 = a.b1 ? *a.b1 : 0.f;
  had_load_head(a, s_w1, s_b0);
  float16_t dcacc[RCH / 32][1];
#pragma unroll
  for (int b = 0; b < RCH / 32; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) dcacc[b][0][v] = 0.f;
  for (int qi = q0; qi < q1; ++qi) {
    const float* qrow = a.q + (int64_t)qi * a.ldq;
    float16_t acc;
    if (need_s) {  // the pairs' scores: column sums of the transposed tiles
      float t = 0.f;
      for (int h0 = 0; h0 < a.h; h0 += PT) {
        acc = had_tile<VEC, false>(a, qrow, c0, h0, s);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int hj = h0 + wj * 32 + gram_row(v, g);
          t += s_w1[hj] * fmaxf(acc[v] + s_b0[hj], 0.f);
        }
      }
      t += __shfl_xor(t, 32, 64);
      if (g == 0) s_col[wj][wi * 32 + r] = t;
      __syncthreads();
    }
    had_row_grads(a, ds, ldds, qi, c0, s_col[0], s_col[1], b1, s_ds);
    const float dv = s_ds[wi * 32 + r];
    float16_t acc2[RCH / 32][1];
#pragma unroll
    for (int b = 0; b < RCH / 32; ++b)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc2[b][0][v] = 0.f;
    for (int h0 = 0; h0 < a.h; h0 += PT) {
      if (!(need_s && one_block)) acc = had_tile<VEC, false>(a, qrow, c0, h0, s);
      bf16x8_t fa[2][3];  // dpre where the tile lies, split into the second product's A fragments
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float wt[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int v = 8 * s2 + u, hj = h0 + wj * 32 + gram_row(v, g);
          wt[u] = acc[v] + s_b0[hj] > 0.f ? dv * s_w1[hj] : 0.f;
        }
        split8(wt, fa[s2][0], fa[s2][1], fa[s2][2]);
      }
      gram2_tile<RCH, 1, HAD_SCHED>(fa, a.w0, a.h, a.d, h0, kc0, s, acc2,
                                    [](float x, uint32_t& b1, uint32_t& b2, uint32_t& b3) { split3(x, b1, b2, b3); });
    }
    // this wave's half of dP (the halves of j add up linearly): dc += dP q[k]; dq's part: the column sums of dP (.) c
#pragma unroll
    for (int b = 0; b < RCH / 32; ++b) {
      const int k = kc0 + 32 * b + r;
      const float qk = k < a.d ? qrow[k] : 0.f;
      float sum = 0.f;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int row = c0 + wi * 32 + gram_row(v, g);
        const float cv = (k < a.d && row < a.nc) ? a.c[(int64_t)row * a.ldc + k] : 0.f;
        dcacc[b][0][v] += acc2[b][0][v] * qk;
        sum += acc2[b][0][v] * cv;
      }
      sum += __shfl_xor(sum, 32, 64);
      if (g == 0) s_cs[wv][32 * b + r] = sum;
      __builtin_amdgcn_sched_barrier(0);  // one block's sixteen loads of c in flight, not all four blocks'
    }
    __syncthreads();
    if (tid < RCH && kc0 + tid < a.d)
      part_q[((int64_t)blockIdx.x * a.nq + qi) * a.d + kc0 + tid] = (s_cs[0][tid] + s_cs[1][tid]) + (s_cs[2][tid] + s_cs[3][tid]);
  }
  float* strip = reinterpret_cast<float*>(&s[0][0]) + wi * 1024;
  gram2_meet<RCH, 1>(dcacc, strip, c0 + wi * 32, kc0, a.nc, a.d, [&](int i, int c, const float (&lo)[1], const float (&hi)[1]) {
    part_c[((int64_t)blockIdx.y * a.nc + i) * a.d + c] = lo[0] + hi[0];
  });
}

// grid: (candidate tiles x query blocks = S, blocks of 64 hidden units, 128-column chunks of d).  part_w [S][h][d]; part_b:
// dw1 [S][h], then db0 [S][h], then db1 [S]
template <bool VEC>
__global__ __launch_bounds__(256) void had_wgrad_kernel(const had_args a, const float* __restrict__ ds, int64_t ldds,
                                                        float* __restrict__ part_w, float* __restrict__ part_b) {
  __shared__ __attribute__((aligned(16))) short s[6][PPLANE];
  __shared__ float s_row[2][1][PT], s_ds[PT], s_col[2][2][PT];
  __shared__ float s_w1[HAD_MAX], s_b0[HAD_MAX];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, g = lane >> 5;
  const int wj = wv >> 1, wi = wv & 1;  // the tile is [pair][hidden]: this lane's hidden unit is hy0 + wi * 32 + r
  const int ctn = (a.nc + PT - 1) / PT, S = gridDim.x;
  const int c0 = (blockIdx.x % ctn) * PT, q0 = (blockIdx.x / ctn) * a.tq, q1 = min(q0 + a.tq, a.nq);
  const int hy0 = blockIdx.y * PT, kc0 = blockIdx.z * HCH;
  const bool need_s = !a.plain_last, one_block = a.h <= PT;
  const float b1 = a.b1 ? *a.b1 : 0.f;
  had_load_head(a, s_w1, s_b0);
  const float w1v = s_w1[hy0 + wi * 32 + r], b0v = s_b0[hy0 + wi * 32 + r];
  float16_t acc2[HCH / 32][1];
#pragma unroll
  for (int b = 0; b < HCH / 32; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc2[b][0][v] = 0.f;
  float cw = 0.f, cb = 0.f, c1 = 0.f;  // this lane's parts of dw1[j], db0[j]; row tid's of db1
  for (int qi = q0; qi < q1; ++qi) {
    const float* qrow = a.q + (int64_t)qi * a.ldq;
    float16_t acc;
    if (need_s) {
      float rs[1][16];
#pragma unroll
      for (int v = 0; v < 16; ++v) rs[0][v] = 0.f;
      for (int h0 = 0; h0 < a.h; h0 += PT) {
        acc = had_tile<VEC, true>(a, qrow, c0, h0, s);
        const int hj = h0 + wi * 32 + r;
        had_fold_rows(acc, s_w1[hj], s_b0[hj], rs[0]);
      }
      gram_rows_meet<1>(rs, s_row);
    }
    c1 += had_row_grads(a, ds, ldds, qi, c0, s_row[0][0], s_row[1][0], b1, s_ds);
    if (!(need_s && one_block)) acc = had_tile<VEC, true>(a, qrow, c0, hy0, s);
    bf16x8_t fa[2][3];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      float wt[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int v = 8 * s2 + u;
        const float dv = s_ds[wj * 32 + gram_row(v, g)], pre = acc[v] + b0v;
        cw += dv * fmaxf(pre, 0.f);
        wt[u] = pre > 0.f ? dv * w1v : 0.f;
        cb += wt[u];
      }
      split8(wt, fa[s2][0], fa[s2][1], fa[s2][2]);
    }
#pragma unroll
    for (int sub = 0; sub < HCH / 64; ++sub) {
      if (kc0 + 64 * sub < a.d) {  // (the whole workgroup)
        had2_stage(a, qrow, c0, kc0 + 64 * sub, s);
        gram2_mfma<1, HAD_SCHED>(fa, s, acc2 + 2 * sub);
      }
    }
  }
  // the column sums meet: the two row groups of a lane pair, then the two halves of the pairs
  cw += __shfl_xor(cw, 32, 64);
  cb += __shfl_xor(cb, 32, 64);
  if (g == 0) {
    s_col[wj][0][wi * 32 + r] = cw;
    s_col[wj][1][wi * 32 + r] = cb;
  }
  __syncthreads();
  if (blockIdx.z == 0 && tid < PT) {
    if (hy0 + tid < a.h) {
      part_b[(int64_t)blockIdx.x * a.h + hy0 + tid] = s_col[0][0][tid] + s_col[1][0][tid];
      part_b[((int64_t)S + blockIdx.x) * a.h + hy0 + tid] = s_col[0][1][tid] + s_col[1][1][tid];
    }
    if (blockIdx.y == 0) {
      const float t = (float)gigl_wave_sum_f64((double)c1);
      if (tid == 0) part_b[2 * (int64_t)S * a.h + blockIdx.x] = t;
    }
  }
  float* strip = reinterpret_cast<float*>(&s[0][0]) + wi * 1024;
  gram2_meet<HCH, 1>(acc2, strip, hy0 + wi * 32, kc0, a.h, a.d, [&](int i, int c, const float (&lo)[1], const float (&hi)[1]) {
    part_w[((int64_t)blockIdx.x * a.h + i) * a.d + c] = lo[0] + hi[0];
  });
}

// out[row][col] = sum over t < T of part[t][row][col] in ascending t within each of four interleaved slices, the slices in
// order; rows ld floats apart.  grid: 64 elements per workgroup.
__global__ __launch_bounds__(256) void had_fold_kernel(const float* __restrict__ part, int T, int64_t n, int cols,
                                                       float* __restrict__ out, int64_t ld) {
  __shared__ double s_f[4][64];
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + lane;
  double acc = 0.0;
  if (i < n)
    for (int t = sl; t < T; t += 4) acc += (double)part[(int64_t)t * n + i];
  s_f[sl][lane] = acc;
  __syncthreads();
  if (sl == 0 && i < n) out[(i / cols) * ld + i % cols] = (float)((s_f[0][lane] + s_f[1][lane]) + (s_f[2][lane] + s_f[3][lane]));
}

void had_fold(hipStream_t st, const float* part, int T, int rows, int cols, float* out, int64_t ld) {
  const int64_t n = (int64_t)rows * cols;
  if (n <= 0 || !out) return;
  hipLaunchKernelGGL(had_fold_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, part, T, n, cols, out, ld);
}

// queries per workgroup: 64, halved while that leaves fewer than 512 workgroups (two per compute unit), at least 4; doubled
// while the query blocks would not fit a grid dimension
int had_tq(int nq, int nc) {
  const int64_t ct = ((int64_t)nc + PT - 1) / PT;
  int tq = 64;
  while (tq > 4 && ct * ((nq + tq - 1) / tq) < 512) tq >>= 1;
  while ((nq + tq - 1) / tq > 65535) tq <<= 1;
  return tq;
}

int32_t had_check(gigl_ctx* ctx, const float* q, int64_t ld_q, const float* c, int64_t ld_c, const float* w0, const float* w1,
                  int32_t nq, int32_t nc, int32_t d, int32_t h) {
  GIGL_REQUIRE(ctx, d >= 1 && d <= HAD_MAX && h >= 1 && h <= HAD_MAX,
               "the hadamard_MLP kernels serve 1 <= D, h <= %d (D=%d, h=%d)", HAD_MAX, d, h);
  GIGL_REQUIRE(ctx, nq >= 0 && nc >= 0 && nc <= (1 << 30), "Q=%d, C=%d out of range", nq, nc);
  GIGL_REQUIRE(ctx, w0 && w1 && (nq == 0 || (q && ld_q >= d)) && (nc == 0 || (c && ld_c >= d)),
               "null argument or a row stride below D");
  return GIGL_OK;
}

bool had_vec(const had_args& a) {
  return a.d % 4 == 0 && a.ldq % 4 == 0 && a.ldc % 4 == 0 && gigl_aligned16(a.q) && gigl_aligned16(a.c) && gigl_aligned16(a.w0);
}

}  // namespace

extern "C" {

int32_t gigl_hadamard_mlp_scores(gigl_ctx* ctx, const float* q, int64_t ld_q, const float* c, int64_t ld_c, const float* w0,
                                 const float* b0, const float* w1, const float* b1, int32_t n_q, int32_t n_c, int32_t d, int32_t h,
                                 int32_t plain_last, float* scores, int64_t ld_s) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const int32_t rc = had_check(ctx, q, ld_q, c, ld_c, w0, w1, n_q, n_c, d, h);
  if (rc != GIGL_OK) return rc;
  if (n_q == 0 || n_c == 0) return GIGL_OK;
  GIGL_REQUIRE(ctx, scores && ld_s >= n_c, "scores is null or its row stride is below C");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const had_args a = {q, c, ld_q, ld_c, w0, b0, w1, b1, n_q, n_c, d, h, had_tq(n_q, n_c), plain_last != 0};
  const dim3 grid((unsigned)((n_c + PT - 1) / PT), (unsigned)((n_q + a.tq - 1) / a.tq));
  dispatch_bool(had_vec(a), [&](auto v) {
    hipLaunchKernelGGL(had_forward_kernel<decltype(v)::value>, grid, dim3(256), 0, ctx->stream, a, scores, ld_s);
  });
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_hadamard_mlp_scores_backward(gigl_ctx* ctx, const float* q, int64_t ld_q, const float* c, int64_t ld_c,
                                          const float* w0, const float* b0, const float* w1, const float* b1,
                                          const float* d_scores, int64_t ld_ds, int32_t n_q, int32_t n_c, int32_t d, int32_t h,
                                          int32_t plain_last, float* dq, int64_t ld_dq, float* dc, int64_t ld_dc, float* dw0,
                                          float* db0, float* dw1, float* db1) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const int32_t rc0 = had_check(ctx, q, ld_q, c, ld_c, w0, w1, n_q, n_c, d, h);
  if (rc0 != GIGL_OK) return rc0;
  GIGL_REQUIRE(ctx, dw0 && dw1 && (n_q == 0 || (dq && ld_dq >= d)) && (n_c == 0 || (dc && ld_dc >= d)),
               "null gradient or a row stride below D");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (n_q == 0 || n_c == 0) {  // no pairs: every gradient is zero
    if (n_q > 0) gigl_zero_rows(st, dq, ld_dq, n_q, d);
    if (n_c > 0) gigl_zero_rows(st, dc, ld_dc, n_c, d);
    gigl_zero_rows(st, dw0, d, h, d);
    gigl_zero_rows(st, dw1, h, 1, h);
    if (db0) gigl_zero_rows(st, db0, h, 1, h);
    if (db1) gigl_zero_rows(st, db1, 1, 1, 1);
    GIGL_HIP_CHECK(ctx, hipGetLastError());
    return GIGL_OK;
  }
  GIGL_REQUIRE(ctx, d_scores && ld_ds >= n_c, "d_scores is null or its row stride is below C");
  const had_args a = {q, c, ld_q, ld_c, w0, b0, w1, b1, n_q, n_c, d, h, had_tq(n_q, n_c), plain_last != 0};
  const int64_t ct = (n_c + PT - 1) / PT, qb = (n_q + a.tq - 1) / a.tq, S = ct * qb;
  GIGL_REQUIRE(ctx, S < ((int64_t)1 << 31), "Q x C too large for one call (%lld workgroups)", (long long)S);
  const int64_t q_bytes = gigl_align_up(ct * n_q * d * 4, 256), c_bytes = gigl_align_up(qb * n_c * d * 4, 256);
  const int64_t w_bytes = gigl_align_up(S * h * d * 4, 256), b_bytes = gigl_align_up((2 * S * h + S) * 4, 256);
  const int32_t rc = gigl_arena_reset(ctx, q_bytes + c_bytes + w_bytes + b_bytes + 1024);
  if (rc != GIGL_OK) return rc;
  float* part_q = (float*)gigl_arena_alloc(ctx, q_bytes);
  float* part_c = (float*)gigl_arena_alloc(ctx, c_bytes);
  float* part_w = (float*)gigl_arena_alloc(ctx, w_bytes);
  float* part_b = (float*)gigl_arena_alloc(ctx, b_bytes);
  GIGL_REQUIRE(ctx, part_q && part_c && part_w && part_b, "scratch arena exhausted");
  const unsigned kz = (unsigned)((d + HCH - 1) / HCH), rz = (unsigned)((d + RCH - 1) / RCH), hy = (unsigned)((h + PT - 1) / PT);
  dispatch_bool(had_vec(a), [&](auto v) {
    constexpr bool V = decltype(v)::value;
    hipLaunchKernelGGL(had_rowgrad_kernel<V>, dim3((unsigned)ct, (unsigned)qb, rz), dim3(256), 0, st, a, d_scores, ld_ds, part_q,
                       part_c);
    hipLaunchKernelGGL(had_wgrad_kernel<V>, dim3((unsigned)S, hy, kz), dim3(256), 0, st, a, d_scores, ld_ds, part_w, part_b);
  });
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  had_fold(st, part_q, (int)ct, n_q, d, dq, ld_dq);
  had_fold(st, part_c, (int)qb, n_c, d, dc, ld_dc);
  had_fold(st, part_w, (int)S, h, d, dw0, d);
  had_fold(st, part_b, (int)S, 1, h, dw1, h);
  had_fold(st, part_b + S * h, (int)S, 1, h, db0, h);
  had_fold(st, part_b + 2 * S * h, (int)S, 1, 1, db1, 1);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

}  // extern "C"
