// contrast.hip — the GRACE two-view contrastive loss (python/gigl/src/common/models/layers/loss.py:362-416) and its gradient
// as Gram-shaped MFMA kernels that write nothing of size n x n.
//
// h1, h2 fp32 [n][d] (rows `ld` floats apart, not normalised), T the temperature.  The reference's formula in log space:
//     a_i = h1_i / max(|h1_i|, 1e-8)   b_i = h2_i / max(|h2_i|, 1e-8)   z11 = a a^T / T   z12 = a b^T / T   z22 = b b^T / T
//     L1_i = log(sum_{j != i} e^{z11_ij} + sum_j e^{z12_ij})     L2_i = log(sum_{j != i} e^{z22_ij} + sum_j e^{z12_ji})
//     loss = (1 / n) sum_i ((L1_i + L2_i) / 2 - z12_ii)
// The reference takes exp(sim / T) of four n x n matrices, row sums and a log — and overflows to NaN at its own default T =
// 0.001; the running maximum below gives the finite value the formula means.
//   prep      one wave per row i: both norms, a_i and b_i as contiguous [n][d], dg_i = <a_i, b_i> / T — the diagonal term
//             of the loss comes from here (fixed order), not from a Gram tile.
//   forward   one workgroup per (view v, 64-row tile I), sweeping every column tile J of its own view and of the other one.
//             The Gram tile (gram_tile.h) is taken TRANSPOSED (rows j, columns i): in the 32 x 32 D layout a lane holds one
//             row i of the loss and sixteen j, so the row's running maximum m and rescaled sum s live in that lane's
//             registers — m' = max(m, z), s = s e^(m - m') + sum e^(z - m') — and update without cross-lane traffic.  The two
//             lane groups (a shuffle) and the two waves (LDS) that share a row meet once, at the end, in a fixed order:
//             L_v[i] = m + log s.  Masks: j >= n everywhere, j == i in the own-view tile.  grace_fold_kernel adds the rows
//             in fp64 in a fixed order.  No atomics: a row has one owner and one order.
//   backward  with w_ij = e^(z_ij - L_v[i]) + e^(z_ij - L_u[j]) (u = v in the own-view tiles, the other view otherwise):
//                 ga_i = (g / (2 n T)) [sum_{j != i} w11_ij a_j + sum_j w12_ij b_j - 2 b_i],   gb_i its mirror image.
//             One workgroup per (view, row tile I, 128-column chunk of d), sweeping every J, two Gram tiles and two second
//             products (own view, other view) per J: the weights are computed from the TRANSPOSED Gram tile, where they
//             lie, and multiplied into the rows by gram_tile.h's second product (which explains the layout), as in
//             pair_backward_kernel (pairwise.hip).  Both operands are split with the plain split3 (a row's weights sum to
//             about 2: nothing here cancels as DirectAU's r_i x_i does); the two halves of j meet in the epilogue through
//             LDS, in a fixed order.
//   norm bwd  one wave per row: gh_i = (ga_i - <ga_i, a_i> a_i) / |h_i|, or ga_i / 1e-8 where |h_i| <= 1e-8 (autograd
//             through the reference's torch.max(norm, eps)).
#include "common.h"
#include "dispatch.h"
#include "gram_tile.h"
#include "wave_reduce.h"

#include <cmath>
#include <cstdint>

namespace {

constexpr int GCH = 128;  // columns of d per backward workgroup
constexpr int GMAXD = 512;
constexpr int32_t GRACE_MAX_N = 1 << 18;
constexpr float GEPS = 1e-8f;

// ---- prep -------------------------------------------------------------------------------------------------------------
// one wave per row: nrm[v n + i] = |h_v,i|, a_i and b_i normalised, dg[i] = <a_i, b_i> / T
__global__ __launch_bounds__(256) void grace_prep_kernel(const float* __restrict__ h1, int64_t ld1, const float* __restrict__ h2,
                                                         int64_t ld2, int n, int d, float inv_t, float* __restrict__ a,
                                                         float* __restrict__ b, float* __restrict__ nrm, float* __restrict__ dg) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float *r1 = h1 + (int64_t)i * ld1, *r2 = h2 + (int64_t)i * ld2;
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < d; c += 64) {
    s1 += r1[c] * r1[c];
    s2 += r2[c] * r2[c];
  }
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_xor(s1, off, 64);
    s2 += __shfl_xor(s2, off, 64);
  }
  const float n1 = sqrtf(s1), n2 = sqrtf(s2);
  // a true division, as the reference's a / max(norm, eps): at d = 1 the rows are EXACTLY +-1 and the normalisation's
  // gradient ga - <ga, a> a is exactly 0, as it is mathematically (a reciprocal's 1 - ulp would leave 1e-7 of ga)
  const float q1 = fmaxf(n1, GEPS), q2 = fmaxf(n2, GEPS);
  float dot = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float x = r1[c] / q1, y = r2[c] / q2;
    a[(int64_t)i * d + c] = x;
    b[(int64_t)i * d + c] = y;
    dot += x * y;
  }
  for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off, 64);
  if (lane == 0) {
    nrm[i] = n1;
    nrm[n + i] = n2;
    dg[i] = dot * inv_t;
  }
}

// ---- forward ------------------------------------------------------------------------------------------------------------
// one part of a running (max, sum) brought to the common maximum M (a part that saw no entry: m = -inf, nothing)
__device__ __forceinline__ float grace_part(float m, float s, float M) { return m == -INFINITY ? 0.f : s * expf(m - M); }

// L[v n + i] for view v = blockIdx.y and the rows of tile blockIdx.x; a, b [n][d] contiguous
template <bool VEC>
__global__ __launch_bounds__(256) void grace_lse_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, int d,
                                                        float inv_t, float* __restrict__ L) {
  __shared__ __attribute__((aligned(16))) short s[6][PPLANE];
  __shared__ float s_m[PT], s_s[PT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, g = lane >> 5;
  const int wj = wv >> 1, wi = wv & 1;  // this wave: rows j of half wj (the product's rows), i block wi (its columns)
  const int view = blockIdx.y, I0 = blockIdx.x * PT;
  const float *own = view ? b : a, *oth = view ? a : b;
  const int i_lane = I0 + wi * 32 + r;
  float m = -INFINITY, sum = 0.f;
  const int tiles = (n + PT - 1) / PT;
  for (int J = 0; J < tiles; ++J) {
    const int J0 = J * PT;
#pragma unroll
    for (int w = 0; w < 2; ++w) {  // the own view, then the other one
      const float16_t gt = gram_tile<VEC>(w ? oth : own, own, n, d, J0, I0, s);  // [j][i]
      float z[16], tm = -INFINITY;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int j = J0 + wj * 32 + gram_row(v, g);
        z[v] = (j < n && (w == 1 || j != i_lane)) ? gt[v] * inv_t : -INFINITY;
        tm = fmaxf(tm, z[v]);
      }
      if (tm > -INFINITY) {
        const float m2 = fmaxf(m, tm);
        float acc = sum * expf(m - m2);  // (m = -inf: 0)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc += expf(z[v] - m2);  // (a masked entry: e^-inf = 0)
        sum = acc;
        m = m2;
      }
    }
  }
  // the two lane groups of a row (g = 0 first), then the two waves (half 0 first)
  const float mo = __shfl_xor(m, 32, 64), so = __shfl_xor(sum, 32, 64);
  const float m0 = g ? mo : m, s0 = g ? so : sum, m1 = g ? m : mo, s1 = g ? sum : so;
  const float mw = fmaxf(m0, m1);
  const float sw = mw == -INFINITY ? 0.f : grace_part(m0, s0, mw) + grace_part(m1, s1, mw);
  if (wj == 1 && g == 0) {
    s_m[wi * 32 + r] = mw;
    s_s[wi * 32 + r] = sw;
  }
  __syncthreads();
  if (wj == 0 && g == 0 && i_lane < n) {
    const float m_hi = s_m[wi * 32 + r], M = fmaxf(mw, m_hi);  // (finite: every row meets its cross-view diagonal)
    const float S = grace_part(mw, sw, M) + grace_part(m_hi, s_s[wi * 32 + r], M);
    L[(int64_t)view * n + i_lane] = (float)((double)M + log((double)S));
  }
}

// *loss = (1 / n) sum_i ((L1_i + L2_i) / 2 - dg_i) in a fixed order (one workgroup, fp64); NaN for n == 0, the mean of nothing
__global__ __launch_bounds__(1024) void grace_fold_kernel(const float* __restrict__ L, const float* __restrict__ dg, int n,
                                                          float* __restrict__ loss) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) acc += 0.5 * ((double)L[i] + (double)L[n + i]) - (double)dg[i];
  const double t = gigl_block1024_sum_f64(acc);
  // (n == 1: the one row is its own only term, L = dg in exact arithmetic)
  if (threadIdx.x == 0) *loss = n == 1 ? 0.f : (float)(t / (double)n);
}

// ---- backward -----------------------------------------------------------------------------------------------------------
constexpr gram2_sched GRACE_SCHED = {{2, 0, 1, 1, 0, 0}, {0, 2, 1, 0, 1, 0}, {0, 0, 0, 0, 0, 0}};  // smallest terms first

// ga[view][i][c] (contiguous [2][n][d]) for view blockIdx.z, row tile blockIdx.x, columns [128 blockIdx.y, +128); coef = 1 / (2 n T)
// (two waves per SIMD: the registers allow two workgroups per CU; left to itself the compiler spends them on one)
template <bool VEC>
__global__ __launch_bounds__(256, 2) void grace_backward_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                             const float* __restrict__ L, int n, int d, float inv_t, float coef,
                                                             const float* __restrict__ gout, float* __restrict__ ga) {
  __shared__ __attribute__((aligned(16))) short s[6][PPLANE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, g = lane >> 5;
  const int wj = wv >> 1, wi = wv & 1;
  const int view = blockIdx.z, I0 = blockIdx.x * PT, c0 = blockIdx.y * GCH;
  const float *own = view ? b : a, *oth = view ? a : b;
  const float *L_own = L + (int64_t)view * n, *L_oth = L + (int64_t)(1 - view) * n;
  const int i_lane = I0 + wi * 32 + r;
  const float Li = i_lane < n ? L_own[i_lane] : 0.f;
  float16_t acc2[GCH / 32][1];
#pragma unroll
  for (int q = 0; q < GCH / 32; ++q)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc2[q][0][v] = 0.f;
  const int tiles = (n + PT - 1) / PT;
  for (int J = 0; J < tiles; ++J) {
    const int J0 = J * PT;
#pragma unroll
    for (int w = 0; w < 2; ++w) {  // the own view, then the other one
      const float* x = w ? oth : own;
      const float* Lj = w ? L_oth : L_own;
      const float16_t gt = gram_tile<VEC>(x, own, n, d, J0, I0, s);  // [j][i]
      // the weights where they lie, split into the second product's A fragments: k = 16 s2 + 8 g + t <-> register 8 s2 + t
      bf16x8_t fa[2][3];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float wt[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int v = 8 * s2 + u;
          const int j = J0 + wj * 32 + gram_row(v, g);
          wt[u] = 0.f;
          if (j < n && i_lane < n && (w == 1 || j != i_lane)) {
            const float z = gt[v] * inv_t;
            wt[u] = expf(z - Li) + expf(z - Lj[j]);
          }
        }
        split8(wt, fa[s2][0], fa[s2][1], fa[s2][2]);
      }
      gram2_tile<GCH, 1, GRACE_SCHED>(fa, x, n, d, J0, c0, s, acc2,
                                      [](float v, uint32_t& b1, uint32_t& b2, uint32_t& b3) { split3(v, b1, b2, b3); });
    }
  }
  // epilogue: the two halves of j meet, 32 columns at a time (half 0 + half 1), then ga = k (acc - 2 other_i)
  float* strip = reinterpret_cast<float*>(&s[0][0]) + wi * 1024;  // [32 rows][32 columns] per i block
  const float k = (gout ? *gout : 1.f) * coef;
  float* out = ga + (int64_t)view * n * d;
  gram2_meet<GCH, 1>(acc2, strip, I0 + wi * 32, c0, n, d, [&](int i, int c, const float (&lo)[1], const float (&hi)[1]) {
    out[(int64_t)i * d + c] = k * ((lo[0] + hi[0]) - 2.f * oth[(int64_t)i * d + c]);
  });
}

// one wave per (row, view): the gradient of the normalisation; h_v's gradient to rows ld floats apart
__global__ __launch_bounds__(256) void grace_norm_backward_kernel(const float* __restrict__ ga, const float* __restrict__ a,
                                                                  const float* __restrict__ b, const float* __restrict__ nrm,
                                                                  int n, int d, float* __restrict__ dh1, int64_t ld1,
                                                                  float* __restrict__ dh2, int64_t ld2) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), view = blockIdx.y;
  if (i >= n) return;
  const float* gr = ga + ((int64_t)view * n + i) * d;
  const float* ar = (view ? b : a) + (int64_t)i * d;
  float* dst = view ? dh2 + (int64_t)i * ld2 : dh1 + (int64_t)i * ld1;
  const float nv = nrm[(int64_t)view * n + i];
  if (nv > GEPS) {
    float dot = 0.f;
    for (int c = lane; c < d; c += 64) dot += gr[c] * ar[c];
    for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off, 64);
    const float inv = 1.f / nv;
    for (int c = lane; c < d; c += 64) dst[c] = (gr[c] - dot * ar[c]) * inv;
  } else {
    for (int c = lane; c < d; c += 64) dst[c] = gr[c] / GEPS;
  }
}

int32_t grace_check(gigl_ctx* ctx, int32_t n, int32_t d, float temperature) {
  GIGL_REQUIRE(ctx, d >= 1 && d <= GMAXD, "the GRACE kernels serve 1 <= d <= %d (d=%d)", GMAXD, d);
  GIGL_REQUIRE(ctx, n >= 0 && n <= GRACE_MAX_N, "n=%d outside [0, %d]", n, GRACE_MAX_N);
  GIGL_REQUIRE(ctx, temperature > 0.f, "temperature=%g is not positive", (double)temperature);
  return GIGL_OK;
}

}  // namespace

extern "C" {

int32_t gigl_grace_loss(gigl_ctx* ctx, const float* h1, int64_t ld1, const float* h2, int64_t ld2, int32_t n, int32_t d,
                        float temperature, float* a_out, float* b_out, float* norm_out, float* dg_out, float* lse_out,
                        float* loss_out) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const int32_t rc0 = grace_check(ctx, n, d, temperature);
  if (rc0 != GIGL_OK) return rc0;
  GIGL_REQUIRE(ctx, loss_out && (n == 0 || (h1 && h2 && a_out && b_out && norm_out && dg_out && lse_out && ld1 >= d && ld2 >= d)),
               "null argument or a row stride < d");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const float inv_t = 1.f / temperature;
  if (n > 0) {
    const unsigned tiles = (unsigned)((n + PT - 1) / PT);
    hipLaunchKernelGGL(grace_prep_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, h1, ld1, h2, ld2, n, d, inv_t, a_out, b_out,
                       norm_out, dg_out);
    dispatch_bool(d % 4 == 0 && gigl_aligned16(a_out) && gigl_aligned16(b_out), [&](auto vec) {
      hipLaunchKernelGGL(grace_lse_kernel<decltype(vec)::value>, dim3(tiles, 2), dim3(256), 0, st, (const float*)a_out,
                         (const float*)b_out, n, d, inv_t, lse_out);
    });
  }
  hipLaunchKernelGGL(grace_fold_kernel, dim3(1), dim3(1024), 0, st, (const float*)lse_out, (const float*)dg_out, n, loss_out);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_grace_loss_backward(gigl_ctx* ctx, const float* a, const float* b, const float* norm, const float* lse, int32_t n,
                                 int32_t d, float temperature, const float* gout_dev, float* dh1, int64_t ld1, float* dh2,
                                 int64_t ld2) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const int32_t rc0 = grace_check(ctx, n, d, temperature);
  if (rc0 != GIGL_OK) return rc0;
  GIGL_REQUIRE(ctx, n == 0 || (dh1 && dh2 && ld1 >= d && ld2 >= d && (n < 2 || (a && b && norm && lse))),
               "null argument or a row stride < d");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (n == 0) return GIGL_OK;
  if (n < 2) {  // the one row is its own only term: the loss is 0 whatever the row
    gigl_zero_rows(st, dh1, ld1, n, d);
    gigl_zero_rows(st, dh2, ld2, n, d);
  } else {
    const int64_t ga_bytes = gigl_align_up(2 * (int64_t)n * d * 4, 256);
    const int32_t rc = gigl_arena_reset(ctx, ga_bytes + 1024);
    if (rc != GIGL_OK) return rc;
    float* ga = (float*)gigl_arena_alloc(ctx, ga_bytes + 256);
    GIGL_REQUIRE(ctx, ga, "scratch arena exhausted");
    const float inv_t = 1.f / temperature;
    const float coef = (float)(1.0 / (2.0 * (double)n * (double)temperature));
    const dim3 grid((unsigned)((n + PT - 1) / PT), (unsigned)((d + GCH - 1) / GCH), 2);
    dispatch_bool(d % 4 == 0 && gigl_aligned16(a) && gigl_aligned16(b), [&](auto vec) {
      hipLaunchKernelGGL(grace_backward_kernel<decltype(vec)::value>, grid, dim3(256), 0, st, a, b, lse, n, d, inv_t, coef, gout_dev,
                         ga);
    });
    hipLaunchKernelGGL(grace_norm_backward_kernel, dim3((unsigned)((n + 3) / 4), 2), dim3(256), 0, st, (const float*)ga, a, b, norm, n, d,
                       dh1, ld1, dh2, ld2);
  }
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

}  // extern "C"
