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
//             products (own view, other view) per J.  The structure is pair_backward_kernel's (pairwise.hip): the first
//             product transposed, so that the weights lie in the second product's A-operand layout and never pass through
//             LDS; the other operand staged transposed ([column][32 j]) under pair_kperm.  Both operands are split with the
//             plain split3 (a row's weights sum to about 2: nothing here cancels as DirectAU's r_i x_i does); the two halves
//             of j meet in the epilogue through LDS, in a fixed order.
//   norm bwd  one wave per row: gh_i = (ga_i - <ga_i, a_i> a_i) / |h_i|, or ga_i / 1e-8 where |h_i| <= 1e-8 (autograd
//             through the reference's torch.max(norm, eps)).
#include "common.h"
#include "gram_tile.h"

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
        const int j = J0 + wj * 32 + 8 * (v >> 2) + 4 * g + (v & 3);
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
  __shared__ double s_w[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double acc = 0.0;
  for (int i = tid; i < n; i += 1024) acc += 0.5 * ((double)L[i] + (double)L[n + i]) - (double)dg[i];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) s_w[w] = acc;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t += s_w[k];
    // (n == 1: the one row is its own only term, L = dg in exact arithmetic)
    *loss = n == 1 ? 0.f : (float)(t / (double)n);
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------
// eight floats -> the three bf16 planes of a fragment
__device__ __forceinline__ void grace_split8(const float (&x)[8], bf16x8_t& f1, bf16x8_t& f2, bf16x8_t& f3) {
  uint32_t b1[8], b2[8], b3[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) split3(x[u], b1[u], b2[u], b3[u]);
  f1 = __builtin_bit_cast(bf16x8_t, make_uint4((b1[0] >> 16) | b1[1], (b1[2] >> 16) | b1[3], (b1[4] >> 16) | b1[5], (b1[6] >> 16) | b1[7]));
  f2 = __builtin_bit_cast(bf16x8_t, make_uint4((b2[0] >> 16) | b2[1], (b2[2] >> 16) | b2[3], (b2[4] >> 16) | b2[5], (b2[6] >> 16) | b2[7]));
  f3 = __builtin_bit_cast(bf16x8_t, make_uint4((b3[0] >> 16) | b3[1], (b3[2] >> 16) | b3[3], (b3[4] >> 16) | b3[5], (b3[6] >> 16) | b3[7]));
}

// ga[view][i][c] (contiguous [2][n][d]) for view blockIdx.z, row tile blockIdx.x, columns [128 blockIdx.y, +128); coef = 1 / (2 n T)
template <bool VEC>
__global__ __launch_bounds__(256) void grace_backward_kernel(const float* __restrict__ a, const float* __restrict__ b,
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
  float16_t acc2[GCH / 32];
#pragma unroll
  for (int q = 0; q < GCH / 32; ++q)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc2[q][v] = 0.f;
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
          const int j = J0 + wj * 32 + 8 * (v >> 2) + 4 * g + (v & 3);
          wt[u] = 0.f;
          if (j < n && i_lane < n && (w == 1 || j != i_lane)) {
            const float z = gt[v] * inv_t;
            wt[u] = expf(z - Li) + expf(z - Lj[j]);
          }
        }
        grace_split8(wt, fa[s2][0], fa[s2][1], fa[s2][2]);
      }
      // acc2[i][c] += W[i][j] X[j][c], 64 columns at a time: planes p + 3 h hold half h of j as [column][32 kpos]
#pragma unroll
      for (int sub = 0; sub < GCH / 64; ++sub) {
        const int cs = c0 + 64 * sub;
        if (cs < d) {  // (the whole workgroup)
          __syncthreads();  // the fragments of the Gram tile / of the previous 64 columns have been read
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
            bf16x8_t f1, f2, f3;
            grace_split8(xv, f1, f2, f3);
            const int o = split_lds_off(lane, kb);
            *reinterpret_cast<bf16x8_t*>(&s[3 * h + 0][o]) = f1;
            *reinterpret_cast<bf16x8_t*>(&s[3 * h + 1][o]) = f2;
            *reinterpret_cast<bf16x8_t*>(&s[3 * h + 2][o]) = f3;
          }
          __syncthreads();
          constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};  // smallest terms first
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
                acc2[2 * sub + cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s2][PA[u]], fb[cb][PB[u]], acc2[2 * sub + cb], 0, 0, 0);
          }
        }
      }
    }
  }
  // epilogue: the two halves of j meet, 32 columns at a time (half 0 + half 1), then ga = k (acc - 2 other_i)
  float* strip = reinterpret_cast<float*>(&s[0][0]) + wi * 1024;  // [32 rows][32 columns] per i block
  const float k = (gout ? *gout : 1.f) * coef;
  float* out = ga + (int64_t)view * n * d;
#pragma unroll
  for (int q = 0; q < GCH / 32; ++q) {
    if (c0 + 32 * q < d) {  // (the whole workgroup)
      __syncthreads();
      if (wj == 1) {
#pragma unroll
        for (int v = 0; v < 16; ++v) strip[(8 * (v >> 2) + 4 * g + (v & 3)) * 32 + r] = acc2[q][v];
      }
      __syncthreads();
      if (wj == 0) {
        const int c = c0 + 32 * q + r;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int il = 8 * (v >> 2) + 4 * g + (v & 3), i = I0 + wi * 32 + il;
          if (i < n && c < d)
            out[(int64_t)i * d + c] = k * ((acc2[q][v] + strip[il * 32 + r]) - 2.f * oth[(int64_t)i * d + c]);
        }
      }
    }
  }
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

__global__ __launch_bounds__(256) void grace_zero_rows_kernel(float* __restrict__ dx, int64_t ld, int n, int d) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (int64_t)n * d) dx[(i / d) * ld + i % d] = 0.f;
}

int32_t grace_check(gigl_ctx* ctx, int32_t n, int32_t d, float temperature) {
  GIGL_REQUIRE(ctx, d >= 1 && d <= GMAXD, "the GRACE kernels serve 1 <= d <= %d (d=%d)", GMAXD, d);
  GIGL_REQUIRE(ctx, n >= 0 && n <= GRACE_MAX_N, "n=%d outside [0, %d]", n, GRACE_MAX_N);
  GIGL_REQUIRE(ctx, temperature > 0.f, "temperature=%g is not positive", (double)temperature);
  return GIGL_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

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
    if (d % 4 == 0 && aligned16(a_out) && aligned16(b_out))
      hipLaunchKernelGGL(grace_lse_kernel<true>, dim3(tiles, 2), dim3(256), 0, st, (const float*)a_out, (const float*)b_out, n, d, inv_t, lse_out);
    else
      hipLaunchKernelGGL(grace_lse_kernel<false>, dim3(tiles, 2), dim3(256), 0, st, (const float*)a_out, (const float*)b_out, n, d, inv_t, lse_out);
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
    hipLaunchKernelGGL(grace_zero_rows_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, dh1, ld1, n, d);
    hipLaunchKernelGGL(grace_zero_rows_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, dh2, ld2, n, d);
  } else {
    const int64_t ga_bytes = gigl_align_up(2 * (int64_t)n * d * 4, 256);
    const int32_t rc = gigl_arena_reset(ctx, ga_bytes + 1024);
    if (rc != GIGL_OK) return rc;
    float* ga = (float*)gigl_arena_alloc(ctx, ga_bytes + 256);
    GIGL_REQUIRE(ctx, ga, "scratch arena exhausted");
    const float inv_t = 1.f / temperature;
    const float coef = (float)(1.0 / (2.0 * (double)n * (double)temperature));
    const dim3 grid((unsigned)((n + PT - 1) / PT), (unsigned)((d + GCH - 1) / GCH), 2);
    if (d % 4 == 0 && aligned16(a) && aligned16(b))
      hipLaunchKernelGGL(grace_backward_kernel<true>, grid, dim3(256), 0, st, a, b, lse, n, d, inv_t, coef, gout_dev, ga);
    else
      hipLaunchKernelGGL(grace_backward_kernel<false>, grid, dim3(256), 0, st, a, b, lse, n, d, inv_t, coef, gout_dev, ga);
    hipLaunchKernelGGL(grace_norm_backward_kernel, dim3((unsigned)((n + 3) / 4), 2), dim3(256), 0, st, (const float*)ga, a, b, norm, n, d,
                       dh1, ld1, dh2, ld2);
  }
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

}  // extern "C"
