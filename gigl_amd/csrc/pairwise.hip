// pairwise.hip — the DirectAU losses over embedding rows (python/gigl/src/common/models/layers/loss.py:591-626): the pairwise
// uniformity loss and its gradient as two Gram-shaped MFMA kernels that write nothing of size n x n, and the alignment loss.
//
// Uniformity.  X fp32 [n][d], t the temperature:
//     w_ij = exp(-t max(0, |x_i - x_j|^2)),  S = sum_{i<j} w_ij,  U = log(2 S / (n (n - 1)))
//     dU/dx_i = (-2 t / S) (r_i x_i - sum_{j != i} w_ij x_j),  r_i = sum_{j != i} w_ij
// The reference is pdist -> pow -> mul -> exp -> mean -> log: n (n - 1) / 2 distances in HBM, forward and again in backward.
//   prep      Xc = X - column mean (distances are translation invariant; two launches, fixed order), sq_i = |xc_i|^2.  The
//             centring keeps sq_i + sq_j - 2 g_ij and r_i x_i - sum w x_j free of cancellation when the rows have collapsed
//             towards one point; sum_i dU/dxc_i = 0, so the gradient with respect to Xc IS the gradient with respect to X.
//   forward   one workgroup per pair of 64-row tiles I <= J.  gram_tile (gram_tile.h): the two panels pass through LDS in K chunks
//             of 32, split on the way in into three bf16 planes (split_planes.h: x = b1 + b2 + b3 exactly), six
//             v_mfma_f32_32x32x16_bf16 per 16 k carry the product at fp32 accuracy; four waves as 2 x 2, a 32 x 32 block of G
//             each, two accumulators so that dependent MFMAs alternate.  Epilogue in registers: w masked to i < j < n, lane ->
//             wave -> workgroup sum, one double per tile pair; pair_fold_kernel adds the partials in a fixed order in fp64.
//   backward  one workgroup per row tile I and 128-column chunk of d, sweeping EVERY column tile J (no atomics: a row's sums
//             have one owner and one order).  The weights of a tile are computed from its TRANSPOSED Gram tile, where they
//             lie, and multiplied into Xc_J by gram_tile.h's second product (which explains the layout): acc[i][c] += W[i][j]
//             Xc[j][c] without W leaving the registers.  Per 32 columns an exact accumulator for the one large term and one
//             for the rest (fixed-point planes, see pair_fix3), 8 accumulators of 32 x 32 for 128 columns; the two halves
//             of j meet in the epilogue through LDS, in a fixed order, with the plane sums of w that rebuild r_i x_i.
//
// Alignment.  mean_i |u_i - p_i|^alpha: one wave per row, a fixed-order fold; backward alpha |.|^(alpha - 2) (u - p) / n,
// zero where u_i == p_i (torch's subgradient of norm).
#include "common.h"
#include "dispatch.h"
#include "gram_tile.h"
#include "wave_reduce.h"

#include <cmath>
#include <cstdint>

namespace {

constexpr int PCH = 128;          // columns of d per backward workgroup (two accumulators per 32: 256 spills)
constexpr int PMAXD = 512;

// ---- prep -------------------------------------------------------------------------------------------------------------
// part[chunk][c] = sum of column c over rows [256 chunk, +256): lane = column, the four waves take rows 4 apart and meet in
// a fixed order
__global__ __launch_bounds__(256) void pair_colsum_kernel(const float* __restrict__ x, int64_t ld, int n, int d,
                                                          float* __restrict__ part) {
  __shared__ float s_p[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane, r0 = blockIdx.y * 256;
  float acc = 0.f;
  if (c < d)
    for (int r = r0 + wv; r < min(n, r0 + 256); r += 4) acc += x[(int64_t)r * ld + c];
  s_p[wv][lane] = acc;
  __syncthreads();
  if (wv == 0 && c < d) part[(int64_t)blockIdx.y * d + c] = (s_p[0][lane] + s_p[1][lane]) + (s_p[2][lane] + s_p[3][lane]);
}

// xc = x - mean, sq = |xc|^2 for 64 rows per workgroup (a wave takes 16 of them); the mean is folded from the chunk sums in
// chunk order by every workgroup.  V4: d, ld multiples of 4 and 16-byte aligned bases -> 16-byte loads and stores
template <bool V4>
__global__ __launch_bounds__(256) void pair_centre_kernel(const float* __restrict__ x, int64_t ld, int n, int d,
                                                          const float* __restrict__ part, int chunks,
                                                          float* __restrict__ xc, float* __restrict__ sq) {
  __shared__ __attribute__((aligned(16))) float s_mean[PMAXD];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float inv_n = 1.f / (float)n;
  for (int c = tid; c < d; c += 256) {
    float s = 0.f;
    for (int k = 0; k < chunks; ++k) s += part[(int64_t)k * d + c];
    s_mean[c] = s * inv_n;
  }
  __syncthreads();
  for (int q = 0; q < 16; ++q) {
    const int row = blockIdx.x * 64 + wv * 16 + q;
    if (row >= n) break;  // (the whole wave)
    const float* src = x + (int64_t)row * ld;
    float* dst = xc + (int64_t)row * d;
    float acc = 0.f;
    if constexpr (V4) {
      for (int c = lane * 4; c < d; c += 256) {
        float4 v = *reinterpret_cast<const float4*>(src + c);
        const float4 m = *reinterpret_cast<const float4*>(&s_mean[c]);
        v.x -= m.x;
        v.y -= m.y;
        v.z -= m.z;
        v.w -= m.w;
        *reinterpret_cast<float4*>(dst + c) = v;
        acc += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
      }
    } else {
      for (int c = lane; c < d; c += 64) {
        const float v = src[c] - s_mean[c];
        dst[c] = v;
        acc += v * v;
      }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) sq[row] = acc;
  }
}

// ---- forward ------------------------------------------------------------------------------------------------------------
// part[p] = sum of w_ij over the entries i < j < n of tile pair p = J (J + 1) / 2 + I, I <= J
template <bool VEC>
__global__ __launch_bounds__(256) void pair_sum_kernel(const float* __restrict__ xc, const float* __restrict__ sq, int n,
                                                       int d, float t, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) short s[6][PPLANE];
  __shared__ double s_w[4];
  const int64_t p = blockIdx.x;
  int64_t J = (int64_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
  while (J * (J + 1) / 2 > p) --J;
  while ((J + 1) * (J + 2) / 2 <= p) ++J;
  const int I = (int)(p - J * (J + 1) / 2);
  const float16_t acc = gram_tile<VEC>(xc, xc, n, d, I * PT, (int)J * PT, s);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, g = lane >> 5;
  const int j = (int)J * PT + (wv & 1) * 32 + r;
  const float sqj = j < n ? sq[j] : 0.f;
  float sum = 0.f;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int i = I * PT + (wv >> 1) * 32 + gram_row(v, g);
    if (i < j && j < n) sum += expf(-t * fmaxf(0.f, (sq[i] + sqj) - 2.f * acc[v]));
  }
  double ds = (double)sum;
  for (int off = 32; off > 0; off >>= 1) ds += __shfl_xor(ds, off, 64);
  if (lane == 0) s_w[wv] = ds;
  __syncthreads();
  if (threadIdx.x == 0) part[p] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// S = the partials added in a fixed order (one workgroup, fp64), U = log(2 S / (n (n - 1))): NaN for n < 2 (0 / 0), as the
// reference's mean over an empty pdist
__global__ __launch_bounds__(1024) void pair_fold_kernel(const double* __restrict__ part, int64_t np, int n,
                                                         double* __restrict__ pair_sum, float* __restrict__ loss) {
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < np; i += 1024) acc += part[i];
  const double S = gigl_block1024_sum_f64(acc);
  if (threadIdx.x == 0) {
    *pair_sum = S;
    *loss = (float)log(2.0 * S / ((double)n * (double)(n - 1)));
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------
// The second product's operands are split in FIXED point, not by split3.  r_i x_i - sum_j w_ij x_j cancels: among (near)
// duplicates w ~ 1 and both terms are ~ their count, while the gradient may be the far rows' e^-8 of that — fp32 accumulators
// that mix the two round the answer away.  So x / q = t1 + t2 / 2^8 + t3 / 2^16 (+ a remainder < 2^-16) with INTEGERS t1 in
// [-128, 128], t2, t3 in [0, 255] and q = scale / 128 (scale: a power of two >= every |xc|), and w = u1 + rem with u1 = floor(256
// w) / 256.  Every plane is exact in bf16.  The products u1 t1 are integers / 256 below 2^15: their sum — the one LARGE term —
// has its own accumulator and is EXACT (up to 2^24 / 2^15 / ... = 256 rows of weight 1 per wave and half; beyond, fp32
// rounding of that term alone), the same integers cancel exactly against R1 t1_i, R1 = sum_j u1_ij.  Everything else (u1 t2, u1
// t3, and rem — as its two leading bf16 planes f2, f3 — against t1, t2) is 2^-8 of that size or carries the small weights, and
// shares a second accumulator.  Dropped: products below 2^-16 of a term — and the epilogue rebuilds r_i x_i from the SAME
// products (the plane sums of w times the planes of x_i), so what is dropped is dropped from the difference x_i - x_j, never
// from one side of it (a weight 1 - 2^-22 between duplicates puts 1 / 256 of the large term into rem: measured, that alone
// was 1.8e-4 of the gradient when r_i x_i kept all of rem).  Rows far below the scale lose RELATIVE precision
// (the planes are absolute): the error is 2^-23 scale per unit of weight, the gradient's own size for rows of comparable norm.
__device__ __forceinline__ void pair_fix3(float x, float inv_q, float& t1, float& t2, float& t3) {
  const float y = x * inv_q;  // (a power of two: exact)
  t1 = floorf(y);
  const float r1 = (y - t1) * 256.f;  // in [0, 256), exact
  t2 = floorf(r1);
  t3 = floorf((r1 - t2) * 256.f);
}
// the planes as the MFMA reads them, in units of q: t1, t2 / 2^8, t3 / 2^16 (bf16 = the float's upper half: <= 9 bits each)
__device__ __forceinline__ void pair_fix3_bits(float x, float inv_q, uint32_t& b1, uint32_t& b2, uint32_t& b3) {
  float t1, t2, t3;
  pair_fix3(x, inv_q, t1, t2, t3);
  b1 = __float_as_uint(t1) & 0xFFFF0000u;
  b2 = __float_as_uint(t2 * (1.f / 256.f)) & 0xFFFF0000u;
  b3 = __float_as_uint(t3 * (1.f / 65536.f)) & 0xFFFF0000u;
}
// (w plane, x plane): u1 t1 alone into [0]; rem's planes against t1, t2 and u1 against t2, t3 into [1], smallest first
constexpr gram2_sched PAIR_SCHED = {{2, 1, 0, 1, 0, 0}, {0, 1, 2, 0, 1, 0}, {1, 1, 1, 1, 1, 0}};

template <bool VEC>
__global__ __launch_bounds__(256) void pair_backward_kernel(const float* __restrict__ xc, const float* __restrict__ sq, int n,
                                                            int d, float t, const double* __restrict__ pair_sum,
                                                            const float* __restrict__ gout, float* __restrict__ dx,
                                                            int64_t ld_dx) {
  __shared__ __attribute__((aligned(16))) short s[6][PPLANE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, g = lane >> 5;
  const int wj = wv >> 1, wi = wv & 1;  // this wave: rows j of half wj (the first product's rows), i block wi (its columns)
  const int I0 = blockIdx.x * PT, c0 = blockIdx.y * PCH;
  const int i_lane = I0 + wi * 32 + r;
  const float sqi = i_lane < n ? sq[i_lane] : 0.f;
  // scale = the power of two above the largest row norm (every workgroup folds the n norms: a few KB from L2)
  __shared__ float s_mx[4];
  {
    float mx = 0.f;
    for (int k = tid; k < n; k += 256) mx = fmaxf(mx, sq[k]);
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) s_mx[wv] = mx;
    __syncthreads();
  }
  int sc_e = 0;
  frexpf(sqrtf(fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]))) * 1.0001f, &sc_e);  // norm < 2^sc_e
  const float inv_q = ldexpf(128.f, -sc_e);  // (all rows zero: sc_e = 0)
  float16_t acc2[PCH / 32][2];  // [.][0]: sum u1 t1, exact; [.][1]: the rest
#pragma unroll
  for (int b = 0; b < PCH / 32; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc2[b][0][v] = acc2[b][1][v] = 0.f;
  double r_u1 = 0.0, r_f2 = 0.0, r_f3 = 0.0;  // sum_j of each plane of w_ij AS THE PRODUCT TAKES IT: r_i x_i is rebuilt from them
  const int tiles = (n + PT - 1) / PT;
  for (int J = 0; J < tiles; ++J) {
    const int J0 = J * PT;
    const float16_t gt = gram_tile<VEC>(xc, xc, n, d, J0, I0, s);  // [j][i]
    // W where it lies, split into the second product's A fragments: fa[s2][plane], k = 16 s2 + 8 g + t <-> register 8 s2 + t
    bf16x8_t fa[2][3];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      uint32_t b1[8], b2[8], b3[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int v = 8 * s2 + u;
        const int j = J0 + wj * 32 + gram_row(v, g);
        float w = 0.f;
        if (j < n && i_lane < n && j != i_lane) w = expf(-t * fmaxf(0.f, (sqi + sq[j]) - 2.f * gt[v]));
        const float u1 = floorf(w * 256.f) * (1.f / 256.f), rem = w - u1;  // (both exact)
        r_u1 += (double)u1;
        uint32_t unused;
        b1[u] = __float_as_uint(u1) & 0xFFFF0000u;  // (<= 9 significant bits: nothing is cut)
        split3(rem, b2[u], b3[u], unused);
        r_f2 += (double)__uint_as_float(b2[u]);
        r_f3 += (double)__uint_as_float(b3[u]);
      }
      fa[s2][0] = __builtin_bit_cast(bf16x8_t, pack8(b1));
      fa[s2][1] = __builtin_bit_cast(bf16x8_t, pack8(b2));
      fa[s2][2] = __builtin_bit_cast(bf16x8_t, pack8(b3));
    }
    gram2_tile<PCH, 2, PAIR_SCHED>(fa, xc, n, d, J0, c0, s, acc2, [inv_q](float x, uint32_t& b1, uint32_t& b2, uint32_t& b3) {
      pair_fix3_bits(x, inv_q, b1, b2, b3);
    });
  }
  // epilogue: the two halves of j meet — r_i and, 32 columns at a time, the accumulators — then dx = coef (r_i xc_i - acc_i)
  r_u1 += __shfl_xor(r_u1, 32, 64);
  r_f2 += __shfl_xor(r_f2, 32, 64);
  r_f3 += __shfl_xor(r_f3, 32, 64);
  __syncthreads();
  double* s_r = reinterpret_cast<double*>(&s[0][0]);               // [2 halves][u1 | f2 | f3][64 rows]
  float* strip = reinterpret_cast<float*>(s_r + 384) + wi * 2048;  // [2 accumulators][32 rows][32 columns] per i block
  if (g == 0) {  // (published by gram2_meet's first barrier)
    s_r[wj * 192 + wi * 32 + r] = r_u1;
    s_r[wj * 192 + 64 + wi * 32 + r] = r_f2;
    s_r[wj * 192 + 128 + wi * 32 + r] = r_f3;
  }
  // (in units of q = 1 / inv_q, put back with the coefficient)
  const double coef = (double)(gout ? *gout : 1.f) * (-2.0 * (double)t / *pair_sum) / (double)inv_q;
  gram2_meet<PCH, 2>(acc2, strip, I0 + wi * 32, c0, n, d, [&](int i, int c, const float (&own)[2], const float (&other)[2]) {
    // r_i x_i rebuilt from the SAME plane products the accumulators hold (so that equal rows cancel exactly and what the
    // products drop is dropped from a difference): the large term R1 t1 against its exact accumulator, the rest against the
    // other one; each half of j on its own, in fp64, before the halves are added
    float t1, t2, t3;
    pair_fix3(xc[(int64_t)i * d + c], inv_q, t1, t2, t3);
    const double x1 = (double)t1, x2 = (double)t2 * (1.0 / 256.0), x3 = (double)t3 * (1.0 / 65536.0);
    const double* rr = s_r + (i - I0);
    const double h0 = (rr[0] * x1 - (double)own[0]) + ((rr[0] * (x2 + x3) + rr[64] * (x1 + x2) + rr[128] * x1) - (double)own[1]);
    const double h1 =
        (rr[192] * x1 - (double)other[0]) + ((rr[192] * (x2 + x3) + rr[256] * (x1 + x2) + rr[320] * x1) - (double)other[1]);
    dx[(int64_t)i * ld_dx + c] = (float)(coef * (h0 + h1));
  });
}

// ---- alignment ----------------------------------------------------------------------------------------------------------
// norm[i] = |u_i - p_i|, one wave per row
__global__ __launch_bounds__(256) void align_rows_kernel(const float* __restrict__ u, int64_t ld_u, const float* __restrict__ p,
                                                         int64_t ld_p, int n, int d, float* __restrict__ norm) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float *ur = u + (int64_t)i * ld_u, *pr = p + (int64_t)i * ld_p;
  float acc = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float v = ur[c] - pr[c];
    acc += v * v;
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) norm[i] = sqrtf(acc);
}

// *loss = mean_i norm[i]^alpha in a fixed order (one workgroup, fp64); NaN for n == 0
__global__ __launch_bounds__(1024) void align_fold_kernel(const float* __restrict__ norm, int n, float alpha,
                                                          float* __restrict__ loss) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const double v = (double)norm[i];
    acc += alpha == 2.f ? v * v : pow(v, (double)alpha);
  }
  const double t = gigl_block1024_sum_f64(acc);
  if (threadIdx.x == 0) *loss = (float)(t / (double)n);
}

// du_i = gout alpha norm_i^(alpha - 2) (u_i - p_i) / n, dp_i = -du_i ([n][d] contiguous); zero rows where norm_i == 0
__global__ __launch_bounds__(256) void align_backward_kernel(const float* __restrict__ u, int64_t ld_u,
                                                             const float* __restrict__ p, int64_t ld_p, int n, int d,
                                                             float alpha, const float* __restrict__ norm,
                                                             const float* __restrict__ gout, float* __restrict__ du,
                                                             float* __restrict__ dp) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float nv = norm[i];
  float k = 0.f;
  if (nv > 0.f) k = (gout ? *gout : 1.f) * alpha * (alpha == 2.f ? 1.f : powf(nv, alpha - 2.f)) / (float)n;
  const float *ur = u + (int64_t)i * ld_u, *pr = p + (int64_t)i * ld_p;
  for (int c = lane; c < d; c += 64) {
    const float v = k * (ur[c] - pr[c]);
    du[(int64_t)i * d + c] = v;
    dp[(int64_t)i * d + c] = -v;
  }
}

constexpr int32_t PAIR_MAX_N = 1 << 18;  // 4096 row tiles: 8.4 M tile pairs, 67 MB of partials

int32_t pair_check(gigl_ctx* ctx, int32_t n, int32_t d) {
  GIGL_REQUIRE(ctx, d >= 1 && d <= PMAXD, "the pairwise kernels serve 1 <= d <= %d (d=%d)", PMAXD, d);
  GIGL_REQUIRE(ctx, n >= 0 && n <= PAIR_MAX_N, "n=%d outside [0, %d]", n, PAIR_MAX_N);
  return GIGL_OK;
}

}  // namespace

extern "C" {

int32_t gigl_uniformity_loss(gigl_ctx* ctx, const float* x, int64_t ld, int32_t n, int32_t d, float temperature,
                             float* xc_out, float* sq_out, double* pair_sum_out, float* loss_out) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const int32_t rc0 = pair_check(ctx, n, d);
  if (rc0 != GIGL_OK) return rc0;
  GIGL_REQUIRE(ctx, pair_sum_out && loss_out && (n == 0 || (x && xc_out && sq_out && ld >= d)), "null argument or ld < d");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int64_t tiles = (n + PT - 1) / PT, pairs = n >= 2 ? tiles * (tiles + 1) / 2 : 0;
  const int chunks = (n + 255) / 256;
  const int64_t part_bytes = gigl_align_up(pairs * 8, 256), cs_bytes = gigl_align_up((int64_t)chunks * d * 4, 256);
  const int32_t rc = gigl_arena_reset(ctx, part_bytes + cs_bytes + 1024);
  if (rc != GIGL_OK) return rc;
  double* part = (double*)gigl_arena_alloc(ctx, part_bytes + 256);
  float* colsum = (float*)gigl_arena_alloc(ctx, cs_bytes + 256);
  GIGL_REQUIRE(ctx, part && colsum, "scratch arena exhausted");
  hipStream_t st = ctx->stream;
  if (n >= 2) {
    hipLaunchKernelGGL(pair_colsum_kernel, dim3((unsigned)((d + 63) / 64), (unsigned)chunks), dim3(256), 0, st, x, ld, n, d, colsum);
    dispatch_bool(d % 4 == 0 && ld % 4 == 0 && gigl_aligned16(x) && gigl_aligned16(xc_out), [&](auto v4) {
      hipLaunchKernelGGL(pair_centre_kernel<decltype(v4)::value>, dim3((unsigned)tiles), dim3(256), 0, st, x, ld, n, d,
                         (const float*)colsum, chunks, xc_out, sq_out);
    });
    dispatch_bool(d % 4 == 0 && gigl_aligned16(xc_out), [&](auto vec) {
      hipLaunchKernelGGL(pair_sum_kernel<decltype(vec)::value>, dim3((unsigned)pairs), dim3(256), 0, st, (const float*)xc_out,
                         (const float*)sq_out, n, d, temperature, part);
    });
  }
  hipLaunchKernelGGL(pair_fold_kernel, dim3(1), dim3(1024), 0, st, (const double*)part, pairs, n, pair_sum_out, loss_out);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_uniformity_loss_backward(gigl_ctx* ctx, const float* xc, const float* sq, int32_t n, int32_t d, float temperature,
                                      const double* pair_sum, const float* gout_dev, float* dx, int64_t ld_dx) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const int32_t rc0 = pair_check(ctx, n, d);
  if (rc0 != GIGL_OK) return rc0;
  GIGL_REQUIRE(ctx, n == 0 || (dx && ld_dx >= d && (n < 2 || (xc && sq && pair_sum))), "null argument or ld_dx < d");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (n == 0) return GIGL_OK;
  if (n < 2) {
    gigl_zero_rows(st, dx, ld_dx, n, d);
  } else {
    const dim3 grid((unsigned)((n + PT - 1) / PT), (unsigned)((d + PCH - 1) / PCH));
    dispatch_bool(d % 4 == 0 && gigl_aligned16(xc), [&](auto vec) {
      hipLaunchKernelGGL(pair_backward_kernel<decltype(vec)::value>, grid, dim3(256), 0, st, xc, sq, n, d, temperature, pair_sum,
                         gout_dev, dx, ld_dx);
    });
  }
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_alignment_loss(gigl_ctx* ctx, const float* u, int64_t ld_u, const float* p, int64_t ld_p, int32_t n, int32_t d,
                            float alpha, float* norm_out, float* loss_out) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const int32_t rc0 = pair_check(ctx, n, d);
  if (rc0 != GIGL_OK) return rc0;
  GIGL_REQUIRE(ctx, loss_out && (n == 0 || (u && p && norm_out && ld_u >= d && ld_p >= d)), "null argument or a row stride < d");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (n > 0)
    hipLaunchKernelGGL(align_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, u, ld_u, p, ld_p, n, d, norm_out);
  hipLaunchKernelGGL(align_fold_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const float*)norm_out, n, alpha, loss_out);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_alignment_loss_backward(gigl_ctx* ctx, const float* u, int64_t ld_u, const float* p, int64_t ld_p, int32_t n,
                                     int32_t d, float alpha, const float* norm, const float* gout_dev, float* du, float* dp) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const int32_t rc0 = pair_check(ctx, n, d);
  if (rc0 != GIGL_OK) return rc0;
  GIGL_REQUIRE(ctx, n == 0 || (u && p && norm && du && dp && ld_u >= d && ld_p >= d), "null argument or a row stride < d");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (n > 0)
    hipLaunchKernelGGL(align_backward_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, u, ld_u, p, ld_p, n, d, alpha,
                       norm, gout_dev, du, dp);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

}  // extern "C"
