// correlate.hip — the two losses over the d x d correlation of two column-standardised views: GBTLoss (graph Barlow Twins,
// python/gigl/src/common/models/layers/loss.py:491-534) and WhiteningDecorrelationLoss (CCA-SSG, loss.py:444-488), forward and
// gradient.  h1, h2 fp32 [n][d] (rows `ld` floats apart).  Per view and column: mean mu, unbiased standard deviation s,
// z = (x - mu) rinv with rinv = 1 / (s + 1e-15) (GBT) or 1 / s (WhiteningDecorrelation).
//     GBT   C = z1^T z2 / n,  loss = sum_a (1 - C_aa)^2 + (1 / d) sum_{a != b} C_ab^2
//     WD    c_k = z_k^T z_k / N,  loss = |z1 - z2|_F / N + lambd (|I - c1|_F + |I - c2|_F),  N = n
// The product contracts along the STRIDED axis of the rows (K = n, output d x d, 1 to 64 tiles of 64 x 64): gram_tile
// (gram_tile.h) contracts along the contiguous one and one workgroup per output tile would leave the chip idle, so the work
// is split along K.  Nothing of size n x n exists, nothing uses atomics, every sum has one owner and a fixed order that
// depends on (n, d) only: the same inputs give the same bits.
//   stats     corr_colsum_kernel<0>, <1>: per (view, 64-column block, row chunk) the column sums, then — with the mean folded
//             from those partials — the sums of centred squares, fp64, a lane per column (a row is one coalesced read), the
//             four waves of a workgroup meeting in wave order.  Never E[x^2] - mu^2.
//   rows      corr_rows_kernel: folds the partials in chunk order (mu, s, rinv per column), writes z for both views ([2][npad]
//             [d], npad = n rounded up to 64, the padding rows zero) and, for WD, dz = z1 - z2 taken in fp64 BEFORE rounding
//             (the views may be close: the difference of the rounded z would lose its leading digits), with the per-column
//             partials of sum dz^2, sum z1 dz and -sum z2 dz.  A column with s == 0 gets z = 0 and rinv = 0 in both modes: for
//             GBT that is the reference's forward value (0 / 1e-15); its autograd gradient there and WD's forward are NaN in
//             the reference — here the column contributes zeros and receives a zero gradient.  A deliberate deviation.
//   tile      corr_tile_kernel, the split-K correlation tile: grid (output tile, row chunk, product).  A workgroup sweeps
//             its row chunk in steps of 32 rows; a thread reads eight consecutive rows of one column (a wave's 64 lanes: 64
//             adjacent columns, so every row is one coalesced 256-byte read), splits them into the three bf16 planes (split8)
//             and stores them TRANSPOSED into LDS as [column][32 kpos] through split_lds_off — the store pattern of
//             gram2_stage — so that the fragments stay one 16-byte LDS read per plane.  Each 16 k: six
//             v_mfma_f32_32x32x16_bf16, smallest terms first, on two alternating accumulators; the next step's global loads
//             are issued before the MFMAs.  Rows >= n and columns >= d enter as zeros.  GBT: one product, every tile; WD:
//             two symmetric products, tiles ta <= tb only, mirrored by the fold.  The fp32 partial tile goes to the workspace
//             ws[chunk][product][d][d].
//             Split: rows per chunk = corr_chunk_rows(n, d, products) (gigl_correlate_chunk_rows): as many chunks as bring
//             products x tiles x chunks to 512 workgroups (two per CU), never a chunk shorter than 64 rows (the last, ragged
//             one apart).  Workspace bound: chunks x products x d^2 floats <= 512 x 16 KB = 8 MB for GBT (every tile is
//             computed), less than twice that for WD (the mirrored tiles have room but are never written); from the ctx's arena.
//   fold      corr_fold_kernel: a workgroup per row a of C adds the partial tiles in chunk order (fp64) and scales by 1 / n;
//             GBT: G = dL/dC (2 (C_aa - 1) on the diagonal, 2 C_ab / d off it) and, from the column a, G^T; WD: E_k = I - c_k,
//             unnormalised.  Per row the fp64 sums the loss needs and r_a = sum_i g_ia z_ia (g = dL/dz), which the
//             standardisation's backward needs, from d x d data alone: r_a = sum_b G_ab C_ab.
//   finish    corr_finish_kernel (one workgroup, gigl_block1024_sum_f64): the loss, the three norms of WD and the backward's
//             scalars alpha_1, alpha_2, beta — device scalars, so no host read — and per column rinv and
//             kcol = r_a t / (s (n - 1)), t = s + eps.  A zero norm gives a zero scalar, not a division.
//   backward  corr_backward_kernel: one workgroup per (view, 64-row tile, 128-column chunk).  g_ia = alpha_v sum_b src_ib M_ab
//             + beta (z_v - z_other)_ia with (GBT) src the OTHER view, M = G or G^T, alpha = 1 / n, beta = 0; (WD) src the
//             view itself, M = E_k, alpha_k = -2 lambd / (N |E_k|), beta = 1 / (N |z1 - z2|_F).  The product is Gram-shaped (K
//             = d contiguous in both panels) and goes through gram_tile itself; its single row bound is not needed because z
//             and M are padded to whole tiles (rows >= n / >= d only reach output elements nobody writes).  The epilogue
//             applies the standardisation's backward in registers, dx = gout rinv (g - z kcol) — the mean(g) term vanishes
//             because the source's columns are centred — and writes dh.  One owner per element.  n == 2: zeros — a
//             standardised column of two rows is +-1 / sqrt 2 whatever the rows, so the true gradient vanishes identically,
//             and the difference g - z kcol would leave 1e-7 of g.
#include "common.h"
#include "dispatch.h"
#include "gram_tile.h"
#include "wave_reduce.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

constexpr int CMAXD = 512;
constexpr int32_t CORR_MAX_N = 1 << 18;
constexpr int CORR_WORKGROUPS = 512;  // what the split aims at: two workgroups per CU
constexpr int CORR_MIN_CHUNK = 64;    // rows: no chunk but the last is shorter
constexpr int CORR_STAT_ROWS = 256, CORR_STAT_CHUNKS = 64;  // statistics: chunks of >= 256 rows, at most 64 of them
constexpr int CCH = 128;              // columns of d per backward workgroup
constexpr double GBT_EPS = 1e-15;
constexpr int MODE_GBT = 0, MODE_WD = 1;

int corr_tiles(int d, int products) {
  const int nt = (d + PT - 1) / PT;
  return products == 1 ? nt * nt : nt * (nt + 1) / 2;
}

// rows per chunk of the split-K sweep: a multiple of 32, a pure function of (n, d, products)
int corr_chunk_rows(int n, int d, int products) {
  const int want = std::max(1, CORR_WORKGROUPS / (products * corr_tiles(d, products)));
  const int chunks = std::min(want, std::max(1, n / CORR_MIN_CHUNK));
  return ((n + chunks - 1) / chunks + PBK - 1) / PBK * PBK;
}

int corr_stat_rows(int n) {
  const int chunks = std::min(CORR_STAT_CHUNKS, (n + CORR_STAT_ROWS - 1) / CORR_STAT_ROWS);
  return (n + chunks - 1) / chunks;
}

// ---- statistics ---------------------------------------------------------------------------------------------------------
// a column's chunk partials (part [chunks][d]) in chunk order
__device__ __forceinline__ double corr_fold(const double* __restrict__ part, int chunks, int d, int col) {
  double t = 0.0;
  for (int ch = 0; ch < chunks; ++ch) t += part[(int64_t)ch * d + col];
  return t;
}

__device__ __forceinline__ double corr_meet4(const double (*s_p)[64], int lane) {
  return ((s_p[0][lane] + s_p[1][lane]) + s_p[2][lane]) + s_p[3][lane];
}

// part[view][chunk][col] = sum over the chunk's rows of x (PASS 0) or of (x - mu)^2 (PASS 1: mu from PASS 0's partials, sums)
template <int PASS>
__global__ __launch_bounds__(256) void corr_colsum_kernel(const float* __restrict__ h1, int64_t ld1, const float* __restrict__ h2,
                                                          int64_t ld2, int n, int d, int rows, int chunks,
                                                          const double* __restrict__ sums, double* __restrict__ part) {
  __shared__ double s_p[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane, ch = blockIdx.y, view = blockIdx.z;
  const float* h = view ? h2 : h1;
  const int64_t ld = view ? ld2 : ld1;
  const bool live = col < d;
  double mu = 0.0, acc = 0.0;
  if (PASS == 1 && live) mu = corr_fold(sums + (int64_t)view * chunks * d, chunks, d, col) / (double)n;
  const int i1 = min(n, (ch + 1) * rows);
  if (live) {
    for (int i = ch * rows + wv; i < i1; i += 4) {
      const double x = (double)h[(int64_t)i * ld + col] - mu;
      acc += PASS == 0 ? x : x * x;
    }
  }
  s_p[wv][lane] = acc;
  __syncthreads();
  if (wv == 0 && live) part[((int64_t)view * chunks + ch) * d + col] = corr_meet4(s_p, lane);
}

// z [2][npad][d], dz [n][d] (WD; NULL for GBT), stat [2][2][d] (per view: s, then rinv), part [chunks][3][d] (sum dz^2, sum z1
// dz, -sum z2 dz per column and chunk); sums, sqs: the two passes' partials [2][chunks][d]
__global__ __launch_bounds__(256) void corr_rows_kernel(const float* __restrict__ h1, int64_t ld1, const float* __restrict__ h2,
                                                        int64_t ld2, int n, int npad, int d, int rows, int chunks, double eps,
                                                        const double* __restrict__ sums, const double* __restrict__ sqs,
                                                        float* __restrict__ z, float* __restrict__ dz, double* __restrict__ stat,
                                                        double* __restrict__ part) {
  __shared__ double s_p[3][4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane, ch = blockIdx.y;
  const bool live = col < d;
  double mu[2] = {0.0, 0.0}, ri[2] = {0.0, 0.0}, acc[3] = {0.0, 0.0, 0.0};
  if (live) {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      mu[v] = corr_fold(sums + (int64_t)v * chunks * d, chunks, d, col) / (double)n;
      const double sd = sqrt(corr_fold(sqs + (int64_t)v * chunks * d, chunks, d, col) / (double)(n - 1));
      ri[v] = sd > 0.0 ? 1.0 / (sd + eps) : 0.0;
      if (ch == 0 && wv == 0) {
        stat[(int64_t)(2 * v) * d + col] = sd;
        stat[(int64_t)(2 * v + 1) * d + col] = ri[v];
      }
    }
    const int i1 = min(n, (ch + 1) * rows), iz = ch == chunks - 1 ? npad : i1;  // (the last chunk zeroes the padding rows)
    float *za = z + col, *zb = z + (int64_t)npad * d + col;
    for (int i = ch * rows + wv; i < iz; i += 4) {
      double z1 = 0.0, z2 = 0.0;
      if (i < n) {
        z1 = ((double)h1[(int64_t)i * ld1 + col] - mu[0]) * ri[0];
        z2 = ((double)h2[(int64_t)i * ld2 + col] - mu[1]) * ri[1];
        const double dd = z1 - z2;
        if (dz) dz[(int64_t)i * d + col] = (float)dd;
        acc[0] += dd * dd;
        acc[1] += z1 * dd;
        acc[2] -= z2 * dd;
      }
      za[(int64_t)i * d] = (float)z1;
      zb[(int64_t)i * d] = (float)z2;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) s_p[j][wv][lane] = acc[j];
  __syncthreads();
  if (wv == 0 && live) {
#pragma unroll
    for (int j = 0; j < 3; ++j) part[((int64_t)ch * 3 + j) * d + col] = corr_meet4(s_p[j], lane);
  }
}

// ---- the split-K correlation tile ---------------------------------------------------------------------------------------
// ws[chunk blockIdx.y][product blockIdx.z][a][b] = sum over the chunk's rows i of za[i][a] zb[i][b] for the 64 x 64 tile
// blockIdx.x; sym: the products are z_k^T z_k (k = product) and only tiles ta <= tb exist; else the one product is z1^T z2.
// (two waves per SIMD, as the Gram backward kernels: 16 prefetched values, 12 fragments and 32 accumulators fit with room)
__global__ __launch_bounds__(256, 2) void corr_tile_kernel(const float* __restrict__ z, int n, int npad, int d, int sym,
                                                           int chunk_rows, float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) short s[6][PPLANE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, g = lane >> 5;
  const int wa = wv >> 1, wb = wv & 1;
  const int nt = (d + PT - 1) / PT, prod = blockIdx.z, nprod = gridDim.z;
  int ta, tb;
  if (sym) {  // the blockIdx.x-th pair ta <= tb, row by row of the upper triangle
    int rem = blockIdx.x;
    for (ta = 0; rem >= nt - ta; ++ta) rem -= nt - ta;
    tb = ta + rem;
  } else {
    ta = blockIdx.x / nt;
    tb = blockIdx.x % nt;
  }
  const float* za = z + (int64_t)(sym ? prod : 0) * npad * d;
  const float* zb = z + (int64_t)(sym ? prod : 1) * npad * d;
  const int a0 = ta * PT, b0 = tb * PT, ca = a0 + lane, cb = b0 + lane;
  const int i0 = blockIdx.y * chunk_rows, i1 = min(n, i0 + chunk_rows);
  float16_t acc0, acc1;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc0[v] = acc1[v] = 0.f;
  float ra[8], rb[8];  // this thread: rows k0 + 8 wv .. + 7 of columns ca (panel a) and cb (panel b)
  auto gload = [&](int k0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int row = k0 + 8 * wv + u;
      ra[u] = (row < i1 && ca < d) ? za[(int64_t)row * d + ca] : 0.f;
      rb[u] = (row < i1 && cb < d) ? zb[(int64_t)row * d + cb] : 0.f;
    }
  };
  gload(i0);
  const int o = split_lds_off(lane, 8 * wv);
  for (int k0 = i0; k0 < i1; k0 += PBK) {
    __syncthreads();
    bf16x8_t pa[3], pb[3];
    split8(ra, pa[0], pa[1], pa[2]);
    split8(rb, pb[0], pb[1], pb[2]);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      *reinterpret_cast<bf16x8_t*>(&s[p][o]) = pa[p];
      *reinterpret_cast<bf16x8_t*>(&s[3 + p][o]) = pb[p];
    }
    __syncthreads();
    if (k0 + PBK < i1) gload(k0 + PBK);  // lands during this step's MFMAs
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
  float* out = ws + ((int64_t)blockIdx.y * nprod + prod) * d * d;
  const int b = b0 + wb * 32 + r;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int a = a0 + wa * 32 + gram_row(v, g);
    if (a < d && b < d) out[(int64_t)a * d + b] = acc0[v] + acc1[v];
  }
}

// ---- fold, loss, dL/dC --------------------------------------------------------------------------------------------------
// C[a][b] of product `prod`: the partial tiles in chunk order, over n.  sym: a tile below the diagonal is its mirror image.
__device__ __forceinline__ double corr_c(const float* __restrict__ ws, int chunks, int nprod, int prod, int d, int a, int b,
                                         bool sym, double inv_n) {
  if (sym && (a >> 6) > (b >> 6)) {
    const int t = a;
    a = b;
    b = t;
  }
  const float* p = ws + ((int64_t)prod * d + a) * d + b;
  const int64_t stride = (int64_t)nprod * d * d;
  double t = 0.0;
  for (int ch = 0; ch < chunks; ++ch) t += (double)p[ch * stride];
  return t * inv_n;
}

// row a = blockIdx.x (< dpad: rows >= d of M are zeroed) of M [2][dpad][d] and of rowpart [4][d]:
//   GBT  M[0] = G, M[1] = G^T; rowpart 0: r of view 1 (sum_b G_ab C_ab), 1: r of view 2 (sum_b G_ba C_ba), 2: the row's loss terms
//   WD   (product k = blockIdx.y) M[k] = E_k; rowpart k: sum_b E_ab c_ab, 2 + k: sum_b E_ab^2
__global__ __launch_bounds__(256) void corr_fold_kernel(const float* __restrict__ ws, int chunks, int n, int d, int dpad, int mode,
                                                        float* __restrict__ M, double* __restrict__ rowpart) {
  __shared__ double s_w[3][4];
  const int tid = threadIdx.x, a = blockIdx.x, k = blockIdx.y;
  float* m0 = M + ((int64_t)k * dpad + a) * d;
  float* m1 = M + ((int64_t)dpad + a) * d;  // (GBT)
  if (a >= d) {  // (the whole workgroup)
    for (int b = tid; b < d; b += 256) {
      m0[b] = 0.f;
      if (mode == MODE_GBT) m1[b] = 0.f;
    }
    return;
  }
  const double inv_n = 1.0 / (double)n;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int b = tid; b < d; b += 256) {
    if (mode == MODE_GBT) {
      const double crow = corr_c(ws, chunks, 1, 0, d, a, b, false, inv_n), ccol = corr_c(ws, chunks, 1, 0, d, b, a, false, inv_n);
      const double grow = a == b ? 2.0 * (crow - 1.0) : 2.0 * crow / d, gcol = a == b ? grow : 2.0 * ccol / d;
      m0[b] = (float)grow;
      m1[b] = (float)gcol;
      acc[0] += grow * crow;
      acc[1] += gcol * ccol;
      acc[2] += a == b ? (1.0 - crow) * (1.0 - crow) : crow * crow / d;
    } else {
      const double c = corr_c(ws, chunks, 2, k, d, a, b, true, inv_n), e = (a == b ? 1.0 : 0.0) - c;
      m0[b] = (float)e;
      acc[0] += e * c;
      acc[1] += e * e;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double t = gigl_wave_sum_f64(acc[j]);
    if ((tid & 63) == 0) s_w[j][tid >> 6] = t;
  }
  __syncthreads();
  if (tid == 0) {
    double t[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = ((s_w[j][0] + s_w[j][1]) + s_w[j][2]) + s_w[j][3];
    if (mode == MODE_GBT) {
      for (int j = 0; j < 3; ++j) rowpart[(int64_t)j * d + a] = t[j];
    } else {
      rowpart[(int64_t)k * d + a] = t[0];
      rowpart[(int64_t)(2 + k) * d + a] = t[1];
    }
  }
}

// one workgroup: *loss, coef [8] = {alpha_1, alpha_2, beta, |z1 - z2|_F / N, |I - c1|_F, |I - c2|_F, 0, 0} (GBT: {1 / n, 1 / n, 0,
// ...}), colv [2][2][d] (per view: rinv, then kcol = r_a t / (s (n - 1))) as floats; part: corr_rows_kernel's, sc chunks
__global__ __launch_bounds__(1024) void corr_finish_kernel(int n, int d, int mode, float lambd, double eps, int sc,
                                                           const double* __restrict__ part, const double* __restrict__ stat,
                                                           const double* __restrict__ rowpart, float* __restrict__ colv,
                                                           float* __restrict__ coef, float* __restrict__ loss) {
  __shared__ double s_tot[3];
  const int tid = threadIdx.x;
  const int sums = mode == MODE_GBT ? 1 : 3;
  for (int j = 0; j < sums; ++j) {  // GBT: the rows' loss terms; WD: sum dz^2, |E_1|^2, |E_2|^2
    double acc = 0.0;
    for (int a = tid; a < d; a += 1024) {
      if (mode == MODE_WD && j == 0) {
        for (int ch = 0; ch < sc; ++ch) acc += part[((int64_t)ch * 3) * d + a];
      } else {
        acc += rowpart[(int64_t)(mode == MODE_GBT ? 2 : 1 + j) * d + a];
      }
    }
    const double t = gigl_block1024_sum_f64(acc);
    if (tid == 0) s_tot[j] = t;
    __syncthreads();  // (and the helper's LDS is free for the next sum)
  }
  const double N = (double)n;
  double al[2], be = 0.0, L, nrm[3] = {0.0, 0.0, 0.0};
  if (mode == MODE_GBT) {
    al[0] = al[1] = 1.0 / N;
    L = s_tot[0];
  } else {
    nrm[0] = sqrt(s_tot[0]) / N;
    nrm[1] = sqrt(s_tot[1]);
    nrm[2] = sqrt(s_tot[2]);
    L = nrm[0] + (double)lambd * (nrm[1] + nrm[2]);
    for (int v = 0; v < 2; ++v) al[v] = nrm[1 + v] > 0.0 ? -2.0 * (double)lambd / (N * nrm[1 + v]) : 0.0;
    be = nrm[0] > 0.0 ? 1.0 / (N * N * nrm[0]) : 0.0;
  }
  if (tid == 0) {
    *loss = (float)L;
    coef[0] = (float)al[0];
    coef[1] = (float)al[1];
    coef[2] = (float)be;
    for (int j = 0; j < 3; ++j) coef[3 + j] = (float)nrm[j];
    coef[6] = coef[7] = 0.f;
  }
  for (int a = tid; a < d; a += 1024) {
    for (int v = 0; v < 2; ++v) {
      const double sd = stat[(int64_t)(2 * v) * d + a];
      double rr = rowpart[(int64_t)v * d + a];
      if (mode == MODE_WD) {
        double q = 0.0;
        for (int ch = 0; ch < sc; ++ch) q += part[((int64_t)ch * 3 + 1 + v) * d + a];
        rr = N * al[v] * rr + be * q;
      }
      colv[(int64_t)(2 * v) * d + a] = (float)stat[(int64_t)(2 * v + 1) * d + a];
      colv[(int64_t)(2 * v + 1) * d + a] = sd > 0.0 ? (float)(rr * (sd + eps) / (sd * (N - 1.0))) : 0.f;
    }
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------
// dh of view blockIdx.z, rows of tile blockIdx.x, columns [128 blockIdx.y, +128).  z [2][npad][d], M [2][dpad][d], dz [n][d] or
// NULL; own_src: the product's rows are the view's own z (WD), else the other view's (GBT).
template <bool VEC>
__global__ __launch_bounds__(256, 2) void corr_backward_kernel(const float* __restrict__ z, const float* __restrict__ dz,
                                                               const float* __restrict__ M, const float* __restrict__ colv,
                                                               const float* __restrict__ coef, int n, int npad, int d, int dpad,
                                                               int own_src, const float* __restrict__ gout, float* __restrict__ dh1,
                                                               int64_t ld1, float* __restrict__ dh2, int64_t ld2) {
  __shared__ __attribute__((aligned(16))) short s[6][PPLANE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, g = lane >> 5;
  const int wa = wv >> 1, wb = wv & 1;
  const int view = blockIdx.z, I0 = blockIdx.x * PT, c0 = blockIdx.y * CCH;
  const float* zv = z + (int64_t)view * npad * d;
  const float* src = own_src ? zv : z + (int64_t)(1 - view) * npad * d;
  const float* Mv = M + (int64_t)view * dpad * d;
  float* dst = view ? dh2 : dh1;
  const int64_t ld = view ? ld2 : ld1;
  const float gl = gout ? *gout : 1.f, al = coef[view], be = view ? -coef[2] : coef[2];
#pragma unroll
  for (int sub = 0; sub < CCH / PT; ++sub) {
    const int a0 = c0 + PT * sub;
    if (a0 < d) {  // (the whole workgroup)
      // rows i of src against rows a of M; both are padded to whole tiles, so the row bound never bites
      const float16_t gt = gram_tile<VEC>(src, Mv, 0x7fffffff, d, I0, a0, s);
      const int a = a0 + wb * 32 + r;
      if (a < d) {
        const float ri = gl * colv[(int64_t)(2 * view) * d + a], kc = colv[(int64_t)(2 * view + 1) * d + a];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int i = I0 + wa * 32 + gram_row(v, g);
          if (i < n) {
            float gz = al * gt[v];
            if (dz) gz += be * dz[(int64_t)i * d + a];
            dst[(int64_t)i * ld + a] = ri * (gz - zv[(int64_t)i * d + a] * kc);
          }
        }
      }
    }
  }
}

int32_t corr_check(gigl_ctx* ctx, int32_t n, int32_t d) {
  GIGL_REQUIRE(ctx, d >= 1 && d <= CMAXD, "the correlation kernels serve 1 <= d <= %d (d=%d)", CMAXD, d);
  GIGL_REQUIRE(ctx, n >= 2 && n <= CORR_MAX_N, "the correlation losses need 2 <= n <= %d rows (n=%d)", CORR_MAX_N, n);
  return GIGL_OK;
}

int32_t corr_forward(gigl_ctx* ctx, int mode, const float* h1, int64_t ld1, const float* h2, int64_t ld2, int32_t n, int32_t d,
                     float lambd, float* z, float* dz, float* M, double* stat, float* colv, float* coef, float* loss) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const int32_t rc0 = corr_check(ctx, n, d);
  if (rc0 != GIGL_OK) return rc0;
  GIGL_REQUIRE(ctx, h1 && h2 && z && M && stat && colv && coef && loss && (mode == MODE_GBT || dz) && ld1 >= d && ld2 >= d,
               "null argument or a row stride < d");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int products = mode == MODE_GBT ? 1 : 2;
  const int npad = (n + PT - 1) / PT * PT, dpad = (d + PT - 1) / PT * PT;
  const int srows = corr_stat_rows(n), sc = (n + srows - 1) / srows;
  const int crows = corr_chunk_rows(n, d, products), chunks = (n + crows - 1) / crows;
  const int64_t stat_bytes = gigl_align_up((int64_t)2 * sc * d * 8, 256), part_bytes = gigl_align_up((int64_t)3 * sc * d * 8, 256);
  const int64_t row_bytes = gigl_align_up((int64_t)4 * d * 8, 256);
  const int64_t ws_bytes = gigl_align_up((int64_t)chunks * products * d * d * 4, 256);
  const int32_t rc = gigl_arena_reset(ctx, 2 * stat_bytes + part_bytes + row_bytes + ws_bytes + 5 * 256 + 1024);
  if (rc != GIGL_OK) return rc;
  double* sums = (double*)gigl_arena_alloc(ctx, stat_bytes);
  double* sqs = (double*)gigl_arena_alloc(ctx, stat_bytes);
  double* part = (double*)gigl_arena_alloc(ctx, part_bytes);
  double* rowpart = (double*)gigl_arena_alloc(ctx, row_bytes);
  float* ws = (float*)gigl_arena_alloc(ctx, ws_bytes);
  GIGL_REQUIRE(ctx, sums && sqs && part && rowpart && ws, "scratch arena exhausted");
  const double eps = mode == MODE_GBT ? GBT_EPS : 0.0;
  const unsigned cbs = (unsigned)((d + 63) / 64);
  hipLaunchKernelGGL(corr_colsum_kernel<0>, dim3(cbs, sc, 2), dim3(256), 0, st, h1, ld1, h2, ld2, n, d, srows, sc,
                     (const double*)nullptr, sums);
  hipLaunchKernelGGL(corr_colsum_kernel<1>, dim3(cbs, sc, 2), dim3(256), 0, st, h1, ld1, h2, ld2, n, d, srows, sc,
                     (const double*)sums, sqs);
  hipLaunchKernelGGL(corr_rows_kernel, dim3(cbs, sc), dim3(256), 0, st, h1, ld1, h2, ld2, n, npad, d, srows, sc, eps,
                     (const double*)sums, (const double*)sqs, z, mode == MODE_GBT ? nullptr : dz, stat, part);
  hipLaunchKernelGGL(corr_tile_kernel, dim3((unsigned)corr_tiles(d, products), (unsigned)chunks, (unsigned)products), dim3(256), 0, st,
                     (const float*)z, n, npad, d, mode == MODE_WD ? 1 : 0, crows, ws);
  hipLaunchKernelGGL(corr_fold_kernel, dim3((unsigned)dpad, (unsigned)products), dim3(256), 0, st, (const float*)ws, chunks, n, d, dpad,
                     mode, M, rowpart);
  hipLaunchKernelGGL(corr_finish_kernel, dim3(1), dim3(1024), 0, st, n, d, mode, lambd, eps, sc, (const double*)part,
                     (const double*)stat, (const double*)rowpart, colv, coef, loss);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t corr_backward(gigl_ctx* ctx, int mode, const float* z, const float* dz, const float* M, const float* colv, const float* coef,
                      int32_t n, int32_t d, const float* gout_dev, float* dh1, int64_t ld1, float* dh2, int64_t ld2) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const int32_t rc0 = corr_check(ctx, n, d);
  if (rc0 != GIGL_OK) return rc0;
  GIGL_REQUIRE(ctx, z && M && colv && coef && dh1 && dh2 && (mode == MODE_GBT || dz) && ld1 >= d && ld2 >= d,
               "null argument or a row stride < d");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (n == 2) {  // a standardised column of two rows is +-1 / sqrt 2 whatever the rows: both losses are locally constant
    gigl_zero_rows(ctx->stream, dh1, ld1, n, d);
    gigl_zero_rows(ctx->stream, dh2, ld2, n, d);
    GIGL_HIP_CHECK(ctx, hipGetLastError());
    return GIGL_OK;
  }
  const int npad = (n + PT - 1) / PT * PT, dpad = (d + PT - 1) / PT * PT;
  const dim3 grid((unsigned)(npad / PT), (unsigned)((d + CCH - 1) / CCH), 2);
  dispatch_bool(d % 4 == 0 && gigl_aligned16(z) && gigl_aligned16(M), [&](auto vec) {
    hipLaunchKernelGGL(corr_backward_kernel<decltype(vec)::value>, grid, dim3(256), 0, ctx->stream, z, mode == MODE_GBT ? nullptr : dz,
                       M, colv, coef, n, npad, d, dpad, mode == MODE_WD ? 1 : 0, gout_dev, dh1, ld1, dh2, ld2);
  });
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

}  // namespace

extern "C" {

int32_t gigl_correlate_chunk_rows(int32_t n, int32_t d, int32_t products) {
  if (n < 1 || d < 1 || d > CMAXD || products < 1 || products > 2) return 0;
  return corr_chunk_rows(n, d, products);
}

int32_t gigl_gbt_loss(gigl_ctx* ctx, const float* h1, int64_t ld1, const float* h2, int64_t ld2, int32_t n, int32_t d, float* z_out,
                      float* m_out, double* stat_out, float* colv_out, float* coef_out, float* loss_out) {
  return corr_forward(ctx, MODE_GBT, h1, ld1, h2, ld2, n, d, 0.f, z_out, nullptr, m_out, stat_out, colv_out, coef_out, loss_out);
}

int32_t gigl_gbt_loss_backward(gigl_ctx* ctx, const float* z, const float* m, const float* colv, const float* coef, int32_t n, int32_t d,
                               const float* gout_dev, float* dh1, int64_t ld1, float* dh2, int64_t ld2) {
  return corr_backward(ctx, MODE_GBT, z, nullptr, m, colv, coef, n, d, gout_dev, dh1, ld1, dh2, ld2);
}

int32_t gigl_whitening_loss(gigl_ctx* ctx, const float* h1, int64_t ld1, const float* h2, int64_t ld2, int32_t n, int32_t d,
                            float lambd, float* z_out, float* dz_out, float* m_out, double* stat_out, float* colv_out, float* coef_out,
                            float* loss_out) {
  return corr_forward(ctx, MODE_WD, h1, ld1, h2, ld2, n, d, lambd, z_out, dz_out, m_out, stat_out, colv_out, coef_out, loss_out);
}

int32_t gigl_whitening_loss_backward(gigl_ctx* ctx, const float* z, const float* dz, const float* m, const float* colv, const float* coef,
                                     int32_t n, int32_t d, const float* gout_dev, float* dh1, int64_t ld1, float* dh2, int64_t ld2) {
  return corr_backward(ctx, MODE_WD, z, dz, m, colv, coef, n, d, gout_dev, dh1, ld1, dh2, ld2);
}

}  // extern "C"
