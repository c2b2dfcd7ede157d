// reconstruct.hip — the FeatureReconstruction task's decoder and scaled-cosine-error loss (GraphMAE: python/gigl/src/common/
// models/layers/task.py:282-348, loss.py:419-441), forward and the row side of the gradient.  The reference applies a Linear to
// ALL N rows of the encoder output E, zeroes the roots' rows, runs GraphConv(out, in) over ALL nodes and edges and keeps the B
// root rows.  On a root row the root term of GraphConv vanishes (its h was just zeroed) and the rest is linear, so for root
// position i with node id r_i the whole decoder is
//     s_i = sum over the in-edges e of r_i whose source col[e] is NOT a root of E[col[e]]          [B, out]
//     t_i = s_i W_ed^T   (reconstruction_enc_dec, no bias)                                         [B, out]
//     p_i = t_i W_rel^T + b_rel   (GraphConv.lin_rel)                                              [B, in]
//     c_i = <x_i / max(|x_i|, 1e-12), p_i / max(|p_i|, 1e-12)>   (x_i = X[r_i], the unmasked features)
//     loss = (1/B) sum_i max(1 - c_i, 0)^alpha   (the clamp: rounding can leave 1 - c at -1e-8, and alpha need not be an integer)
// — B rows of work instead of N, and no [N, in] intermediate.  GraphConv.lin_root gets no gradient at all; dE is zero on every
// root row and on every row no root lists.  No float atomics, one owner per element, every sum in a fixed order: the same
// inputs give the same bits.
//   roots     fr_roots_kernel: the is_root byte table (a byte per node, cleared before; duplicated root ids are separate rows i
//             and set the same flag) and, per root position, where its row of the by-destination CSR starts and ends.
//   forward   fr_forward_kernel, one workgroup of 256 per 64-row tile of root positions, three phases.
//             gather: a wave owns sixteen of the tile's roots, one after the other.  A lane carries a 16-byte segment of the out
//             columns (two beyond 256; four scalar loads where out % 4 != 0 or the rows are not aligned); where a row needs
//             fewer than 64 lanes the wave splits into 64 / lanes-per-row groups that take the root's edges in turn, and every
//             group has four neighbour rows in flight: ids, then flags, then rows, three round trips per 4 x groups edges
//             instead of one chain per neighbour.  Sources flagged in is_root (the root's own self loop, any other root) are
//             skipped.  A group adds its edges in CSR order, the groups meet by butterfly: s_i -> s_out.
//             first product: t = s W_ed^T by gram_tile's general form, the A panel this workgroup's rows of s_out (visible
//             after a barrier; rows >= B enter as zeros through the panel's row bound); 64 x 64 blocks of t go to t_out and into
//             LDS as fp32 rows out + 4 floats apart (fr_ld): 64 x 516 x 4 = 129 KB at out = 512, beside the 24 KB of
//             gram_tile's planes, 1.5 KB of row sums and 256 B of root ids, under gfx950's 160 KB: out <= 512.
//             second product: p = t W_rel^T + b, the A panel from LDS, a 64 x 64 block of p at a time — `in` costs no LDS.  A
//             block goes to p_out and its contributions to the three row sums |p|^2, p.x, |x|^2 are taken from the accumulators,
//             x read in place through the root list.  The rows meet (gram_rows_meet), 64 threads write the row stats and
//             max(1 - c, 0)^alpha, whose tile sum (fp64) goes to the arena; fr_fold_kernel (one workgroup) adds the tiles'
//             sums in tile order.
//   backward  fr_backward_kernel, the same tiles.  A wave rebuilds sixteen rows of
//                 g_i = dL/dp_i = -(alpha / B) (1 - c_i)^(alpha - 1) (x^_i - c_i p^_i) / max(|p_i|, 1e-12)
//             from p_out, the targets and the row stats into g_out (a row with |p| <= 1e-12 follows torch autograd through
//             F.normalize, which clamps the norm's VALUE: p^ = p / 1e-12 and there is no norm term; in = 1: a cosine is a sign,
//             exact zeros).  dT = G W_rel reads g_out back as its A panel (K = in, so G does not fit LDS), goes to dt_out and
//             into LDS; dS = dT W_ed -> ds_out.  Both contract over the weights' ROW index: W_rel^T and W_ed^T are written once
//             per call into the arena (in <= 8192: at most 16 MB).
//             dE[j] = sum of dS_i over the root positions i whose row lists j, j not a root: gigl_transposed_rows_build over the
//             per-root row bounds gives every node its readers in arrival order (integer atomics only), fr_sort_lists_kernel
//             ranks each list ascending, and fr_scatter_rows_kernel WRITES every one of dE's N rows once — zeros for roots and
//             unlisted nodes.
//   no decoder  w_ed == NULL: p_i = e_i (FeatureReconstructionLoss on already-decoded rows): the row stats, the fold and g alone.
#include "common.h"
#include "dispatch.h"
#include "gram_tile.h"
#include "wave_reduce.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

constexpr int FR_MAX_OUT = 512;
constexpr int FR_MAX_IN = 8192;
constexpr int32_t FR_MAX_B = 1 << 18;
constexpr float FR_EPS = 1e-12f;
constexpr int FR_STAT = 3;  // row sums: |p|^2, p.x, |x|^2

struct fr_args {
  const float* e;  // the encoder's rows [n_nodes][out] (forward) — or, without a decoder, the predictions [b][in]
  int64_t lde;
  const int32_t* col;      // sources of the by-destination CSR
  const uint8_t* is_root;  // [n_nodes]
  const int32_t* roots;    // [b], or NULL: target row i is x's row i
  const float* x;          // the targets' matrix
  int64_t ldx;
  const float *w_ed, *w_rel, *b_rel;  // forward: W_ed [out][out], W_rel [in][out]; backward: W_ed^T, W_rel^T [out][in]
  int n_nodes, b, out, in;
  float alpha;
};

__host__ __device__ inline int fr_ld(int k) { return (k + 3) / 4 * 4 + 4; }  // floats between the rows of an LDS tile

// lanes that carry one row of `out` floats as 16-byte segments: a power of two, at most 64
inline int fr_lanes_per_row(int out) {
  int lpr = 1;
  while (lpr < 64 && lpr * 4 < out) lpr <<= 1;
  return lpr;
}

template <bool VEC>
__device__ __forceinline__ void fr_store4(float* __restrict__ row, int d, int k, float4_t v) {
  if constexpr (VEC) {
    if (k < d) *reinterpret_cast<float4_t*>(row + k) = v;
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (k + t < d) row[k + t] = v[t];
  }
}

// root_rows [2][b]: where root position i's CSR row starts and ends (an id outside [0, n_nodes): an empty row)
__global__ __launch_bounds__(256) void fr_roots_kernel(const int32_t* __restrict__ roots, const int32_t* __restrict__ rowptr, int b,
                                                       int n_nodes, uint8_t* __restrict__ is_root, int32_t* __restrict__ root_rows) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= b) return;
  const int r = roots[i];
  const bool ok = (unsigned)r < (unsigned)n_nodes;
  if (ok) is_root[r] = 1;
  root_rows[i] = ok ? rowptr[r] : 0;
  root_rows[b + i] = ok ? rowptr[r + 1] : 0;
}

// s_out[i] for this wave's sixteen root positions from I0 + 16 wave
template <bool VEC>
__device__ __forceinline__ void fr_gather(const fr_args& a, const int32_t* __restrict__ root_rows, int lpr, int I0,
                                          float* __restrict__ s_out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int gl = lane & (lpr - 1), grp = lane / lpr, groups = 64 / lpr;
  const int nq = a.out > 256 ? 2 : 1;  // segments per lane
  for (int il = wv * 16; il < wv * 16 + 16; ++il) {
    const int i = I0 + il;
    if (i >= a.b) break;  // (the whole wave)
    const int e0 = root_rows[i], e1 = root_rows[a.b + i];
    float4_t acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int eb = e0; eb < e1; eb += 4 * groups) {
      int j[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = eb + u * groups + grp;
        j[u] = e < e1 ? a.col[e] : -1;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if ((unsigned)j[u] >= (unsigned)a.n_nodes || a.is_root[j[u]]) j[u] = -1;
      float4_t v[4][2];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          v[u][q] = float4_t{0.f, 0.f, 0.f, 0.f};
          if (q < nq && j[u] >= 0) v[u][q] = pair_load4<VEC>(a.e, a.n_nodes, a.lde, a.out, j[u], 4 * (gl + 64 * q));
        }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[q] += v[u][q];
    }
    for (int off = lpr; off < 64; off <<= 1)  // the groups meet: every lane adds the same pairs
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[q][t] += __shfl_xor(acc[q][t], off, 64);
    if (grp == 0)
      for (int q = 0; q < nq; ++q) fr_store4<VEC>(s_out + (int64_t)i * a.out, a.out, 4 * (gl + 64 * q), acc[q]);
  }
}

// grid: row tiles.  s_out, t_out [b][out], p_out [b][in], stat_out [FR_STAT][b], part [tiles].  Dynamic LDS: the t tile, 64 rows
// fr_ld(out) floats apart (none without a decoder).
template <bool VEC>
__global__ __launch_bounds__(256) void fr_forward_kernel(const fr_args a, const int32_t* __restrict__ root_rows, int lpr,
                                                         float* __restrict__ s_out, float* __restrict__ t_out,
                                                         float* __restrict__ p_out, float* __restrict__ stat_out,
                                                         double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float ts[];
  __shared__ __attribute__((aligned(16))) short s[6][PPLANE];
  __shared__ float s_row[2][FR_STAT][PT];
  __shared__ int s_rid[PT];  // the tile's target rows (-1: none)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, g = lane >> 5;
  const int wa = wv >> 1, wb = wv & 1;
  const int I0 = blockIdx.x * PT, b = a.b, out = a.out, in = a.in;
  const bool dec = a.w_ed != nullptr;
  const int tld = fr_ld(out);
  if (tid < PT) {
    int rid = -1;
    if (I0 + tid < b) {
      rid = a.roots ? a.roots[I0 + tid] : I0 + tid;
      if (a.roots && (unsigned)rid >= (unsigned)a.n_nodes) rid = -1;
    }
    s_rid[tid] = rid;
  }
  if (dec) {
    fr_gather<VEC>(a, root_rows, lpr, I0, s_out);
    __threadfence_block();
    __syncthreads();  // this workgroup's rows of s are visible to all its threads
    for (int h0 = 0; h0 < out; h0 += PT) {
      const float16_t acc = gram_tile<VEC>(s_out, b, out, a.w_ed, out, out, out, I0, h0, s);
      const int c = h0 + wb * 32 + r;
      if (c < out) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int il = wa * 32 + gram_row(v, g);
          ts[il * tld + c] = acc[v];
          if (I0 + il < b) t_out[(int64_t)(I0 + il) * out + c] = acc[v];
        }
      }
    }
  }
  __syncthreads();  // (the second product's first loads precede its own barrier)
  float rs[FR_STAT][16];
#pragma unroll
  for (int j = 0; j < FR_STAT; ++j)
#pragma unroll
    for (int v = 0; v < 16; ++v) rs[j][v] = 0.f;
  for (int c0 = 0; c0 < in; c0 += PT) {
    float16_t acc = {};
    if (dec) acc = gram_tile<VEC>(ts, PT, tld, a.w_rel, in, out, out, 0, c0, s);
    const int c = c0 + wb * 32 + r;
    if (c < in) {
      const float bias = dec ? a.b_rel[c] : 0.f;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int il = wa * 32 + gram_row(v, g), i = I0 + il;
        if (i < b) {
          const int rid = s_rid[il];
          const float p = dec ? acc[v] + bias : a.e[(int64_t)i * a.lde + c];
          const float xv = rid >= 0 ? a.x[(int64_t)rid * a.ldx + c] : 0.f;
          if (dec) p_out[(int64_t)i * in + c] = p;
          rs[0][v] += p * p;
          rs[1][v] += p * xv;
          rs[2][v] += xv * xv;
        }
      }
    }
  }
  gram_rows_meet<FR_STAT>(rs, s_row);
  if (wv == 0) {  // a row per lane
    const int i = I0 + lane;
    double term = 0.0;
    if (i < b) {
      float t[FR_STAT];
#pragma unroll
      for (int j = 0; j < FR_STAT; ++j) {
        t[j] = s_row[0][j][lane] + s_row[1][j][lane];
        stat_out[(int64_t)j * b + i] = t[j];
      }
      const float c = t[1] / (fmaxf(sqrtf(t[0]), FR_EPS) * fmaxf(sqrtf(t[2]), FR_EPS));
      term = (double)powf(fmaxf(1.f - c, 0.f), a.alpha);
    }
    term = gigl_wave_sum_f64(term);
    if (lane == 0) part[blockIdx.x] = term;
  }
}

// one workgroup: the tiles' sums in tile order per thread, then in thread order
__global__ __launch_bounds__(1024) void fr_fold_kernel(const double* __restrict__ part, int tiles, int b, float* __restrict__ loss) {
  double acc = 0.0;
  for (int t = threadIdx.x; t < tiles; t += 1024) acc += part[t];
  const double tot = gigl_block1024_sum_f64(acc);
  if (threadIdx.x == 0) *loss = (float)(tot / (double)b);  // (b == 0: NaN)
}

// grid: row tiles.  a.e: the predictions (p_out, or the caller's rows without a decoder), a.w_rel / a.w_ed: the TRANSPOSED
// weights.  g_out [b][in] rows ldg apart.  Dynamic LDS: the dT tile, 64 rows fr_ld(out) floats apart (none without a decoder).
template <bool VIN, bool VOUT>
__global__ __launch_bounds__(256) void fr_backward_kernel(const fr_args a, const float* __restrict__ stat,
                                                          const float* __restrict__ gout, float* __restrict__ g_out, int64_t ldg,
                                                          float* __restrict__ dt_out, float* __restrict__ ds_out) {
  extern __shared__ __attribute__((aligned(16))) float dts[];
  __shared__ __attribute__((aligned(16))) short s[6][PPLANE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, g = lane >> 5;
  const int wa = wv >> 1, wb = wv & 1;
  const int I0 = blockIdx.x * PT, b = a.b, out = a.out, in = a.in;
  const int dld = fr_ld(out);
  const float gl = (gout ? *gout : 1.f) / (float)b;
  for (int il = wv * 16; il < wv * 16 + 16; ++il) {  // a wave: sixteen rows, the lanes along a row
    const int i = I0 + il;
    if (i >= b) break;  // (the whole wave; the products' row bound supplies the zeros)
    int rid = a.roots ? a.roots[i] : i;
    if (a.roots && (unsigned)rid >= (unsigned)a.n_nodes) rid = -1;
    const float pp = stat[i], np = sqrtf(pp), cp = fmaxf(np, FR_EPS), cx = fmaxf(sqrtf(stat[2 * (int64_t)b + i]), FR_EPS);
    const float c = stat[(int64_t)b + i] / (cp * cx);
    const float k = -gl * a.alpha * powf(fmaxf(1.f - c, 0.f), a.alpha - 1.f);
    float ax = k / (cp * cx), bp = np > FR_EPS ? k * c / (cp * np) : 0.f;  // g = ax x - bp p
    // in == 1: a cosine is the sign of p x, constant wherever |p| > 1e-12 — zeros, not the 1e-7 of the first term that the
    // difference of two equal terms would leave (as bootstrap.hip at out == 1)
    if (in == 1 && np > FR_EPS) ax = bp = 0.f;
    for (int c1 = lane; c1 < in; c1 += 64) {
      const float xv = rid >= 0 ? a.x[(int64_t)rid * a.ldx + c1] : 0.f;
      g_out[(int64_t)i * ldg + c1] = ax * xv - bp * a.e[(int64_t)i * a.lde + c1];
    }
  }
  if (!a.w_ed) return;  // (the whole grid)
  __threadfence_block();
  __syncthreads();  // this workgroup's rows of G are visible to all its threads
  for (int h0 = 0; h0 < out; h0 += PT) {  // dT = G W_rel: rows of G against rows of W_rel^T [out][in]
    const float16_t acc = gram_tile<VIN>(g_out, b, ldg, a.w_rel, out, in, in, I0, h0, s);
    const int c = h0 + wb * 32 + r;
    if (c < out) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int il = wa * 32 + gram_row(v, g);
        dts[il * dld + c] = acc[v];
        if (I0 + il < b) dt_out[(int64_t)(I0 + il) * out + c] = acc[v];
      }
    }
  }
  __syncthreads();
  for (int c0 = 0; c0 < out; c0 += PT) {  // dS = dT W_ed: rows of the dT tile against rows of W_ed^T [out][out]
    const float16_t acc = gram_tile<VOUT>(dts, PT, dld, a.w_ed, out, out, out, 0, c0, s);
    const int c = c0 + wb * 32 + r;
    if (c < out) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int i = I0 + wa * 32 + gram_row(v, g);
        if (i < b) ds_out[(int64_t)i * out + c] = acc[v];
      }
    }
  }
}

// a wave per node: its readers (root positions, in the arrival order of the build's slot allocation) -> ascending, by rank
// (equal entries — a doubled edge — keep their order: the same sum either way).  Roots' lists are never read.
__global__ __launch_bounds__(256) void fr_sort_lists_kernel(const uint8_t* __restrict__ is_root, const int32_t* __restrict__ cnt,
                                                            const int32_t* __restrict__ ptr, const int32_t* __restrict__ list,
                                                            int n_nodes, int32_t* __restrict__ sorted) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = (gridDim.x * blockDim.x) >> 6;
  for (int j = wave; j < n_nodes; j += waves) {
    const int c = is_root[j] ? 0 : cnt[j], p0 = ptr[j];
    for (int k = lane; k < c; k += 64) {
      const int v = list[p0 + k];
      int rank = 0;
      for (int m = 0; m < c; ++m) {
        const int u = list[p0 + m];
        rank += (u < v || (u == v && m < k)) ? 1 : 0;
      }
      sorted[p0 + rank] = v;
    }
  }
}

// de[j] = the sum of ds[i] over node j's sorted readers, lpr lanes per node; every row below n_nodes is written
template <bool VEC>
__global__ __launch_bounds__(256) void fr_scatter_rows_kernel(const float* __restrict__ ds, int b, int out,
                                                              const uint8_t* __restrict__ is_root, const int32_t* __restrict__ cnt,
                                                              const int32_t* __restrict__ ptr, const int32_t* __restrict__ sorted,
                                                              int n_nodes, int lpr, float* __restrict__ de, int64_t ldd) {
  const int lane = threadIdx.x & 63, sub = lane / lpr, l = lane & (lpr - 1), groups = 64 / lpr;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = (gridDim.x * blockDim.x) >> 6;
  for (int j = wave * groups + sub; j < n_nodes; j += waves * groups) {
    const int c = is_root[j] ? 0 : cnt[j], p0 = ptr[j];
    for (int k0 = 4 * l; k0 < out; k0 += 4 * lpr) {
      float4_t acc = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < c; ++k) acc += pair_load4<VEC>(ds, b, out, out, sorted[p0 + k], k0);
      fr_store4<VEC>(de + (int64_t)j * ldd, out, k0, acc);
    }
  }
}

int32_t fr_check(gigl_ctx* ctx, int32_t b, int32_t out, int32_t in, int32_t n_nodes, float alpha, bool dec) {
  GIGL_REQUIRE(ctx, !dec || (out >= 1 && out <= FR_MAX_OUT), "the reconstruction kernels serve 1 <= out <= %d (out=%d)", FR_MAX_OUT, out);
  GIGL_REQUIRE(ctx, in >= 1 && in <= FR_MAX_IN, "the reconstruction kernels serve 1 <= in <= %d (in=%d)", FR_MAX_IN, in);
  GIGL_REQUIRE(ctx, b >= 0 && b <= FR_MAX_B, "b=%d outside [0, %d]", b, FR_MAX_B);
  GIGL_REQUIRE(ctx, !dec || n_nodes >= 0, "n_nodes=%d is negative", n_nodes);
  GIGL_REQUIRE(ctx, alpha == alpha, "alpha is NaN");
  return GIGL_OK;
}

// opt in to more than 64 KB of dynamic LDS (a per-device setting of the function: repeated on every call, which is cheap)
template <typename K>
hipError_t fr_lds(K kernel, size_t bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

extern "C" {

int32_t gigl_feature_reconstruction_loss(gigl_ctx* ctx, const float* e, int64_t ld_e, const int32_t* rowptr, const int32_t* col,
                                         int32_t n_nodes, const int32_t* roots, const float* x, int64_t ld_x, const float* w_ed,
                                         const float* w_rel, const float* b_rel, int32_t b, int32_t out, int32_t in, float alpha,
                                         uint8_t* is_root_out, int32_t* root_rows_out, float* s_out, float* t_out, float* p_out,
                                         float* stat_out, float* loss_out) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const bool dec = w_ed != nullptr;
  const int32_t rc0 = fr_check(ctx, b, out, in, n_nodes, alpha, dec);
  if (rc0 != GIGL_OK) return rc0;
  GIGL_REQUIRE(ctx, loss_out && (b == 0 || (e && x && stat_out && ld_x >= in && ld_e >= (dec ? out : in))),
               "null argument or a row stride below the row's width");
  GIGL_REQUIRE(ctx, !dec || b == 0 || (rowptr && col && roots && w_rel && b_rel && is_root_out && root_rows_out && s_out && t_out &&
                                       p_out && n_nodes >= 1),
               "null argument (the decoder needs the graph, the roots, lin_rel and the four outputs)");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int tiles = (b + PT - 1) / PT;
  const int32_t rc = gigl_arena_reset(ctx, (int64_t)tiles * 8 + 1024);
  if (rc != GIGL_OK) return rc;
  double* part = (double*)gigl_arena_alloc(ctx, (int64_t)tiles * 8 + 256);
  GIGL_REQUIRE(ctx, part, "scratch arena exhausted");
  if (b > 0) {
    if (dec) {
      gigl_fill_u32(st, is_root_out, 0u, ((int64_t)n_nodes + 3) / 4);
      hipLaunchKernelGGL(fr_roots_kernel, dim3((unsigned)((b + 255) / 256)), dim3(256), 0, st, roots, rowptr, b, n_nodes, is_root_out,
                         root_rows_out);
    }
    const fr_args a = {e, ld_e, col, is_root_out, roots, x, ld_x, w_ed, w_rel, b_rel, n_nodes, b, out, in, alpha};
    const size_t lds = dec ? (size_t)PT * fr_ld(out) * 4 : 0;
    const bool vec = dec && out % 4 == 0 && ld_e % 4 == 0 && gigl_aligned16(e) && gigl_aligned16(w_ed) && gigl_aligned16(w_rel) &&
                     gigl_aligned16(s_out);
    hipError_t err = hipSuccess;
    dispatch_bool(vec, [&](auto v) {
      auto kernel = fr_forward_kernel<decltype(v)::value>;
      err = fr_lds(kernel, lds);
      if (err == hipSuccess)
        hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(256), lds, st, a, (const int32_t*)root_rows_out,
                           fr_lanes_per_row(dec ? out : 1), s_out, t_out, p_out, stat_out, part);
    });
    GIGL_HIP_CHECK(ctx, err);
  }
  hipLaunchKernelGGL(fr_fold_kernel, dim3(1), dim3(1024), 0, st, (const double*)part, tiles, b, loss_out);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_feature_reconstruction_loss_backward(gigl_ctx* ctx, const float* p, int64_t ld_p, const float* stat, const int32_t* roots,
                                                  const float* x, int64_t ld_x, const float* w_ed, const float* w_rel,
                                                  const uint8_t* is_root, const int32_t* root_rows, const int32_t* col,
                                                  int32_t n_nodes, int64_t edges_cap, int32_t b, int32_t out, int32_t in, float alpha,
                                                  const float* gout_dev, float* g_out, int64_t ld_g, float* dt_out, float* ds_out,
                                                  float* de, int64_t ld_de) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const bool dec = w_ed != nullptr;
  const int32_t rc0 = fr_check(ctx, b, out, in, n_nodes, alpha, dec);
  if (rc0 != GIGL_OK) return rc0;
  GIGL_REQUIRE(ctx, b == 0 || (p && stat && x && g_out && ld_p >= in && ld_x >= in && ld_g >= in),
               "null argument or a row stride below the row's width");
  GIGL_REQUIRE(ctx, !dec || (de && ld_de >= out && (b == 0 || (roots && w_rel && is_root && root_rows && col && dt_out && ds_out &&
                                                               ld_g == in && edges_cap >= 0 && edges_cap < ((int64_t)1 << 31)))),
               "null argument, a row stride of de below out, g_out not contiguous or edges_cap outside [0, 2^31)");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (b == 0) {
    if (dec && n_nodes > 0) gigl_zero_rows(st, de, ld_de, n_nodes, out);
    GIGL_HIP_CHECK(ctx, hipGetLastError());
    return GIGL_OK;
  }
  float *w_relt = nullptr, *w_edt = nullptr;
  int32_t *counts = nullptr, *lists = nullptr, *sorted = nullptr;
  const int64_t src_cap = std::max(n_nodes, b), words = gigl_transposed_rows_words(src_cap, edges_cap);
  if (dec) {
    const int64_t rel_bytes = gigl_align_up((int64_t)in * out * 4, 256), ed_bytes = gigl_align_up((int64_t)out * out * 4, 256);
    const int64_t list_bytes = gigl_align_up(words * 4, 256), sorted_bytes = gigl_align_up(edges_cap * 4 + 4, 256);
    const int32_t rc = gigl_arena_reset(ctx, rel_bytes + ed_bytes + list_bytes + sorted_bytes + 256 + 2048);
    if (rc != GIGL_OK) return rc;
    w_relt = (float*)gigl_arena_alloc(ctx, rel_bytes);
    w_edt = (float*)gigl_arena_alloc(ctx, ed_bytes);
    counts = (int32_t*)gigl_arena_alloc(ctx, 256);
    lists = (int32_t*)gigl_arena_alloc(ctx, list_bytes);
    sorted = (int32_t*)gigl_arena_alloc(ctx, sorted_bytes);
    GIGL_REQUIRE(ctx, w_relt && w_edt && counts && lists && sorted, "scratch arena exhausted");
    gigl_transpose_f32(st, w_rel, in, out, w_relt);
    gigl_transpose_f32(st, w_ed, out, out, w_edt);
  }
  const fr_args a = {p, ld_p, col, is_root, roots, x, ld_x, w_edt, w_relt, nullptr, n_nodes, b, out, in, alpha};
  const size_t lds = dec ? (size_t)PT * fr_ld(out) * 4 : 0;
  const bool vin = dec && in % 4 == 0 && gigl_aligned16(g_out), vout = dec && out % 4 == 0;
  hipError_t err = hipSuccess;
  dispatch_bool(vin, [&](auto v1) {
    dispatch_bool(vout, [&](auto v2) {
      auto kernel = fr_backward_kernel<decltype(v1)::value, decltype(v2)::value>;
      err = fr_lds(kernel, lds);
      if (err == hipSuccess)
        hipLaunchKernelGGL(kernel, dim3((unsigned)((b + PT - 1) / PT)), dim3(256), lds, st, a, stat, gout_dev, g_out, ld_g, dt_out, ds_out);
    });
  });
  GIGL_HIP_CHECK(ctx, err);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  if (!dec || n_nodes == 0) return GIGL_OK;
  // who reads node j?  counts: the number of root positions and of nodes, as the build takes them
  gigl_fill_u32(st, counts, (uint32_t)b, 1);
  gigl_fill_u32(st, counts + 1, (uint32_t)n_nodes, 1);
  const int32_t rc = gigl_transposed_rows_build(ctx, root_rows, root_rows + b, col, counts, b, counts + 1, src_cap, edges_cap, lists);
  if (rc != GIGL_OK) return rc;
  const int32_t* cnt = lists;  // (gigl_transposed_rows_build's layout)
  const int32_t* ptr = lists + 2 * src_cap + 16;
  const int32_t* list = ptr + src_cap;
  const unsigned sort_wgs = (unsigned)std::min<int64_t>(2048, ((int64_t)n_nodes + 3) / 4);
  hipLaunchKernelGGL(fr_sort_lists_kernel, dim3(sort_wgs), dim3(256), 0, st, is_root, cnt, ptr, list, n_nodes, sorted);
  const int lpr = fr_lanes_per_row(out);
  const unsigned wgs = (unsigned)std::min<int64_t>(4096, ((int64_t)n_nodes * lpr / 64 + 3) / 4 + 1);
  dispatch_bool(out % 4 == 0 && ld_de % 4 == 0 && gigl_aligned16(de) && gigl_aligned16(ds_out), [&](auto v) {
    hipLaunchKernelGGL(fr_scatter_rows_kernel<decltype(v)::value>, dim3(wgs), dim3(256), 0, st, (const float*)ds_out, b, out, is_root,
                       cnt, ptr, (const int32_t*)sorted, n_nodes, lpr, de, ld_de);
  });
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

}  // extern "C"
