// bootstrap.hip — the bootstrap tasks' predictor head and row-wise cosine loss (BGRL, TBGRL: python/gigl/src/common/models/
// layers/task.py:483-654, loss.py:537-588), forward and the row side of the gradient, and the offline encoder's moving average.
// Per view v: H_v = relu(E_v W1^T + b1), Q_v = H_v W2^T + b2, and with cos(a, b) = a.b / (max(|a|, 1e-8) max(|b|, 1e-8))
//     BGRL   2 - mean_i cos(q1_i, y2_i) - mean_i cos(q2_i, y1_i)
//     TBGRL  lambda (mean cos(q1, yneg) + mean cos(q2, yneg)) - (1 - lambda) (mean cos(q1, y2) + mean cos(q2, y1))
// over a few thousand rows of a hundred-odd floats: launches are the cost, so each direction is ONE kernel over (64-row tile,
// view) and the intermediate of the two chained products never leaves the chip.  No atomics, one owner per element, every sum
// in a fixed order: the same inputs give the same bits.
//   forward   boot_forward_kernel.  Both products are Gram-shaped (rows times rows, the torch Linear layout) and go through
//             gram_tile's general form (gram_tile.h: own row bound and row stride per panel).  H's 64 x 64 blocks are written
//             once to hid_out (the backward's ReLU mask and the weight gradient's operand) and into LDS as fp32 rows hid + 4
//             floats apart (the padding spreads the loader's eight rows over the banks): 64 x 516 x 4 = 129 KB at hid = 512,
//             beside the 24 KB of gram_tile's planes and 2.5 KB of row sums, under gfx950's 160 KB.  (Split planes would be 6
//             bytes an element: 192 KB.)  The second product reads its A panel from there, a 64 x 64 block of Q at a time; a block goes to q_out and
//             its contributions to the five row sums |q|^2, q.y, |y|^2, q.yneg, |yneg|^2 are taken from the accumulators, sixteen
//             rows per lane.  After the last block the 32 lanes of a row meet by butterfly, the two column halves through
//             LDS, and 64 threads write the row stats and the row's cosines, whose tile sums (fp64) go to the arena.
//             boot_fold_kernel (one workgroup) adds the tiles' partials in tile order: the loss.
//   backward  boot_backward_kernel, the same tiles.  A wave rebuilds sixteen rows of dQ from q_out, the targets and the row
//             stats (a row with |q| <= 1e-8: the norm's VALUE clamped, its derivative kept, as autograd through
//             F.cosine_similarity, which clamps in place outside the graph; |q| = 0: no norm term) into LDS (rows >= n as
//             zeros) and dq_out; dH = (dQ W2) . [H > 0] goes to dh_out, and — visible to the workgroup after a barrier —
//             is read back as the A panel of dE = dH W1.  Both products contract over the weights' ROW index, so
//             gigl_transpose_f32_kernel writes W2^T and W1^T once per call into the arena (at most 1 MB each) and the products
//             stay Gram-shaped, rather than staging transposed panels in every workgroup.  dq_out / dh_out and hid_out / the
//             encoder rows then feed gigl_linear_weight_grad (agg.hip) for the weights and biases, 2n stacked rows each.
//   no head   W1 == NULL: q_v = e_v (BGRLLoss / TBGRLLoss on already-projected rows): the same kernels without the products.
//   ema       ema_kernel: dst = mm dst + (1 - mm) src for a device table of tensors, a row of workgroups per tensor.
#include "common.h"
#include "dispatch.h"
#include "gram_tile.h"
#include "wave_reduce.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

constexpr int BMAXD = 512;
constexpr int32_t BOOT_MAX_N = 1 << 18;
constexpr float BEPS = 1e-8f;
constexpr int BSTAT = 5;  // row sums: |q|^2, q.y, |y|^2, q.yneg, |yneg|^2

struct boot_args {
  const float* e[2];  // per view: the online encoder's rows (or, without a head, q)
  int64_t lde[2];
  const float* y[2];  // per view: the target the view's q is compared with (view 1: y2, view 2: y1)
  int64_t ldy[2];
  const float* yneg;  // or NULL
  int64_t ldn;
  const float *w1, *b1, *w2, *b2;  // forward: W1 [hid][out], W2 [out][hid]; backward: W1^T [out][hid], W2^T [hid][out]
  int n, out, hid;
};

__host__ __device__ inline int boot_ld(int k) { return (k + 3) / 4 * 4 + 4; }  // floats between the rows of an LDS tile

__device__ __forceinline__ float boot_cos(float dot, float qq, float yy) {
  return dot / (fmaxf(sqrtf(qq), BEPS) * fmaxf(sqrtf(yy), BEPS));
}

// grid (row tile, view).  hid_out [2][n][hid], q_out [2][n][out], stat_out [2][BSTAT][n], part [2][tiles][2] (the tile's sums of
// cos(q, y) and cos(q, yneg)).  Dynamic LDS: the H tile, 64 rows boot_ld(hid) floats apart (none without a head).
template <bool VEC>
__global__ __launch_bounds__(256) void boot_forward_kernel(const boot_args a, float* __restrict__ hid_out, float* __restrict__ q_out,
                                                           float* __restrict__ stat_out, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float hs[];
  __shared__ __attribute__((aligned(16))) short s[6][PPLANE];
  __shared__ float s_row[2][BSTAT][PT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, g = lane >> 5;
  const int wa = wv >> 1, wb = wv & 1;
  const int view = blockIdx.y, I0 = blockIdx.x * PT, n = a.n, out = a.out, hid = a.hid;
  const float* e = a.e[view];
  const float* y = a.y[view];
  const int64_t lde = a.lde[view], ldy = a.ldy[view];
  const bool head = a.w1 != nullptr;
  const int hld = boot_ld(hid);
  if (head) {
    for (int h0 = 0; h0 < hid; h0 += PT) {
      const float16_t acc = gram_tile<VEC>(e, n, lde, a.w1, hid, out, out, I0, h0, s);
      const int c = h0 + wb * 32 + r;
      if (c < hid) {
        const float b = a.b1[c];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int il = wa * 32 + gram_row(v, g);
          const float h = fmaxf(acc[v] + b, 0.f);
          hs[il * hld + c] = h;
          if (I0 + il < n) hid_out[((int64_t)view * n + I0 + il) * hid + c] = h;
        }
      }
    }
    __syncthreads();  // (the second product's first loads precede its own barrier)
  }
  float rs[BSTAT][16];
#pragma unroll
  for (int j = 0; j < BSTAT; ++j)
#pragma unroll
    for (int v = 0; v < 16; ++v) rs[j][v] = 0.f;
  for (int c0 = 0; c0 < out; c0 += PT) {
    float16_t acc = {};
    if (head) acc = gram_tile<VEC>(hs, PT, hld, a.w2, out, hid, hid, 0, c0, s);
    const int c = c0 + wb * 32 + r;
    if (c < out) {
      const float b = head ? a.b2[c] : 0.f;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int i = I0 + wa * 32 + gram_row(v, g);
        if (i < n) {
          const float q = head ? acc[v] + b : e[(int64_t)i * lde + c];
          const float yv = y[(int64_t)i * ldy + c];
          q_out[((int64_t)view * n + i) * out + c] = q;
          rs[0][v] += q * q;
          rs[1][v] += q * yv;
          rs[2][v] += yv * yv;
          if (a.yneg) {
            const float yn = a.yneg[(int64_t)i * a.ldn + c];
            rs[3][v] += q * yn;
            rs[4][v] += yn * yn;
          }
        }
      }
    }
  }
  gram_rows_meet<BSTAT>(rs, s_row);
  if (wv == 0) {  // a row per lane
    const int i = I0 + lane;
    float t[BSTAT];
#pragma unroll
    for (int j = 0; j < BSTAT; ++j) t[j] = s_row[0][j][lane] + s_row[1][j][lane];
    double cy = 0.0, cn = 0.0;
    if (i < n) {
#pragma unroll
      for (int j = 0; j < BSTAT; ++j) stat_out[((int64_t)view * BSTAT + j) * n + i] = t[j];
      cy = (double)boot_cos(t[1], t[0], t[2]);
      if (a.yneg) cn = (double)boot_cos(t[3], t[0], t[4]);
    }
    cy = gigl_wave_sum_f64(cy);
    cn = gigl_wave_sum_f64(cn);
    if (lane == 0) {
      double* p = part + ((int64_t)view * gridDim.x + blockIdx.x) * 2;
      p[0] = cy;
      p[1] = cn;
    }
  }
}

// one workgroup: the four sums over tiles (view x {y, yneg}), each in tile order per thread and then in thread order
__global__ __launch_bounds__(1024) void boot_fold_kernel(const double* __restrict__ part, int tiles, int n, int tbgrl, float neg_lambda,
                                                         float* __restrict__ loss) {
  __shared__ double s_tot[2];
  for (int k = 0; k < 2; ++k) {  // cos(q, y), cos(q, yneg): both views' tiles
    double acc = 0.0;
    for (int t = threadIdx.x; t < 2 * tiles; t += 1024) acc += part[(int64_t)t * 2 + k];
    const double tot = gigl_block1024_sum_f64(acc);
    if (threadIdx.x == 0) s_tot[k] = tot;
    __syncthreads();  // (and the helper's LDS is free for the next sum)
  }
  if (threadIdx.x == 0) {
    const double my = s_tot[0] / (double)n, mn = s_tot[1] / (double)n, lam = (double)neg_lambda;  // (n == 0: NaN)
    *loss = (float)(tbgrl ? lam * mn - (1.0 - lam) * my : 2.0 - my);
  }
}

// grid (row tile, view).  ky, kn: the loss's coefficients of mean cos(q, y) and mean cos(q, yneg).  Dynamic LDS: the dQ tile, 64
// rows boot_ld(out) floats apart (none without a head, where dQ is the result: de1 / de2).
template <bool VEC>
__global__ __launch_bounds__(256) void boot_backward_kernel(const boot_args a, const float* __restrict__ q, const float* __restrict__ stat,
                                                            const float* __restrict__ hid_in, float ky, float kn,
                                                            const float* __restrict__ gout, float* __restrict__ dq_out,
                                                            float* __restrict__ dh_out, float* __restrict__ de1, int64_t ldd1,
                                                            float* __restrict__ de2, int64_t ldd2) {
  extern __shared__ __attribute__((aligned(16))) float ds[];
  __shared__ __attribute__((aligned(16))) short s[6][PPLANE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, g = lane >> 5;
  const int wa = wv >> 1, wb = wv & 1;
  const int view = blockIdx.y, I0 = blockIdx.x * PT, n = a.n, out = a.out, hid = a.hid;
  const float* y = a.y[view];
  const int64_t ldy = a.ldy[view], ldd = view ? ldd2 : ldd1;
  float* de = view ? de2 : de1;
  const bool head = a.w1 != nullptr;
  const int old = boot_ld(out);
  const float gl = (gout ? *gout : 1.f) / (float)n;
  for (int il = wv * 16; il < wv * 16 + 16; ++il) {  // a wave: sixteen rows, the lanes along a row
    const int i = I0 + il;
    float ay = 0.f, an = 0.f, bq = 0.f;  // dq = ay y + an yneg - bq q
    if (i < n) {
      const float* st = stat + (int64_t)view * BSTAT * n + i;
      const float qq = st[0], nq = sqrtf(qq), cq = fmaxf(nq, BEPS);
      const float cy = fmaxf(sqrtf(st[2 * (int64_t)n]), BEPS);
      ay = gl * ky / (cq * cy);
      if (nq > 0.f) bq = gl * ky * boot_cos(st[n], qq, st[2 * (int64_t)n]) / (cq * nq);
      if (a.yneg) {
        const float cn = fmaxf(sqrtf(st[4 * (int64_t)n]), BEPS);
        an = gl * kn / (cq * cn);
        if (nq > 0.f) bq += gl * kn * boot_cos(st[3 * (int64_t)n], qq, st[4 * (int64_t)n]) / (cq * nq);
      }
      // out == 1: a cosine is the sign of q y, constant wherever |q| > 1e-8 — zeros, not the 1e-7 of the first term that the
      // difference of two equal terms would leave (as correlate.hip at n == 2)
      if (out == 1 && nq > BEPS) ay = an = bq = 0.f;
    }
    for (int c = lane; c < out; c += 64) {
      float d = 0.f;
      if (i < n) {
        d = ay * y[(int64_t)i * ldy + c] - bq * q[((int64_t)view * n + i) * out + c];
        if (a.yneg) d += an * a.yneg[(int64_t)i * a.ldn + c];
        if (head)
          dq_out[((int64_t)view * n + i) * out + c] = d;
        else
          de[(int64_t)i * ldd + c] = d;
      }
      if (head) ds[il * old + c] = d;
    }
  }
  if (!head) return;  // (the whole grid)
  __syncthreads();
  const float* hv = hid_in + (int64_t)view * n * hid;
  float* dhv = dh_out + (int64_t)view * n * hid;
  for (int h0 = 0; h0 < hid; h0 += PT) {  // dH = (dQ W2) . [H > 0]: rows of the dQ tile against rows of W2^T [hid][out]
    const float16_t acc = gram_tile<VEC>(ds, PT, old, a.w2, hid, out, out, 0, h0, s);
    const int c = h0 + wb * 32 + r;
    if (c < hid) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int i = I0 + wa * 32 + gram_row(v, g);
        if (i < n) dhv[(int64_t)i * hid + c] = hv[(int64_t)i * hid + c] > 0.f ? acc[v] : 0.f;
      }
    }
  }
  __threadfence_block();
  __syncthreads();  // this workgroup's rows of dH are visible to all its threads
  for (int c0 = 0; c0 < out; c0 += PT) {  // dE = dH W1: rows of dH against rows of W1^T [out][hid]
    const float16_t acc = gram_tile<VEC>(dhv, n, hid, a.w1, out, hid, hid, I0, c0, s);
    const int c = c0 + wb * 32 + r;
    if (c < out) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int i = I0 + wa * 32 + gram_row(v, g);
        if (i < n) de[(int64_t)i * ldd + c] = acc[v];
      }
    }
  }
}

struct ema_entry {
  float* dst;
  const float* src;
  int64_t count;
};

// grid (workgroups per tensor, tensor)
__global__ __launch_bounds__(256) void ema_kernel(const ema_entry* __restrict__ table, float mm, float rest) {
  const ema_entry t = table[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < t.count; i += (int64_t)gridDim.x * 256)
    t.dst[i] = mm * t.dst[i] + rest * t.src[i];
}

int32_t boot_check(gigl_ctx* ctx, int32_t n, int32_t out, int32_t hid, bool head) {
  GIGL_REQUIRE(ctx, out >= 1 && out <= BMAXD, "the bootstrap kernels serve 1 <= out <= %d (out=%d)", BMAXD, out);
  GIGL_REQUIRE(ctx, !head || (hid >= 1 && hid <= BMAXD), "the bootstrap kernels serve 1 <= hid <= %d (hid=%d)", BMAXD, hid);
  GIGL_REQUIRE(ctx, n >= 0 && n <= BOOT_MAX_N, "n=%d outside [0, %d]", n, BOOT_MAX_N);
  return GIGL_OK;
}

bool boot_vec(const boot_args& a, bool head) {
  bool ok = a.out % 4 == 0 && (!head || a.hid % 4 == 0);
  for (const float* p : {a.e[0], a.e[1], a.w1, a.w2}) ok = ok && gigl_aligned16(p);
  return ok && a.lde[0] % 4 == 0 && a.lde[1] % 4 == 0;
}

// opt in to more than 64 KB of dynamic LDS (a per-device setting of the function: repeated on every call, which is cheap)
template <typename K>
hipError_t boot_lds(K kernel, size_t bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

extern "C" {

int32_t gigl_bootstrap_loss(gigl_ctx* ctx, const float* e1, int64_t ld_e1, const float* e2, int64_t ld_e2, const float* y1,
                            int64_t ld_y1, const float* y2, int64_t ld_y2, const float* yneg, int64_t ld_yneg, const float* w1,
                            const float* b1, const float* w2, const float* b2, int32_t n, int32_t out, int32_t hid, float neg_lambda,
                            float* hid_out, float* q_out, float* stat_out, float* loss_out) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const bool head = w1 != nullptr;
  const int32_t rc0 = boot_check(ctx, n, out, hid, head);
  if (rc0 != GIGL_OK) return rc0;
  GIGL_REQUIRE(ctx, loss_out && (n == 0 || (e1 && e2 && y1 && y2 && q_out && stat_out && ld_e1 >= out && ld_e2 >= out && ld_y1 >= out &&
                                            ld_y2 >= out && (!yneg || ld_yneg >= out) && (!head || (b1 && w2 && b2 && hid_out)))),
               "null argument or a row stride < out");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int tiles = (n + PT - 1) / PT;
  const int32_t rc = gigl_arena_reset(ctx, (int64_t)tiles * 32 + 1024);
  if (rc != GIGL_OK) return rc;
  double* part = (double*)gigl_arena_alloc(ctx, (int64_t)tiles * 32 + 256);
  GIGL_REQUIRE(ctx, part, "scratch arena exhausted");
  if (n > 0) {
    const boot_args a = {{e1, e2}, {ld_e1, ld_e2}, {y2, y1}, {ld_y2, ld_y1}, yneg, ld_yneg, w1, b1, w2, b2, n, out, hid};
    const size_t lds = head ? (size_t)PT * boot_ld(hid) * 4 : 0;
    hipError_t err = hipSuccess;
    dispatch_bool(boot_vec(a, head), [&](auto vec) {
      auto kernel = boot_forward_kernel<decltype(vec)::value>;
      err = boot_lds(kernel, lds);
      if (err == hipSuccess) hipLaunchKernelGGL(kernel, dim3((unsigned)tiles, 2), dim3(256), lds, st, a, hid_out, q_out, stat_out, part);
    });
    GIGL_HIP_CHECK(ctx, err);
  }
  hipLaunchKernelGGL(boot_fold_kernel, dim3(1), dim3(1024), 0, st, (const double*)part, tiles, n, yneg ? 1 : 0, neg_lambda, loss_out);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_bootstrap_loss_backward(gigl_ctx* ctx, const float* q, const float* stat, const float* hid_in, const float* y1,
                                     int64_t ld_y1, const float* y2, int64_t ld_y2, const float* yneg, int64_t ld_yneg,
                                     const float* w1, const float* w2, int32_t n, int32_t out, int32_t hid, float neg_lambda,
                                     const float* gout_dev, float* dq_out, float* dh_out, float* de1, int64_t ld_d1, float* de2,
                                     int64_t ld_d2) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  const bool head = w1 != nullptr;
  const int32_t rc0 = boot_check(ctx, n, out, hid, head);
  if (rc0 != GIGL_OK) return rc0;
  GIGL_REQUIRE(ctx, n == 0 || (q && stat && y1 && y2 && de1 && de2 && ld_y1 >= out && ld_y2 >= out && (!yneg || ld_yneg >= out) &&
                               ld_d1 >= out && ld_d2 >= out && (!head || (w2 && hid_in && dq_out && dh_out))),
               "null argument or a row stride < out");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (n == 0) return GIGL_OK;
  float *w1t = nullptr, *w2t = nullptr;
  if (head) {
    const int64_t w_bytes = gigl_align_up((int64_t)out * hid * 4, 256);
    const int32_t rc = gigl_arena_reset(ctx, 2 * w_bytes + 1024);
    if (rc != GIGL_OK) return rc;
    w1t = (float*)gigl_arena_alloc(ctx, w_bytes);
    w2t = (float*)gigl_arena_alloc(ctx, w_bytes);
    GIGL_REQUIRE(ctx, w1t && w2t, "scratch arena exhausted");
    const unsigned tb = (unsigned)std::min<int64_t>(1024, ((int64_t)out * hid + 255) / 256);
    hipLaunchKernelGGL(gigl_transpose_f32_kernel, dim3(tb), dim3(256), 0, st, w1, hid, out, w1t);
    hipLaunchKernelGGL(gigl_transpose_f32_kernel, dim3(tb), dim3(256), 0, st, w2, out, hid, w2t);
  }
  // (e: the backward reads none of the encoder rows; its row panels are the dQ tile and dh_out)
  const boot_args a = {{dh_out, dh_out}, {hid, hid}, {y2, y1}, {ld_y2, ld_y1}, yneg, ld_yneg, w1t, nullptr, w2t, nullptr, n, out, hid};
  const float lam = neg_lambda, ky = yneg ? -(1.f - lam) : -1.f, kn = yneg ? lam : 0.f;
  const size_t lds = head ? (size_t)PT * boot_ld(out) * 4 : 0;
  hipError_t err = hipSuccess;
  dispatch_bool(boot_vec(a, head), [&](auto vec) {
    auto kernel = boot_backward_kernel<decltype(vec)::value>;
    err = boot_lds(kernel, lds);
    if (err == hipSuccess)
      hipLaunchKernelGGL(kernel, dim3((unsigned)((n + PT - 1) / PT), 2), dim3(256), lds, st, a, q, stat, hid_in, ky, kn, gout_dev, dq_out,
                         dh_out, de1, ld_d1, de2, ld_d2);
  });
  GIGL_HIP_CHECK(ctx, err);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_ema_update(gigl_ctx* ctx, const void* table_dev, int32_t n_tensors, int64_t max_count, double mm) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  GIGL_REQUIRE(ctx, n_tensors >= 0 && n_tensors <= 65535 && max_count >= 0 && (n_tensors == 0 || table_dev),
               "n_tensors=%d outside [0, 65535], a negative count or no table", n_tensors);
  GIGL_REQUIRE(ctx, mm >= 0.0 && mm <= 1.0, "momentum=%g outside [0, 1]", mm);
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (n_tensors == 0 || max_count == 0 || mm == 1.0) return GIGL_OK;  // (mm == 1: dst keeps its bits, signed zeros included)
  const unsigned wgs = (unsigned)std::min<int64_t>(256, (max_count + 1023) / 1024);
  hipLaunchKernelGGL(ema_kernel, dim3(wgs, (unsigned)n_tensors), dim3(256), 0, ctx->stream, (const ema_entry*)table_dev, (float)mm,
                     (float)(1.0 - mm));
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

}  // extern "C"
