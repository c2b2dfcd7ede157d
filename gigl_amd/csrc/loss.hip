// loss.hip — retrieval loss of the link-prediction head, fused: temperature -> sampling-probability correction ->
// duplicate / accidental-hit masking -> log-softmax -> cross-entropy against the diagonal, one pass over the scores.
//
// Replaces RetrievalLoss.calculate_batch_retrieval_loss and its two mask builders
// (python/gigl/src/common/models/layers/loss.py:209-277, :279-305, :307-331), which materialise four [Q, C]
// tensors (labels, duplicates, two masks) around CrossEntropyLoss(reduction="sum").  Here row i of the score matrix is
// read once by one 256-thread workgroup:
//     s_ij  = scores_ij / temperature - log(max(p_j, 1e-10))
//     column j != i is EXCLUDED when it is another row of the same query (j < Q and query_ids[j] == query_ids[i]) or,
//     with accidental-hit removal, holds the positive's candidate (candidate_ids[j] == candidate_ids[i]) — the
//     reference adds finfo.min to such a logit, which makes its softmax term exactly 0 in fp32
//     loss_i = logsumexp_j s_ij - s_ii
// Row results go to row_lse / row_loss; a second single-workgroup launch adds the rows in a fixed order (the sum is
// reproducible run to run).  Backward: dscores_ij = g * (softmax_ij - [i == j]) / temperature, 0 for excluded columns.
// HBM-bound: 4*Q*C bytes read forward, read + written backward.
// The training plan's head runs the same kernels over its validity words (LossArgs::valid) through the LpTaskHead interface.
// Further down: the Margin and Softmax tasks over the training plan's score matrix (gigl_lp_task_loss), the count-min sketch of
// the sampling correction, the evaluation's rank metrics, the node-classification score pass (gigl_nc_eval_metrics).
#include "common.h"
#include "dispatch.h"

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace {

struct LossArgs {
  const float* scores;
  int64_t ld;
  int32_t q, c;
  float temperature;  // <= 0: none
  const float* cand_prob;
  const int64_t* query_ids;
  const int64_t* cand_ids;
  const int32_t* valid;  // [c] or NULL (every row and column takes part): the plan's head — column j, and row i < q, take part
  int64_t g_scores;  // grid.y = independent batches: batch g's score block starts g_scores floats on, its ids / prob
                     // / per-row outputs follow the previous batch's (q or c entries each; the batched entry has no valid)
};

__device__ __forceinline__ float logit(const LossArgs& a, float raw, int j) {
  float s = a.temperature > 0.f ? raw / a.temperature : raw;
  if (a.cand_prob) s -= logf(fmaxf(a.cand_prob[j], 1e-10f));
  return s;
}

__device__ __forceinline__ bool excluded(const LossArgs& a, int i, int j, int64_t qid_i, int64_t cid_i) {
  if (a.valid && !a.valid[j]) return true;
  if (j == i) return false;
  if (a.query_ids && j < a.q && a.query_ids[j] == qid_i) return true;  // another positive of the same query (loss.py:279-305)
  return a.cand_ids && a.cand_ids[j] == cid_i;  // the positive itself among the other candidates (:307-331)
}

// merge two (max, sum of exp relative to max) states
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  if (mm == -INFINITY) return;
  s = s * expf(m - mm) + s2 * expf(m2 - mm);
  m = mm;
}

__global__ __launch_bounds__(256) void retrieval_rows_kernel(LossArgs a0, float* __restrict__ masked_out,
                                                             float* __restrict__ row_lse,
                                                             float* __restrict__ row_loss) {
  __shared__ float s_m[4], s_s[4];
  LossArgs a = a0;
  if (const int64_t g = blockIdx.y) {
    a.scores += g * a.g_scores;
    if (a.cand_prob) a.cand_prob += g * a.c;
    if (a.query_ids) a.query_ids += g * a.q;
    if (a.cand_ids) a.cand_ids += g * a.c;
    if (masked_out) masked_out += g * a.q * a.c;
    row_lse += g * a.q;
    row_loss += g * a.q;
  }
  const int i = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (a.valid && !a.valid[i]) {
    if (tid == 0) row_lse[i] = row_loss[i] = 0.f;
    return;
  }
  const float* row = a.scores + (int64_t)i * a.ld;
  const int64_t qid_i = a.query_ids ? a.query_ids[i] : 0;
  const int64_t cid_i = a.cand_ids ? a.cand_ids[i] : 0;
  float m = -INFINITY, s = 0.f;
  for (int j = tid; j < a.c; j += 256) {
    const float v = logit(a, row[j], j);
    const bool ex = excluded(a, i, j, qid_i, cid_i);
    if (masked_out) masked_out[(int64_t)i * a.c + j] = ex ? v + (-FLT_MAX) : v;  // the reference's masked logits
    if (ex) continue;
    if (v > m) {
      s = s * expf(m - v) + 1.f;
      m = v;
    } else {
      s += expf(v - m);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float m2 = __shfl_xor(m, off, 64), s2 = __shfl_xor(s, off, 64);
    lse_merge(m, s, m2, s2);
  }
  if (lane == 0) {
    s_m[w] = m;
    s_s[w] = s;
  }
  __syncthreads();
  if (tid == 0) {
    float mm = s_m[0], ss = s_s[0];
    for (int k = 1; k < 4; ++k) lse_merge(mm, ss, s_m[k], s_s[k]);
    const float lse = mm + logf(ss);
    row_lse[i] = lse;
    row_loss[i] = lse - logit(a, row[i], i);
  }
}

// fixed-order sum of n floats into *out (one workgroup; accumulates in double)
__global__ __launch_bounds__(1024) void sum_rows_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
  __shared__ double s_w[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  v += (int64_t)blockIdx.x * n;  // (one workgroup per batch)
  out += blockIdx.x;
  double acc = 0.0;
  for (int i = tid; i < n; i += 1024) acc += (double)v[i];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) s_w[w] = acc;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t += s_w[k];
    *out = (float)t;
  }
}

// The scale of the stand-alone entries is g / temperature (g = *grad_loss or 1).  The plan (out3 != NULL: its loss words, out3[1]
// the valid rows) takes the mean's gradient times the task's weight, 1 / temperature / rows x weight — two roundings that
// differ, both kept.
__global__ __launch_bounds__(256) void retrieval_backward_kernel(LossArgs a, const float* __restrict__ row_lse,
                                                                 const float* __restrict__ grad_loss,
                                                                 const float* __restrict__ out3, float weight,
                                                                 float* __restrict__ dscores, int64_t ldd) {
  const int i = blockIdx.x;
  float* out = dscores + (int64_t)i * ldd;
  if (a.valid && !a.valid[i]) {
    for (int j = threadIdx.x; j < a.c; j += 256) out[j] = 0.f;
    return;
  }
  const float* row = a.scores + (int64_t)i * a.ld;
  const int64_t qid_i = a.query_ids ? a.query_ids[i] : 0;
  const int64_t cid_i = a.cand_ids ? a.cand_ids[i] : 0;
  const float lse = row_lse[i];
  float scale;
  if (out3) {
    scale = (a.temperature > 0.f ? 1.f / a.temperature : 1.f) / (out3[1] > 0.f ? out3[1] : 1.f) * weight;
  } else {
    const float g = grad_loss ? *grad_loss : 1.f;
    scale = a.temperature > 0.f ? g / a.temperature : g;
  }
  for (int j = threadIdx.x; j < a.c; j += 256) {
    const float raw = row[j];  // (before the mask's dependent loads: one round trip less per column)
    float d = 0.f;
    if (!excluded(a, i, j, qid_i, cid_i)) d = (expf(logit(a, raw, j) - lse) - (j == i ? 1.f : 0.f)) * scale;
    out[j] = d;
  }
}

int32_t make_args(gigl_ctx* ctx, LossArgs& a, const float* scores, int64_t ld, int32_t q, int32_t c, float temperature,
                  const float* cand_prob, const int64_t* query_ids, const int64_t* cand_ids) {
  GIGL_REQUIRE(ctx, scores && q >= 1 && c >= q && ld >= c,
               "Number of queries should be less than or equal to number of candidates in a batch (q=%d, c=%d)", q, c);
  a.scores = scores;
  a.ld = ld;
  a.q = q;
  a.c = c;
  a.temperature = temperature;
  a.cand_prob = cand_prob;
  a.query_ids = query_ids;
  a.cand_ids = cand_ids;
  return GIGL_OK;
}


// ---- count-min sketch of candidate ids (the Retrieval task's candidate-sampling correction,
// python/gigl/src/common/models/layers/count_min_sketch.py:11-95 used by task.py:140-205).  The reference keeps a
// depth x width int32 table on the host and walks ids one at a time through Python's hash((item, i)) % width; here
// the table lives in HBM, one thread per (id, row) adds with an atomic, one thread per id takes the minimum.  The
// hash is CPython's (>= 3.8) tuple hash of two ints restated — lanes hash(int) = x mod (2^61 - 1) with the sign kept,
// xxHash-style accumulation — so a table built here equals the reference's for the same ids, cell for cell.
__device__ __forceinline__ uint64_t py_int_hash(int64_t x) {
  const uint64_t P = (1ull << 61) - 1;
  const uint64_t ax = x < 0 ? (uint64_t)0 - (uint64_t)x : (uint64_t)x;
  int64_t h = (int64_t)(ax % P);
  if (x < 0) h = -h;
  if (h == -1) h = -2;
  return (uint64_t)h;
}
__device__ __forceinline__ int64_t py_tuple2_hash(int64_t x, int64_t i) {
  const uint64_t P1 = 11400714785074694791ull, P2 = 14029467366897019727ull, P5 = 2870177450012600261ull;
  uint64_t acc = P5;
  acc += py_int_hash(x) * P2;
  acc = (acc << 31) | (acc >> 33);
  acc *= P1;
  acc += py_int_hash(i) * P2;
  acc = (acc << 31) | (acc >> 33);
  acc *= P1;
  acc += 2ull ^ (P5 ^ 3527539ull);
  if (acc == ~0ull) return 1546275796;
  return (int64_t)acc;
}
__device__ __forceinline__ int cms_cell(int64_t id, int row, int width) {
  const int64_t h = py_tuple2_hash(id, row);
  int64_t r = h % width;  // Python's %: the result takes the divisor's sign
  if (r < 0) r += width;
  return (int)r;
}
__global__ __launch_bounds__(256) void cms_add_kernel(int32_t* __restrict__ table, int width, int depth,
                                                      const int64_t* __restrict__ ids, int64_t n) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * depth) return;
  const int64_t k = t / depth;
  const int row = (int)(t - k * depth);
  atomicAdd(&table[(int64_t)row * width + cms_cell(ids[k], row, width)], 1);
}
__global__ __launch_bounds__(256) void cms_estimate_kernel(const int32_t* __restrict__ table, int width, int depth,
                                                           const int64_t* __restrict__ ids, int64_t n,
                                                           int64_t* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int64_t id = ids[k];
  int32_t best = 0x7FFFFFFF;
  for (int row = 0; row < depth; ++row) best = min(best, table[(int64_t)row * width + cms_cell(id, row, width)]);
  out[k] = best;
}

// ---- rank metrics of a score matrix (the evaluation's hit_rate_at_k / mean_reciprocal_rank,
// python/gigl/src/common/utils/eval_metrics.py:6-73, which the trainer calls once per anchor).  One wave per anchor:
// for each of its p = min(pos_cnt, P) positives the lanes stride over the negatives and count those that score STRICTLY
// higher (a tie counts for the positive); rank = 1 + that count.  part[a] = {mean_j 1 / rank_j, 1, mean_j [rank_j <= k]
// per k}, all zero for an anchor without a positive.
struct RankKs {
  int32_t k[GIGL_LP_EVAL_MAX_KS];
};

__global__ __launch_bounds__(256) void lp_rank_rows_kernel(const float* __restrict__ scores, int64_t ld, int b, int P,
                                                           const int32_t* __restrict__ pos_cnt, int n_neg, int neg_col0,
                                                           const int32_t* __restrict__ neg_valid, RankKs ks, int n_ks,
                                                           double* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int a = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (a >= b) return;
  const int W = 2 + n_ks;
  double* out = part + (int64_t)a * W;
  const int p = min(pos_cnt[a], P);
  if (p <= 0) {
    if (lane < W) out[lane] = 0.0;
    return;
  }
  double mrr = 0.0;
  int hits[GIGL_LP_EVAL_MAX_KS] = {0};
  for (int j = 0; j < p; ++j) {
    const int64_t q = (int64_t)a * P + j;
    const float* row = scores + q * ld;
    const float pos = row[q];
    int cnt = 0;
    for (int c = lane; c < n_neg; c += 64)
      if ((!neg_valid || neg_valid[c]) && row[neg_col0 + c] > pos) ++cnt;
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    const int rank = 1 + cnt;
    mrr += 1.0 / (double)rank;
#pragma unroll
    for (int k = 0; k < GIGL_LP_EVAL_MAX_KS; ++k) hits[k] += (k < n_ks && rank <= ks.k[k]) ? 1 : 0;
  }
  if (lane == 0) {
    out[0] = mrr / (double)p;
    out[1] = 1.0;
#pragma unroll
    for (int k = 0; k < GIGL_LP_EVAL_MAX_KS; ++k)
      if (k < n_ks) out[2 + k] = (double)hits[k] / (double)p;
  }
}

// acc[MRR_SUM | RANK_NODES | HITS0 + k] += the column sums of part [b][2 + n_ks], in a fixed order (one workgroup); skipped
// when either meta word reports an overflowed batch (the plan's evaluation: such a batch adds nothing)
__global__ __launch_bounds__(1024) void lp_rank_sum_kernel(const double* __restrict__ part, int b, int n_ks,
                                                           const int32_t* __restrict__ meta_a,
                                                           const int32_t* __restrict__ meta_b, double* __restrict__ acc) {
  constexpr int WMAX = 2 + GIGL_LP_EVAL_MAX_KS;
  __shared__ double s_w[16][WMAX];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, W = 2 + n_ks;
  double v[WMAX];
#pragma unroll
  for (int c = 0; c < WMAX; ++c) v[c] = 0.0;
  for (int i = tid; i < b; i += 1024) {
#pragma unroll
    for (int c = 0; c < WMAX; ++c)
      if (c < W) v[c] += part[(int64_t)i * W + c];
  }
#pragma unroll
  for (int c = 0; c < WMAX; ++c) {
    for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_xor(v[c], off, 64);
    if (lane == 0) s_w[w][c] = v[c];
  }
  __syncthreads();
  if (tid < W) {
    if (meta_a && (meta_a[GIGL_META_OVERFLOW] != 0 || meta_b[GIGL_META_OVERFLOW] != 0)) return;
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t += s_w[k][tid];
    acc[tid == 0 ? GIGL_LP_EVAL_MRR_SUM : tid == 1 ? GIGL_LP_EVAL_RANK_NODES : GIGL_LP_EVAL_HITS0 + tid - 2] += t;
  }
}

// ---- accuracy and cross-entropy of rows of class logits against labels (the loop body of the node-classification
// trainer's score(), node_classification_modeling_task_spec.py:190-227: argmax, ==, .sum() and a host read per batch).
// A row takes a group of 2^lg adjacent lanes (its four-column chunks rounded up to a power of two, at most a wave): lane s
// of the group reads chunks s, s + 2^lg, ...  The row is read once for (maximum, its first index) — torch.argmax's choice:
// a NaN beats every number, among equals the lowest index wins — and once more, from cache, for the exponentials.
// row_loss[i] = logsumexp(row) - row[label]; row_bits[i] = [prediction == label] | [0 <= label < width] << 1 (a label
// outside the row is evaluated, never correct, and has no loss).  A skipped call (*skip_flag != 0) writes nothing.
constexpr uint32_t NC_ROW_CORRECT = 1u, NC_ROW_HAS_LOSS = 2u;

// (v, i) replaces (bv, bi) when torch.argmax would prefer it
__device__ __forceinline__ void argmax_take(float& bv, int& bi, float v, int i) {
  const bool vn = v != v, bn = bv != bv;
  const bool better = vn ? (!bn || i < bi) : (!bn && (v > bv || (v == bv && i < bi)));
  if (better) {
    bv = v;
    bi = i;
  }
}

template <bool V4>  // V4: width % 4 == 0 and every row starts on a 16-byte boundary -> one 16-byte load per chunk
__global__ __launch_bounds__(256) void nc_eval_rows_kernel(const float* __restrict__ rows, int width, int64_t row_stride,
                                                           const int32_t* __restrict__ row_index,
                                                           const int64_t* __restrict__ labels, int n, int lg,
                                                           const int32_t* __restrict__ skip_flag,
                                                           float* __restrict__ row_loss, uint32_t* __restrict__ row_bits,
                                                           int64_t* __restrict__ pred_out) {
  if (skip_flag && *skip_flag != 0) return;
  const int G = 1 << lg, sub = threadIdx.x & (G - 1);
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> lg;
  if (i >= n) return;  // (the whole group leaves: the shuffles below stay inside a group)
  const float* row = rows + (row_index ? (int64_t)row_index[i] : i) * row_stride;
  const int chunks = (width + 3) >> 2;
  float bv = -INFINITY;
  int bi = 0x7FFFFFFF;  // (a lane without a column loses every tie)
  for (int j = sub; j < chunks; j += G) {
    const int c = j << 2;
    if constexpr (V4) {
      const float4 q = *reinterpret_cast<const float4*>(row + c);
      argmax_take(bv, bi, q.x, c);
      argmax_take(bv, bi, q.y, c + 1);
      argmax_take(bv, bi, q.z, c + 2);
      argmax_take(bv, bi, q.w, c + 3);
    } else {
      for (int k = c; k < min(c + 4, width); ++k) argmax_take(bv, bi, row[k], k);
    }
  }
  for (int off = G >> 1; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    argmax_take(bv, bi, ov, oi);
  }
  float se = 0.f;
  for (int j = sub; j < chunks; j += G) {
    const int c = j << 2;
    if constexpr (V4) {
      const float4 q = *reinterpret_cast<const float4*>(row + c);
      se += (gigl_ce_exp(q.x, bv) + gigl_ce_exp(q.y, bv)) + (gigl_ce_exp(q.z, bv) + gigl_ce_exp(q.w, bv));
    } else {
      for (int k = c; k < min(c + 4, width); ++k) se += gigl_ce_exp(row[k], bv);
    }
  }
  for (int off = G >> 1; off > 0; off >>= 1) se += __shfl_xor(se, off, 64);
  if (sub != 0) return;
  const int64_t lab = labels[i];
  const bool has_loss = lab >= 0 && lab < width;
  row_loss[i] = has_loss ? gigl_ce_lse(bv - row[lab], se) : 0.f;
  row_bits[i] = ((int64_t)bi == lab ? NC_ROW_CORRECT : 0u) | (has_loss ? NC_ROW_HAS_LOSS : 0u);
  if (pred_out) pred_out[i] = bi;
}

// acc[GIGL_NC_EVAL_*] += the n rows' words, added in a fixed order in fp64 (one workgroup); a skipped call adds 1 to
// acc[GIGL_NC_EVAL_SKIPPED] and nothing else
__global__ __launch_bounds__(1024) void nc_eval_sum_kernel(const float* __restrict__ row_loss,
                                                           const uint32_t* __restrict__ row_bits, int n,
                                                           const int32_t* __restrict__ skip_flag, double* __restrict__ acc) {
  __shared__ double s_w[16][3];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (skip_flag && *skip_flag != 0) {
    if (tid == 0) acc[GIGL_NC_EVAL_SKIPPED] += 1.0;
    return;
  }
  double v[3] = {0.0, 0.0, 0.0};  // correct, rows with a loss, their loss
  for (int i = tid; i < n; i += 1024) {
    const uint32_t bits = row_bits[i];
    v[0] += (bits & NC_ROW_CORRECT) ? 1.0 : 0.0;
    if (bits & NC_ROW_HAS_LOSS) {
      v[1] += 1.0;
      v[2] += (double)row_loss[i];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_xor(v[c], off, 64);
    if (lane == 0) s_w[w][c] = v[c];
  }
  __syncthreads();
  if (tid != 0) return;
  double t[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < 16; ++k)
    for (int c = 0; c < 3; ++c) t[c] += s_w[k][c];
  acc[GIGL_NC_EVAL_CORRECT] += t[0];
  acc[GIGL_NC_EVAL_EVALUATED] += (double)n;
  acc[GIGL_NC_EVAL_LOSS_SUM] += t[2];
  acc[GIGL_NC_EVAL_LOSS_ROWS] += t[1];
  acc[GIGL_NC_EVAL_CALLS] += 1.0;
}


// ---- the Margin and Softmax tasks over the plan's score matrix (task.py:62-105, MarginLoss / SoftmaxLoss loss.py:21-174;
// the contract is in include/gigl_hip.h at gigl_lp_task_loss).  Row q = i P + j is anchor i's positive j, its score the
// diagonal entry; its negatives are the valid columns among its OWN anchor's H hard negatives and the valid random
// negatives — 1 + H + n_rn entries of a C-wide row are read.  Three launches, as the retrieval loss': rows (one workgroup
// per query row -> two partial words per row), sum (one workgroup, fp64, fixed order), backward (the whole dscores row).
template <int KIND>
struct TaskAcc;
template <>
struct TaskAcc<GIGL_LP_TASK_MARGIN> {  // x: hinge sum, y: active pairs (a pair at exactly 0 is active: clamp_min's gradient)
  float x = 0.f, y = 0.f;
  __device__ __forceinline__ void take(float s, float pos, float margin) {
    const float h = (margin - pos) + s;
    if (h >= 0.f) {
      x += h;
      y += 1.f;
    }
  }
  __device__ __forceinline__ void merge(float x2, float y2) {
    x += x2;
    y += y2;
  }
};
template <>
struct TaskAcc<GIGL_LP_TASK_SOFTMAX> {
  // x: running maximum m, y: sum of exp(v - m) over the terms seen WITHOUT the maximum's own 1 — lse = m + log1p(y): a row whose
  // positive dominates has y ~ 1e-7 and a loss of that size, which 1 + y would round away
  float x = -INFINITY, y = 0.f;
  __device__ __forceinline__ void take(float s, float, float temperature) { merge(s / temperature, 0.f); }
  __device__ __forceinline__ void merge(float x2, float y2) {
    if (x2 > x) {
      y = y2 + (y + 1.f) * expf(x - x2);  // (x == -inf: exp gives 0, nothing was seen)
      x = x2;
    } else if (x2 != -INFINITY) {
      y += (y2 + 1.f) * expf(x2 - x);
    }
  }
};

__device__ __forceinline__ bool task_row_valid(const LpTaskHead& a, int q, int i) {
  return a.valid[q] != 0 && (!a.pos_cnt || q - i * a.P < a.pos_cnt[i]);
}
__device__ __forceinline__ bool task_hard_valid(const LpTaskHead& a, int i, int k) {
  return a.valid[a.b * a.P + i * a.H + k] != 0 && (!a.pos_cnt || k < a.pos_cnt[a.b + i]);
}

template <int KIND>
__global__ __launch_bounds__(256) void lp_task_rows_kernel(LpTaskHead a, float* __restrict__ row_a, float* __restrict__ row_b) {
  __shared__ float s_x[4], s_y[4];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = q / a.P, Q = a.b * a.P, R0 = Q + a.b * a.H;
  if (!task_row_valid(a, q, i)) {
    if (tid == 0) {
      row_a[q] = 0.f;
      row_b[q] = 0.f;
    }
    return;
  }
  const float* row = a.scores + (int64_t)q * a.ld;
  const float pos = row[q];
  TaskAcc<KIND> acc;
  if (KIND == GIGL_LP_TASK_SOFTMAX && tid == 0) acc.x = pos / a.param;  // the positive's own term
  for (int k = tid; k < a.H; k += 256)
    if (task_hard_valid(a, i, k)) acc.take(row[Q + i * a.H + k], pos, a.param);
  // the random negatives' span: scalar up to a 16-byte boundary, then four columns per load, then the tail
  const float* rn = row + R0;
  const int32_t* vr = a.valid + R0;
  int head = (int)((4u - (unsigned)(((uintptr_t)rn >> 2) & 3u)) & 3u);
  if (head > a.n_rn) head = a.n_rn;
  if (tid < head && vr[tid]) acc.take(rn[tid], pos, a.param);
  const int nvec = (a.n_rn - head) >> 2;
  for (int v = tid; v < nvec; v += 256) {
    const int c = head + 4 * v;
    const float4 x = *reinterpret_cast<const float4*>(rn + c);
    if (vr[c]) acc.take(x.x, pos, a.param);
    if (vr[c + 1]) acc.take(x.y, pos, a.param);
    if (vr[c + 2]) acc.take(x.z, pos, a.param);
    if (vr[c + 3]) acc.take(x.w, pos, a.param);
  }
  {
    const int c = head + 4 * nvec + tid;
    if (c < a.n_rn && vr[c]) acc.take(rn[c], pos, a.param);
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float x2 = __shfl_xor(acc.x, off, 64), y2 = __shfl_xor(acc.y, off, 64);
    acc.merge(x2, y2);
  }
  if (lane == 0) {
    s_x[w] = acc.x;
    s_y[w] = acc.y;
  }
  __syncthreads();
  if (tid == 0) {
    TaskAcc<KIND> t;
    t.x = s_x[0];
    t.y = s_y[0];
    for (int k = 1; k < 4; ++k) t.merge(s_x[k], s_y[k]);
    if (KIND == GIGL_LP_TASK_MARGIN) {
      row_a[q] = t.x;
      row_b[q] = t.y;
    } else {  // lse as two words, m and log(sum exp(v - m)): their sum would round the small one away
      row_a[q] = t.x;
      row_b[q] = log1pf(t.y);
    }
  }
}

// {weighted loss, valid rows, normaliser} in a fixed order, fp64 and integers (one workgroup).  Margin: sum of the hinge sums /
// N, N = the valid rows' negative counts (64-bit); Softmax and Retrieval: sum of the row losses / valid rows (Retrieval writes no
// normaliser word).  Training (eval_acc == NULL): -> out3, a failed batch (either meta word) gives a NaN loss, *step (may be
// NULL) moves when it did not fail.  Evaluation: acc[LOSS_SUM] += the fp32 loss word, acc[BATCHES] += 1, or *overflow_acc += 1.
template <int KIND>
__global__ __launch_bounds__(1024) void lp_task_sum_kernel(LpTaskHead a, const float* __restrict__ row_a,
                                                           const float* __restrict__ row_b, float* __restrict__ out3,
                                                           int32_t* __restrict__ step, const int32_t* __restrict__ meta_a,
                                                           const int32_t* __restrict__ meta_b, double* __restrict__ eval_acc,
                                                           int32_t* __restrict__ overflow_acc) {
  __shared__ double s_w[16];
  __shared__ long long s_p[16];
  __shared__ int s_n[16];
  __shared__ int s_rn;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int Q = a.b * a.P, R0 = Q + a.b * a.H;
  int n_rn_valid = 0;
  if (KIND == GIGL_LP_TASK_MARGIN) {  // the valid random negatives: every valid row has them all
    int c = 0;
    for (int r = tid; r < a.n_rn; r += 1024) c += a.valid[R0 + r] ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if (lane == 0) s_n[w] = c;
    __syncthreads();
    if (tid == 0) {
      int t = 0;
      for (int k = 0; k < 16; ++k) t += s_n[k];
      s_rn = t;
    }
    __syncthreads();
    n_rn_valid = s_rn;
    __syncthreads();
  }
  double acc = 0.0;
  long long pairs = 0;
  int n = 0;
  for (int q = tid; q < Q; q += 1024) {
    if (KIND == GIGL_LP_TASK_RETRIEVAL) {  // row_b = row_loss, 0 on an invalid row
      acc += (double)row_b[q];
      n += a.valid[q] ? 1 : 0;
      continue;
    }
    const int i = q / a.P;
    if (!task_row_valid(a, q, i)) continue;
    ++n;
    if (KIND == GIGL_LP_TASK_MARGIN) {
      acc += (double)row_a[q];
      int nh = 0;
      for (int k = 0; k < a.H; ++k) nh += task_hard_valid(a, i, k) ? 1 : 0;
      pairs += nh + n_rn_valid;
    } else {  // lse - pos / T, the two large words subtracted first: exactly 0 for a row without negatives
      const float vp = a.scores[(int64_t)q * a.ld + q] / a.param;
      acc += (double)row_b[q] + ((double)row_a[q] - (double)vp);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    acc += __shfl_xor(acc, off, 64);
    pairs += __shfl_xor(pairs, off, 64);
    n += __shfl_xor(n, off, 64);
  }
  if (lane == 0) {
    s_w[w] = acc;
    s_p[w] = pairs;
    s_n[w] = n;
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    long long pp = 0;
    int nn = 0;
    for (int k = 0; k < 16; ++k) {
      t += s_w[k];
      pp += s_p[k];
      nn += s_n[k];
    }
    const double norm = KIND == GIGL_LP_TASK_MARGIN ? (double)pp : (double)nn;
    // (Retrieval keeps its own rounding: the mean as a float, then the weight — x 1.0f gives the same bits)
    const float loss = KIND == GIGL_LP_TASK_RETRIEVAL ? (float)(t / (double)(nn > 0 ? nn : 1)) * a.weight
                                                      : (float)((double)a.weight * t / (norm > 0.0 ? norm : 1.0));
    const bool failed = meta_a && (meta_a[GIGL_META_OVERFLOW] != 0 || meta_b[GIGL_META_OVERFLOW] != 0);
    if (eval_acc) {
      if (failed) {
        *overflow_acc += 1;
      } else {
        eval_acc[GIGL_LP_EVAL_LOSS_SUM] += (double)loss;
        eval_acc[GIGL_LP_EVAL_BATCHES] += 1.0;
      }
      return;
    }
    out3[0] = failed ? __builtin_nanf("") : loss;
    out3[1] = (float)nn;
    if (KIND != GIGL_LP_TASK_RETRIEVAL) out3[2] = (float)norm;
    if (step && !failed) *step += 1;
  }
}

// the whole dscores row (rows ldd floats apart) in one element-wise pass: the diagonal, the row's own hard negatives, the
// random negatives; exactly 0 on every other column and on an invalid row.  The weight enters through one scale word, so a
// weight halved halves every bit pattern exactly.
template <int KIND>
__global__ __launch_bounds__(256) void lp_task_backward_kernel(LpTaskHead a, const float* __restrict__ row_a,
                                                               const float* __restrict__ row_b, const float* __restrict__ out3,
                                                               float* __restrict__ dscores, int64_t ldd) {
  const int q = blockIdx.x, i = q / a.P, Q = a.b * a.P, R0 = Q + a.b * a.H, Cn = R0 + a.n_rn;
  float* out = dscores + (int64_t)q * ldd;
  if (!task_row_valid(a, q, i)) {
    for (int j = threadIdx.x; j < Cn; j += 256) out[j] = 0.f;
    return;
  }
  const float* row = a.scores + (int64_t)q * a.ld;
  const float pos = row[q];
  const float norm = out3[2] > 0.f ? out3[2] : 1.f;
  const float scale = KIND == GIGL_LP_TASK_MARGIN ? a.weight / norm : a.weight / (a.param * norm);
  const float ra = row_a[q], rb = row_b[q];
  const int h0 = Q + i * a.H;
  for (int j = threadIdx.x; j < Cn; j += 256) {
    float d = 0.f;
    if (j == q) {
      d = KIND == GIGL_LP_TASK_MARGIN ? 0.f - rb * scale : expm1f((pos / a.param - ra) - rb) * scale;
    } else if (j >= R0 ? a.valid[j] != 0 : (j >= h0 && j < h0 + a.H && task_hard_valid(a, i, j - h0))) {
      const float s = row[j];
      if (KIND == GIGL_LP_TASK_MARGIN) d = (a.param - pos) + s >= 0.f ? scale : 0.f;
      else d = expf((s / a.param - ra) - rb) * scale;
    }
    out[j] = d;
  }
}

}  // namespace

int32_t gigl_lp_task_check(gigl_ctx* ctx, int32_t kind, float param, float weight) {
  GIGL_REQUIRE(ctx, kind == GIGL_LP_TASK_RETRIEVAL || kind == GIGL_LP_TASK_MARGIN || kind == GIGL_LP_TASK_SOFTMAX,
               "task kind %d is none of GIGL_LP_TASK_RETRIEVAL / _MARGIN / _SOFTMAX", kind);
  GIGL_REQUIRE(ctx, kind != GIGL_LP_TASK_SOFTMAX || (std::isfinite(param) && param > 0.f), "Softmax: the temperature must be finite and > 0");
  GIGL_REQUIRE(ctx, kind != GIGL_LP_TASK_MARGIN || std::isfinite(param), "Margin: the margin must be finite");
  GIGL_REQUIRE(ctx, std::isfinite(weight) && weight > 0.f, "the task's weight must be finite and > 0");
  return GIGL_OK;
}

namespace {
// the retrieval loss over a head's layout: q = b P query rows, every candidate column, the temperature in param
LossArgs retrieval_args(const LpTaskHead& h) {
  LossArgs a{};
  a.scores = h.scores;
  a.ld = h.ld;
  a.q = h.b * h.P;
  a.c = h.b * (h.P + h.H) + h.n_rn;
  a.temperature = h.param;
  a.query_ids = h.qid;
  a.cand_ids = h.cid;
  a.valid = h.valid;
  return a;
}

template <typename F>
void dispatch_task(int32_t kind, F&& f) {
  dispatch_int<GIGL_LP_TASK_RETRIEVAL, GIGL_LP_TASK_MARGIN, GIGL_LP_TASK_SOFTMAX>(kind, f);
}
}  // namespace

void gigl_lp_task_rows_enqueue(hipStream_t st, const LpTaskHead& h, float* row_a, float* row_b) {
  const dim3 grid((unsigned)(h.b * h.P));
  dispatch_task(h.kind, [&](auto k) {
    constexpr int KIND = decltype(k)::value;
    if constexpr (KIND == GIGL_LP_TASK_RETRIEVAL)
      hipLaunchKernelGGL(retrieval_rows_kernel, grid, dim3(256), 0, st, retrieval_args(h), (float*)nullptr, row_a, row_b);
    else
      hipLaunchKernelGGL(lp_task_rows_kernel<KIND>, grid, dim3(256), 0, st, h, row_a, row_b);
  });
}

void gigl_lp_task_sum_enqueue(hipStream_t st, const LpTaskHead& h, const float* row_a, const float* row_b, float* out3,
                              int32_t* step, const int32_t* meta_a, const int32_t* meta_b, double* eval_acc,
                              int32_t* overflow_acc) {
  dispatch_task(h.kind, [&](auto k) {
    hipLaunchKernelGGL(lp_task_sum_kernel<decltype(k)::value>, dim3(1), dim3(1024), 0, st, h, row_a, row_b, out3, step, meta_a,
                       meta_b, eval_acc, overflow_acc);
  });
}

void gigl_lp_task_backward_enqueue(hipStream_t st, const LpTaskHead& h, const float* row_a, const float* row_b,
                                   const float* out3, float* dscores, int64_t ldd) {
  const dim3 grid((unsigned)(h.b * h.P));
  dispatch_task(h.kind, [&](auto k) {
    constexpr int KIND = decltype(k)::value;
    if constexpr (KIND == GIGL_LP_TASK_RETRIEVAL)
      hipLaunchKernelGGL(retrieval_backward_kernel, grid, dim3(256), 0, st, retrieval_args(h), row_a, (const float*)nullptr,
                         out3, h.weight, dscores, ldd);
    else
      hipLaunchKernelGGL(lp_task_backward_kernel<KIND>, grid, dim3(256), 0, st, h, row_a, row_b, out3, dscores, ldd);
  });
}

namespace {
// the stand-alone entries' arguments -> h (Margin and Softmax: the retrieval loss needs the ids, see gigl_retrieval_loss)
int32_t lp_task_head(gigl_ctx* ctx, LpTaskHead& h, int32_t kind, float param, float weight, const float* scores, int64_t ld,
                     int32_t b, int32_t P, int32_t H, int32_t n_rn, const int32_t* pos_cnt, const int32_t* valid) {
  const int32_t rc = gigl_lp_task_check(ctx, kind, param, weight);
  if (rc != GIGL_OK) return rc;
  GIGL_REQUIRE(ctx, kind != GIGL_LP_TASK_RETRIEVAL, "the retrieval loss masks by ids: gigl_retrieval_loss");
  GIGL_REQUIRE(ctx, scores && valid && b >= 1 && P >= 1 && H >= 0 && n_rn >= 0, "bad arguments");
  const int64_t Cn = (int64_t)b * (P + H) + n_rn;
  GIGL_REQUIRE(ctx, Cn <= 0x7FFFFFFFll && ld >= Cn, "the score rows (ld=%lld) do not hold the %lld candidates' columns",
               (long long)ld, (long long)Cn);
  h = LpTaskHead{kind, param, weight, scores, ld, b, P, H, n_rn, pos_cnt, valid};
  return GIGL_OK;
}
}  // namespace

int32_t gigl_lp_rank_metrics_enqueue(gigl_ctx* ctx, hipStream_t st, const float* scores, int64_t ld, int32_t b, int32_t P,
                                     const int32_t* pos_cnt, int32_t n_neg, int32_t neg_col0, const int32_t* neg_valid,
                                     const int32_t* ks, int32_t n_ks, const int32_t* meta_a, const int32_t* meta_b,
                                     double* part, double* acc) {
  GIGL_REQUIRE(ctx, scores && pos_cnt && ks && part && acc && b >= 1 && P >= 1 && n_neg >= 0 && neg_col0 >= 0, "bad arguments");
  GIGL_REQUIRE(ctx, ld >= (int64_t)b * P && (n_neg == 0 || ld >= (int64_t)neg_col0 + n_neg),
               "the score rows (ld=%lld) do not hold the positives' and negatives' columns", (long long)ld);
  GIGL_REQUIRE(ctx, n_ks >= 1 && n_ks <= GIGL_LP_EVAL_MAX_KS, "n_ks=%d outside [1, %d]", n_ks, GIGL_LP_EVAL_MAX_KS);
  RankKs k{};
  for (int i = 0; i < n_ks; ++i) {
    GIGL_REQUIRE(ctx, ks[i] >= 1, "ks must be greater-or-equal to 1 (got %d)", ks[i]);
    k.k[i] = ks[i];
  }
  hipLaunchKernelGGL(lp_rank_rows_kernel, dim3((unsigned)((b + 3) / 4)), dim3(256), 0, st, scores, ld, b, P, pos_cnt, n_neg,
                     neg_col0, neg_valid, k, n_ks, part);
  hipLaunchKernelGGL(lp_rank_sum_kernel, dim3(1), dim3(1024), 0, st, (const double*)part, b, n_ks, meta_a, meta_b, acc);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

extern "C" {

int32_t gigl_lp_rank_metrics(gigl_ctx* ctx, const float* scores, int64_t ld, int32_t b, int32_t P, const int32_t* pos_cnt,
                             int32_t n_neg, int32_t neg_col0, const int32_t* neg_valid, const int32_t* ks, int32_t n_ks,
                             double* acc) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  GIGL_REQUIRE(ctx, b >= 1 && b <= (1 << 24), "b=%d", b);
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int64_t bytes = (int64_t)b * (2 + GIGL_LP_EVAL_MAX_KS) * (int64_t)sizeof(double);
  const int32_t rc = gigl_arena_reset(ctx, bytes + 256);
  if (rc != GIGL_OK) return rc;
  double* part = (double*)gigl_arena_alloc(ctx, bytes);
  return gigl_lp_rank_metrics_enqueue(ctx, ctx->stream, scores, ld, b, P, pos_cnt, n_neg, neg_col0, neg_valid, ks, n_ks, nullptr,
                                      nullptr, part, acc);
}

int32_t gigl_nc_eval_metrics(gigl_ctx* ctx, const float* rows, int32_t width, int64_t row_stride, const int32_t* row_index,
                             const int64_t* labels, int32_t n, const int32_t* skip_flag, double* acc, int64_t* pred_out) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  GIGL_REQUIRE(ctx, rows && labels && acc, "null rows, labels or acc");
  GIGL_REQUIRE(ctx, width >= 1 && n >= 0, "width=%d (at least 1), n=%d (not negative)", width, n);
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  float* row_loss = nullptr;
  uint32_t* row_bits = nullptr;
  if (n > 0) {
    const int64_t bytes = gigl_align_up((int64_t)n * 4, 256);
    const int32_t rc = gigl_arena_reset(ctx, 2 * bytes + 256);
    if (rc != GIGL_OK) return rc;
    row_loss = (float*)gigl_arena_alloc(ctx, bytes);
    row_bits = (uint32_t*)gigl_arena_alloc(ctx, bytes);
    int lg = 0;  // lanes per row: the row's four-column chunks rounded up to a power of two, at most a wave
    while (lg < 6 && (1 << lg) < (width + 3) / 4) ++lg;
    const unsigned grid = (unsigned)((((int64_t)n << lg) + 255) / 256);
    const bool v4 = width % 4 == 0 && row_stride % 4 == 0 && ((uintptr_t)rows & 15) == 0;
    if (v4)
      hipLaunchKernelGGL(nc_eval_rows_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, rows, width, row_stride, row_index,
                         labels, n, lg, skip_flag, row_loss, row_bits, pred_out);
    else
      hipLaunchKernelGGL(nc_eval_rows_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, rows, width, row_stride, row_index,
                         labels, n, lg, skip_flag, row_loss, row_bits, pred_out);
  }
  hipLaunchKernelGGL(nc_eval_sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const float*)row_loss,
                     (const uint32_t*)row_bits, n, skip_flag, acc);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}


int32_t gigl_retrieval_loss(gigl_ctx* ctx, const float* scores, int64_t ld, int32_t q, int32_t c, float temperature,
                            const float* cand_prob, const int64_t* query_ids, const int64_t* cand_ids,
                            float* masked_scores, float* row_lse, float* row_loss, float* loss) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  LossArgs a{};
  int32_t rc = make_args(ctx, a, scores, ld, q, c, temperature, cand_prob, query_ids, cand_ids);
  if (rc != GIGL_OK) return rc;
  GIGL_REQUIRE(ctx, row_lse && row_loss && loss, "null output");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(retrieval_rows_kernel, dim3((unsigned)q), dim3(256), 0, ctx->stream, a, masked_scores, row_lse,
                     row_loss);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(1024), 0, ctx->stream, row_loss, q, loss);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_retrieval_loss_batched(gigl_ctx* ctx, const float* scores, int64_t ld, int64_t batch_stride, int32_t q,
                                    int32_t c, int32_t batches, float temperature, const float* cand_prob,
                                    const int64_t* query_ids, const int64_t* cand_ids, float* row_lse, float* row_loss,
                                    float* loss) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  LossArgs a{};
  int32_t rc = make_args(ctx, a, scores, ld, q, c, temperature, cand_prob, query_ids, cand_ids);
  if (rc != GIGL_OK) return rc;
  GIGL_REQUIRE(ctx, row_lse && row_loss && loss && batches >= 1 && batches <= 65535 && batch_stride >= 0,
               "bad arguments (batches=%d)", batches);
  a.g_scores = batch_stride;
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(retrieval_rows_kernel, dim3((unsigned)q, (unsigned)batches), dim3(256), 0, ctx->stream, a,
                     (float*)nullptr, row_lse, row_loss);
  hipLaunchKernelGGL(sum_rows_kernel, dim3((unsigned)batches), dim3(1024), 0, ctx->stream, row_loss, q, loss);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_retrieval_loss_backward(gigl_ctx* ctx, const float* scores, int64_t ld, int32_t q, int32_t c,
                                     float temperature, const float* cand_prob, const int64_t* query_ids,
                                     const int64_t* cand_ids, const float* row_lse, const float* grad_loss,
                                     float* dscores) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  LossArgs a{};
  int32_t rc = make_args(ctx, a, scores, ld, q, c, temperature, cand_prob, query_ids, cand_ids);
  if (rc != GIGL_OK) return rc;
  GIGL_REQUIRE(ctx, row_lse && dscores, "null argument");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(retrieval_backward_kernel, dim3((unsigned)q), dim3(256), 0, ctx->stream, a, row_lse, grad_loss,
                     (const float*)nullptr, 1.f, dscores, (int64_t)c);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_lp_task_loss(gigl_ctx* ctx, int32_t kind, float param, float weight, const float* scores, int64_t ld, int32_t b,
                          int32_t P, int32_t H, int32_t n_rn, const int32_t* pos_cnt, const int32_t* valid, float* row_a,
                          float* row_b, float* out3) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  LpTaskHead h{};
  const int32_t rc = lp_task_head(ctx, h, kind, param, weight, scores, ld, b, P, H, n_rn, pos_cnt, valid);
  if (rc != GIGL_OK) return rc;
  GIGL_REQUIRE(ctx, row_a && row_b && out3, "null output");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  gigl_lp_task_rows_enqueue(ctx->stream, h, row_a, row_b);
  gigl_lp_task_sum_enqueue(ctx->stream, h, row_a, row_b, out3, nullptr, nullptr, nullptr, nullptr, nullptr);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_lp_task_loss_backward(gigl_ctx* ctx, int32_t kind, float param, float weight, const float* scores, int64_t ld,
                                   int32_t b, int32_t P, int32_t H, int32_t n_rn, const int32_t* pos_cnt, const int32_t* valid,
                                   const float* row_a, const float* row_b, const float* out3, float* dscores) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  LpTaskHead h{};
  const int32_t rc = lp_task_head(ctx, h, kind, param, weight, scores, ld, b, P, H, n_rn, pos_cnt, valid);
  if (rc != GIGL_OK) return rc;
  GIGL_REQUIRE(ctx, row_a && row_b && out3 && dscores, "null argument");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  gigl_lp_task_backward_enqueue(ctx->stream, h, row_a, row_b, out3, dscores, (int64_t)b * (P + H) + n_rn);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_cms_add(gigl_ctx* ctx, int32_t* table, int32_t width, int32_t depth, const int64_t* ids, int64_t n) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  GIGL_REQUIRE(ctx, table && width > 0 && depth > 0 && n >= 0 && (ids || n == 0), "bad arguments");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (n == 0) return GIGL_OK;
  hipLaunchKernelGGL(cms_add_kernel, dim3((unsigned)((n * depth + 255) / 256)), dim3(256), 0, ctx->stream, table, width,
                     depth, ids, n);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_cms_estimate(gigl_ctx* ctx, const int32_t* table, int32_t width, int32_t depth, const int64_t* ids,
                          int64_t n, int64_t* counts) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  GIGL_REQUIRE(ctx, table && width > 0 && depth > 0 && n >= 0 && ((ids && counts) || n == 0), "bad arguments");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (n == 0) return GIGL_OK;
  hipLaunchKernelGGL(cms_estimate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, table, width,
                     depth, ids, n, counts);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

}  // extern "C"
