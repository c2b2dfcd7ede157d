// keyed.hip — the TopK / RandomWeighted sampling ops of the typed DAG sampler: per frontier node, the f neighbours with
// the largest keys drawn from a named edge feature.
//
// Replaces (paths relative to the reference root):
//   SamplingOp.top_k / random_weighted        proto/snapchat/research/gbml/subgraph_sampling_strategy.proto:7-58
//   the Nebula translation of both            scala_spark35/common/src/main/scala/graphdb/nebula/
//                                             NebulaQueryResponseTranslator.scala:39-104
//       TopK:           ORDER BY e.<edgeFeatName> DESC | LIMIT k
//       RandomWeighted: ORDER BY e.<edgeFeatName> * rand() DESC | LIMIT k   (":71-73: not TRUE RandomWeighted sampling")
//
// Results contract (include/gigl_hip.h, gigl_expand_frontier_keyed): key[i] = w[i] (TopK) or fl32(w[i] * u[i])
// (RandomWeighted, u[i] = ((xxh64(i + 1 + K + seed*counter) >> 40) + 1) * 2^-24, the hash of the uniform rule); the f
// largest keys win, NaN lowest, -0 == +0, ties to the lower position; written in position (= ascending id) order.
//
// Kernel shape (gfx950): three launches, no host synchronisation (the typed plan may be captured into a hipGraph).
//   keyed_rows_kernel   one WAVE per frontier slot: empty slots and rows with n <= f are finished here (row copy); rows
//                       with f < n <= 64 are ranked in registers (one 64-bit composite per lane, count-greater over the
//                       wave by readlane) and compacted in position order (ballot + mbcnt); longer rows are appended to
//                       the heavy list.
//   keyed_heavy_kernel  one WORKGROUP per heavy row (persistent grid over the list): radix select of the f-th largest
//                       composite, 8-bit digits from the top, at most 8 passes over the row (the composites sit in LDS up
//                       to KEYED_LDS_CAP edges; longer rows recompute them from global memory on every pass), then one
//                       ordered compaction of every composite >= that threshold.
// The selection is integer work on unique composites (order-preserving key bits << 32 | ~position): the result does
// not depend on the order of work; LDS integer atomics only, no float atomics.
#include "common.h"

namespace {

constexpr int KEYED_TB = 256;
constexpr int KEYED_LIGHT = 64;        // rows up to one wave's width are ranked in registers
constexpr int KEYED_LDS_CAP = 4096;    // composites of a heavy row kept in LDS (32 KiB)
constexpr int KEYED_HEAVY_WGS = 1024;  // persistent grid of the heavy pass (4 workgroups per CU at this LDS size)

struct KeyedArgs {
  const int64_t* rowptr;
  const uint32_t* col;
  const float* key;  // one weight per edge, `col` order
  int64_t n_nodes;
  const uint32_t* nodes;
  const uint32_t* ksums;
  int64_t m;
  int32_t f;
  uint32_t hash_add;
  int32_t method;
  uint32_t* out_nbr;
  int32_t* out_cnt;
  int32_t* heavy;        // [m] slots left to the heavy pass
  int32_t* heavy_count;  // [1]
};

// XXH64 of one little-endian int32 under seed 42 (Spark's xxhash64 expression), the raw unsigned value
__device__ __forceinline__ uint64_t xxh64_i32_raw(uint32_t x) {
  constexpr uint64_t P1 = 0x9E3779B185EBCA87ULL, P2 = 0xC2B2AE3D27D4EB4FULL, P3 = 0x165667B19E3779F9ULL,
                     P5 = 0x27D4EB2F165667C5ULL;
  uint64_t h = (42ULL + P5 + 4ULL) ^ ((uint64_t)x * P1);
  h = ((h << 23) | (h >> 41)) * P2 + P3;
  h ^= h >> 33;
  h *= P2;
  h ^= h >> 29;
  h *= P3;
  h ^= h >> 32;
  return h;
}

// fp32 -> uint32 in IEEE order: NaN -> 0 (below -inf), -0 -> +0
__device__ __forceinline__ uint32_t order_bits(float k) {
  uint32_t u = __float_as_uint(k);
  const uint32_t a = u & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return 0u;
  if (a == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// larger = preferred; unique per row (the low word is the position, inverted: the lower position wins a tie)
__device__ __forceinline__ uint64_t composite(const KeyedArgs& a, int64_t s, uint32_t i, uint32_t base) {
  float k = a.key[s + i];
  if (a.method == GIGL_SAMPLE_RANDOM_WEIGHTED) {
    const uint64_t h = xxh64_i32_raw(base + i + 1u);  // 1-based position, int32 wrap == uint32 wrap
    const float u = (float)((uint32_t)(h >> 40) + 1u) * 0x1p-24f;  // exact: a 25-bit integer times a power of two
    k = __fmul_rn(k, u);
  }
  return ((uint64_t)order_bits(k) << 32) | (uint64_t)(~i);
}

__global__ void keyed_zero_kernel(int32_t* count) { *count = 0; }

__global__ __launch_bounds__(KEYED_TB) void keyed_rows_kernel(KeyedArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * (KEYED_TB / 64) + (threadIdx.x >> 6);
  if (p >= a.m) return;
  const int f = a.f;
  const uint32_t v = a.nodes[p];
  uint32_t* out = a.out_nbr + p * f;
  if (v == GIGL_INVALID || (int64_t)v >= a.n_nodes) {
    for (int j = lane; j < f; j += 64) out[j] = GIGL_INVALID;
    if (lane == 0) a.out_cnt[p] = 0;
    return;
  }
  const int64_t s = a.rowptr[v];
  const int64_t n = a.rowptr[v + 1] - s;
  if (n <= f) {  // every neighbour, no key read
    for (int j = lane; j < f; j += 64) out[j] = j < n ? a.col[s + j] : GIGL_INVALID;
    if (lane == 0) a.out_cnt[p] = (int32_t)n;
    return;
  }
  if (n > KEYED_LIGHT) {
    if (lane == 0) a.heavy[atomicAdd(a.heavy_count, 1)] = (int32_t)p;
    return;
  }
  // f < n <= 64: one composite per lane, rank = how many are larger
  const uint32_t base = a.ksums[p] + a.hash_add;
  const bool have = lane < n;
  const uint64_t c = have ? composite(a, s, (uint32_t)lane, base) : 0ull;  // (0 is below every real composite)
  int rank = 0;
  for (int l = 0; l < (int)n; ++l) {
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(c >> 32), l);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)c, l);  // (int -> uint32: no sign extension)
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    rank += o > c ? 1 : 0;
  }
  const bool take = have && rank < f;
  const unsigned long long bm = __ballot(take);
  const int pos = (int)__popcll(bm & ((1ull << lane) - 1ull));
  if (take) out[pos] = a.col[s + lane];
  if (lane == 0) a.out_cnt[p] = f;
}

__global__ __launch_bounds__(KEYED_TB) void keyed_heavy_kernel(KeyedArgs a) {
  __shared__ uint64_t s_c[KEYED_LDS_CAP];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_wcnt[KEYED_TB / 64];
  __shared__ uint32_t s_digit, s_need, s_stop;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int32_t n_heavy = *a.heavy_count;
  const uint32_t f = (uint32_t)a.f;
  for (int32_t h = blockIdx.x; h < n_heavy; h += gridDim.x) {
    const int64_t p = a.heavy[h];
    const uint32_t v = a.nodes[p];
    const int64_t s = a.rowptr[v];
    const uint32_t n = (uint32_t)(a.rowptr[v + 1] - s);
    const uint32_t base = a.ksums[p] + a.hash_add;
    const bool cached = n <= (uint32_t)KEYED_LDS_CAP;
    if (cached)
      for (uint32_t i = tid; i < n; i += KEYED_TB) s_c[i] = composite(a, s, i, base);
    // radix select from the top digit: `need` = how many of the composites that share `prefix` (under `mask`) still
    // have to be taken
    uint64_t prefix = 0, mask = 0;
    uint32_t need = f;
    for (int shift = 56; shift >= 0; shift -= 8) {
      s_hist[tid] = 0u;
      __syncthreads();
      for (uint32_t i = tid; i < n; i += KEYED_TB) {
        const uint64_t c = cached ? s_c[i] : composite(a, s, i, base);
        if ((c & mask) == prefix) atomicAdd(&s_hist[(uint32_t)(c >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (w == 0) {  // lane l owns digits 4l .. 4l+3; suffix sums from the top digit down
        const uint32_t h0 = s_hist[4 * lane], h1 = s_hist[4 * lane + 1], h2 = s_hist[4 * lane + 2],
                       h3 = s_hist[4 * lane + 3];
        const uint32_t own = h0 + h1 + h2 + h3;
        uint32_t incl = own;
        for (int off = 1; off < 64; off <<= 1) {
          const uint32_t t = __shfl_down(incl, off, 64);
          if (lane + off < 64) incl += t;
        }
        const uint32_t above = incl - own;
        if (above < need && need <= incl) {  // exactly one lane
          const uint32_t hs[4] = {h0, h1, h2, h3};
          uint32_t cum = above;
          int d = 4 * lane;
          uint32_t hd = h0;
          for (int b = 3; b >= 0; --b) {
            if (cum + hs[b] >= need) {
              d = 4 * lane + b;
              hd = hs[b];
              break;
            }
            cum += hs[b];
          }
          s_digit = (uint32_t)d;
          s_need = need - cum;
          s_stop = hd == need - cum ? 1u : 0u;  // every composite under the new prefix is taken
        }
      }
      __syncthreads();
      prefix |= (uint64_t)s_digit << shift;
      mask |= 0xFFull << shift;
      need = s_need;
      if (s_stop) break;  // (block-uniform)
    }
    // exactly f composites are >= prefix (lower bits zero): write them in position order
    uint32_t* out = a.out_nbr + p * (int64_t)f;
    uint32_t run = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += KEYED_TB) {
      const uint32_t i = i0 + (uint32_t)tid;
      bool take = false;
      if (i < n) take = (cached ? s_c[i] : composite(a, s, i, base)) >= prefix;
      const unsigned long long bm = __ballot(take);
      if (lane == 0) s_wcnt[w] = (uint32_t)__popcll(bm);
      __syncthreads();
      uint32_t pos = run + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
      for (int k = 0; k < w; ++k) pos += s_wcnt[k];
      if (take && pos < f) out[pos] = a.col[s + i];
      run += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
      __syncthreads();
    }
    if (tid == 0) a.out_cnt[p] = (int32_t)f;
  }
}

}  // namespace

extern "C" int32_t gigl_expand_frontier_keyed(gigl_ctx* ctx, gigl_graph* graph, const float* key_col, int32_t method,
                                              const uint32_t* nodes, const uint32_t* ksums, int64_t m, int32_t f,
                                              int32_t hash_add, uint32_t* out_nbr, int32_t* out_cnt) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  GIGL_REQUIRE(ctx, graph && (graph->e == 0 || key_col) && (m == 0 || (nodes && ksums && out_nbr && out_cnt)),
               "null argument");
  GIGL_REQUIRE(ctx, method == GIGL_SAMPLE_TOPK || method == GIGL_SAMPLE_RANDOM_WEIGHTED, "bad keyed sampling method %d",
               method);
  GIGL_REQUIRE(ctx, m >= 0 && m < ((int64_t)1 << 31), "bad sizes");
  if (f < 1 || f > GIGL_MAX_FANOUT)
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "fanout %d outside [1,%d]", f, GIGL_MAX_FANOUT);
  if (graph->multi)
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "keyed sampling needs rows without repeated ids");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (m == 0) return GIGL_OK;
  int32_t rc = gigl_arena_reset(ctx, m * 4 + 1024);
  if (rc != GIGL_OK) return rc;
  int32_t* heavy = (int32_t*)gigl_arena_alloc(ctx, m * 4);
  int32_t* heavy_count = (int32_t*)gigl_arena_alloc(ctx, 256);
  if (!heavy || !heavy_count) return gigl_fail(ctx, GIGL_E_OOM, "arena exhausted");
  KeyedArgs a{};
  a.rowptr = graph->rowptr;
  a.col = graph->col;
  a.key = key_col;
  a.n_nodes = graph->n;
  a.nodes = nodes;
  a.ksums = ksums;
  a.m = m;
  a.f = f;
  a.hash_add = (uint32_t)hash_add;
  a.method = method;
  a.out_nbr = out_nbr;
  a.out_cnt = out_cnt;
  a.heavy = heavy;
  a.heavy_count = heavy_count;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(keyed_zero_kernel, dim3(1), dim3(1), 0, st, heavy_count);
  hipLaunchKernelGGL(keyed_rows_kernel, dim3((unsigned)((m + KEYED_TB / 64 - 1) / (KEYED_TB / 64))), dim3(KEYED_TB), 0,
                     st, a);
  const int64_t wgs = m < KEYED_HEAVY_WGS ? m : KEYED_HEAVY_WGS;
  hipLaunchKernelGGL(keyed_heavy_kernel, dim3((unsigned)wgs), dim3(KEYED_TB), 0, st, a);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}
