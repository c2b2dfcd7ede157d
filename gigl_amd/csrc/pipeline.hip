// pipeline.hip — one-call batch pipeline: k-hop sample -> batch union graph -> GraphSAGE forward ->
// per-root rows.  Everything a batch needs is enqueued by ONE host call on the ctx stream (the host
// side of the hop loop / layer loop lives here, in C++, like the reference's compiled sampler), and
// optionally replayed from hipGraphs so that the ~28 launches of a batch cost one or two host calls.
//
// Replaces, for a RootedNodeNeighborhood batch (paths relative to the reference root):
//   NodeAnchorBasedLinkPredictionModelingTaskSpec.infer_batch
//       python/gigl/src/common/modeling_task_specs/node_anchor_based_link_prediction_modeling_task_spec.py:626-655
//       (`model(data)[root_node_indices]`), and NodeClassificationModelingTaskSpec.infer_batch
//       (.../node_classification_modeling_task_spec.py:176-187),
//   fed by process_raw_pyg_samples_and_collate_fn (rooted_node_neighborhood_data_loader.py:161-241).
#include "common.h"
#include "philox.h"
#include "step_parts.h"
#include "wave_reduce.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

namespace {

// what one call of a plan is given
struct RunArgs {
  const uint32_t* roots;
  int32_t seed, mode;
  float* out;
};

// one thing a plan does for a batch (the step_* functions below), for layer `layer`; `kernels`: the profile ids
// (1 << GIGL_K_*) of the launchers it calls.  A plan's list holds only steps that launch something (plan_build_steps)
struct Step {
  int32_t (*run)(gigl_sage_plan* p, int layer, const RunArgs& a) = nullptr;
  int layer = 0;
  uint32_t kernels = 0;
};

// steps [0, plan->graph_steps) = sample + union [+ the GCN kind's dinv] (the GRAPH part: integer work, latency-bound,
// independent of the weights)
constexpr int MAX_STEPS = 3 + 2 * GIGL_MAX_HOPS;

// a maximal run of consecutive steps: either replayed from a captured graph or launched eagerly
// (steps that contain launches selected for HIP-event timing stay eager: events recorded inside a
// captured graph cannot be timed on this runtime)
struct Segment {
  int s0 = 0, s1 = 0;  // steps [s0, s1)
  hipGraphExec_t exec = nullptr;
};

// launches issued while one of these lives go to `st` instead of the ctx stream
struct StreamScope {
  gigl_ctx* ctx;
  hipStream_t keep;
  StreamScope(gigl_ctx* c, hipStream_t st) : ctx(c), keep(c->stream) { c->stream = st; }
  ~StreamScope() { ctx->stream = keep; }
};

}  // namespace

// the one-call plan: a batch-graph workspace (common.h; its `owned` holds the layer buffers too) and the layers' state
struct gigl_sage_plan : BatchGraph {
  gigl_feat* feat = nullptr;
  int32_t dims[GIGL_MAX_HOPS + 1] = {0};  // dims[0] = input dim, dims[l+1] = output dim of layer l
  const float* w[GIGL_MAX_HOPS] = {nullptr};     // fused [dims[l+1]][2*dims[l]] (= [W_l | W_r]), device, borrowed
  const float* bias[GIGL_MAX_HOPS] = {nullptr};  // device, borrowed, may be null
  int32_t act_last = 0;
  int32_t aggr = GIGL_AGGR_MEAN;  // the SAGE layers' reduction (gigl_sage_plan_set_aggr)
  // projected input (gigl_sage_plan_set_projected_input): [W_l x | W_r x] of EVERY node, [graph nodes][2*dims[1]]
  // fp32, device, borrowed — the first layer is then one gather (+ self row + bias + activation), no projection
  const float* proj = nullptr;
  // first layer over two fp16 planes per operand (three MFMAs instead of six), each operand brought into the top of the
  // half range by a power of two: hs_sa from the table's largest magnitude (plan_refresh_half_split: at create /
  // set_weights / set_aggr; 0 = the table keeps the layer on the bf16 planes), the weights' scale found on the device
  // at every run from the weights as they are (hs_dev = {s_a, s_w, 1 / (s_a s_w)}, gigl_hs_scale_update)
  bool hs0 = false;
  float hs_sa = 0.f;
  float* hs_dev = nullptr;
  // kind 1: GAT layers instead of SAGE layers (gigl_gat_plan_create): w[l] = lin weight [heads*channels][dims[l]],
  // layer 0 from the input side in one row pass (gigl_gat_input_layer_fused), layers >= 1 projection + attention
  // kind 2: TwoLayerGCN at inference (gigl_gcn_plan_create): w[l] = conv{l+1}.lin.weight [dims[l+1]][dims[l]], over the
  // GENERIC union; `proj` is then P = X W1^T [feature rows][dims[1]] (gigl_gcn_plan_set_projected_input)
  int32_t kind = 0;
  float* dinv = nullptr;       // kind 2: 1 / sqrt(deg) of every node of the batch graph [un.cap_nodes] (the graph part's)
  float* gcn_a = nullptr;      // kind 2: a layer's aggregated rows [act_rows][max(dims[0], dims[1])] (aggregate-first / fallback)
  bool gcn_fuse_want = false;  // gigl_gcn_plan_set_fused_root (off by default: measured, DESIGN.md §4 "GCN inference plan")
  bool gcn_fused = false;      // the last layer runs as gcn_root_layer_kernel (decided when the list of steps is built)
  int32_t heads[GIGL_MAX_HOPS] = {0}, channels[GIGL_MAX_HOPS] = {0};
  const float* att_src[GIGL_MAX_HOPS] = {nullptr};
  const float* att_dst[GIGL_MAX_HOPS] = {nullptr};
  float slope = 0.2f;
  float* gat_scratch = nullptr;    // first layer: folded vectors + the per-head tiled operands
  float* alpha_scratch = nullptr;  // layers >= 1: per-node attention dots [2 * act_rows * max heads]
  float* hw = nullptr;             // layers >= 1: projected source rows [act_rows][max heads*channels]
  // edge features (gigl_gat_plan_set_edge_features: the workspace's efeat / eid, and per layer)
  const float* att_edge[GIGL_MAX_HOPS] = {nullptr};  // folded [heads_l][De], device, borrowed
  const float* w_msg[GIGL_MAX_HOPS] = {nullptr};     // [heads_l*channels_l][De] or null, device, borrowed
  float* ze = nullptr;      // first layer: sum_e alpha_e e per row and head [act_rows][heads_0][De] (edge messages)
  bool l2_normalize = false;  // the b output rows become x / max(|x|_2, 1e-12) (gigl_sage_plan_set_l2_normalize)
  float* abuf = nullptr;  // [act_rows][2*max_in]
  // the aggregated matrix in the projection's tiled layout ([row tile of 128][K chunk of 32][128][32]): a tile's chunk
  // is 16 KB contiguous instead of 128 pieces of 128 B at a stride of one row (agg.hip)
  bool tiled = false;
  bool two_source = false;  // the projection takes the self half of [mean | self] from the source rows (no self copy)
  float* hbuf[2] = {nullptr, nullptr};  // ping-pong [act_rows][max_out]
  // fused two-layer projection (agg.hip linear_fused2x_kernel; two-layer SAGE, hidden 256, 2 * out <= 96, half-split first
  // layer over an fp32 table): layer 0's projection applies the last layer's [W_l | W_r] to its hidden rows before they
  // leave the workgroup — hbuf[0] then holds p = [W_l h | W_r h] ([act_rows][96]) instead of hidden rows, and the last
  // layer is one reduction over p rows written straight into the caller's `out`
  // layers >= 1 on the half split too (round 5): their operands are previous-layer outputs, bounded from the previous
  // layer's own scales (gigl_hs_chain_update) — hs_layer[l] = {s_h, s_w, 1 / (s_h s_w)} of layer l, chained from hs_dev
  float* hs_layer[GIGL_MAX_HOPS] = {nullptr};
  bool f2_ok = false;
  float* f2_dev = nullptr;  // {s_h, s_w2, 1 / (s_h s_w2)}: the second product's scales (gigl_fused2_prepare, per run)
  void* w2h = nullptr;      // W1's and W2's fp16 images (gigl_fused2_prepare)
  // what a call runs, in order, for the plan as it is configured now (plan_build_steps: at creation and wherever the
  // configuration changes; a run only walks it)
  Step steps[MAX_STEPS];
  int n_steps = 0;
  int graph_steps = 2;  // the leading steps that make up the GRAPH part
  bool fused2 = false;  // fused2_on() when the list was built
  // hipGraph replay
  bool use_graph = false;
  float* out_buf = nullptr;       // (placeholder `out` of the captures; the step that writes `out` runs eagerly)
  Segment segs[MAX_STEPS];
  int n_segs = 0;
  int32_t cap_seed = 0, cap_mode = -1;
  uint32_t cap_prof_mask = 0;
  uint64_t cap_arena_gen = 0;  // the ctx arena the captured launches point into
  bool captured = false;
  // gigl_sage_plan_set_graph_stream: the GRAPH part of every call is issued on this stream (the caller's, typically of a
  // HIGHER priority than the ctx stream) and the layers wait for it on an event — with several plans in flight the
  // latency-bound sampler / union launches of one call are then dispatched ahead of the other calls' bandwidth-bound
  // layers instead of queueing for CUs behind them
  hipStream_t gstream = nullptr;
  bool split = false;
  hipEvent_t ev_in = nullptr, ev_graph = nullptr;
};

namespace {

// The activation buffers hold b*(1 + f0 + ...) rows — the number of nodes of level < hops when no root is another
// root's sampled neighbour.  Roots that ARE neighbours of each other add the children of those occurrences to the
// inner levels (up to the whole tree in a clique of roots): such a batch does not fit the workspace; its level
// counts are zeroed so that no later kernel touches the buffers, and it is reported through
// meta[GIGL_META_OVERFLOW] (the batch's rows are then invalid, like an LDS-sort overflow).
__global__ void guard_levels_kernel(int32_t* meta, int hops, int32_t act_rows) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  bool over = false;
  for (int l = 0; l < hops; ++l) over = over || meta[GIGL_META_LEVEL0 + l] > act_rows;
  if (over) {  // nothing is computed for this batch (rows would index past the workspace)
    for (int l = 0; l < hops; ++l) meta[GIGL_META_LEVEL0 + l] = 0;
    atomicAdd(&meta[GIGL_META_OVERFLOW], 1);
  }
}

__global__ void overflow_add_kernel(const int32_t* __restrict__ meta, int32_t* __restrict__ acc) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && meta[GIGL_META_OVERFLOW] != 0) atomicAdd(acc, 1);
}

// Edge ids of the plan's union graph: eid[p] = position in the resident graph's `col` (= row of the edge table) of the
// edge stored at position p of un.col, for every row that has in-edges (levels < hops).  The union is leaf-global: rows
// >= *n_local_dev hold GLOBAL source ids, rows below it local ids that go through un.nodes (n_local_dev == NULL: every
// row).  One wave per destination row, lanes over its edges (rows reach hundreds of edges); the resident row is ascending
// in global id: a lower-bound search over rowptr[dst] .. rowptr[dst + 1] (the first of equal ids, as gigl_union_edge_ids);
// -1 when the edge is not there.  int32 is enough: the graph build refuses 2^31 edges.
__global__ __launch_bounds__(256) void plan_edge_ids_kernel(const int64_t* __restrict__ g_rowptr, const uint32_t* __restrict__ g_col,
                                                            int64_t g_n, const uint32_t* __restrict__ nodes,
                                                            const int32_t* __restrict__ rowptr, const int32_t* __restrict__ rowend,
                                                            const int32_t* __restrict__ col, const int32_t* __restrict__ n_rows_dev,
                                                            const int32_t* __restrict__ n_local_dev, int64_t rows_cap,
                                                            int64_t pos_cap, int32_t* __restrict__ eid) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  int64_t n_rows = *n_rows_dev;
  if (n_rows > rows_cap) n_rows = rows_cap;
  const int64_t n_local = n_local_dev ? *n_local_dev : 0x7FFFFFFF;
  for (int64_t i = wave; i < n_rows; i += waves) {
    const uint32_t dst = nodes[i];
    const int64_t p0 = rowptr[i], p1 = rowend[i];
    const bool known = (int64_t)dst < g_n;
    const int64_t r0 = known ? g_rowptr[dst] : 0, r1 = known ? g_rowptr[(int64_t)dst + 1] : 0;
    const bool local = i < n_local;
    for (int64_t p = p0 + lane; p < p1 && p < pos_cap; p += 64) {
      if (p < 0) continue;
      const int32_t j = col[p];
      const uint32_t s = local ? nodes[j] : (uint32_t)j;
      int64_t lo = r0, hi = r1;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (g_col[mid] < s) lo = mid + 1;
        else hi = mid;
      }
      eid[p] = (lo < r1 && g_col[lo] == s) ? (int32_t)lo : -1;
    }
  }
}

// out[i] = out[i] / max(|out[i]|_2, 1e-12) for the b rows of a call (torch.nn.functional.normalize): one wave per row.
// NaN rows (a failed batch set) stay NaN.
__global__ __launch_bounds__(256) void l2_normalize_rows_kernel(float* __restrict__ out, int b, int d) {
  const int lane = threadIdx.x & 63;
  const int i = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (i >= b) return;
  float* row = out + (int64_t)i * d;
  float ss = 0.f;
  for (int c = lane; c < d; c += 64) ss += row[c] * row[c];
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float nrm = sqrtf(ss);
  const float den = nrm < 1e-12f ? 1e-12f : nrm;  // (NaN < x is false: a NaN norm stays)
  for (int c = lane; c < d; c += 64) row[c] = row[c] / den;
}

// exact work counts of the last batch set, accumulated into acc[GIGL_STATS_LEN] (see gigl_sage_plan_stats)
struct StatsArgs {
  const uint32_t* roots;
  const uint32_t* nbr[GIGL_MAX_HOPS];
  const int32_t* cnt[GIGL_MAX_HOPS];
  int32_t fan[GIGL_MAX_HOPS];
  int64_t parents[GIGL_MAX_HOPS];  // parent slots of hop k
  int32_t hops;
  const int64_t* g_rowptr;  // resident graph (in-degrees of the frontier nodes)
  const int32_t* meta;
  const int32_t* rowptr;
  const int32_t* rowend;
  int64_t rows_cap;
};

__device__ __forceinline__ void stats_add(unsigned long long* acc, int slot, long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(&acc[slot], (unsigned long long)v);
}

__global__ __launch_bounds__(256) void plan_stats_kernel(StatsArgs a, unsigned long long* acc) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int L = a.hops;
  long long sampled = 0, bytes = 0;
#pragma unroll
  for (int k = 0; k < GIGL_MAX_HOPS; ++k) {
    if (k >= L) break;
    const uint32_t* par = k == 0 ? a.roots : a.nbr[k - 1];
    for (int64_t p = t0; p < a.parents[k]; p += stride) {
      const uint32_t v = par[p];
      if (v == GIGL_INVALID) continue;
      const long long deg = a.g_rowptr[(int64_t)v + 1] - a.g_rowptr[v];
      // what a POSITION-keyed sampler must move per frontier node (round 5; SURVEY 8(d)'s `16 + 4 deg + 8 min(deg, f)`
      // charges the whole adjacency row, which the reference's rule never needs: the key of entry i is a function of the
      // position i alone, SamplingStrategy.scala:55): the row bounds (16 B); a row of <= f neighbours itself (4 deg);
      // otherwise the <= lambda = f + 4 sqrt(f) + 4 (position, key) pairs of the window's threshold list that can hold
      // the f smallest keys (8 B each) and the f chosen ids (4 f); the sampled (src, dst) pairs out (8 min(deg, f))
      const long long f = a.fan[k];
      const long long lam = f + (long long)(4.0f * sqrtf((float)f)) + 4;
      bytes += 16 + (deg <= f ? 4 * deg : 8 * (deg < lam ? deg : lam) + 4 * f) + 8 * (deg < f ? deg : f);
      sampled += a.cnt[k][p];
    }
  }
  long long agg[GIGL_MAX_HOPS] = {0, 0, 0, 0};
  const int32_t n_rows = a.meta[GIGL_META_LEVEL0 + L - 1];
  for (int64_t i = t0; i < n_rows && i < a.rows_cap; i += stride) {
    const long long len = a.rowend[i] - a.rowptr[i];
#pragma unroll
    for (int l = 0; l < GIGL_MAX_HOPS; ++l)
      if (l < L && i < a.meta[GIGL_META_LEVEL0 + (L - 1 - l)]) agg[l] += len;  // layer l computes rows of level <= L-1-l
  }
  long long agg_all = 0;
#pragma unroll
  for (int l = 0; l < GIGL_MAX_HOPS; ++l) agg_all += agg[l];
  stats_add(acc, GIGL_STATS_SAMPLED, sampled);
  stats_add(acc, GIGL_STATS_AGGREGATED, agg_all);
  stats_add(acc, GIGL_STATS_EXPAND_BYTES, bytes);
#pragma unroll
  for (int l = 0; l < GIGL_MAX_HOPS; ++l) stats_add(acc, GIGL_STATS_AGG_LAYER0 + l, agg[l]);
  if (t0 == 0) {
    atomicAdd(&acc[GIGL_STATS_UNION_EDGES], (unsigned long long)a.meta[GIGL_META_N_EDGES]);
    atomicAdd(&acc[GIGL_STATS_UNION_NODES], (unsigned long long)a.meta[GIGL_META_N_NODES]);
    atomicAdd(&acc[GIGL_STATS_OVERFLOW], (unsigned long long)a.meta[GIGL_META_OVERFLOW]);
    for (int l = 0; l < L; ++l)
      atomicAdd(&acc[GIGL_STATS_ROWS_LAYER0 + l], (unsigned long long)a.meta[GIGL_META_LEVEL0 + (L - 1 - l)]);
  }
}

// (A/B knob: GIGL_PLAN_HS_LAYERS=0 keeps layers >= 1 on the three bf16 planes)
bool hs_layers_on() {
  static const bool on = [] {
    const char* e = getenv("GIGL_PLAN_HS_LAYERS");
    return !(e && e[0] == '0');
  }();
  return on;
}

// the fused two-layer projection applies to this plan as it is configured now.  The answer is cached in p->fused2 by
// plan_build_steps (the steps and gigl_sage_plan_fused_layers read the cache), so every input of the decision — weights
// and bias pointers, reduction, projected input, half split — must go through plan_invalidate when it changes
bool fused2_on(const gigl_sage_plan* p) {
  return p->f2_ok && p->kind == 0 && p->hops == 2 && p->tiled && p->two_source && p->hs0 && !p->proj &&
         p->feat->dtype == GIGL_DTYPE_F32 && (p->aggr == GIGL_AGGR_MEAN || p->aggr == GIGL_AGGR_SUM) &&
         (((uintptr_t)p->bias[0]) & 15) == 0;
}

// (A/B knob: GIGL_F2_ALL_WR set = the fused projection is not told how many of its rows are roots)
bool f2_all_wr() {
  static const bool on = getenv("GIGL_F2_ALL_WR") != nullptr;
  return on;
}

// ---- the batch-graph workspace (BatchGraph, common.h), for batches of b roots on ctx.  number_every_node: the generic
// union (the layers read every source row through un.nodes); else leaf-global where the build allows it — no wide
// workspaces, hops <= 2, ids below 2^31 (row values are compared as int32) and a last fan-out the two-hop builds keep in
// a 64-bit mask (beyond it, the workgroup-per-row sampler path, the generic build) — two hops with the aliased layout
int32_t batch_graph_init(BatchGraph* g, gigl_ctx* ctx, gigl_graph* graph, int32_t b, const int32_t* fanouts, int32_t hops,
                         bool number_every_node) {
  g->ctx = ctx;
  g->graph = graph;
  g->b = b;
  g->group_roots = b;
  g->hops = hops;
  for (int k = 0; k < hops; ++k) g->fanouts[k] = fanouts[k];
  g->wide = ctx->wide;
  g->leaf_global = !number_every_node && !g->wide && hops <= 2 && graph->n < ((int64_t)1 << 31) &&
                   !(hops == 2 && fanouts[1] > GIGL_FAST_FANOUT);
  // activations exist only for nodes of level < hops (leaves are read straight from the feature table)
  g->act_rows = gigl_level_rows(g->wide, b, fanouts, hops, hops - 1);
  g->col_positions = gigl_batch_buffers_alloc(g->owned, b, fanouts, hops, g->leaf_global && hops == 2, &g->tree, &g->un);
  g->roots_buf = (uint32_t*)plan_alloc(g->owned, (size_t)b * 4);
  g->zero_dev = (int32_t*)plan_alloc(g->owned, 64);
  if (g->col_positions && g->roots_buf && g->zero_dev && hipMemset(g->zero_dev, 0, 64) == hipSuccess) return GIGL_OK;
  return gigl_fail(ctx, GIGL_E_OOM, "hipMalloc of the batch workspace failed (cap_nodes=%lld)", (long long)g->un.cap_nodes);
}

void batch_graph_free(BatchGraph* g) {
  for (void* q : g->owned) hipFree(q);
  g->owned.clear();
}

// A leaf-global union numbers the nodes of level <= L-2 only: the rows of level L-1 — behind this device count; every row
// of a one-hop plan — keep their sources as GLOBAL ids.  Null: every row holds local ids
const int32_t* first_global_row(const BatchGraph* g) {
  if (!g->leaf_global) return nullptr;
  return g->hops >= 2 ? g->un.meta + GIGL_META_LEVEL0 + (g->hops - 2) : g->zero_dev;
}

// the graph part reads `table` (one row per resident edge) in place from now on: eid is sized once, for every later run
// (nothing is allocated inside a run: the graph part is captured), and filled with -1
int32_t batch_graph_attach_edge_table(BatchGraph* g, gigl_feat* table) {
  if (!g->eid) {
    g->eid = (int32_t*)plan_alloc(g->owned, (size_t)g->col_positions * 4);
    if (!g->eid) return gigl_fail(g->ctx, GIGL_E_OOM, "hipMalloc of the batch workspace's edge ids failed");
    GIGL_HIP_CHECK(g->ctx, hipMemset(g->eid, 0xFF, (size_t)g->col_positions * 4));
  }
  g->efeat = table;
  return GIGL_OK;
}

// the graph part of one batch, on g's ctx stream: the sampled tree of `roots` ...
int32_t batch_graph_sample(BatchGraph* g, const uint32_t* roots, int32_t seed, int32_t mode) {
  return gigl_sample_khop(g->ctx, g->graph, roots, g->b, g->fanouts, g->hops, seed, mode, &g->tree);
}
// ... and its union graph, the level guard and, with an edge table, the edge ids
int32_t batch_graph_union(BatchGraph* g, const uint32_t* roots) {
  gigl_ctx* ctx = g->ctx;
  const int L = g->hops;
  int32_t rc = gigl_union_build_impl(ctx, roots, &g->tree, g->group_roots, &g->un,
                                     g->leaf_global ? (1 | (g->graph->multi ? 2 : 0)) : 0);
  if (rc != GIGL_OK) return rc;
  hipLaunchKernelGGL(guard_levels_kernel, dim3(1), dim3(64), 0, ctx->stream, g->un.meta, g->hops,
                     (int32_t)(g->act_rows < 0x7FFFFFFF ? g->act_rows : 0x7FFFFFFF));
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  if (g->efeat) {  // the edge ids belong to the GRAPH part: integer work over the union, independent of the weights
    const int64_t rows_cap = gigl_level_rows(g->wide, g->b, g->fanouts, L, L - 1);
    int64_t blocks = (rows_cap + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(plan_edge_ids_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, g->graph->rowptr, g->graph->col,
                       g->graph->n, g->un.nodes, g->un.rowptr, g->un.rowend, g->un.col, g->un.meta + GIGL_META_LEVEL0 + (L - 1),
                       first_global_row(g), rows_cap, g->col_positions, g->eid);
    GIGL_HIP_CHECK(ctx, hipGetLastError());
  }
  return GIGL_OK;
}

// both, for g's own roots_buf
int32_t batch_graph_enqueue(BatchGraph* g, int32_t seed, int32_t mode) {
  const int32_t rc = batch_graph_sample(g, g->roots_buf, seed, mode);
  return rc != GIGL_OK ? rc : batch_graph_union(g, g->roots_buf);
}

// layer l computes the nodes of level <= L-1-l: at most b*(1 + f0 + f0*f1 + ...) of them — the launch is
// sized for that bound, not for the whole union (the exact count is read on the device)
struct LayerRows {
  const int32_t* n_rows;
  int64_t rows_cap;
  int d, act;
};

LayerRows layer_rows(const gigl_sage_plan* p, int l) {
  const int L = p->hops;
  return {p->un.meta + GIGL_META_LEVEL0 + (L - 1 - l), gigl_level_rows(p->wide, p->b, p->fanouts, L, L - 1 - l), p->dims[l],
          (l < L - 1 || p->act_last) ? 1 : 0};
}

// ---- the steps of one batch.  Each enqueues on the ctx stream; which of them a plan runs: plan_build_steps

// (the GRAPH part as two steps: their launches are timed under different profile ids)
int32_t step_sample(gigl_sage_plan* p, int, const RunArgs& a) { return batch_graph_sample(p, a.roots, a.seed, a.mode); }
int32_t step_union(gigl_sage_plan* p, int, const RunArgs& a) { return batch_graph_union(p, a.roots); }

// two-source operand: the projection reads the self half from the fp32 source rows themselves (the feature table
// through union.nodes, or the previous layer's output), the gather writes the reduced half only
// (an fp16 table's rows serve as the self half too when the layer runs the half split: they are its h1 plane)
bool sage_self_half(const gigl_sage_plan* p, int l) { return l == 0 && p->hs0 && p->feat->dtype == GIGL_DTYPE_F16; }
bool sage_two_source(const gigl_sage_plan* p, int l) {
  return p->tiled && p->two_source && (l > 0 || p->feat->dtype == GIGL_DTYPE_F32 || sage_self_half(p, l));
}

// SAGE layer l, first half: the reduced neighbour rows (tiled: the mean chunks, or [mean | self]) into abuf
int32_t step_sage_reduce(gigl_sage_plan* p, int l, const RunArgs&) {
  gigl_ctx* ctx = p->ctx;
  const LayerRows r = layer_rows(p, l);
  const int d = r.d;
  if (p->tiled) {
    const bool two_src = sage_two_source(p, l);
    const int32_t nkc = ((two_src ? d : 2 * d) + 31) / 32;
    if (l == 0)
      return gigl_gather_reduce_mixed(ctx, p->feat->rows, p->feat->dtype, d, p->un.nodes, p->un.rowptr, p->un.rowend, p->un.col,
                                      r.n_rows, r.rows_cap, p->aggr, first_global_row(p), p->abuf, nkc, nullptr, nullptr, nullptr,
                                      two_src ? 1 : 0);
    return gigl_gather_reduce_mixed(ctx, p->hbuf[(l - 1) & 1], GIGL_DTYPE_F32, d, nullptr, p->un.rowptr, p->un.rowend,
                                    p->un.col, r.n_rows, r.rows_cap, p->aggr, nullptr, p->abuf, nkc, nullptr, nullptr, nullptr,
                                    two_src ? 1 : 0);
  }
  if (l == 0 && p->leaf_global)
    return gigl_gather_reduce_mixed(ctx, p->feat->rows, p->feat->dtype, d, p->un.nodes, p->un.rowptr, p->un.rowend,
                                    p->un.col, r.n_rows, r.rows_cap, p->aggr, first_global_row(p), p->abuf);
  if (l == 0)
    return gigl_gather_reduce(ctx, p->feat->rows, p->feat->dtype, d, p->un.nodes, p->un.rowptr, p->un.rowend,
                              p->un.col, r.n_rows, r.rows_cap, p->aggr, p->abuf);
  return gigl_gather_reduce(ctx, p->hbuf[(l - 1) & 1], GIGL_DTYPE_F32, d, nullptr, p->un.rowptr, p->un.rowend,
                            p->un.col, r.n_rows, r.rows_cap, p->aggr, p->abuf);
}

// SAGE layer l, second half: act([reduced | self] W^T + b) into hbuf[l & 1] — by the half split (first layer), the chained
// half split (layers >= 1), the fused pair of layers, the two-source, tiled or row-major projection
int32_t step_sage_project(gigl_sage_plan* p, int l, const RunArgs&) {
  gigl_ctx* ctx = p->ctx;
  const LayerRows r = layer_rows(p, l);
  const int d = r.d;
  const bool two_src = sage_two_source(p, l);
  const float* hs_scale = nullptr;
  if (l == 0 && p->hs0 && p->tiled) {  // the weights' scale follows the weights as they are now (training rewrites them in place)
    uint32_t* a_max = nullptr;  // a sum: the scale follows the operand as the gather wrote it (hs_dev[7]: zero between runs)
    if (p->aggr == GIGL_AGGR_SUM) {
      a_max = reinterpret_cast<uint32_t*>(p->hs_dev + 7);
      const int32_t rc_m = gigl_tiled_absmax(ctx, p->abuf, r.n_rows, r.rows_cap, two_src ? d : 2 * d, a_max);
      if (rc_m != GIGL_OK) return rc_m;
    }
    const int32_t rc = gigl_hs_scale_update(ctx, p->w[0], (int64_t)p->dims[1] * 2 * d, p->hs_sa, p->hs_dev, a_max,
                                            p->feat->absmax > 0.f ? p->feat->absmax : 0.f);
    if (rc != GIGL_OK) return rc;
    hs_scale = p->hs_dev;
  }
  if (l >= 1 && two_src && p->hs0 && !p->proj && p->hs_layer[l] && hs_layers_on()) {
    // half split for a layer >= 1: three fp16 products instead of six bf16 ones
    const float* prev = l == 1 ? p->hs_dev : p->hs_layer[l - 1];
    uint32_t* sum_max = nullptr;  // (a sum of hidden rows: measured, hs_layer[l][7] — zero between runs)
    if (p->aggr == GIGL_AGGR_SUM) {
      sum_max = reinterpret_cast<uint32_t*>(p->hs_layer[l] + 7);
      const int32_t rc_m = gigl_tiled_absmax(ctx, p->abuf, r.n_rows, r.rows_cap, d, sum_max);
      if (rc_m != GIGL_OK) return rc_m;
    }
    int32_t rc = gigl_hs_chain_update(ctx, prev, p->bias[l - 1], p->dims[l], 2 * p->dims[l - 1], sum_max, p->w[l],
                                      (int64_t)p->dims[l + 1] * 2 * d, p->hs_layer[l]);
    if (rc != GIGL_OK) return rc;
    return gigl_linear_tiled(ctx, p->abuf, p->w[l], p->bias[l], r.n_rows, r.rows_cap, 2 * d, p->dims[l + 1], r.act,
                             p->hbuf[l & 1], p->hbuf[(l - 1) & 1], nullptr, d, d, p->hs_layer[l]);
  }
  if (l == 0 && p->fused2) {  // hbuf[0] takes p = [W_l h | W_r h] of the last layer instead of hidden rows (step_roots)
    int32_t rc = gigl_fused2_prepare(ctx, p->hs_dev, p->bias[0], p->w[0], p->w[1], p->dims[2], 2 * d, p->f2_dev, p->w2h);
    if (rc != GIGL_OK) return rc;
    return gigl_linear_fused2(ctx, p->abuf, p->bias[0], r.n_rows, r.rows_cap, 2 * d, p->hbuf[0], (const float*)p->feat->rows,
                              p->un.nodes, d, d, hs_scale, p->f2_dev, p->w2h,
                              f2_all_wr() ? nullptr : p->un.meta + GIGL_META_LEVEL0);
  }
  if (two_src)
    return gigl_linear_tiled(ctx, p->abuf, p->w[l], p->bias[l], r.n_rows, r.rows_cap, 2 * d, p->dims[l + 1], r.act,
                             p->hbuf[l & 1], l == 0 ? (const float*)p->feat->rows : p->hbuf[(l - 1) & 1],
                             l == 0 ? p->un.nodes : nullptr, d, d, hs_scale, sage_self_half(p, l));
  if (p->tiled)
    return gigl_linear_tiled(ctx, p->abuf, p->w[l], p->bias[l], r.n_rows, r.rows_cap, 2 * d, p->dims[l + 1], r.act,
                             p->hbuf[l & 1], nullptr, nullptr, 0, 0, hs_scale);
  return gigl_linear(ctx, p->abuf, p->w[l], p->bias[l], r.n_rows, r.rows_cap, 2 * d, p->dims[l + 1], r.act,
                     p->hbuf[l & 1]);
}

// the first SAGE layer over a projected input — lin_l(mean_j x_j) = mean_j lin_l(x_j): the rows arrive projected, the
// layer is the reduction plus the self row, no projection
int32_t step_sage_projected_input(gigl_sage_plan* p, int, const RunArgs&) {
  const LayerRows r = layer_rows(p, 0);
  return gigl_gather_project_mixed(p->ctx, p->proj, p->proj + p->dims[1], 2 * p->dims[1], p->dims[1], p->un.nodes, p->un.rowptr,
                                   p->un.rowend, p->un.col, r.n_rows, r.rows_cap, p->aggr, first_global_row(p), p->bias[0], r.act,
                                   p->hbuf[0]);
}

// the first GAT layer from the input side: aggregation + every head's projection in one row pass
int32_t step_gat_input(gigl_sage_plan* p, int, const RunArgs&) {
  gigl_ctx* ctx = p->ctx;
  const LayerRows r = layer_rows(p, 0);
  if (p->hs0) {
    const int32_t rc = gigl_hs_scale_update(ctx, p->w[0], (int64_t)p->heads[0] * p->channels[0] * r.d, p->hs_sa, p->hs_dev);
    if (rc != GIGL_OK) return rc;
  }
  gigl_gat_edge_terms et{};
  if (p->efeat) {
    et.eid = p->eid;
    et.table = (const float*)p->efeat->rows;
    et.edge_dim = p->efeat->d;
    et.att_edge_folded = p->att_edge[0];
    et.w_edge_msg = p->w_msg[0];
    et.ze = p->ze;
  }
  return gigl_gat_input_layer_fused_hs(ctx, p->feat->rows, p->feat->dtype, r.d, p->un.nodes, first_global_row(p), p->w[0],
                                       p->att_src[0], p->att_dst[0], p->heads[0], p->channels[0], p->slope, p->un.rowptr,
                                       p->un.rowend, p->un.col, r.n_rows, r.rows_cap, p->bias[0], r.act, p->gat_scratch, p->hbuf[0],
                                       p->hs0 ? p->hs_dev : nullptr, p->efeat ? &et : nullptr);
}

// sources of GAT layer l >= 1: the rows layer l-1 computed (level <= L-l) — rows_cap plus the slots of hop L-1-l
int64_t gat_src_cap(const gigl_sage_plan* p, int l, int64_t rows_cap) {
  if (p->wide) return rows_cap;  // (rows_cap is the whole tree already)
  int64_t width = p->b;
  for (int i = 0; i <= p->hops - 1 - l; ++i) width *= p->fanouts[i];
  return rows_cap + width;
}

// GAT layer l >= 1, first half: hw = h W^T of its source rows
int32_t step_gat_project(gigl_sage_plan* p, int l, const RunArgs&) {
  const LayerRows r = layer_rows(p, l);
  return gigl_linear(p->ctx, p->hbuf[(l - 1) & 1], p->w[l], nullptr, p->un.meta + GIGL_META_LEVEL0 + (p->hops - l),
                     gat_src_cap(p, l, r.rows_cap), r.d, p->dims[l + 1], 0, p->hw);
}

// GAT layer l >= 1, second half: attention over hw into hbuf[l & 1], with the edge terms of an edge-featured plan
int32_t step_gat_attend(gigl_sage_plan* p, int l, const RunArgs&) {
  gigl_ctx* ctx = p->ctx;
  const LayerRows r = layer_rows(p, l);
  const int32_t* n_src = p->un.meta + GIGL_META_LEVEL0 + (p->hops - l);
  const int64_t src_cap = gat_src_cap(p, l, r.rows_cap);
  if (p->efeat)  // (a_edge lies behind the 2 * src_cap * heads node dots of alpha_scratch)
    return gigl_gat_aggregate_edge_indexed(ctx, p->hw, p->att_src[l], p->att_dst[l], p->heads[l], p->channels[l], p->slope, 1,
                                           p->un.rowptr, p->un.rowend, p->un.col, n_src, src_cap, r.n_rows, r.rows_cap, p->bias[l],
                                           r.act, (const float*)p->efeat->rows, p->eid, p->efeat->d, p->col_positions,
                                           p->att_edge[l], p->w_msg[l],
                                           p->alpha_scratch, p->hbuf[l & 1]);
  return gigl_gat_aggregate(ctx, p->hw, p->att_src[l], p->att_dst[l], p->heads[l], p->channels[l], p->slope, 1,
                            p->un.rowptr, p->un.rowend, p->un.col, n_src, src_cap, r.n_rows, r.rows_cap, p->bias[l], r.act,
                            p->alpha_scratch, p->hbuf[l & 1]);
}

// the roots' rows into the caller's `out`: taken from the last layer's output — a fused plan's last layer IS this step, one
// reduction over the p rows of the fused projection per root — then normalised when the plan says so
int32_t step_roots(gigl_sage_plan* p, int l, const RunArgs& a) {
  gigl_ctx* ctx = p->ctx;
  const int dout = p->dims[l + 1];
  if (p->fused2) {
    const int32_t rc = gigl_sage_fused_out(ctx, p->hbuf[0], p->un.rowptr, p->un.rowend, p->un.col, p->un.root_local, p->b,
                                           dout, p->bias[l], p->act_last ? 1 : 0, p->aggr, p->un.meta, a.out);
    if (rc != GIGL_OK) return rc;
  } else {
    gigl_take_rows(ctx->stream, p->hbuf[l & 1], p->un.root_local, p->b, dout, p->un.meta, a.out);
  }
  if (p->l2_normalize)
    hipLaunchKernelGGL(l2_normalize_rows_kernel, dim3((unsigned)((p->b + 3) / 4)), dim3(256), 0, ctx->stream, a.out, p->b, dout);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

// ---- the GCN kind (TwoLayerGCN at inference, homogeneous.py:488-546 / node_classification_modeling_task_spec.py:176-187)

// A_hat's normalisation over every node of the union: integer-side work on the batch graph alone — the graph part's
int32_t step_gcn_dinv(gigl_sage_plan* p, int, const RunArgs&) {
  return gigl_gcn_dinv(p->ctx, p->un.rowptr, p->un.rowend, p->un.col, p->un.meta + GIGL_META_N_NODES, p->un.cap_nodes, p->dinv);
}

// layer l, aggregate-first, first half: A_hat over the table through un.nodes (l = 0) or over h1 (l = 1), for the rows the
// layer computes
int32_t step_gcn_gather(gigl_sage_plan* p, int l, const RunArgs&) {
  const LayerRows r = layer_rows(p, l);
  if (l == 0)
    return gigl_gcn_gather(p->ctx, p->feat->rows, p->feat->dtype, r.d, p->un.nodes, p->dinv, p->un.rowptr, p->un.rowend, p->un.col,
                           r.n_rows, r.rows_cap, p->gcn_a);
  return gigl_gcn_gather(p->ctx, p->hbuf[0], GIGL_DTYPE_F32, r.d, nullptr, p->dinv, p->un.rowptr, p->un.rowend, p->un.col, r.n_rows,
                         r.rows_cap, p->gcn_a);
}

// ... second half: the projection with bias (and the rectifier below the last layer) into hbuf[l]
int32_t step_gcn_project(gigl_sage_plan* p, int l, const RunArgs&) {
  const LayerRows r = layer_rows(p, l);
  return gigl_linear(p->ctx, p->gcn_a, p->w[l], p->bias[l], r.n_rows, r.rows_cap, r.d, p->dims[l + 1], r.act, p->hbuf[l]);
}

// layer 1 over the projected table: one gather over hid-wide rows + bias + rectifier
int32_t step_gcn_projected_input(gigl_sage_plan* p, int, const RunArgs&) {
  const LayerRows r = layer_rows(p, 0);
  return gigl_gcn_layer_rows(p->ctx, p->proj, p->dims[1], p->un.nodes, p->dinv, p->un.rowptr, p->un.rowend, p->un.col, r.n_rows,
                             r.rows_cap, p->bias[0], p->hbuf[0]);
}

// layer 2 and the roots' rows in one launch, into the caller's `out`
int32_t step_gcn_root(gigl_sage_plan* p, int, const RunArgs& a) {
  return gigl_gcn_root_layer(p->ctx, p->hbuf[0], p->dims[1], p->dims[2], p->dinv, p->un.rowptr, p->un.rowend, p->un.col,
                             p->un.root_local, p->b, p->w[1], p->bias[1], p->l2_normalize ? 1 : 0, p->un.meta, a.out);
}

int32_t run_steps(gigl_sage_plan* p, int s0, int s1, const RunArgs& a) {
  for (int s = s0; s < s1; ++s) {
    const int32_t rc = p->steps[s].run(p, p->steps[s].layer, a);
    if (rc != GIGL_OK) return rc;
  }
  return GIGL_OK;
}

// the ordered steps of one batch for the plan as it is configured now: kind, hops, projected input, fused pair of layers.
// (Edge features change what step_union and the GAT steps launch, not which steps run.)  Only steps that launch something
// are listed, each with the profile ids its launchers record under
void plan_build_steps(gigl_sage_plan* p) {
  const uint32_t gather = 1u << GIGL_K_GATHER_MEAN, linear = 1u << GIGL_K_LINEAR;
  const int L = p->hops;
  p->fused2 = fused2_on(p);
  int n = 0;
  auto add = [&](decltype(Step::run) run, int layer, uint32_t kernels) { p->steps[n++] = Step{run, layer, kernels}; };
  add(step_sample, 0, (1u << GIGL_K_EXPAND) | (1u << GIGL_K_EXPAND_HEAVY) | (1u << GIGL_K_FIND_HEAVY));
  add(step_union, 0, (1u << GIGL_K_UNION_INSERT) | (1u << GIGL_K_UNION_RELAX) | (1u << GIGL_K_UNION_NODES) |
                         (1u << GIGL_K_UNION_EDGE_SORT) | (1u << GIGL_K_UNION_CSR));
  p->graph_steps = n;
  if (p->kind == 2) {
    add(step_gcn_dinv, 0, gather);
    p->graph_steps = n;
    p->gcn_fused = p->gcn_fuse_want && gigl_gcn_root_layer_ok(p->dims[1], p->dims[2], p->w[1]);
    if (p->proj) {
      add(step_gcn_projected_input, 0, gather);
    } else {
      add(step_gcn_gather, 0, gather);
      add(step_gcn_project, 0, linear);
    }
    if (p->gcn_fused) {
      add(step_gcn_root, 1, gather);
    } else {
      add(step_gcn_gather, 1, gather);
      add(step_gcn_project, 1, linear);
      add(step_roots, 1, 0);
    }
    p->n_steps = n;
    return;
  }
  for (int l = 0; l < L; ++l) {
    if (p->kind == 1) {
      if (l == 0) {  // (the row pass records as a gather, the heads' projection behind it as a linear)
        add(step_gat_input, 0, gather | linear);
      } else {
        add(step_gat_project, l, linear);
        add(step_gat_attend, l, gather);
      }
    } else if (l == 0 && p->proj) {
      add(step_sage_projected_input, 0, gather);
    } else if (l == 1 && p->fused2) {
      // (layer 0's projection applied this layer's weights already; its reduction is step_roots)
    } else {
      add(step_sage_reduce, l, gather);
      add(step_sage_project, l, linear);
    }
  }
  add(step_roots, L - 1, p->fused2 ? gather : 0);
  p->n_steps = n;
}

void drop_graphs(gigl_sage_plan* p) {
  for (int i = 0; i < p->n_segs; ++i)
    if (p->segs[i].exec) hipGraphExecDestroy(p->segs[i].exec);
  p->n_segs = 0;
  p->captured = false;
}

// the configuration changed: what the captured launches hold is stale, and so may be the list of steps
void plan_invalidate(gigl_sage_plan* p) {
  if (p->captured) {
    hipStreamSynchronize(p->ctx->stream);
    drop_graphs(p);
  }
  plan_build_steps(p);
}

// split the steps into timed (eager) and untimed (captured) segments, by the steps' own kernel ids, and capture the latter
int32_t capture_segments(gigl_sage_plan* p, int32_t sampling_seed, int32_t mode) {
  gigl_ctx* ctx = p->ctx;
  const int n = p->n_steps;
  const uint32_t mask = ctx->prof_mask;
  // (the last step — the roots' rows into the caller's `out` — stays out of the graphs: launched eagerly with the
  // pointer of the call, instead of a captured write to a static buffer and a device copy of it per call)
  auto timed = [&](int s) { return s == n - 1 || (p->steps[s].kernels & mask) != 0; };
  for (int s = 0; s < n;) {
    int e = s + 1;  // (the last step is a segment of its own; a split plan's graph part ends one)
    while (e < n - 1 && timed(e) == timed(s) && !(p->split && e == p->graph_steps)) ++e;
    Segment& sg = p->segs[p->n_segs] = Segment{s, e, nullptr};
    if (!timed(s)) {
      // (a graph-part segment of a split plan is captured from — and later launched on — the plan's graph stream)
      StreamScope on(ctx, p->split && e <= p->graph_steps ? p->gstream : ctx->stream);
      char what[64];  // (the message keeps its wording; the numbers are positions in the plan's list of steps)
      snprintf(what, sizeof what, "stages [%d,%d) of the batch pipeline", s, e);
      const int32_t rc = gigl_capture(ctx, ctx->stream, what, &sg.exec,
                                      [&] { return run_steps(p, s, e, {p->roots_buf, sampling_seed, mode, p->out_buf}); });
      if (rc != GIGL_OK) return rc;
    }
    ++p->n_segs;
    s = e;
  }
  return GIGL_OK;
}

// ---- training step (gigl_sage_train_plan_*)

// cross-entropy on the roots' rows: one wave per root.  loss_rows[i] = lse(out[rl]) - out[rl][label] for the n_valid real
// roots (0 for padding); the gradient (softmax - onehot) / n_valid is ADDED to dout[rl] (zeroed before; two roots of a
// batch that are the same node share a row, hence the atomics — a row with one root gets plain values)
__device__ __forceinline__ void ce_root_row(const float* __restrict__ out, int width, const int32_t* __restrict__ root_local,
                                            const int64_t* __restrict__ labels, const int32_t* __restrict__ n_valid_dev, int b,
                                            const int32_t* __restrict__ meta, float* __restrict__ dout,
                                            float* __restrict__ loss_rows) {
  const int lane = threadIdx.x & 63;
  const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (i >= b) return;
  const int n_valid = *n_valid_dev;
  const int32_t rl = root_local[i];
  if (i >= n_valid || rl < 0 || meta[GIGL_META_OVERFLOW] != 0) {
    if (lane == 0) loss_rows[i] = meta[GIGL_META_OVERFLOW] != 0 ? __builtin_nanf("") : 0.f;
    return;
  }
  const float* row = out + (int64_t)rl * width;
  float mx = -3.402823466e38f;
  for (int c = lane; c < width; c += 64) mx = fmaxf(mx, row[c]);
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float se = 0.f;
  for (int c = lane; c < width; c += 64) se += gigl_ce_exp(row[c], mx);
  for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
  const float lse = gigl_ce_lse(mx, se);
  const int64_t lab = labels[i];
  if (lab < 0 || lab >= width) {
    // (torch's cross_entropy asserts on such a target; here the batch is reported failed — NaN loss, no update — instead
    // of reading past the row: an ignore_index-style -1 or an output narrower than the label space)
    if (lane == 0) {
      loss_rows[i] = __builtin_nanf("");
      atomicAdd(const_cast<int32_t*>(&meta[GIGL_META_OVERFLOW]), 1);
    }
    return;
  }
  const float inv = 1.0f / (float)n_valid;
  for (int c = lane; c < width; c += 64) {
    const float pr = __expf(row[c] - lse);
    atomicAdd(&dout[(int64_t)rl * width + c], (pr - (c == (int)lab ? 1.f : 0.f)) * inv);
  }
  if (lane == 0) loss_rows[i] = lse - row[lab];
}

__global__ __launch_bounds__(256) void ce_roots_kernel(const float* __restrict__ out, int width, const int32_t* __restrict__ root_local,
                                                       const int64_t* __restrict__ labels, const int32_t* __restrict__ n_valid_dev,
                                                       int b, const int32_t* __restrict__ meta, float* __restrict__ dout,
                                                       float* __restrict__ loss_rows) {
  ce_root_row(out, width, root_local, labels, n_valid_dev, b, meta, dout, loss_rows);
}

// ---- round 6: the node-classification step's small launches folded together (each costs ~5 us of a 0.22-ms step) ----
// prep: the cleared block (the dh rows that are ADDED to) and the transposed weights of layers >= 1 (the backward's
// da = dh . W needs W^T as the projection's weight operand; the weights only change in the previous step's Adam), in ONE launch
struct TrainPrep {
  uint32_t* zero;
  int64_t zero_words;
  const float* w[GIGL_MAX_HOPS];
  float* wt[GIGL_MAX_HOPS];
  int32_t rows[GIGL_MAX_HOPS], cols[GIGL_MAX_HOPS];
  int32_t n_t;
};
// the step's inputs into the static buffers the captured launches read — labels, the number of real roots, where the
// caller wants the loss — in one launch (was: a device copy, a 32-bit fill and, after the step, another device copy)
__global__ __launch_bounds__(256) void train_stage_kernel(const int64_t* __restrict__ labels, int n_valid, int64_t* __restrict__ labels_buf,
                                                          int32_t* __restrict__ n_valid_buf, float** __restrict__ loss_slot,
                                                          float* loss_out, TrainPrep a) {
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = t0; i < n_valid; i += stride) labels_buf[i] = labels[i];
  if (t0 == 0) {
    n_valid_buf[0] = n_valid;
    *loss_slot = loss_out;
  }
  // ... and the prep work (this launch is eager, ahead of the captured layers: one node less in the replayed graph)
  for (int64_t i = t0; i < a.zero_words; i += stride) a.zero[i] = 0u;
  for (int q = 0; q < a.n_t; ++q) {
    const int64_t n = (int64_t)a.rows[q] * a.cols[q];
    for (int64_t i = t0; i < n; i += stride) {
      const int r = (int)(i / a.cols[q]), c = (int)(i - (int64_t)r * a.cols[q]);
      a.wt[q][(int64_t)c * a.rows[q] + r] = a.w[q][i];
    }
  }
}

// loss = sum_i loss_rows[i] / n_valid in a fixed order (one workgroup); the optimiser's step counter moves on
__global__ __launch_bounds__(1024) void loss_sum_kernel(const float* __restrict__ loss_rows, int b,
                                                        const int32_t* __restrict__ n_valid_dev, float* __restrict__ loss,
                                                        int32_t* __restrict__ step, const int32_t* __restrict__ meta,
                                                        int32_t* __restrict__ halt, float* const* loss_slot) {
  __shared__ float s_p[16];
  float v = 0.f;
  for (int i = threadIdx.x; i < b; i += 1024) v += loss_rows[i];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < 16; ++k) t += s_p[k];
    *loss = t / (float)(*n_valid_dev > 0 ? *n_valid_dev : 1);
    // (a failed batch applies no update — adam_kernel returns — so Adam's bias-correction exponent must not move either)
    // `halt` is STICKY: once a batch has failed, every later step of the queue trains nothing either (NaN loss) until the
    // host has seen it (gigl_sage_train_plan_resume) — steps are issued without a host read in between, and the batches
    // behind a failed one must not be applied ahead of its redo
    if (*halt != 0) *loss = __builtin_nanf("");
    else if (meta[GIGL_META_OVERFLOW] == 0) *step += 1;
    else *halt = 1;
    // (round 6: the caller's loss slot, set by train_stage_kernel — no device copy after the step)
    if (*loss_slot) **loss_slot = *loss;
  }
}

// dy[i][c] = 0 where the layer's activated output is 0 (relu'), rows below *n_rows
__global__ __launch_bounds__(256) void relu_mask_kernel(float* __restrict__ dy, const float* __restrict__ y,
                                                        const int32_t* __restrict__ n_rows_dev, int width) {
  const int64_t n = (int64_t)(*n_rows_dev) * width;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (!(y[i] > 0.f)) dy[i] = 0.f;
}

// ---- dropout between the training plans' layers (include/gigl_hip.h: gigl_sage_train_plan_set_dropout; philox.h)

// rows a kernel may touch: the device count, bounded by the buffer's capacity
__device__ __forceinline__ int64_t rows_below_cap(const int32_t* __restrict__ n_rows_dev, int64_t rows_cap) {
  const int64_t n = *n_rows_dev;
  return n < 0 ? 0 : (n > rows_cap ? rows_cap : n);
}

// h[r][c] = kept ? h[r][c] * scale : 0, in place on a layer's activated output, rows below *n_rows_dev.  A lane takes the four
// columns of one Philox block: one 16-byte load and store when the rows are whole float4s (width % 4 == 0), else — rows
// that do not start on 16 bytes — the block's columns one by one (the last block of a row may hold fewer than four).
// *step_dev is read BEFORE the step's loss launch moves it on: the plan's count of applied steps.  A row takes 2^lg lanes
// (lg = dropout_lanes_log2: the blocks of a row rounded up to a power of two, so that row and block come from a shift and
// a mask — a 64-bit division per block cost more than the block's ten rounds)
__global__ __launch_bounds__(256) void dropout_rows_kernel(float* __restrict__ h, const int32_t* __restrict__ n_rows_dev,
                                                           int64_t rows_cap, int width, const int32_t* __restrict__ step_dev,
                                                           DropoutMask m, int lg) {
  const int groups = (width + 3) >> 2;
  const int64_t n = rows_below_cap(n_rows_dev, rows_cap) << lg;
  const uint32_t step = (uint32_t)*step_dev;
  const bool whole = (width & 3) == 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i >> lg;
    const int g = (int)(i & ((1 << lg) - 1));
    if (g >= groups) continue;
    uint32_t w[4];
    gigl_dropout_words(m, (uint32_t)r, (uint32_t)g, step, w);
    float* q = h + r * width + 4 * g;
    if (whole) {
      float4 v = *reinterpret_cast<const float4*>(q);
      v.x = w[0] >= m.thresh ? v.x * m.scale : 0.f;
      v.y = w[1] >= m.thresh ? v.y * m.scale : 0.f;
      v.z = w[2] >= m.thresh ? v.z * m.scale : 0.f;
      v.w = w[3] >= m.thresh ? v.w * m.scale : 0.f;
      *reinterpret_cast<float4*>(q) = v;
    } else {
      const int cols = width - 4 * g < 4 ? width - 4 * g : 4;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cols) q[k] = w[k] >= m.thresh ? q[k] * m.scale : 0.f;
    }
  }
}

// dy = y > 0 ? dy * scale : 0 — the rectifier's and the dropout's backward in one pass: a dropped element's output is 0 as a
// rectified one's, a kept one's gradient carries the forward's scale.  Rows below *n_rows_dev; whole: width % 4 == 0 and
// both buffers start on 16 bytes (dy may be carved out of a block behind tensors of any size): 16-byte accesses
__global__ __launch_bounds__(256) void dropout_relu_mask_kernel(float* __restrict__ dy, const float* __restrict__ y,
                                                                const int32_t* __restrict__ n_rows_dev, int64_t rows_cap,
                                                                int width, float scale, int whole) {
  const int64_t n = rows_below_cap(n_rows_dev, rows_cap) * width;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  if (whole) {
    for (int64_t i = t0; i < (n >> 2); i += stride) {
      const float4 a = reinterpret_cast<const float4*>(y)[i];
      float4 g = reinterpret_cast<const float4*>(dy)[i];
      g.x = a.x > 0.f ? g.x * scale : 0.f;
      g.y = a.y > 0.f ? g.y * scale : 0.f;
      g.z = a.z > 0.f ? g.z * scale : 0.f;
      g.w = a.w > 0.f ? g.w * scale : 0.f;
      reinterpret_cast<float4*>(dy)[i] = g;
    }
  } else {
    for (int64_t i = t0; i < n; i += stride) dy[i] = y[i] > 0.f ? dy[i] * scale : 0.f;
  }
}

// keep[r][c] = 1 where the mask keeps element (r, c) (gigl_dropout_mask): a lane per Philox block, 2^lg lanes per row
__global__ __launch_bounds__(256) void dropout_keep_kernel(uint8_t* __restrict__ keep, int64_t rows, int width, uint32_t step,
                                                           DropoutMask m, int lg) {
  const int groups = (width + 3) >> 2;
  const int64_t n = rows << lg;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i >> lg;
    const int g = (int)(i & ((1 << lg) - 1));
    if (g >= groups) continue;
    uint32_t w[4];
    gigl_dropout_words(m, (uint32_t)r, (uint32_t)g, step, w);
    const int cols = width - 4 * g < 4 ? width - 4 * g : 4;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cols) keep[r * width + 4 * g + k] = w[k] >= m.thresh ? 1 : 0;
  }
}

// Adam with L2 weight decay (torch.optim.Adam: the decay joins the gradient), every parameter tensor in one launch.
// A tensor's gradient is the sum of up to two SOURCES (the two encodes of a link-prediction step share the weights).  A
// source is a plain vector g, or the weight-gradient kernel's per-chunk PARTIAL sums (part != NULL: [chunks][n] floats, the
// chunks below ceil(*rows / rc) hold real rows) added up here in chunk order — one reduce launch less per layer; source 0
// may hold both (the GAT plan: the folded attention vectors' share of W0's gradient beside the projections' partial sums)
constexpr int ADAM_MAX = 24;  // tensors (or slices of tensors: the GAT plan's heads, up to 2 * 4 + 6, and its six edge
                               // tensors) per launch — 88 bytes each: the pack stays near 2 KB of kernel arguments
struct AdamPack {
  float* p[ADAM_MAX];
  float* m[ADAM_MAX];
  float* v[ADAM_MAX];
  int64_t n[ADAM_MAX];
  const float* g[2][ADAM_MAX];
  const float* part[2][ADAM_MAX];
  const int32_t* rows[2][ADAM_MAX];
  int32_t rc[2][ADAM_MAX];
  int32_t count;
  // 1: gradient = source 0 (node classification); 2: source 0 + source 1 — the order of reduce + reduce + add; a tensor
  // without a second source adds 0
  int32_t n_src;
  float lr, beta1, beta2, eps, wd;
  // torch.optim.lr_scheduler.ConstantLR, stepped after the optimiser: Adam's step t (1-based) runs at lr_warm (= lr * factor,
  // multiplied once on the host) while t - 1 < warm_iters, at lr from then on.  warm_iters 0: no schedule
  float lr_warm;
  int32_t warm_iters;
};

// (sixteen chunks' loads in flight, added in chunk order)
__device__ __forceinline__ float chunk_sum(const float* __restrict__ part, int chunks, int64_t n, int64_t i) {
  float s = 0.f;
  int c = 0;
  for (; c + 15 < chunks; c += 16) {
    float pv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) pv[q] = part[(int64_t)(c + q) * n + i];
#pragma unroll
    for (int q = 0; q < 16; ++q) s += pv[q];
  }
  for (; c < chunks; ++c) s += part[(int64_t)c * n + i];
  return s;
}

// element i of tensor k's RAW gradient — its sources added up, before clipping and before the decay: the one expression
// both the norm pass and Adam evaluate (ch0 / ch1: the chunks of source 0 / 1 that hold real rows)
__device__ __forceinline__ float adam_raw_grad(const AdamPack& a, int k, int ch0, int ch1, int64_t i) {
  const float *g0 = a.g[0][k], *g1 = a.g[1][k], *part0 = a.part[0][k], *part1 = a.part[1][k];
  float ga = part0 ? chunk_sum(part0, ch0, a.n[k], i) : g0[i];
  if (part0 && g0) ga += g0[i];
  if (a.n_src == 2) {
    const float gb = part1 ? chunk_sum(part1, ch1, a.n[k], i) : (g1 ? g1[i] : 0.f);
    return ga + gb;
  }
  return ga;
}

// a failed batch trains nothing (its loss is NaN).  meta_b: the second encode's batch (NULL: the step has one); halt: the
// sticky "a batch failed" word (NULL: the plan has none)
__device__ __forceinline__ bool adam_batch_failed(const int32_t* meta_a, const int32_t* meta_b, const int32_t* halt) {
  return meta_a[GIGL_META_OVERFLOW] != 0 || (meta_b && meta_b[GIGL_META_OVERFLOW] != 0) || (halt && *halt != 0);
}

// Gradient clipping (torch.nn.utils.clip_grad_norm_, 2-norm over all parameters) needs the norm of gradients that only
// exist inside the Adam kernel — partial sums, two sources — so it takes a pass of its own over the same pack, on the same
// grid (x: a tensor's elements, y: the tensor): every workgroup squares the raw gradients of its elements into fp64, reduces
// them over the wave and then over its four waves in LDS, and stores ONE partial at [blockIdx.y][blockIdx.x].  A pack entry
// counts once (a shared tensor is one entry, the per-head slices partition W0).  No atomics, no tickets: grad_norm_final_kernel
// adds the partials in index order.
constexpr int ADAM_GRID_X_MAX = 208;
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(AdamPack a, const int32_t* __restrict__ meta_a,
                                                          const int32_t* __restrict__ meta_b, const int32_t* __restrict__ halt,
                                                          double* __restrict__ partials) {
  if (adam_batch_failed(meta_a, meta_b, halt)) return;
  __shared__ double s_w[4];
  const int k = (int)blockIdx.y;  // (gridDim.y == a.count)
  const int ch0 = a.part[0][k] ? (*a.rows[0][k] + a.rc[0][k] - 1) / a.rc[0][k] : 0;
  const int ch1 = a.part[1][k] ? (*a.rows[1][k] + a.rc[1][k] - 1) / a.rc[1][k] : 0;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n[k]; i += (int64_t)gridDim.x * blockDim.x) {
    const double g = (double)adam_raw_grad(a, k, ch0, ch1, i);
    acc += g * g;
  }
  acc = gigl_wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// total_norm = sqrt(sum of the n partials, lane-strided then butterfly then wave order: fixed), coef = min(1, max_norm /
// (total_norm + 1e-6)) -> out2 = {total_norm, coef}; one workgroup.  A NaN norm gives a NaN coef, as torch's clamp does.
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const double* __restrict__ partials, int n, float max_norm,
                                                              const int32_t* __restrict__ meta_a,
                                                              const int32_t* __restrict__ meta_b,
                                                              const int32_t* __restrict__ halt, float* __restrict__ out2) {
  if (adam_batch_failed(meta_a, meta_b, halt)) return;  // (the words keep the last trained step's)
  __shared__ double s_w[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += partials[i];
  acc = gigl_wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double norm = sqrt(((s_w[0] + s_w[1]) + s_w[2]) + s_w[3]);
    const double c = (double)max_norm / (norm + 1e-6);
    out2[0] = (float)norm;
    out2[1] = (float)(c > 1.0 ? 1.0 : c);
  }
}

// CLIP: every raw gradient is multiplied by clip[1] (the coef grad_norm_final_kernel left) before the decay joins it.  The
// CLIP = false instantiation (clip NULL) is the kernel as it was before clipping existed: the same arithmetic, the same bits.
template <bool CLIP>
__global__ __launch_bounds__(256) void adam_kernel(AdamPack a, const int32_t* __restrict__ step_dev,
                                                   const int32_t* __restrict__ meta_a, const int32_t* __restrict__ meta_b,
                                                   const int32_t* __restrict__ halt, const float* __restrict__ clip) {
  if (adam_batch_failed(meta_a, meta_b, halt)) return;
  const int32_t step = *step_dev;
  const double t = (double)step;
  const float bc1 = (float)(1.0 - pow((double)a.beta1, t)), bc2s = (float)sqrt(1.0 - pow((double)a.beta2, t));
  const float step_size = (step - 1 < a.warm_iters ? a.lr_warm : a.lr) / bc1;
  float coef = 1.f;
  if constexpr (CLIP) coef = clip[1];
  // gridDim.y > 1: one slice of the grid per tensor (the partial sums are chains of dependent-latency loads: the tensors'
  // chains run side by side instead of one after the other)
  const int k_lo = gridDim.y > 1 ? (int)blockIdx.y : 0, k_hi = gridDim.y > 1 ? (int)blockIdx.y + 1 : a.count;
  for (int k = k_lo; k < k_hi && k < a.count; ++k) {
    float* p = a.p[k];
    float* m = a.m[k];
    float* v = a.v[k];
    const int ch0 = a.part[0][k] ? (*a.rows[0][k] + a.rc[0][k] - 1) / a.rc[0][k] : 0;
    const int ch1 = a.part[1][k] ? (*a.rows[1][k] + a.rc[1][k] - 1) / a.rc[1][k] : 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n[k]; i += (int64_t)gridDim.x * blockDim.x) {
      const float w = p[i];
      float g = adam_raw_grad(a, k, ch0, ch1, i);
      if constexpr (CLIP) {
        g *= coef;
        // (the product is rounded here, as torch's grad.mul_(coef) rounds it: the empty statement keeps the compiler from
        // contracting it into the decay's multiply-add, so coef = 1 gives the bits of the unclipped kernel)
        asm volatile("" : "+v"(g));
      }
      const float gr = g + a.wd * w;
      const float mm = m[i] + (gr - m[i]) * (1.f - a.beta1);
      const float vv = v[i] * a.beta2 + (1.f - a.beta2) * gr * gr;
      m[i] = mm;
      v[i] = vv;
      p[i] = w - step_size * (mm / (sqrtf(vv) / bc2s + a.eps));
    }
  }
}

// where a plan keeps its clipping state (gigl_nablp_train_plan_set_clip_grad_norm); max_norm 0: off
struct AdamClip {
  float max_norm = 0.f;
  double* partials = nullptr;  // [ADAM_MAX][ADAM_GRID_X_MAX]
  float* out2 = nullptr;       // {total_norm, coef} of the last trained step
};

// the optimiser's launches over `ap` on a (gx, ap.count) grid: Adam alone, or — clipping on — the norm pass and its
// finalising launch ahead of it
void launch_adam(hipStream_t st, unsigned gx, const AdamPack& ap, const int32_t* step_dev, const int32_t* meta_a,
                 const int32_t* meta_b, const int32_t* halt, const AdamClip* clip) {
  const dim3 grid(gx, (unsigned)ap.count);
  if (!clip || !(clip->max_norm > 0.f)) {
    hipLaunchKernelGGL(adam_kernel<false>, grid, dim3(256), 0, st, ap, step_dev, meta_a, meta_b, halt, (const float*)nullptr);
    return;
  }
  hipLaunchKernelGGL(grad_sqnorm_kernel, grid, dim3(256), 0, st, ap, meta_a, meta_b, halt, clip->partials);
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, st, (const double*)clip->partials, (int)(gx * ap.count),
                     clip->max_norm, meta_a, meta_b, halt, clip->out2);
  hipLaunchKernelGGL(adam_kernel<true>, grid, dim3(256), 0, st, ap, step_dev, meta_a, meta_b, halt, (const float*)clip->out2);
}

}  // namespace

extern "C" {

int32_t gigl_sage_plan_destroy(gigl_sage_plan* p) {
  if (!p) return GIGL_OK;
  if (p->ctx) {
    hipSetDevice(p->ctx->device);
    hipStreamSynchronize(p->ctx->stream);
  }
  if (p->gstream) hipStreamSynchronize(p->gstream);
  drop_graphs(p);
  if (p->ev_in) hipEventDestroy(p->ev_in);
  if (p->ev_graph) hipEventDestroy(p->ev_graph);
  batch_graph_free(p);
  delete p;
  return GIGL_OK;
}

static int32_t plan_create(gigl_ctx* ctx, gigl_graph* graph, gigl_feat* feat, int32_t b, const int32_t* fanouts,
                           int32_t hops, const int32_t* dims, const float* const* w, const float* const* bias,
                           int32_t act_last, bool with_abuf, gigl_sage_plan** out, bool number_every_node = false);
static int32_t plan_refresh_half_split(gigl_sage_plan* p);

int32_t gigl_sage_plan_create(gigl_ctx* ctx, gigl_graph* graph, gigl_feat* feat, int32_t b,
                              const int32_t* fanouts, int32_t hops, const int32_t* dims,
                              const float* const* w, const float* const* bias, int32_t act_last,
                              gigl_sage_plan** out) {
  return plan_create(ctx, graph, feat, b, fanouts, hops, dims, w, bias, act_last, true, out);
}

// what every plan's layers need of their shapes and parameters: widths >= 1 from the table's, no null weight
static int32_t plan_check_layers(gigl_ctx* ctx, const gigl_feat* feat, int32_t hops, const int32_t* dims, const float* const* w) {
  GIGL_REQUIRE(ctx, dims[0] == feat->d, "dims[0]=%d != feature dim %d", dims[0], feat->d);
  for (int k = 0; k < hops; ++k) GIGL_REQUIRE(ctx, w[k], "weight %d is null", k);
  for (int k = 0; k <= hops; ++k) GIGL_REQUIRE(ctx, dims[k] >= 1, "dims[%d]=%d", k, dims[k]);
  return GIGL_OK;
}

// with_abuf false: no [mean | self] operand buffer (the GAT plan aggregates into its own per-head operands, the GCN plan
// into plain rows); number_every_node: the generic union (the GCN plan)
static int32_t plan_create(gigl_ctx* ctx, gigl_graph* graph, gigl_feat* feat, int32_t b, const int32_t* fanouts,
                           int32_t hops, const int32_t* dims, const float* const* w, const float* const* bias,
                           int32_t act_last, bool with_abuf, gigl_sage_plan** out, bool number_every_node) {
  if (!ctx || !out) return GIGL_E_INVALID_ARG;
  *out = nullptr;
  GIGL_REQUIRE(ctx, graph && feat && fanouts && dims && w, "null argument");
  GIGL_REQUIRE(ctx, hops >= 1 && hops <= GIGL_MAX_HOPS && b >= 1, "bad plan shape");
  int32_t rc = plan_check_layers(ctx, feat, hops, dims, w);
  if (rc != GIGL_OK) return rc;
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  gigl_sage_plan* p = new (std::nothrow) gigl_sage_plan();
  if (!p) return gigl_fail(ctx, GIGL_E_OOM, "host OOM");
  rc = batch_graph_init(p, ctx, graph, b, fanouts, hops, number_every_node);
  if (rc != GIGL_OK) {
    gigl_sage_plan_destroy(p);
    return rc;
  }
  p->feat = feat;
  p->act_last = act_last;
  int32_t max_in = 0, max_out = 0;
  for (int k = 0; k < hops; ++k) {
    p->w[k] = w[k];
    p->bias[k] = bias ? bias[k] : nullptr;
  }
  for (int k = 0; k <= hops; ++k) {
    p->dims[k] = dims[k];
    if (k < hops && dims[k] > max_in) max_in = dims[k];
    if (k > 0 && dims[k] > max_out) max_out = dims[k];
  }
  auto alloc = [&](size_t bytes) { return plan_alloc(p->owned, bytes); };
  bool ok = true;
  p->tiled = true;
  p->two_source = getenv("GIGL_PLAN_SELF_COPY") == nullptr;  // (A/B knob: set = gather writes [mean | self])
  for (int k = 0; k < hops; ++k)
    if ((dims[k] & 3) != 0 || dims[k] > 2048) p->tiled = false;
  if (with_abuf) {
    const size_t row_tiles = ((size_t)p->act_rows + 127) / 128, nkc = ((size_t)2 * max_in + 31) / 32;
    p->abuf = (float*)alloc(p->tiled ? row_tiles * nkc * 4096 * 4 : (size_t)p->act_rows * 2 * max_in * 4);
  }
  p->hbuf[0] = (float*)alloc((size_t)p->act_rows * max_out * 4);
  p->hbuf[1] = hops > 1 ? (float*)alloc((size_t)p->act_rows * max_out * 4) : p->hbuf[0];
  p->out_buf = (float*)alloc((size_t)b * dims[hops] * 4);
  p->hs_dev = reinterpret_cast<float*>(p->zero_dev + 4);  // [4..7): the scales, [8..10): their running maximum + ticket (zero)
  for (int k = 1; k < hops && with_abuf; ++k) {
    p->hs_layer[k] = (float*)alloc(64);
    ok = ok && p->hs_layer[k] && hipMemset(p->hs_layer[k], 0, 64) == hipSuccess;
  }
  if (with_abuf && hops == 2 && gigl_fused2_shape_ok(dims[0], dims[1], dims[2]) && getenv("GIGL_PLAN_NO_FUSE2") == nullptr &&
      (int64_t)max_out >= 2 * gigl_fused2_row_floats()) {
    p->f2_dev = (float*)alloc(64);
    p->w2h = alloc((size_t)gigl_fused2_w2h_bytes(2 * dims[0]));
    p->f2_ok = p->f2_dev && p->w2h && hipMemset(p->f2_dev, 0, 64) == hipSuccess;
    ok = ok && p->f2_ok;
  }
  ok = ok && (p->abuf || !with_abuf) && p->hbuf[0] && p->hbuf[1] && p->out_buf;
  if (!ok) {
    gigl_sage_plan_destroy(p);
    return gigl_fail(ctx, GIGL_E_OOM, "hipMalloc of the batch workspace failed (cap_nodes=%lld)",
                     (long long)p->un.cap_nodes);
  }
  {
    const int32_t rc_hs = plan_refresh_half_split(p);
    if (rc_hs != GIGL_OK) {
      gigl_sage_plan_destroy(p);
      return rc_hs;
    }
  }
  plan_build_steps(p);
  *out = p;
  return GIGL_OK;
}

int32_t gigl_gat_plan_create(gigl_ctx* ctx, gigl_graph* graph, gigl_feat* feat, int32_t b, const int32_t* fanouts,
                             int32_t hops, const int32_t* heads, const int32_t* channels, const float* const* w,
                             const float* const* att_src, const float* const* att_dst, const float* const* bias,
                             float negative_slope, int32_t act_last, gigl_sage_plan** out) {
  if (!ctx || !out) return GIGL_E_INVALID_ARG;
  *out = nullptr;
  GIGL_REQUIRE(ctx, graph && feat && fanouts && heads && channels && w && att_src && att_dst, "null argument");
  GIGL_REQUIRE(ctx, hops >= 1 && hops <= GIGL_MAX_HOPS && b >= 1, "bad plan shape");
  int32_t dims[GIGL_MAX_HOPS + 1];
  dims[0] = feat->d;
  int32_t max_h = 1, max_hc = 1;
  for (int l = 0; l < hops; ++l) {
    GIGL_REQUIRE(ctx, heads[l] >= 1 && channels[l] >= 1 && att_src[l] && att_dst[l], "layer %d: bad heads / channels", l);
    dims[l + 1] = heads[l] * channels[l];
    if (heads[l] > max_h) max_h = heads[l];
    if (dims[l + 1] > max_hc) max_hc = dims[l + 1];
  }
  const int P = (feat->d + 255) / 256;
  if ((feat->d & 3) || (heads[0] != 1 && heads[0] != 2 && heads[0] != 4) || P > 4 ||
      (feat->dtype != GIGL_DTYPE_F32 && feat->dtype != GIGL_DTYPE_F16))
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "GAT plan: feature dim %d / %d heads outside the shapes the first layer is "
                     "built for (gigl_gat_input_layer_fused)", feat->d, heads[0]);
  gigl_sage_plan* p = nullptr;
  int32_t rc = plan_create(ctx, graph, feat, b, fanouts, hops, dims, w, bias, act_last, false, &p);
  if (rc != GIGL_OK) return rc;
  p->kind = 1;
  p->slope = negative_slope;
  for (int l = 0; l < hops; ++l) {
    p->heads[l] = heads[l];
    p->channels[l] = channels[l];
    p->att_src[l] = att_src[l];
    p->att_dst[l] = att_dst[l];
  }
  auto alloc = [&](size_t bytes) { return plan_alloc(p->owned, bytes); };
  p->gat_scratch = (float*)alloc((size_t)gigl_gat_input_layer_fused_scratch(feat->d, heads[0], p->act_rows) * 4);
  p->alpha_scratch = (float*)alloc((size_t)2 * p->act_rows * max_h * 4);
  p->hw = (float*)alloc((size_t)p->act_rows * max_hc * 4);
  if (!p->gat_scratch || !p->alpha_scratch || !p->hw) {
    gigl_sage_plan_destroy(p);
    return gigl_fail(ctx, GIGL_E_OOM, "hipMalloc of the GAT plan's workspace failed");
  }
  rc = plan_refresh_half_split(p);
  if (rc != GIGL_OK) {
    gigl_sage_plan_destroy(p);
    return rc;
  }
  plan_build_steps(p);  // (the list plan_create left is a SAGE plan's)
  *out = p;
  return GIGL_OK;
}

int32_t gigl_gat_plan_set_weights(gigl_sage_plan* p, const float* const* w, const float* const* att_src,
                                  const float* const* att_dst, const float* const* bias) {
  if (!p || !w || !att_src || !att_dst || p->kind != 1) return GIGL_E_INVALID_ARG;
  for (int l = 0; l < p->hops; ++l) {
    GIGL_REQUIRE(p->ctx, w[l] && att_src[l] && att_dst[l], "layer %d: null weight", l);
    p->w[l] = w[l];
    p->att_src[l] = att_src[l];
    p->att_dst[l] = att_dst[l];
    p->bias[l] = bias ? bias[l] : nullptr;
  }
  plan_invalidate(p);  // (weight pointers are baked into the captured kernels)
  return plan_refresh_half_split(p);
}

int32_t gigl_gat_plan_set_edge_features(gigl_sage_plan* p, gigl_feat* edge_table, const float* const* att_edge_folded,
                                        const float* const* w_edge_msg) {
  if (!p) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = p->ctx;
  GIGL_REQUIRE(ctx, p->kind == 1, "edge features apply to GAT plans (gigl_gat_plan_create)");
  GIGL_REQUIRE(ctx, edge_table && att_edge_folded, "null argument");
  GIGL_REQUIRE(ctx, edge_table->dtype == GIGL_DTYPE_F32 && edge_table->n == p->graph->e,
               "the edge table holds one fp32 row per resident edge (%lld rows, %lld edges)", (long long)edge_table->n,
               (long long)p->graph->e);
  const int32_t De = edge_table->d;
  if (De < 1 || De > 64)  // (the first layer keeps one lane per component of an edge row: gigl_gat_input_layer_fused)
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "GAT plan: edge_dim %d outside [1,64]", De);
  for (int l = 0; l < p->hops; ++l) GIGL_REQUIRE(ctx, att_edge_folded[l], "layer %d: null folded att_edge", l);
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  plan_invalidate(p);  // (the pointers are baked into the captured kernels)
  auto alloc = [&](size_t bytes) { return plan_alloc(p->owned, bytes); };
  int32_t max_h = 1;
  for (int l = 0; l < p->hops; ++l) max_h = p->heads[l] > max_h ? p->heads[l] : max_h;
  if (!p->eid) {  // the first table: alpha_scratch grows by the edges' logits (sized once, the plan is captured)
    GIGL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (alpha_scratch is replaced: no launch may still use it)
    float* alpha = (float*)alloc((size_t)(2 * p->act_rows + p->col_positions) * max_h * 4);
    if (!alpha) return gigl_fail(ctx, GIGL_E_OOM, "hipMalloc of the GAT plan's edge workspace failed");
    p->alpha_scratch = alpha;
  }
  const size_t ze_floats = (size_t)p->act_rows * p->heads[0] * 64;
  if (w_edge_msg && w_edge_msg[0] && !p->ze) {
    p->ze = (float*)alloc(ze_floats * 4);
    if (!p->ze) return gigl_fail(ctx, GIGL_E_OOM, "hipMalloc of the GAT plan's edge workspace failed");
  }
  for (int l = 0; l < p->hops; ++l) {
    p->att_edge[l] = att_edge_folded[l];
    p->w_msg[l] = w_edge_msg ? w_edge_msg[l] : nullptr;
  }
  return batch_graph_attach_edge_table(p, edge_table);
}

int32_t gigl_gcn_plan_create(gigl_ctx* ctx, gigl_graph* graph, gigl_feat* feat, int32_t b, const int32_t* fanouts,
                             const int32_t* dims, const float* const* w, const float* const* bias, gigl_sage_plan** out) {
  if (!ctx || !out) return GIGL_E_INVALID_ARG;
  *out = nullptr;
  GIGL_REQUIRE(ctx, feat && (feat->dtype == GIGL_DTYPE_F32 || feat->dtype == GIGL_DTYPE_F16), "bad feature table");
  gigl_sage_plan* p = nullptr;
  int32_t rc = plan_create(ctx, graph, feat, b, fanouts, 2, dims, w, bias, 0, false, &p, true);
  if (rc != GIGL_OK) return rc;
  p->kind = 2;
  const int32_t widest = dims[0] > dims[1] ? dims[0] : dims[1];
  p->dinv = (float*)plan_alloc(p->owned, (size_t)p->un.cap_nodes * 4);
  p->gcn_a = (float*)plan_alloc(p->owned, (size_t)p->act_rows * widest * 4);
  if (!p->dinv || !p->gcn_a) {
    gigl_sage_plan_destroy(p);
    return gigl_fail(ctx, GIGL_E_OOM, "hipMalloc of the GCN plan's workspace failed");
  }
  plan_build_steps(p);  // (the list plan_create left is a SAGE plan's)
  *out = p;
  return GIGL_OK;
}

int32_t gigl_gcn_plan_set_weights(gigl_sage_plan* p, const float* const* w, const float* const* bias) {
  if (!p || !w || p->kind != 2) return GIGL_E_INVALID_ARG;
  for (int l = 0; l < 2; ++l) {
    GIGL_REQUIRE(p->ctx, w[l], "layer %d: null weight", l);
    p->w[l] = w[l];
    p->bias[l] = bias ? bias[l] : nullptr;
  }
  plan_invalidate(p);  // (weight pointers are baked into the captured kernels; W2's alignment decides the fused root layer)
  return GIGL_OK;
}

int32_t gigl_gcn_plan_set_projected_input(gigl_sage_plan* p, const float* proj) {
  if (!p || p->kind != 2) return GIGL_E_INVALID_ARG;
  const bool changed = p->proj != proj;
  p->proj = proj;
  if (changed) plan_invalidate(p);  // (the pointer is baked into the captured launches)
  return GIGL_OK;
}

int32_t gigl_gcn_plan_set_fused_root(gigl_sage_plan* p, int32_t on) {
  if (!p || p->kind != 2) return GIGL_E_INVALID_ARG;
  const bool changed = p->gcn_fuse_want != (on != 0);
  p->gcn_fuse_want = on != 0;
  if (changed) plan_invalidate(p);
  return GIGL_OK;
}

int32_t gigl_gcn_plan_fused_root(gigl_sage_plan* p) { return p && p->kind == 2 && p->gcn_fused ? 1 : 0; }

int32_t gigl_sage_plan_set_l2_normalize(gigl_sage_plan* p, int32_t on) {
  if (!p) return GIGL_E_INVALID_ARG;
  p->l2_normalize = on != 0;  // (the step that writes `out` runs eagerly: no captured graph holds the decision)
  return GIGL_OK;
}

// The first layer's operands are rows of the feature table reduced by mean / max (|.| <= the table's largest magnitude),
// by sum (<= fan-out times it) or by softmax weights (GAT: convex combinations), and the layer's weights.  The layer's
// projection runs over two fp16 planes per operand, each operand multiplied by a power of two that puts its largest
// magnitude into [2^14, 2^15) (undone in the epilogue; all exact): the table's factor is fixed here from the table's
// cached largest magnitude — or the table keeps the layer on the bf16 planes, see gigl_feat_half_split_scale — and the
// weights' factor is found on the device at every run.  Nothing here looks at the weights or synchronises (beyond the
// table's first look), so trainers may call _set_weights every step, also inside a capture.
static int32_t plan_refresh_half_split(gigl_sage_plan* p) {
  const bool before = p->hs0;
  const float sa_before = p->hs_sa;
  p->hs0 = false;
  p->hs_sa = 0.f;
  const bool gat = p->kind == 1 && p->gat_scratch;
  const bool sage = p->kind == 0 && p->tiled && p->abuf;  // (SAGE plans own abuf)
  if ((gat || sage) && p->feat && p->w[0] && p->hs_dev) {
    // (mean, max and softmax weights stay inside the table's range.  A SUM does not, and no fan-out bounds it: a union row
    // merges the samples of every occurrence of its node — each sampled with its own hash key — up to the node's whole
    // in-row.  The summed half is measured on the device at every run instead: gigl_tiled_absmax in step_sage_project.)
    const float fan = 1.f;
    const int32_t rc = gigl_feat_half_split_scale(p->ctx, p->feat, fan, &p->hs_sa);
    if (rc != GIGL_OK) return rc;
    p->hs0 = p->hs_sa > 0.f;
  }
  if (before != p->hs0 || sa_before != p->hs_sa) plan_invalidate(p);
  return GIGL_OK;
}

int32_t gigl_sage_plan_set_weights(gigl_sage_plan* p, const float* const* w, const float* const* bias) {
  if (!p || !w) return GIGL_E_INVALID_ARG;
  for (int k = 0; k < p->hops; ++k) {
    if (!w[k]) return gigl_fail(p->ctx, GIGL_E_INVALID_ARG, "weight %d is null", k);
    p->w[k] = w[k];
    p->bias[k] = bias ? bias[k] : nullptr;
  }
  plan_invalidate(p);  // (weight pointers are baked into the captured kernels)
  return plan_refresh_half_split(p);
}

int32_t gigl_sage_plan_half_split(gigl_sage_plan* p) { return p && p->hs0 ? 1 : 0; }

int32_t gigl_sage_plan_fused_layers(gigl_sage_plan* p) { return p && p->fused2 ? 1 : 0; }

int32_t gigl_sage_plan_set_aggr(gigl_sage_plan* p, int32_t aggr) {
  if (!p) return GIGL_E_INVALID_ARG;
  GIGL_REQUIRE(p->ctx, aggr == GIGL_AGGR_MEAN || aggr == GIGL_AGGR_SUM || aggr == GIGL_AGGR_MAX, "bad aggr %d", aggr);
  GIGL_REQUIRE(p->ctx, p->kind == 0, "the reduction applies to SAGE layers");
  const bool changed = p->aggr != aggr;
  p->aggr = aggr;
  if (changed) plan_invalidate(p);  // (the reduction is baked into the captured launches)
  return plan_refresh_half_split(p);  // (a sum's operand is bounded by fan-out times the table's largest magnitude)
}

int32_t gigl_sage_plan_set_projected_input(gigl_sage_plan* p, const float* proj) {
  if (!p) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = p->ctx;
  GIGL_REQUIRE(ctx, p->kind == 0, "projected input applies to SAGE plans");
  if (proj) {
    GIGL_REQUIRE(ctx, p->aggr == GIGL_AGGR_MEAN || p->aggr == GIGL_AGGR_SUM,
                 "projected input needs a linear reduction: lin(max_j x_j) != max_j lin(x_j)");
    GIGL_REQUIRE(ctx, (p->dims[1] & 3) == 0 && p->dims[1] <= 2048, "projected input: first-layer width %d", p->dims[1]);
  }
  const bool changed = p->proj != proj;
  p->proj = proj;
  if (changed) plan_invalidate(p);  // (the pointer is baked into the captured launches)
  return GIGL_OK;
}

int32_t gigl_sage_plan_set_groups(gigl_sage_plan* p, int32_t group_roots) {
  if (!p) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = p->ctx;
  GIGL_REQUIRE(ctx, group_roots >= 1 && p->b % group_roots == 0, "group_roots=%d does not divide the plan's b=%d",
               group_roots, p->b);
  p->group_roots = group_roots;
  plan_invalidate(p);  // (the group split is baked into the captured kernels)
  return GIGL_OK;
}

int32_t gigl_sage_plan_buffers(gigl_sage_plan* p, gigl_tree* tree, gigl_union* un) {
  if (!p) return GIGL_E_INVALID_ARG;
  if (tree) *tree = p->tree;
  if (un) {
    *un = p->un;
    un->cap_edges = p->col_positions;  // rowptr / rowend may point into the aliased tree segments
  }
  return GIGL_OK;
}

int32_t gigl_sage_plan_stats(gigl_sage_plan* p, const uint32_t* roots, int64_t* acc) {
  if (!p) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = p->ctx;
  GIGL_REQUIRE(ctx, roots && acc, "null argument");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  StatsArgs a{};
  a.roots = roots;
  a.hops = p->hops;
  int64_t parents = p->b, most = p->b;
  for (int k = 0; k < p->hops; ++k) {
    a.nbr[k] = p->tree.nbr[k];
    a.cnt[k] = p->tree.cnt[k];
    a.fan[k] = p->fanouts[k];
    a.parents[k] = parents;
    if (parents > most) most = parents;
    parents *= p->fanouts[k];
  }
  a.g_rowptr = p->graph->rowptr;
  a.meta = p->un.meta;
  a.rowptr = p->un.rowptr;
  a.rowend = p->un.rowend;
  a.rows_cap = p->un.cap_nodes;
  int64_t blocks = (most + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(plan_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, a, (unsigned long long*)acc);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_sage_plan_overflow_add(gigl_sage_plan* p, int32_t* acc) {
  if (!p) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = p->ctx;
  GIGL_REQUIRE(ctx, acc, "null argument");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(overflow_add_kernel, dim3(1), dim3(64), 0, ctx->stream, p->un.meta, acc);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_sage_plan_use_graph(gigl_sage_plan* p, int32_t on) {
  if (!p) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = p->ctx;
  if (on && ctx->stream == nullptr)
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED,
                     "hipGraph replay needs a non-default stream (the legacy default stream cannot be captured): "
                     "bind the ctx to a created stream first (gigl_ctx_set_stream)");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  GIGL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  drop_graphs(p);
  p->use_graph = on != 0;
  return GIGL_OK;
}

int32_t gigl_sage_plan_flush_profile(gigl_sage_plan* p) {
  if (!p) return GIGL_E_INVALID_ARG;
  GIGL_HIP_CHECK(p->ctx, hipStreamSynchronize(p->ctx->stream));
  return GIGL_OK;
}

int32_t gigl_sage_plan_run_part(gigl_sage_plan* p, const uint32_t* roots, int32_t sampling_seed, int32_t mode,
                                float* out, int32_t part) {
  if (!p) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = p->ctx;
  GIGL_REQUIRE(ctx, roots && out && (part == GIGL_PLAN_PART_GRAPH || part == GIGL_PLAN_PART_LAYERS), "bad argument");
  if (mode == GIGL_MODE_REPLACE)
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "the one-call plan needs duplicate-free trees (no with-replacement mode)");
  const RunArgs a{roots, sampling_seed, mode, out};
  return part == GIGL_PLAN_PART_GRAPH ? run_steps(p, 0, p->graph_steps, a) : run_steps(p, p->graph_steps, p->n_steps, a);
}

int32_t gigl_sage_plan_run(gigl_sage_plan* p, const uint32_t* roots, int32_t sampling_seed, int32_t mode,
                           float* out) {
  if (!p) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = p->ctx;
  GIGL_REQUIRE(ctx, roots && out, "null argument");
  if (mode == GIGL_MODE_REPLACE)
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "the one-call plan needs duplicate-free trees (no with-replacement mode)");
  if (!p->use_graph) return run_steps(p, 0, p->n_steps, {roots, sampling_seed, mode, out});

  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // (another plan on this ctx may have grown — reallocated — the arena since the capture: the graphs' scratch addresses
  // are then stale)
  if (!p->captured || p->cap_mode != mode || p->cap_seed != sampling_seed || p->cap_prof_mask != ctx->prof_mask ||
      p->cap_arena_gen != ctx->arena_gen) {
    GIGL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    drop_graphs(p);
    // one eager run first: sizes the arena, builds the hash threshold table, sets kernel attributes — none of
    // which may happen inside a capture.  (This batch is produced by that run.)
    const uint32_t keep_mask = ctx->prof_mask;
    ctx->prof_mask = 0;
    int32_t rc = run_steps(p, 0, p->n_steps, {roots, sampling_seed, mode, out});
    ctx->prof_mask = keep_mask;
    if (rc != GIGL_OK) return rc;
    GIGL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    rc = capture_segments(p, sampling_seed, mode);
    if (rc != GIGL_OK) {
      drop_graphs(p);
      return rc;
    }
    p->captured = true;
    p->cap_mode = mode;
    p->cap_seed = sampling_seed;
    p->cap_prof_mask = ctx->prof_mask;
    p->cap_arena_gen = ctx->arena_gen;
    return GIGL_OK;
  }
  // A split plan runs its graph part on the plan's graph stream: behind whatever produced `roots` on the ctx stream, and
  // behind the layers of the previous call (they read the union graph this call's graph part rewrites).  Without a graph
  // stream the graph part's stream is the ctx stream, and nothing has to wait
  hipStream_t cs = ctx->stream, gs = p->split ? p->gstream : cs;
  if (p->split) {
    GIGL_HIP_CHECK(ctx, hipEventRecord(p->ev_in, cs));
    GIGL_HIP_CHECK(ctx, hipStreamWaitEvent(gs, p->ev_in, 0));
  }
  GIGL_HIP_CHECK(ctx, hipMemcpyAsync(p->roots_buf, roots, (size_t)p->b * 4, hipMemcpyDeviceToDevice, gs));
  bool joined = !p->split;
  for (int i = 0; i < p->n_segs; ++i) {
    const Segment& sg = p->segs[i];
    const bool gpart = sg.s1 <= p->graph_steps;
    if (!gpart && !joined) {  // the layers wait for the graph part
      GIGL_HIP_CHECK(ctx, hipEventRecord(p->ev_graph, gs));
      GIGL_HIP_CHECK(ctx, hipStreamWaitEvent(cs, p->ev_graph, 0));
      joined = true;
    }
    StreamScope on(ctx, gpart ? gs : cs);
    if (sg.exec) {
      GIGL_HIP_CHECK(ctx, hipGraphLaunch(sg.exec, ctx->stream));
    } else {
      const int32_t rc = run_steps(p, sg.s0, sg.s1, {p->roots_buf, sampling_seed, mode, out});
      if (rc != GIGL_OK) return rc;
    }
  }
  return GIGL_OK;
}

int32_t gigl_sage_plan_set_graph_stream(gigl_sage_plan* p, void* hip_stream, int32_t on) {
  if (!p) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = p->ctx;
  GIGL_REQUIRE(ctx, !on || hip_stream, "the graph part needs a created stream of its own");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  GIGL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (p->gstream) GIGL_HIP_CHECK(ctx, hipStreamSynchronize(p->gstream));
  drop_graphs(p);
  if (on && !p->ev_in) {
    if (hipEventCreateWithFlags(&p->ev_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev_graph, hipEventDisableTiming) != hipSuccess)
      return gigl_fail(ctx, GIGL_E_HIP, "hipEventCreate failed");
  }
  p->gstream = on ? (hipStream_t)hip_stream : nullptr;
  p->split = on != 0;
  return GIGL_OK;
}


// ---- gigl_sage_train_plan: one TRAINING step per call, all of it in the library —
//   sample -> batch union graph (the one-call plan's leaf-global build) -> GraphSAGE forward keeping every layer's
//   operand and output -> cross-entropy on the roots -> backward (weight gradients as gigl_linear_weight_grad_parts'
//   partial sums, the layers' input gradients by one projection over the transposed weights + the mean's backward) -> Adam,
//   which adds the partial sums up.
// Replaces the loop body of NodeClassificationModelingTaskSpec._train
// (python/gigl/src/common/modeling_task_specs/node_classification_modeling_task_spec.py:134-173) for batches sampled in
// HBM: ~25 launches and two memsets, no torch kernel between them, replayed from hipGraphs.
// The step has two parts.  The GRAPH part (sample + union) does not depend on the weights: it runs on a ctx and stream of
// the plan's own, into one of two workspaces, and a step that is told the NEXT batch (roots_next) starts that batch's graph part while the
// LAYERS part (forward, loss, backward, Adam: the caller's ctx and stream) of the current batch runs — a training step
// is a chain of small launches (one batch: the weights change between batches), so the two chains share the GPU well.
// graph workspaces of the training plan: the current batch + the next.  (Three — two batches ahead, two graph parts in
// flight on streams of their own — was measured: 0.266 against 0.245 ms/step; the second graph part takes more from the
// layers than it hides.  roots_next2 of _step2 is then not used.  Also measured: the first layer's aggregation — it
// depends on no weight — moved into the graph part, out of the layers' serial chain: 0.257 against 0.245 ms/step; the
// two parts already share the GPU, the step follows the SUM of the launches more than the longer chain.)
constexpr int TRAIN_WS = 3;
// the input gradient of layers >= 1 by gigl_gather_mean_backward_transposed (every row written once, no cleared block, no
// float atomics) when the hidden widths allow float4 rows
static bool train_bwd_gather(const int32_t* dims, int32_t hops) {
  for (int l = 1; l < hops; ++l)
    if (dims[l] & 3) return false;
  return true;
}

// ---- the GraphSAGE training encoder, written once: the node-classification plan runs one encode per step, the
// link-prediction plan two (main batch, random negatives) over the SHARED weights

// what the encodes of a plan share: the layers' shapes, the parameters, Adam's state
struct SageTrainShared {
  gigl_feat* feat = nullptr;  // the node features every encode's first layer gathers
  int32_t L = 0, act_last = 0;
  int32_t dims[GIGL_MAX_HOPS + 1] = {0};
  float* w[GIGL_MAX_HOPS] = {nullptr};  // fused [dims[l+1]][2 dims[l]]: borrowed, UPDATED IN PLACE
  float* bias[GIGL_MAX_HOPS] = {nullptr};
  float* mom[4 * GIGL_MAX_HOPS] = {nullptr};  // m_w, v_w, m_b, v_b per layer
  // W_l^T of layers >= 1 (the backward's da = dh . W needs it as the projection's weight operand), laid out ONCE per step
  float* wt_l[GIGL_MAX_HOPS] = {nullptr};
  bool bwd_gather = false;  // layers >= 1 hand their input gradient down by the transposed gather (train_bwd_gather)
  float lr = 0.f, beta1 = 0.9f, beta2 = 0.999f, eps = 1e-8f, wd = 0.f;
  // dropout after every activated layer (gigl_*_train_plan_set_dropout; 0: none, the launches of a plan without it)
  float drop_p = 0.f;
  uint64_t drop_seed = 0;
};

// one encode's state
struct SageTrainEnc {
  BatchGraph* base = nullptr;      // (link-prediction plans) batch graph of this encode's roots, set per step
  int32_t b = 0;                   // roots
  int64_t rows_cap[GIGL_MAX_HOPS] = {0};  // rows layer l may compute
  float* a[GIGL_MAX_HOPS] = {nullptr};    // [rows_cap[l]][2 dims[l]]: the layer's [mean | self] operand
  float* h[GIGL_MAX_HOPS] = {nullptr};    // [rows_cap[l]][dims[l+1]]: its output (activated below the last layer)
  float* dh[GIGL_MAX_HOPS] = {nullptr};   // gradient of h[l]
  // the weight gradients' per-chunk partial sums: added up inside the Adam kernel, no reduce launch per layer
  float* part_w[GIGL_MAX_HOPS] = {nullptr};
  float* part_b[GIGL_MAX_HOPS] = {nullptr};
  int32_t part_rc[GIGL_MAX_HOPS] = {0};
  // the gradients themselves, where a plan hands them out (gigl_nablp_train_plan_grads adds the partial sums up on demand)
  float* gw[GIGL_MAX_HOPS] = {nullptr};
  float* gb[GIGL_MAX_HOPS] = {nullptr};
  float* emb = nullptr;  // (link prediction) [b][d_out]: the roots' embeddings (normalised when the model says so)
  float* inv = nullptr;  // (link prediction) [b]: 1 / max(|h_r|, 1e-12) (1 without normalisation; 0: no such root)
};

namespace {

// the shapes and parameters (s.L is set), Adam's moments (zero) and the W_l^T buffers
bool sage_shared_alloc(SageTrainShared& s, std::vector<void*>& owned, const int32_t* dims, float* const* w, float* const* bias) {
  bool ok = true;
  for (int l = 0; l <= s.L; ++l) s.dims[l] = dims[l];
  s.bwd_gather = train_bwd_gather(dims, s.L);
  for (int l = 0; l < s.L; ++l) {
    s.w[l] = w[l];
    s.bias[l] = bias ? bias[l] : nullptr;
    const size_t nw = (size_t)dims[l + 1] * 2 * dims[l];
    for (int k = 0; k < 4; ++k) {
      const size_t n = k < 2 ? nw : (size_t)dims[l + 1];
      s.mom[4 * l + k] = (float*)plan_alloc(owned, n * 4);
      ok = ok && s.mom[4 * l + k] && hipMemset(s.mom[4 * l + k], 0, n * 4) == hipSuccess;
    }
    if (l >= 1) {
      s.wt_l[l] = (float*)plan_alloc(owned, nw * 4);
      ok = ok && s.wt_l[l];
    }
  }
  return ok;
}

// (the input gradient of a layer below the last is written whole by the transposed gather: not part of a cleared block)
bool sage_dh_cleared(const SageTrainShared& s, int l) { return !(s.bwd_gather && l < s.L - 1); }

// one encode's buffers for its e.b roots.  Its share of the plan's cleared block — the dh rows that are ADDED to, and with
// `grads` gw | gb — is counted into *zero_floats and handed out by sage_enc_carve once the block exists; *da_floats
// grows to the operand-gradient scratch its backward needs
bool sage_enc_alloc(const SageTrainShared& s, SageTrainEnc& e, std::vector<void*>& owned, bool wide, const int32_t* fanouts,
                    bool grads, size_t* zero_floats, size_t* da_floats) {
  bool ok = true;
  for (int l = 0; l < s.L; ++l) {
    const int n_out = s.dims[l + 1], k2 = 2 * s.dims[l];
    const int64_t rows = gigl_level_rows(wide, e.b, fanouts, s.L, s.L - 1 - l);  // layer l computes the nodes of level <= L-1-l
    e.rows_cap[l] = rows;
    if (grads) *zero_floats += (size_t)n_out * k2 + n_out;
    if (l >= 1) *da_floats = std::max(*da_floats, (size_t)rows * k2);
    e.a[l] = (float*)plan_alloc(owned, (size_t)rows * k2 * 4);
    e.h[l] = (float*)plan_alloc(owned, (size_t)rows * n_out * 4);
    if (sage_dh_cleared(s, l)) {
      *zero_floats += (size_t)rows * n_out;
    } else {
      e.dh[l] = (float*)plan_alloc(owned, (size_t)rows * n_out * 4);
      ok = ok && e.dh[l];
    }
    const int64_t chunks = gigl_linear_weight_grad_chunks(rows, n_out, k2, &e.part_rc[l]);
    e.part_w[l] = (float*)plan_alloc(owned, (size_t)chunks * n_out * k2 * 4);
    e.part_b[l] = (float*)plan_alloc(owned, (size_t)chunks * n_out * 4);
    ok = ok && e.a[l] && e.h[l] && e.part_w[l] && e.part_b[l];
  }
  return ok;
}

// the encode's share of the cleared block at z, per layer gw | gb | dh -> the end of the share
float* sage_enc_carve(const SageTrainShared& s, SageTrainEnc& e, bool grads, float* z) {
  for (int l = 0; l < s.L; ++l) {
    if (grads) {
      e.gw[l] = z;
      z += (size_t)s.dims[l + 1] * 2 * s.dims[l];
      e.gb[l] = z;
      z += s.dims[l + 1];
    }
    if (sage_dh_cleared(s, l)) {
      e.dh[l] = z;
      z += (size_t)e.rows_cap[l] * s.dims[l + 1];
    }
  }
  return z;
}

// the transposed lists of layers >= 1 for one workspace (cap_edges: its union graph's) of the encode
bool sage_tlists_alloc(const SageTrainShared& s, const SageTrainEnc& e, std::vector<void*>& owned, int64_t cap_edges, int32_t** tl) {
  for (int l = 1; l < s.L && s.bwd_gather; ++l) {
    tl[l] = (int32_t*)plan_alloc(owned, (size_t)gigl_transposed_rows_words(e.rows_cap[l - 1], cap_edges) * 4);
    if (!tl[l]) return false;
  }
  return true;
}

// the graph part of one root set, on workspace p's ctx: sample + union (+ the level guard, the edge ids) ...
int32_t sage_enqueue_graph(const SageTrainShared& s, const SageTrainEnc& e, BatchGraph* p, int32_t* const* tl,
                           int32_t sampling_seed, int32_t mode) {
  int32_t rc = batch_graph_enqueue(p, sampling_seed, mode);
  // ... and who reads which source row in the backward of layers >= 1 (a function of the batch graph alone)
  for (int l = 1; l < s.L && rc == GIGL_OK && s.bwd_gather; ++l)
    rc = gigl_transposed_rows_build(p->ctx, p->un.rowptr, p->un.rowend, p->un.col, p->un.meta + GIGL_META_LEVEL0 + (s.L - 1 - l),
                                    e.rows_cap[l], p->un.meta + GIGL_META_LEVEL0 + (s.L - l), e.rows_cap[l - 1], p->un.cap_edges,
                                    tl[l]);
  return rc;
}

// launch blocks of 256 lanes over n items, a grid-stride loop beyond 4096 of them
unsigned blocks_256(int64_t n) {
  const int64_t blocks = (n + 255) / 256;
  return (unsigned)(blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks));
}

// lanes per row of the dropout kernels, as a power of two: the row's Philox blocks (four columns each) rounded up
int dropout_lanes_log2(int width) {
  int lg = 0;
  while ((1 << lg) < (width + 3) / 4) ++lg;
  return lg;
}

// forward over workspace p's batch graph, on ctx: every layer's operand a[l] and output h[l] are kept.  train: a training
// step's forward — with s.drop_p > 0 every activated output is masked and scaled in place (dropout_rows_kernel: the mask of
// this `encode` at the step *step_dev counts); an evaluation's forward (train == false) runs without
int32_t sage_enc_forward(gigl_ctx* ctx, const SageTrainShared& s, const SageTrainEnc& e, const BatchGraph* p, bool train,
                         int encode, const int32_t* step_dev) {
  const int L = s.L;
  int32_t rc = GIGL_OK;
  const int32_t* n_local = first_global_row(p);
  for (int l = 0; l < L; ++l) {
    const int32_t* n_rows = p->un.meta + GIGL_META_LEVEL0 + (L - 1 - l);
    const int d = s.dims[l];
    if (l == 0)
      rc = gigl_gather_reduce_mixed(ctx, s.feat->rows, s.feat->dtype, d, p->un.nodes, p->un.rowptr, p->un.rowend, p->un.col,
                                    n_rows, e.rows_cap[0], GIGL_AGGR_MEAN, n_local, e.a[0]);
    else
      rc = gigl_gather_reduce(ctx, e.h[l - 1], GIGL_DTYPE_F32, d, nullptr, p->un.rowptr, p->un.rowend, p->un.col, n_rows,
                              e.rows_cap[l], GIGL_AGGR_MEAN, e.a[l]);
    if (rc != GIGL_OK) return rc;
    rc = gigl_linear(ctx, e.a[l], s.w[l], s.bias[l], n_rows, e.rows_cap[l], 2 * d, s.dims[l + 1],
                     (l < L - 1 || s.act_last) ? 1 : 0, e.h[l]);
    if (rc != GIGL_OK) return rc;
    if (train && s.drop_p > 0.f && (l < L - 1 || s.act_last)) {
      const int width = s.dims[l + 1];
      const int lg = dropout_lanes_log2(width);
      hipLaunchKernelGGL(dropout_rows_kernel, dim3(blocks_256(e.rows_cap[l] << lg)), dim3(256), 0, ctx->stream, e.h[l], n_rows,
                         e.rows_cap[l], width, step_dev, gigl_dropout_mask_args(s.drop_seed, s.drop_p, encode, l), lg);
      GIGL_HIP_CHECK(ctx, hipGetLastError());
    }
  }
  return GIGL_OK;
}

// backward from dh[L - 1] down, on ctx: the weight gradients as partial sums (part_w / part_b: Adam adds them up), the
// layers' input gradients by one projection over W_l^T (s.wt_l, laid out before) into `da` + the mean's backward over
// workspace p's batch graph (tl: its transposed lists).  wctx != NULL: the weight gradients run on that ctx's stream
// beside the chain, each behind ev_w (nothing in the chain waits for them; the caller joins wctx before Adam)
int32_t sage_enc_backward(gigl_ctx* ctx, const SageTrainShared& s, const SageTrainEnc& e, const BatchGraph* p,
                          int32_t* const* tl, float* da, gigl_ctx* wctx, hipEvent_t ev_w) {
  hipStream_t st = ctx->stream;
  const int L = s.L;
  int32_t rc = GIGL_OK;
  for (int l = L - 1; l >= 0; --l) {
    const int32_t* n_rows = p->un.meta + GIGL_META_LEVEL0 + (L - 1 - l);
    const int d = s.dims[l], n_out = s.dims[l + 1];
    const bool act = l < L - 1 || s.act_last;
    auto relu_mask = [&]() {
      int64_t blocks = (e.rows_cap[l] * n_out + 255) / 256;
      if (blocks > 4096) blocks = 4096;
      hipLaunchKernelGGL(relu_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, st, e.dh[l], (const float*)e.h[l], n_rows, n_out);
    };
    // with dropout the mask carries the kept elements' scale: it runs first, in both paths, and the weight gradient takes
    // the masked rows as they are (the masked READ of the unforked path below would lose the scale)
    const bool drop = act && s.drop_p > 0.f;
    auto drop_mask = [&]() {
      const int whole = (n_out & 3) == 0 && (((uintptr_t)e.dh[l] | (uintptr_t)e.h[l]) & 15) == 0;
      hipLaunchKernelGGL(dropout_relu_mask_kernel, dim3(blocks_256(e.rows_cap[l] * n_out / (whole ? 4 : 1))), dim3(256), 0, st,
                         e.dh[l], (const float*)e.h[l], n_rows, e.rows_cap[l], n_out, 1.0f / (1.0f - s.drop_p), whole);
    };
    if (drop && !wctx) {
      drop_mask();
      rc = gigl_linear_weight_grad_parts(ctx, e.dh[l], e.a[l], nullptr, n_rows, e.rows_cap[l], n_out, 2 * d, e.part_w[l],
                                         s.bias[l] ? e.part_b[l] : nullptr);
    } else if (wctx) {
      // the mask first (the chain needs the masked rows anyway), then the gradient of the MASKED rows beside the chain: the
      // same products as the masked read of the unmasked rows
      if (drop) drop_mask();
      else if (act) relu_mask();
      GIGL_HIP_CHECK(ctx, hipEventRecord(ev_w, st));
      GIGL_HIP_CHECK(ctx, hipStreamWaitEvent(wctx->stream, ev_w, 0));
      rc = gigl_linear_weight_grad_parts(wctx, e.dh[l], e.a[l], nullptr, n_rows, e.rows_cap[l], n_out, 2 * d, e.part_w[l],
                                         s.bias[l] ? e.part_b[l] : nullptr);
    } else {
      rc = gigl_linear_weight_grad_parts(ctx, e.dh[l], e.a[l], act ? e.h[l] : nullptr, n_rows, e.rows_cap[l], n_out, 2 * d,
                                         e.part_w[l], s.bias[l] ? e.part_b[l] : nullptr);
    }
    if (rc != GIGL_OK) return rc;
    if (l == 0) break;  // (the first layer's input is the feature table: no gradient)
    if (act && !wctx && !drop) relu_mask();
    rc = gigl_linear(ctx, e.dh[l], s.wt_l[l], nullptr, n_rows, e.rows_cap[l], n_out, 2 * d, 0, da);
    if (rc != GIGL_OK) return rc;
    if (s.bwd_gather)
      rc = gigl_gather_mean_backward_lists(ctx, da, d, p->un.rowptr, p->un.rowend, n_rows, p->un.meta + GIGL_META_LEVEL0 + (L - l),
                                           e.rows_cap[l - 1], tl[l], GIGL_AGGR_MEAN, e.dh[l - 1]);
    else
      rc = gigl_gather_mean_backward(ctx, da, d, p->un.rowptr, p->un.rowend, p->un.col, n_rows, e.rows_cap[l], e.dh[l - 1]);
    if (rc != GIGL_OK) return rc;
  }
  return GIGL_OK;
}

// Adam's pack over the partial sums of one encode (e1 == NULL) or of two, each over its workspace's batch
AdamPack sage_adam_pack(const SageTrainShared& s, const SageTrainEnc* e0, const BatchGraph* p0, const SageTrainEnc* e1,
                        const BatchGraph* p1) {
  AdamPack ap{};
  const SageTrainEnc* e[2] = {e0, e1};
  const BatchGraph* p[2] = {p0, p1};
  ap.n_src = e1 ? 2 : 1;
  for (int l = 0; l < s.L; ++l)
    for (int is_bias = 0; is_bias < (s.bias[l] ? 2 : 1); ++is_bias) {
      const int k = ap.count++;
      ap.p[k] = is_bias ? s.bias[l] : s.w[l];
      ap.m[k] = s.mom[4 * l + 2 * is_bias];
      ap.v[k] = s.mom[4 * l + 2 * is_bias + 1];
      ap.n[k] = is_bias ? (int64_t)s.dims[l + 1] : (int64_t)s.dims[l + 1] * 2 * s.dims[l];
      for (int q = 0; q < ap.n_src; ++q) {
        ap.part[q][k] = is_bias ? e[q]->part_b[l] : e[q]->part_w[l];
        ap.rows[q][k] = p[q]->un.meta + GIGL_META_LEVEL0 + (s.L - 1 - l);
        ap.rc[q][k] = e[q]->part_rc[l];
      }
    }
  ap.lr = s.lr;
  ap.beta1 = s.beta1;
  ap.beta2 = s.beta2;
  ap.eps = s.eps;
  ap.wd = s.wd;
  return ap;
}

// Adam's moments of tensor `index` (2 l: layer l's weights, 2 l + 1: its bias) -> m, v (device; either may be NULL), on ctx's stream
int32_t sage_moments_copy(gigl_ctx* ctx, const SageTrainShared& s, int index, float* m, float* v) {
  const int l = index >> 1, is_bias = index & 1;
  const size_t n = is_bias ? (size_t)s.dims[l + 1] : (size_t)s.dims[l + 1] * 2 * s.dims[l];
  float* dst[2] = {m, v};
  for (int k = 0; k < 2; ++k)
    if (dst[k])
      GIGL_HIP_CHECK(ctx, hipMemcpyAsync(dst[k], s.mom[4 * l + 2 * is_bias + k], n * 4, hipMemcpyDeviceToDevice, ctx->stream));
  return GIGL_OK;
}

// every moment of src into dst's (plans of the same shape), on ctx's stream
int32_t sage_moments_adopt(gigl_ctx* ctx, const SageTrainShared& dst, const SageTrainShared& src) {
  GIGL_REQUIRE(ctx, dst.L == src.L, "plans of different depth");
  for (int l = 0; l <= dst.L; ++l) GIGL_REQUIRE(ctx, dst.dims[l] == src.dims[l], "plans of different widths");
  for (int i = 0; i < 2 * dst.L; ++i) {
    const int32_t rc = sage_moments_copy(ctx, src, i, dst.mom[4 * (i >> 1) + 2 * (i & 1)], dst.mom[4 * (i >> 1) + 2 * (i & 1) + 1]);
    if (rc != GIGL_OK) return rc;
  }
  return GIGL_OK;
}

// ---- the workspace ring of a training plan, written once for the node-classification and the link-prediction plans.
// A step is two parts (see above): the GRAPH part of a batch runs on the side stream of one of the ring's slots, into that
// slot's batch graphs; the LAYERS part that reads them runs on the caller's stream.  A batch ANNOUNCED ahead is
// issued into a later slot right away and recognised when its step comes by the ADDRESS of its roots (include/gigl_hip.h:
// CONTRACT of an announced batch).  Both parts go through gigl_run_part: eager once, captured, replayed.
extern "C++" {  // (a member template: this file's definitions sit in one extern "C" block)
struct PlanRing {
  enum Family { TRAIN = 0, EVAL = 1 };  // whose graph part: a training step's, gigl_nablp_train_plan_eval's
  struct Slot {
    gigl_ctx* side = nullptr;                      // private ctx with a stream of its own: the graph part's launches and arena
    BatchGraph base[2];                            // batch graphs of the plan's root sets, on the side ctx
    hipEvent_t ev_graph = nullptr;                 // end of the graph part last issued for the slot (its side stream)
    hipEvent_t ev_layers = nullptr;                // end of the layers part that last read it (the caller's stream)
    PartGraph graph[2], layers;                    // graph part per family (an evaluation's seed / mode need not be the steps')
    bool fetched = false;                          // the slot holds the graph of an announced batch ...
    const uint32_t* key[2] = {nullptr, nullptr};   // ... announced as these buffers (the step must name the same ones)
  } slot[TRAIN_WS];
  gigl_ctx* ctx = nullptr;  // the caller's: HIP's failures are reported on it
  int n = 0, n_base = 0;    // slots in use (2 or 3), root sets per slot
  int cur = 0;              // slot of the next step
  hipEvent_t ev_now = nullptr;  // "the caller's stream, now": the roots a graph part copies were written before it
  int32_t seed[2] = {0, 0}, mode[2] = {-1, -1};  // what each family's captured graph parts were captured with

  // per slot a side ctx, a batch graph per root set (nb[i] roots; number_every_node: batch_graph_init) and its events
  int32_t create(gigl_ctx* caller, int slots, int root_sets, const int32_t* nb, gigl_graph* graph, const int32_t* fanouts,
                 int32_t hops, bool number_every_node) {
    ctx = caller;
    n = slots;
    n_base = root_sets;
    int32_t rc = GIGL_OK;
    for (int k = 0; k < n && rc == GIGL_OK; ++k) {
      Slot& s = slot[k];
      rc = gigl_ctx_create(ctx->device, &s.side);
      if (rc != GIGL_OK) break;
      s.side->wide = ctx->wide;
      for (int i = 0; i < n_base && rc == GIGL_OK; ++i) {
        rc = batch_graph_init(&s.base[i], s.side, graph, nb[i], fanouts, hops, number_every_node);
        if (rc != GIGL_OK) gigl_fail(ctx, rc, "%s", gigl_last_error(s.side));
      }
      if (rc == GIGL_OK && (hipEventCreateWithFlags(&s.ev_graph, hipEventDisableTiming) != hipSuccess ||
                            hipEventCreateWithFlags(&s.ev_layers, hipEventDisableTiming) != hipSuccess))
        rc = GIGL_E_HIP;
    }
    if (rc == GIGL_OK && hipEventCreateWithFlags(&ev_now, hipEventDisableTiming) != hipSuccess) rc = GIGL_E_HIP;
    return rc;
  }

  // the graph part of slot k for these roots (count[i] of root set i; 0: the set is absent), on its side stream; ev_graph
  // marks its end.  A training step's is remembered under the roots' addresses until consume() or reseed()
  template <typename Body>
  int32_t issue_graph_part(int k, Family fam, const uint32_t* const* roots, const size_t* count, bool capture_ok, Body&& body) {
    Slot& s = slot[k];
    hipStream_t ss = s.side->stream;
    // the workspace is free once the layers part that last read it is done; the roots were written on the caller's stream
    GIGL_HIP_CHECK(ctx, hipStreamWaitEvent(ss, s.ev_layers, 0));
    GIGL_HIP_CHECK(ctx, hipEventRecord(ev_now, ctx->stream));
    GIGL_HIP_CHECK(ctx, hipStreamWaitEvent(ss, ev_now, 0));
    for (int i = 0; i < n_base; ++i)
      if (count[i])
        GIGL_HIP_CHECK(ctx, hipMemcpyAsync(s.base[i].roots_buf, roots[i], count[i] * 4, hipMemcpyDeviceToDevice, ss));
      else
        gigl_fill_u32(ss, s.base[i].roots_buf, GIGL_INVALID, 1);
    const int32_t rc = gigl_run_part(s.side, s.side, &s.graph[fam], capture_ok, "training step", body);
    if (rc != GIGL_OK) return gigl_fail(ctx, rc, "%s", gigl_last_error(s.side));
    GIGL_HIP_CHECK(ctx, hipEventRecord(s.ev_graph, ss));
    if (fam == EVAL) return GIGL_OK;  // (an evaluation batch is consumed by the call that samples it: nothing to recognise later)
    s.fetched = true;
    s.key[0] = roots[0];
    s.key[1] = n_base > 1 ? roots[1] : nullptr;
    return GIGL_OK;
  }
  bool holds(int k, const uint32_t* r0, const uint32_t* r1 = nullptr) const {
    return slot[k].fetched && slot[k].key[0] == r0 && slot[k].key[1] == r1;
  }
  void consume(int k) { slot[k].fetched = false; }

  // seed and mode are baked into a family's captured graph parts: a change drops every slot's.  What was announced was
  // sampled under the training steps' old seed: a change of theirs forgets it (the step samples again)
  void reseed(Family fam, int32_t sampling_seed, int32_t sampling_mode) {
    if (seed[fam] == sampling_seed && mode[fam] == sampling_mode) return;
    for (Slot& s : slot) {
      if (s.graph[fam].exec) hipStreamSynchronize(s.side->stream);
      s.graph[fam].drop();
      if (fam == TRAIN) s.fetched = false;
    }
    seed[fam] = sampling_seed;
    mode[fam] = sampling_mode;
  }

  // destruction in two steps, around the plan's own buffers (the caller's stream is synchronised already): the side
  // streams drained, every captured graph gone before the ctx whose stream it was captured on, batch graphs before their ctx
  void release() {
    for (Slot& s : slot)
      if (s.side) hipStreamSynchronize(s.side->stream);
    for (Slot& s : slot) {
      s.graph[TRAIN].drop();
      s.layers.drop();
      s.graph[EVAL].drop();
      if (s.ev_graph) hipEventDestroy(s.ev_graph);
      if (s.ev_layers) hipEventDestroy(s.ev_layers);
      for (BatchGraph& b : s.base) batch_graph_free(&b);
    }
    if (ev_now) hipEventDestroy(ev_now);
  }
  void destroy_ctxs() {
    for (Slot& s : slot)
      if (s.side) gigl_ctx_destroy(s.side);
  }
};
}  // extern "C++"

// (A/B knob of the training plans: GIGL_TRAIN_PLAN_EAGER=1 both parts eager, =graph / =layers only that part)
bool train_part_captures(int part) {
  static const char* ev = getenv("GIGL_TRAIN_PLAN_EAGER");
  return !(ev && (ev[0] == '1' || (ev[0] == 'g' && part == 0) || (ev[0] == 'l' && part == 1)));
}

// ---- what the node-classification training plans (GraphSAGE, GCN) share beyond their layers: the workspace ring, the step's
// static inputs, the loss on the roots and the step itself, written once
struct NcTrainState {
  gigl_ctx* ctx = nullptr;         // the caller's (its stream carries the layers part; errors are reported on it)
  // two ctxs of the plan's own, for their ARENAS: scratch addresses are baked into the captured launches, and another
  // plan on the caller's ctx (the inference plan of an evaluation pass between epochs) may grow — reallocate — that arena
  gigl_ctx* lctx = nullptr;        // layers part (bound to the caller's stream at every step)
  // TRAIN_WS workspaces, one root set each (each on its own side ctx / stream: two graph parts — of the next batch and of
  // the one after — can be in flight)
  PlanRing ring;
  int32_t b = 0;                          // roots per batch
  float** loss_slot = nullptr;            // where the caller wants the step's loss (set by train_stage_kernel)
  void* zero_base = nullptr;              // the gradient rows that are added to: cleared at the start of every step
  size_t zero_bytes = 0;
  int64_t* labels_buf = nullptr;
  int32_t* n_valid_buf = nullptr;  // [0] real roots of the batch, [1] Adam's step counter, [2] sticky "a batch failed" (halt)
  float* loss_rows = nullptr;
  float* loss = nullptr;
  bool stepped = false;  // a step has run: what the captured layers part launches is final (gigl_*_train_plan_set_dropout)
  std::vector<void*> owned;
};

// the step's static buffers and the cleared block of zero_floats floats (zeroed words, no loss slot yet)
bool nc_state_alloc(NcTrainState& t, size_t zero_floats) {
  auto alloc = [&](size_t bytes) { return plan_alloc(t.owned, bytes); };
  t.zero_base = alloc(zero_floats * 4);
  t.zero_bytes = zero_floats * 4;
  t.labels_buf = (int64_t*)alloc((size_t)t.b * 8);
  t.n_valid_buf = (int32_t*)alloc(16);
  t.loss_rows = (float*)alloc((size_t)t.b * 4);
  t.loss = (float*)alloc(16);
  // (measured, round 6: the loss sum on a BRANCH of the captured layers — forked after the loss rows, joined before Adam —
  // took the step from 0.201 to 0.263 ms: a graph with a second branch is replayed through two queues with a barrier
  // packet per edge.  The layers part stays one stream)
  t.loss_slot = (float**)alloc(16);
  return t.zero_base && t.labels_buf && t.n_valid_buf && t.loss_rows && t.loss && t.loss_slot &&
         hipMemset(t.n_valid_buf, 0, 16) == hipSuccess && hipMemset(t.loss_slot, 0, 16) == hipSuccess;
}

// everything a plan holds through its NcTrainState (the caller deletes the plan itself)
void nc_state_release(NcTrainState* t) {
  if (t->ctx) {
    hipSetDevice(t->ctx->device);
    hipStreamSynchronize(t->ctx->stream);
  }
  t->ring.release();
  for (void* q : t->owned) hipFree(q);
  t->ring.destroy_ctxs();
  if (t->lctx) {
    gigl_ctx_set_stream(t->lctx, nullptr);  // (the stream is the caller's)
    gigl_ctx_destroy(t->lctx);
  }
}

// loss on the roots of workspace p's batch over out [*][width], its gradient ADDED into dout (cleared before)
void nc_loss_launches(const NcTrainState* t, hipStream_t st, const BatchGraph* p, const float* out, int width, float* dout) {
  // (the loss rows and their sum stay two launches: folding the sum into the last workgroup of the first — a ticket behind
  // device-scope fences — took 22.7 us instead of 5.0 + 5.1, and the L2 write-backs of its 256 fences slowed the next batch's
  // graph part on the side stream: measured, round 6)
  hipLaunchKernelGGL(ce_roots_kernel, dim3((unsigned)((t->b + 3) / 4)), dim3(256), 0, st, out, width,
                     (const int32_t*)p->un.root_local, (const int64_t*)t->labels_buf, (const int32_t*)t->n_valid_buf, t->b,
                     (const int32_t*)p->un.meta, dout, t->loss_rows);
  hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(1024), 0, st, (const float*)t->loss_rows, t->b,
                     (const int32_t*)t->n_valid_buf, t->loss, t->n_valid_buf + 1, (const int32_t*)p->un.meta,
                     t->n_valid_buf + 2, (float* const*)t->loss_slot);
}

// a plan's private ctx (own arena) follows the caller's stream: every launch of the step goes there
static int32_t train_bind_stream(gigl_ctx* ctx, gigl_ctx* lctx) {
  if (lctx->stream == ctx->stream && !lctx->own_stream) return GIGL_OK;
  const int32_t rs = gigl_ctx_set_stream(lctx, ctx->stream);
  return rs == GIGL_OK ? GIGL_OK : gigl_fail(ctx, rs, "%s", gigl_last_error(lctx));
}

extern "C++" {
// One step (gigl_sage_train_plan_step2's contract, include/gigl_hip.h).  graph_body(kk): the graph part of the batch in
// workspace kk's roots_buf, on that workspace's side ctx; layers_body(k): everything after it over workspace k, on lctx.
// pa: what train_stage_kernel clears and transposes ahead of the layers
template <typename GraphBody, typename LayersBody>
int32_t nc_train_step(NcTrainState* t, const uint32_t* roots, const int64_t* labels, int32_t n_valid, const uint32_t* roots_next,
                      const uint32_t* roots_next2, int32_t sampling_seed, int32_t mode, float* loss_out, const TrainPrep& pa,
                      GraphBody&& graph_body, LayersBody&& layers_body) {
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, roots && labels && n_valid >= 1 && n_valid <= t->b, "bad argument");
  if (mode == GIGL_MODE_REPLACE)
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "the training plan needs duplicate-free trees (no with-replacement mode)");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  t->stepped = true;
  hipStream_t st = ctx->stream;
  PlanRing& ring = t->ring;
  ring.reseed(PlanRing::TRAIN, sampling_seed, mode);
  const int k = ring.cur;
  auto graph_part = [&](int kk, const uint32_t* r) {
    const size_t count = (size_t)t->b;
    return ring.issue_graph_part(kk, PlanRing::TRAIN, &r, &count, train_part_captures(0), [&, kk]() { return graph_body(kk); });
  };
  // (a prefetched workspace belongs to the roots it was announced with: an epoch cut short, a reshuffle or an evaluation
  // between two steps hands in other roots — the graph part is then issued again instead of training these labels
  // against the old batch's graph; as gigl_hgt_infer_run's guard)
  if (!ring.holds(k, roots)) {  // the graph part of THIS batch now (the layers wait for it)
    const int32_t rc = graph_part(k, roots);
    if (rc != GIGL_OK) return rc;
  }
  ring.consume(k);
  // the NEXT batch's graph part goes to the side stream BEFORE this batch's layers are enqueued: it waits for what the
  // caller's stream holds now (roots_next was written there; the layers that last read the other workspace), not for
  // the layers about to be enqueued
  // (two batches ahead: the graph parts are chains of small latency-bound launches, two of them in flight on their own
  // streams take little more than one)
  const uint32_t* ahead[2] = {roots_next, roots_next ? roots_next2 : nullptr};
  for (int d = 0; d < 2; ++d) {
    const int kk = (k + 1 + d) % TRAIN_WS;
    if (!ahead[d] || ring.holds(kk, ahead[d]) || kk == k) continue;
    const int32_t rc = graph_part(kk, ahead[d]);
    if (rc != GIGL_OK) return rc;
  }
  // the step's inputs go into the static buffers the (captured) launches read — labels, the number of real roots, where the
  // caller wants the loss (the loss kernel writes it there itself) — in the launch that also clears the cleared block and
  // lays out the transposed weights
  int64_t blocks = (pa.zero_words + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 64) blocks = 64;
  // (the layers of the previous step read labels_buf / the cleared block: this launch is behind them on the stream)
  hipLaunchKernelGGL(train_stage_kernel, dim3((unsigned)blocks), dim3(256), 0, st, labels, n_valid, t->labels_buf, t->n_valid_buf,
                     t->loss_slot, loss_out, pa);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  GIGL_HIP_CHECK(ctx, hipStreamWaitEvent(st, ring.slot[k].ev_graph, 0));
  const int32_t rs = train_bind_stream(ctx, t->lctx);
  if (rs != GIGL_OK) return rs;
  PartGraph& layers = ring.slot[k].layers;
  const int32_t rc = gigl_run_part(t->lctx, t->lctx, &layers, train_part_captures(1), "training step", [&]() { return layers_body(k); });
  if (rc != GIGL_OK) return gigl_fail(ctx, rc, "%s", gigl_last_error(t->lctx));
  // (the layers' scratch is the plan's, not a workspace's: one eager run has sized it for every slot's capture)
  if (layers.warm)
    for (PlanRing::Slot& s : ring.slot) s.layers.warm = true;
  GIGL_HIP_CHECK(ctx, hipEventRecord(ring.slot[k].ev_layers, st));
  ring.cur = (k + 1) % TRAIN_WS;
  return GIGL_OK;
}
}  // extern "C++"

// clears the device-side halt a failed batch left, on the plan's stream
int32_t nc_resume(NcTrainState* t) {
  GIGL_HIP_CHECK(t->ctx, hipSetDevice(t->ctx->device));
  GIGL_HIP_CHECK(t->ctx, hipMemsetAsync(t->n_valid_buf + 2, 0, 4, t->ctx->stream));
  return GIGL_OK;
}

// Adam's step counter of src into dst, behind the moments' copies on dst's stream; both streams are synchronised
int32_t nc_adopt_counter(NcTrainState* dst, const NcTrainState* src) {
  gigl_ctx* ctx = dst->ctx;
  GIGL_HIP_CHECK(ctx, hipMemcpyAsync(dst->n_valid_buf + 1, src->n_valid_buf + 1, 4, hipMemcpyDeviceToDevice, ctx->stream));
  GIGL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return GIGL_OK;
}

}  // namespace

struct gigl_sage_train_plan : SageTrainShared, NcTrainState {
  SageTrainEnc enc;                       // the step's one encode (over the batch graph ring.slot[k].base[0] the step reads)
  int32_t* tlists[TRAIN_WS][GIGL_MAX_HOPS] = {{nullptr}};  // its transposed lists per workspace and layer >= 1, built by the graph part
  float* da = nullptr;                    // [max rows_cap[l >= 1]][2 max dims]: gradient of a layer's operand
};

namespace {

// everything after the graph part, over workspace k, on lctx's stream (the caller's); train_stage_kernel ran ahead of it
int32_t train_enqueue_layers(gigl_sage_train_plan* t, int k) {
  BatchGraph* p = &t->ring.slot[k].base[0];
  gigl_ctx* ctx = t->lctx;
  const int L = t->L;
  hipStream_t st = ctx->stream;
  const SageTrainEnc& e = t->enc;
  int32_t rc = sage_enc_forward(ctx, *t, e, p, true, 0, t->n_valid_buf + 1);
  if (rc != GIGL_OK) return rc;
  // ---- loss on the roots, its gradient into dh[L - 1]
  nc_loss_launches(t, st, p, e.h[L - 1], t->dims[L], e.dh[L - 1]);
  rc = sage_enc_backward(ctx, *t, e, p, t->tlists[k], t->da, nullptr, nullptr);
  if (rc != GIGL_OK) return rc;
  const AdamPack ap = sage_adam_pack(*t, &e, p, nullptr, nullptr);
  launch_adam(st, 208, ap, (const int32_t*)(t->n_valid_buf + 1), (const int32_t*)p->un.meta, (const int32_t*)nullptr,
              (const int32_t*)(t->n_valid_buf + 2), nullptr);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

}  // namespace

int32_t gigl_sage_train_plan_destroy(gigl_sage_train_plan* t) {
  if (!t) return GIGL_OK;
  nc_state_release(t);
  delete t;
  return GIGL_OK;
}

int32_t gigl_sage_train_plan_create(gigl_ctx* ctx, gigl_graph* graph, gigl_feat* feat, int32_t b, const int32_t* fanouts,
                                    int32_t hops, const int32_t* dims, float* const* w, float* const* bias,
                                    int32_t act_last, float lr, float beta1, float beta2, float eps, float weight_decay,
                                    gigl_sage_train_plan** out) {
  if (!ctx || !out) return GIGL_E_INVALID_ARG;
  *out = nullptr;
  GIGL_REQUIRE(ctx, graph && feat && fanouts && dims && w, "null argument");
  GIGL_REQUIRE(ctx, hops >= 1 && hops <= GIGL_MAX_HOPS && b >= 1, "bad plan shape");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  gigl_sage_train_plan* t = new (std::nothrow) gigl_sage_train_plan();
  if (!t) return gigl_fail(ctx, GIGL_E_OOM, "host OOM");
  t->ctx = ctx;
  t->feat = feat;
  int32_t rc = gigl_ctx_create(ctx->device, &t->lctx);
  if (rc == GIGL_OK) rc = plan_check_layers(ctx, feat, hops, dims, w);
  if (rc == GIGL_OK) rc = t->ring.create(ctx, TRAIN_WS, 1, &b, graph, fanouts, hops, false);
  if (rc != GIGL_OK) {
    gigl_sage_train_plan_destroy(t);
    return rc;
  }
  t->L = hops;
  t->b = t->enc.b = b;
  t->act_last = act_last;
  t->lr = lr;
  t->beta1 = beta1;
  t->beta2 = beta2;
  t->eps = eps;
  t->wd = weight_decay;
  size_t zero_floats = 0, da_floats = 16;
  bool ok = sage_shared_alloc(*t, t->owned, dims, w, bias);
  // (no entry point hands this plan's gradients out: the cleared block is the dh rows alone)
  ok = sage_enc_alloc(*t, t->enc, t->owned, ctx->wide, fanouts, false, &zero_floats, &da_floats) && ok;
  ok = nc_state_alloc(*t, zero_floats) && ok;
  if (t->zero_base) sage_enc_carve(*t, t->enc, false, (float*)t->zero_base);
  for (int k = 0; k < TRAIN_WS; ++k) ok = sage_tlists_alloc(*t, t->enc, t->owned, t->ring.slot[k].base[0].un.cap_edges, t->tlists[k]) && ok;
  t->da = (float*)plan_alloc(t->owned, da_floats * 4);
  ok = ok && t->da;
  if (!ok) {
    gigl_sage_train_plan_destroy(t);
    return gigl_fail(ctx, GIGL_E_OOM, "hipMalloc of the training workspace failed");
  }
  *out = t;
  return GIGL_OK;
}

int32_t gigl_sage_train_plan_step(gigl_sage_train_plan* t, const uint32_t* roots, const int64_t* labels, int32_t n_valid,
                                  const uint32_t* roots_next, int32_t sampling_seed, int32_t mode, float* loss_out) {
  return gigl_sage_train_plan_step2(t, roots, labels, n_valid, roots_next, nullptr, sampling_seed, mode, loss_out);
}

int32_t gigl_sage_train_plan_step2(gigl_sage_train_plan* t, const uint32_t* roots, const int64_t* labels, int32_t n_valid,
                                   const uint32_t* roots_next, const uint32_t* roots_next2, int32_t sampling_seed,
                                   int32_t mode, float* loss_out) {
  if (!t) return GIGL_E_INVALID_ARG;
  // what train_stage_kernel does ahead of the layers: it clears the dh block and lays out W_l^T of layers >= 1
  TrainPrep pa{};
  pa.zero = (uint32_t*)t->zero_base;
  pa.zero_words = (int64_t)(t->zero_bytes / 4);
  for (int l = 1; l < t->L; ++l) {
    pa.w[pa.n_t] = t->w[l];
    pa.wt[pa.n_t] = t->wt_l[l];
    pa.rows[pa.n_t] = t->dims[l + 1];
    pa.cols[pa.n_t] = 2 * t->dims[l];
    ++pa.n_t;
  }
  return nc_train_step(
      t, roots, labels, n_valid, roots_next, roots_next2, sampling_seed, mode, loss_out, pa,
      [&](int kk) { return sage_enqueue_graph(*t, t->enc, &t->ring.slot[kk].base[0], t->tlists[kk], sampling_seed, mode); },
      [&](int k) { return train_enqueue_layers(t, k); });
}

const float* gigl_sage_train_plan_loss(gigl_sage_train_plan* t) { return t ? t->loss : nullptr; }

namespace {
// the setters' shared half: the plan has not stepped (its layers part is captured with or without the dropout launches),
// 0 <= p < 1
// (S: whatever holds a plan's drop_p / drop_seed — SageTrainShared, gigl_gcn_train_plan)
extern "C++" template <typename S>
int32_t sage_set_dropout(gigl_ctx* ctx, S& s, bool stepped, float p, uint64_t seed) {
  GIGL_REQUIRE(ctx, !stepped, "dropout is set after create and before the first step (the step is captured)");
  GIGL_REQUIRE(ctx, p >= 0.f && p < 1.f, "dropout: p must be in [0, 1)");  // (false for a NaN too)
  s.drop_p = p;
  s.drop_seed = seed;
  return GIGL_OK;
}
}  // namespace

int32_t gigl_sage_train_plan_set_dropout(gigl_sage_train_plan* t, float p, uint64_t seed) {
  if (!t) return GIGL_E_INVALID_ARG;
  return sage_set_dropout(t->ctx, *t, t->stepped, p, seed);
}

int32_t gigl_dropout_mask(gigl_ctx* ctx, uint64_t seed, uint32_t step, int32_t encode, int32_t layer, int64_t rows, int32_t cols,
                          float p, uint8_t* keep) {
  if (!ctx) return GIGL_E_INVALID_ARG;
  GIGL_REQUIRE(ctx, (keep || rows == 0) && rows >= 0 && rows <= 0xFFFFFFFFll && cols >= 1, "bad mask shape / null output");
  GIGL_REQUIRE(ctx, p >= 0.f && p < 1.f, "dropout: p must be in [0, 1)");
  GIGL_REQUIRE(ctx, encode >= 0 && encode < (1 << 24) && layer >= 0 && layer < 256, "encode / layer outside the counter word");
  if (rows == 0) return GIGL_OK;
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int lg = dropout_lanes_log2(cols);
  hipLaunchKernelGGL(dropout_keep_kernel, dim3(blocks_256(rows << lg)), dim3(256), 0, ctx->stream, keep, rows, cols, step,
                     gigl_dropout_mask_args(seed, p, encode, layer), lg);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gigl_sage_train_plan_resume(gigl_sage_train_plan* t) {
  return t ? nc_resume(t) : GIGL_E_INVALID_ARG;
}

// ------------------------------------------------------------------------------------------------------------------
// gigl_gcn_train_plan: the same step for the reference's STOCK node-classification model, TwoLayerGCN
// (python/gigl/src/common/models/pyg/homogeneous.py:488-546: conv1 -> relu -> dropout -> conv2, PyG GCNConv): two layers,
// each AGGREGATED FIRST (A_hat (X W) == (A_hat X) W: only the rows a layer needs are projected),
//   a1 = A_hat x[nodes] -> h1 = relu(a1 W1^T + b1) [-> dropout] -> a2 = A_hat h1 -> out = a2 W2^T + b2 -> cross-entropy on the roots
//   -> dW2, db2 -> da2 = g2 W2 -> dh1 = A_hat^T da2 -> rectifier / dropout mask -> dW1, db1 -> Adam
// over the GENERIC union graph (every node numbered, as gigl_union_build numbers them: a leaf occurrence of a node that is
// also an inner node needs that node's degree).  What depends on the batch graph alone — A_hat's dinv over every node,
// the root rows' transposed lists — belongs to the graph part.  Ring, step, loss, Adam and the dropout kernels are the
// GraphSAGE plan's (NcTrainState).
struct gigl_gcn_train_plan : NcTrainState {
  gigl_feat* feat = nullptr;
  int32_t dims[3] = {0, 0, 0};     // input, hidden, output width
  float* w[2] = {nullptr, nullptr};     // conv{1,2}.lin.weight [dims[l+1]][dims[l]]: borrowed, UPDATED IN PLACE
  float* bias[2] = {nullptr, nullptr};  // conv{1,2}.bias (may be NULL)
  float* mom[8] = {nullptr};            // m_w, v_w, m_b, v_b per layer
  float* wt2 = nullptr;                 // W2^T [hid][out], laid out once per step (train_stage_kernel)
  float lr = 0.f, beta1 = 0.9f, beta2 = 0.999f, eps = 1e-8f, wd = 0.f;
  float drop_p = 0.f;  // dropout on h1 (gigl_gcn_train_plan_set_dropout; 0: none)
  uint64_t drop_seed = 0;
  int64_t rows_cap[2] = {0, 0};  // rows layer l may compute: the nodes of level <= 1 - l
  float *a1 = nullptr, *h1 = nullptr, *a2 = nullptr, *out = nullptr;
  float *g2 = nullptr, *da2 = nullptr, *dh1 = nullptr;  // gradients of out (in the cleared block), a2, h1
  float* part_w[2] = {nullptr, nullptr};  // the weight gradients' per-chunk partial sums (Adam adds them up)
  float* part_b[2] = {nullptr, nullptr};
  int32_t part_rc[2] = {0, 0};
  float* dinv[TRAIN_WS] = {nullptr};      // per workspace: 1 / sqrt(deg) of every node of its batch graph
  int32_t* tlists[TRAIN_WS] = {nullptr};  // ... and who reads which level-<=1 node among the root rows
};

namespace {

const int32_t* gcn_level(const BatchGraph* p, int level) { return p->un.meta + GIGL_META_LEVEL0 + level; }

// the graph part of workspace p's roots_buf: sample + union, then what the layers need of the batch graph alone
int32_t gcn_enqueue_graph(const gigl_gcn_train_plan* t, BatchGraph* p, float* dinv, int32_t* tl, int32_t sampling_seed, int32_t mode) {
  int32_t rc = batch_graph_enqueue(p, sampling_seed, mode);
  if (rc != GIGL_OK) return rc;
  rc = gigl_gcn_dinv(p->ctx, p->un.rowptr, p->un.rowend, p->un.col, p->un.meta + GIGL_META_N_NODES, p->un.cap_nodes, dinv);
  if (rc != GIGL_OK) return rc;
  return gigl_transposed_rows_build(p->ctx, p->un.rowptr, p->un.rowend, p->un.col, gcn_level(p, 0), t->rows_cap[1],
                                    gcn_level(p, 1), t->rows_cap[0], p->un.cap_edges, tl);
}

// everything after the graph part, over workspace k, on lctx's stream (the caller's); train_stage_kernel ran ahead of it
int32_t gcn_enqueue_layers(gigl_gcn_train_plan* t, int k) {
  const BatchGraph* p = &t->ring.slot[k].base[0];
  gigl_ctx* ctx = t->lctx;
  hipStream_t st = ctx->stream;
  const gigl_union& un = p->un;
  const int32_t *n0 = gcn_level(p, 0), *n1 = gcn_level(p, 1);
  const int d_in = t->dims[0], hid = t->dims[1], width = t->dims[2];
  const int64_t rows1 = t->rows_cap[0], rows0 = t->rows_cap[1];
  const int32_t* step_dev = t->n_valid_buf + 1;
  int32_t rc = gigl_gcn_gather(ctx, t->feat->rows, t->feat->dtype, d_in, un.nodes, t->dinv[k], un.rowptr, un.rowend, un.col, n1,
                               rows1, t->a1);
  if (rc == GIGL_OK) rc = gigl_linear(ctx, t->a1, t->w[0], t->bias[0], n1, rows1, d_in, hid, 1, t->h1);
  if (rc != GIGL_OK) return rc;
  if (t->drop_p > 0.f) {  // (*step_dev is read before the loss launch moves it on)
    const int lg = dropout_lanes_log2(hid);
    hipLaunchKernelGGL(dropout_rows_kernel, dim3(blocks_256(rows1 << lg)), dim3(256), 0, st, t->h1, n1, rows1, hid, step_dev,
                       gigl_dropout_mask_args(t->drop_seed, t->drop_p, 0, 0), lg);
    GIGL_HIP_CHECK(ctx, hipGetLastError());
  }
  rc = gigl_gcn_gather(ctx, t->h1, GIGL_DTYPE_F32, hid, nullptr, t->dinv[k], un.rowptr, un.rowend, un.col, n0, rows0, t->a2);
  if (rc == GIGL_OK) rc = gigl_linear(ctx, t->a2, t->w[1], t->bias[1], n0, rows0, hid, width, 0, t->out);
  if (rc != GIGL_OK) return rc;
  nc_loss_launches(t, st, p, t->out, width, t->g2);
  // ---- backward: layer 2's weights, its operand's gradient through W2 (g2 . W2 over W2^T as the projection's weight
  // operand), A_hat^T, the rectifier (with dropout: the mask that carries the kept elements' scale), layer 1's weights
  rc = gigl_linear_weight_grad_parts(ctx, t->g2, t->a2, nullptr, n0, rows0, width, hid, t->part_w[1], t->bias[1] ? t->part_b[1] : nullptr);
  if (rc == GIGL_OK) rc = gigl_linear(ctx, t->g2, t->wt2, nullptr, n0, rows0, width, hid, 0, t->da2);
  if (rc == GIGL_OK)
    rc = gigl_gcn_gather_backward_lists(ctx, t->da2, hid, t->dinv[k], un.rowptr, un.rowend, n0, n1, rows1, t->tlists[k], t->dh1);
  if (rc != GIGL_OK) return rc;
  if (t->drop_p > 0.f) {
    const int whole = (hid & 3) == 0 && (((uintptr_t)t->dh1 | (uintptr_t)t->h1) & 15) == 0;
    hipLaunchKernelGGL(dropout_relu_mask_kernel, dim3(blocks_256(rows1 * hid / (whole ? 4 : 1))), dim3(256), 0, st, t->dh1,
                       (const float*)t->h1, n1, rows1, hid, 1.0f / (1.0f - t->drop_p), whole);
  } else {
    hipLaunchKernelGGL(relu_mask_kernel, dim3(blocks_256(rows1 * hid)), dim3(256), 0, st, t->dh1, (const float*)t->h1, n1, hid);
  }
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  // (the first layer's input is the feature table: no gradient)
  rc = gigl_linear_weight_grad_parts(ctx, t->dh1, t->a1, nullptr, n1, rows1, hid, d_in, t->part_w[0], t->bias[0] ? t->part_b[0] : nullptr);
  if (rc != GIGL_OK) return rc;
  AdamPack ap{};
  ap.n_src = 1;
  for (int l = 0; l < 2; ++l)
    for (int is_bias = 0; is_bias < (t->bias[l] ? 2 : 1); ++is_bias) {
      const int q = ap.count++;
      ap.p[q] = is_bias ? t->bias[l] : t->w[l];
      ap.m[q] = t->mom[4 * l + 2 * is_bias];
      ap.v[q] = t->mom[4 * l + 2 * is_bias + 1];
      ap.n[q] = is_bias ? (int64_t)t->dims[l + 1] : (int64_t)t->dims[l + 1] * t->dims[l];
      ap.part[0][q] = is_bias ? t->part_b[l] : t->part_w[l];
      ap.rows[0][q] = gcn_level(p, 1 - l);
      ap.rc[0][q] = t->part_rc[l];
    }
  ap.lr = t->lr;
  ap.beta1 = t->beta1;
  ap.beta2 = t->beta2;
  ap.eps = t->eps;
  ap.wd = t->wd;
  launch_adam(st, 208, ap, step_dev, (const int32_t*)un.meta, (const int32_t*)nullptr, (const int32_t*)(t->n_valid_buf + 2), nullptr);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

// elements of layer l's weight (is_bias: of its bias)
size_t gcn_tensor_floats(const gigl_gcn_train_plan* t, int l, int is_bias) {
  return is_bias ? (size_t)t->dims[l + 1] : (size_t)t->dims[l + 1] * t->dims[l];
}

}  // namespace

int32_t gigl_gcn_train_plan_destroy(gigl_gcn_train_plan* t) {
  if (!t) return GIGL_OK;
  nc_state_release(t);
  delete t;
  return GIGL_OK;
}

int32_t gigl_gcn_train_plan_create(gigl_ctx* ctx, gigl_graph* graph, gigl_feat* feat, int32_t b, const int32_t* fanouts,
                                   const int32_t* dims, float* const* w, float* const* bias, float lr, float beta1, float beta2,
                                   float eps, float weight_decay, gigl_gcn_train_plan** out) {
  if (!ctx || !out) return GIGL_E_INVALID_ARG;
  *out = nullptr;
  GIGL_REQUIRE(ctx, graph && feat && fanouts && dims && w, "null argument");
  GIGL_REQUIRE(ctx, b >= 1, "bad plan shape");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  gigl_gcn_train_plan* t = new (std::nothrow) gigl_gcn_train_plan();
  if (!t) return gigl_fail(ctx, GIGL_E_OOM, "host OOM");
  t->ctx = ctx;
  t->feat = feat;
  t->b = b;
  int32_t rc = gigl_ctx_create(ctx->device, &t->lctx);
  if (rc == GIGL_OK) rc = plan_check_layers(ctx, feat, 2, dims, w);
  if (rc == GIGL_OK) rc = t->ring.create(ctx, TRAIN_WS, 1, &b, graph, fanouts, 2, true);
  if (rc != GIGL_OK) {
    gigl_gcn_train_plan_destroy(t);
    return rc;
  }
  t->lr = lr;
  t->beta1 = beta1;
  t->beta2 = beta2;
  t->eps = eps;
  t->wd = weight_decay;
  auto floats = [&](size_t n) { return (float*)plan_alloc(t->owned, n * 4); };
  bool ok = true;
  for (int l = 0; l <= 2; ++l) t->dims[l] = dims[l];
  for (int l = 0; l < 2; ++l) {
    t->w[l] = w[l];
    t->bias[l] = bias ? bias[l] : nullptr;
    t->rows_cap[l] = gigl_level_rows(ctx->wide, b, fanouts, 2, 1 - l);
    for (int q = 0; q < 4; ++q) {
      const size_t n = gcn_tensor_floats(t, l, q >> 1);
      t->mom[4 * l + q] = floats(n);
      ok = ok && t->mom[4 * l + q] && hipMemset(t->mom[4 * l + q], 0, n * 4) == hipSuccess;
    }
    const int64_t chunks = gigl_linear_weight_grad_chunks(t->rows_cap[l], dims[l + 1], dims[l], &t->part_rc[l]);
    t->part_w[l] = floats((size_t)chunks * gcn_tensor_floats(t, l, 0));
    t->part_b[l] = floats((size_t)chunks * dims[l + 1]);
    ok = ok && t->part_w[l] && t->part_b[l];
  }
  const size_t rows1 = (size_t)t->rows_cap[0], rows0 = (size_t)t->rows_cap[1];
  t->wt2 = floats(gcn_tensor_floats(t, 1, 0));
  t->a1 = floats(rows1 * dims[0]);
  t->h1 = floats(rows1 * dims[1]);
  t->dh1 = floats(rows1 * dims[1]);
  t->a2 = floats(rows0 * dims[1]);
  t->da2 = floats(rows0 * dims[1]);
  t->out = floats(rows0 * dims[2]);
  // (the cleared block: the roots' loss gradient is ADDED to — two roots of a batch may be one node)
  ok = nc_state_alloc(*t, rows0 * dims[2]) && ok;
  t->g2 = (float*)t->zero_base;
  for (int k = 0; k < TRAIN_WS; ++k) {
    const gigl_union& un = t->ring.slot[k].base[0].un;
    t->dinv[k] = floats((size_t)un.cap_nodes);
    t->tlists[k] = (int32_t*)plan_alloc(t->owned, (size_t)gigl_transposed_rows_words(t->rows_cap[0], un.cap_edges) * 4);
    ok = ok && t->dinv[k] && t->tlists[k];
  }
  ok = ok && t->wt2 && t->a1 && t->h1 && t->dh1 && t->a2 && t->da2 && t->out;
  if (!ok) {
    gigl_gcn_train_plan_destroy(t);
    return gigl_fail(ctx, GIGL_E_OOM, "hipMalloc of the training workspace failed");
  }
  *out = t;
  return GIGL_OK;
}

int32_t gigl_gcn_train_plan_step2(gigl_gcn_train_plan* t, const uint32_t* roots, const int64_t* labels, int32_t n_valid,
                                  const uint32_t* roots_next, const uint32_t* roots_next2, int32_t sampling_seed, int32_t mode,
                                  float* loss_out) {
  if (!t) return GIGL_E_INVALID_ARG;
  TrainPrep pa{};  // train_stage_kernel clears the roots' loss gradient and lays out W2^T
  pa.zero = (uint32_t*)t->zero_base;
  pa.zero_words = (int64_t)(t->zero_bytes / 4);
  pa.w[0] = t->w[1];
  pa.wt[0] = t->wt2;
  pa.rows[0] = t->dims[2];
  pa.cols[0] = t->dims[1];
  pa.n_t = 1;
  return nc_train_step(
      t, roots, labels, n_valid, roots_next, roots_next2, sampling_seed, mode, loss_out, pa,
      [&](int kk) { return gcn_enqueue_graph(t, &t->ring.slot[kk].base[0], t->dinv[kk], t->tlists[kk], sampling_seed, mode); },
      [&](int k) { return gcn_enqueue_layers(t, k); });
}

const float* gigl_gcn_train_plan_loss(gigl_gcn_train_plan* t) { return t ? t->loss : nullptr; }

int32_t gigl_gcn_train_plan_resume(gigl_gcn_train_plan* t) { return t ? nc_resume(t) : GIGL_E_INVALID_ARG; }

int32_t gigl_gcn_train_plan_set_dropout(gigl_gcn_train_plan* t, float p, uint64_t seed) {
  if (!t) return GIGL_E_INVALID_ARG;
  return sage_set_dropout(t->ctx, *t, t->stepped, p, seed);
}

int32_t gigl_gcn_train_plan_moments(gigl_gcn_train_plan* t, int32_t layer, float* m_w, float* v_w, float* m_b, float* v_b) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, layer >= 0 && layer < 2, "layer %d", layer);
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  float* dst[4] = {m_w, v_w, m_b, v_b};
  for (int q = 0; q < 4; ++q)
    if (dst[q])
      GIGL_HIP_CHECK(ctx, hipMemcpyAsync(dst[q], t->mom[4 * layer + q], gcn_tensor_floats(t, layer, q >> 1) * 4,
                                         hipMemcpyDeviceToDevice, ctx->stream));
  return GIGL_OK;
}

int32_t gigl_gcn_train_plan_adopt(gigl_gcn_train_plan* dst, gigl_gcn_train_plan* src) {
  if (!dst || !src) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = dst->ctx;
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  GIGL_HIP_CHECK(ctx, hipStreamSynchronize(src->ctx->stream));
  for (int l = 0; l <= 2; ++l) GIGL_REQUIRE(ctx, dst->dims[l] == src->dims[l], "plans of different widths");
  for (int q = 0; q < 8; ++q)
    GIGL_HIP_CHECK(ctx, hipMemcpyAsync(dst->mom[q], src->mom[q], gcn_tensor_floats(dst, q >> 2, (q >> 1) & 1) * 4,
                                       hipMemcpyDeviceToDevice, ctx->stream));
  return nc_adopt_counter(dst, src);
}

// ------------------------------------------------------------------------------------------------------------------
// gigl_nablp_train_plan: one LINK-PREDICTION training step per call, all of it in the library (round 5) —
//   NodeAnchorBasedLinkPredictionModelingTaskSpec.train's loop body
//   (python/gigl/src/common/modeling_task_specs/node_anchor_based_link_prediction_modeling_task_spec.py:334-451):
//   infer_task_inputs (utils/infer.py: two encoder forwards — main batch, random-negative batch — query / positive /
//   random-negative embeddings by root index, inner-product scores of the repeated queries against cat(pos, rand_neg):
//   decoder.py:64-70), Retrieval.forward -> RetrievalLoss (loss.py:209-331: temperature, same-query and accidental-hit
//   masks, cross-entropy against the diagonal, summed, / rows), backward, Adam.
// with the reference's default encoder (GraphSAGE, mean, optional L2-normalised output).  Main batch = b anchors x
// (1 + P) rooted trees, anchor-major (anchor, its P positive slots; a missing positive repeats the anchor and is masked
// out by pos_cnt); random negatives = n_rn roots.  Everything is capacity-shaped (Q = b P query rows, C = Q + n_rn
// candidates, validity masks on the device): no host read, no torch kernel, one captured hipGraph per step.
// A plan created while gigl_ctx_set_lp_hard_negatives(ctx, H) holds H > 0 carries H HARD-NEGATIVE slots per anchor (the
// user-defined negative label edges of UserDefinedLabelsNodeAnchorBasedLinkPredictionTask): the main batch is b x T trees,
// T = 1 + P + H (anchor, positive slots, hard-negative slots; an empty slot repeats the anchor), pos_cnt is [2 b] words —
// positives per anchor, then hard negatives per anchor — and the candidates are cat(positives, hard negatives, random
// negatives) as in infer_task_inputs: columns [0, Q) the positives, Q + i H + k hard negative k of anchor i, Q + b H
// onwards the random negatives (C = Q + b H + n_rn).  A hard negative is a candidate of EVERY query row, whether or not
// its own anchor has a positive; the same-query mask covers the positives' block only, the accidental-hit mask every
// column.  The evaluation ranks against the random negatives alone (the reference's validate), its loss sees every column.
// H = 0 is the plan without them: the same launches, the same [b] counts.
namespace {
// The GAT kind's trainable tensors live in ONE table whose index is the one gigl_nablp_train_plan_moments publishes:
// 4 l + {w, att_src, att_dst, bias} for the core tensors, 8 + 3 l + {lin_edge.weight, att_edge, lin_edge_message.weight}
// for the edge tensors of gigl_gat_nablp_train_plan_set_edge_features.  gat_slot is the only place that computes it.
enum GatPart { GAT_W, GAT_ATT_SRC, GAT_ATT_DST, GAT_BIAS, GAT_W_EDGE, GAT_ATT_EDGE, GAT_W_MSG };
constexpr int GAT_CORE = 8, GAT_TENSORS = 14;
constexpr int gat_slot(GatPart part, int l) { return part < GAT_W_EDGE ? 4 * l + part : GAT_CORE + 3 * l + (part - GAT_W_EDGE); }
static_assert(gat_slot(GAT_W, 0) == 0 && gat_slot(GAT_ATT_SRC, 0) == 1 && gat_slot(GAT_ATT_DST, 0) == 2 && gat_slot(GAT_BIAS, 0) == 3 &&
              gat_slot(GAT_W, 1) == 4 && gat_slot(GAT_ATT_SRC, 1) == 5 && gat_slot(GAT_ATT_DST, 1) == 6 && gat_slot(GAT_BIAS, 1) == 7 &&
              gat_slot(GAT_W_EDGE, 0) == 8 && gat_slot(GAT_ATT_EDGE, 0) == 9 && gat_slot(GAT_W_MSG, 0) == 10 &&
              gat_slot(GAT_W_EDGE, 1) == 11 && gat_slot(GAT_ATT_EDGE, 1) == 12 && gat_slot(GAT_W_MSG, 1) == 13,
              "the published tensor indices");
// a forked step's second stream accumulates into slots of its own only where its backward writes a gradient directly: the
// second layer's attention vectors and bias, the edge weights (att_edge's comes from the fold of d v, after the join)
constexpr bool gat_slot_forks(int s) {
  return s < GAT_CORE ? s > gat_slot(GAT_W, 1) : s != gat_slot(GAT_ATT_EDGE, 0) && s != gat_slot(GAT_ATT_EDGE, 1);
}
struct PlanTensor {
  float* p = nullptr;                // the parameter: borrowed, UPDATED IN PLACE
  float* g[2] = {nullptr, nullptr};  // its gradient on the caller's stream; the forked stream's accumulator, or NULL
  float *m = nullptr, *v = nullptr;  // Adam's moments
  int64_t n = 0;                     // elements; 0: absent (no Adam entry, no export)
  void set(float* prm, int64_t elems) { p = prm; n = prm ? elems : 0; }
};
// what ONE stream's backward writes: sc[0] is sized for the larger encode (unforked, both encodes use it one after the
// other), sc[1] for the random negatives' and exists only when the step forks
struct GatScratch {
  gigl_ctx* ctx = nullptr;   // the stream's ctx: the plan's lctx (the caller's stream), actx (the forked one)
  int64_t rows1 = 0, b = 0;  // the row capacities it is sized for: nodes of level <= 1, roots
  float *alpha = nullptr, *dxw = nullptr, *ds = nullptr, *dd = nullptr, *dh0 = nullptr, *dh0s = nullptr, *dz = nullptr;
  float* du = nullptr;  // d u, laid out as u (out of the plan's cleared block: both encodes ADD)
  // edge features: d v laid out as v (out of the edge block), W_msg^T dy [rows1][H][De], layer 1's sum_e alpha_e e [b][De]
  float *dv = nullptr, *dze = nullptr, *z1 = nullptr;
};
}  // namespace

struct gigl_nablp_train_plan : SageTrainShared {  // (the GAT kind uses its L, dims, act_last and hyper-parameters only)
  gigl_ctx* ctx = nullptr;
  gigl_ctx* lctx = nullptr;  // private ctx (own arena) bound to the caller's stream: every launch of the step
  SageTrainEnc enc[2];       // 0: main batch, 1: random negatives
  int32_t b = 0, P = 0, H = 0, n_rn = 0, normalize = 0, remove_hits = 1;  // H: ctx->lp_hard_negatives at creation
  float temperature = 0.07f;
  // the job's one task (gigl_nablp_train_plan_set_task): GIGL_LP_TASK_*, Margin's margin | Softmax's temperature, its weight
  int32_t task_kind = GIGL_LP_TASK_RETRIEVAL;
  float task_param = 0.f, task_weight = 1.f;
  float* da = nullptr;        // gradient of a layer's operand (SAGE)
  void* zero_base = nullptr;  // both encodes' gw | gb | dh: cleared at the start of every step
  size_t zero_bytes = 0;
  // the head: repeated queries, candidates, ids, validity, scores and their gradients
  float *rq = nullptr, *cand = nullptr, *cand_t = nullptr, *scores = nullptr, *dscores = nullptr, *d_rq = nullptr, *d_cand = nullptr;
  int64_t *qid = nullptr, *cid = nullptr;
  int32_t* valid = nullptr;    // [C]: candidate column j takes part (rows i < Q use valid[i])
  int cand_cols() const { return b * (P + H) + n_rn; }                // C
  size_t cnt_words() const { return (size_t)b * (H > 0 ? 2 : 1); }   // of pos_cnt
  int32_t* pos_cnt = nullptr;  // [b] (H > 0: [2 b], the hard negatives' counts behind the positives') static copy of the step's input
  int32_t* consts = nullptr;   // device {Q, C, Adam step, ...}
  // loss[0] = the step's loss, loss[1] = valid query rows, loss[2] = a Margin / Softmax task's normaliser; row_lse / row_loss
  // hold that task's two row partials (gigl_lp_task_loss's row_a / row_b)
  float *row_lse = nullptr, *row_loss = nullptr, *loss = nullptr;
  // ---- GAT encoder (kind == 1, gigl_gat_nablp_train_plan_create): two layers, the first from the INPUT side
  int kind = 0;
  struct Gat {
    int32_t heads = 1, c0 = 0, c1 = 0, d_in = 0;
    float slope = 0.2f;
    PlanTensor tensor[GAT_TENSORS];  // parameters, gradients (both encodes ADD), Adam's moments
    PlanTensor& at(GatPart part, int l) { return tensor[gat_slot(part, l)]; }
    const PlanTensor& at(GatPart part, int l) const { return tensor[gat_slot(part, l)]; }
    float* u = nullptr;  // folded attention vectors [2H][d]
    // forward state per encode: z [H][rows1][d], xw [rows1][c1], out_pre [b][c1]
    float *z[2] = {nullptr, nullptr}, *xw[2] = {nullptr, nullptr}, *out_pre[2] = {nullptr, nullptr};
    GatScratch sc[2];  // backward scratch and accumulators per STREAM (a forked step folds sc[1]'s into sc[0]'s after the join)
    // (as the SAGE plans) the projections' weight gradients stay per-chunk partial sums — per encode: W1's, and W0's / b0's
    // per head — added up inside the Adam kernel; W1^T and the heads' W0^T are laid out once per step
    float* part_w1[2] = {nullptr, nullptr};
    int32_t rc_w1[2] = {0, 0};
    float* part_w0[2][4] = {{nullptr}};
    float* part_b0[2][4] = {{nullptr}};
    int32_t rc_w0[2] = {0, 0};
    float* wt1 = nullptr;
    float* wt0[4] = {nullptr};
    bool parts_pending = false;  // the gradient buffers do not hold the partial sums yet (gigl_gat_nablp_train_plan_grads adds them)
    // edge features (gigl_gat_nablp_train_plan_set_edge_features): the resident table is read in place through the batch
    // graphs' eid (written by the graph part).  The message weight's slot holds NULL (GATConv), its own buffer, or — shared —
    // lin_edge.weight's parameter AND gradient slots with n == 0: one tensor, one Adam entry, one update
    struct Edge {
      gigl_feat* table = nullptr;
      int32_t De = 0;
      float* v = nullptr;                 // folded att_edge, per step: [H][De] of layer 0, then [De] of layer 1
      void* zero_base = nullptr;          // the edge gradients | dv (| the forked stream's): cleared at the start of every step
      size_t zero_bytes = 0;
      float* ze[2] = {nullptr, nullptr};  // forward state per encode: sum_e alpha_e e of layer 0 [rows1][H][De]
    } e;
  } gat;
  __attribute__((noinline)) gigl_nablp_train_plan() = default;  // (out of line, as ever: the dynamic symbol table stays what it was)
  bool stepped = false;  // a step has run: the plan's shape is final
  // the optimiser's two other knobs (set after create, before the first step: the step is captured)
  AdamClip clip;           // gigl_nablp_train_plan_set_clip_grad_norm
  float lr_warm = 0.f;     // gigl_nablp_train_plan_set_constant_lr: lr * factor ...
  int32_t warm_iters = 0;  // ... for Adam's first warm_iters steps
  std::vector<void*> owned;
  // Two workspaces of trees + union graphs, two root sets each (0: main batch, 1: random negatives): the graph part of the
  // NEXT step's roots (sample + union of both root sets: latency-bound launches) runs on a side stream beside this step's layers
  static constexpr int WS = 2;
  PlanRing ring;
  int32_t* tlists[WS][2][GIGL_MAX_HOPS] = {{{nullptr}}};  // transposed lists of layers >= 1 per workspace and encode (SAGE; built by the graph part)
  // (round 6; GIGL_LP_FORK=0 turns it off) the random negatives' encode — ~15 launches of a 512-root batch, all latency — runs
  // on a stream of its own beside the main batch's, forward and backward: forked after the step's shared preparation, joined
  // before the scores, forked again after the loss's backward, joined before Adam.  Its only shared scratch is `da`.
  gigl_ctx* actx = nullptr;
  float* da2 = nullptr;
  hipEvent_t ev_fork[2] = {nullptr, nullptr}, ev_join[2] = {nullptr, nullptr};
  bool fork = false;
  // ... and the MAIN batch's weight gradients on a third: nothing in the backward chain waits for them (Adam does), each is a
  // 40-65 us matrix kernel between the chain's latency-bound ones
  gigl_ctx* wctx = nullptr;
  hipEvent_t ev_w = nullptr, ev_wjoin = nullptr;
  double* rank_part = nullptr;            // [b][2 + GIGL_LP_EVAL_MAX_KS]: the rank metrics' per-anchor values
};

namespace {

// e[r] = h[root_local[r]] (x 1 / max(|.|, 1e-12) when normalising: torch.nn.functional.normalize), one wave per root
__global__ __launch_bounds__(256) void lp_take_norm_kernel(const float* __restrict__ h, const int32_t* __restrict__ root_local,
                                                           int b, int d, int normalize, const int32_t* __restrict__ meta,
                                                           float* __restrict__ emb, float* __restrict__ inv) {
  const int lane = threadIdx.x & 63;
  const int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (r >= b) return;
  const bool failed = meta[GIGL_META_OVERFLOW] != 0;
  const int32_t l = failed ? -1 : root_local[r];
  float* o = emb + (int64_t)r * d;
  if (l < 0) {
    const float v = failed ? __builtin_nanf("") : 0.f;
    for (int c = lane; c < d; c += 64) o[c] = v;
    if (lane == 0) inv[r] = 0.f;
    return;
  }
  const float* row = h + (int64_t)l * d;
  float ss = 0.f;
  for (int c = lane; c < d; c += 64) ss += row[c] * row[c];
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
  const float iv = normalize ? 1.f / fmaxf(sqrtf(ss), 1e-12f) : 1.f;
  for (int c = lane; c < d; c += 64) o[c] = row[c] * iv;
  if (lane == 0) inv[r] = iv;
}

// the head's operands from the two encodes: row q = (anchor i, positive slot j) of rq = the anchor's embedding, row q of
// cand = that positive's; rows Q + i H + k of cand = hard negative k of anchor i (a candidate whether or not the anchor
// has a positive: the reference concatenates every root's); rows Q + b H.. = the random negatives'; ids for the loss
// masks; validity of every candidate
__global__ __launch_bounds__(256) void lp_pack_kernel(const float* __restrict__ e_main, const float* __restrict__ e_rn,
                                                      const uint32_t* __restrict__ roots_main,
                                                      const uint32_t* __restrict__ roots_rn,
                                                      const int32_t* __restrict__ pos_cnt, const float* __restrict__ inv_main,
                                                      const float* __restrict__ inv_rn, int b, int P, int H, int n_rn,
                                                      int d, float* __restrict__ rq, float* __restrict__ cand,
                                                      int64_t* __restrict__ qid, int64_t* __restrict__ cid,
                                                      int32_t* __restrict__ valid) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int Q = b * P, T = 1 + P + H, R0 = Q + b * H;
  if (row >= R0 + n_rn) return;
  if (row < Q) {
    const int i = row / P, j = row - i * P;
    const int ra = i * T, rp = ra + 1 + j;
    const uint32_t aid = roots_main[ra], pid = roots_main[rp];
    const bool ok = aid != GIGL_INVALID && pid != GIGL_INVALID && j < pos_cnt[i] && inv_main[ra] != 0.f && inv_main[rp] != 0.f;
    const float* qa = e_main + (int64_t)ra * d;
    const float* pa = e_main + (int64_t)rp * d;
    for (int c = lane; c < d; c += 64) {
      rq[(int64_t)row * d + c] = ok ? qa[c] : 0.f;
      cand[(int64_t)row * d + c] = ok ? pa[c] : 0.f;
    }
    if (lane == 0) {
      qid[row] = (int64_t)aid;
      cid[row] = (int64_t)pid;
      valid[row] = ok ? 1 : 0;
    }
  } else if (row < R0) {
    const int i = (row - Q) / H, k = (row - Q) - i * H;
    const int ra = i * T, rh = ra + 1 + P + k;
    const uint32_t id = roots_main[rh];
    const bool ok = roots_main[ra] != GIGL_INVALID && id != GIGL_INVALID && k < pos_cnt[b + i] && inv_main[rh] != 0.f;
    const float* ea = e_main + (int64_t)rh * d;
    for (int c = lane; c < d; c += 64) cand[(int64_t)row * d + c] = ok ? ea[c] : 0.f;
    if (lane == 0) {
      cid[row] = (int64_t)id;
      valid[row] = ok ? 1 : 0;
    }
  } else {
    const int r = row - R0;
    const uint32_t id = roots_rn[r];
    const bool ok = id != GIGL_INVALID && inv_rn[r] != 0.f;
    const float* ea = e_rn + (int64_t)r * d;
    for (int c = lane; c < d; c += 64) cand[(int64_t)row * d + c] = ok ? ea[c] : 0.f;
    if (lane == 0) {
      cid[row] = (int64_t)id;
      valid[row] = ok ? 1 : 0;
    }
  }
}

// d emb of the two encodes from d rq / d cand: an anchor's row sums its P query rows, a positive's row is its candidate
// row, a hard negative's and a random negative's their own; then through the normalisation (dx = (g - y <y, g>) / max(|x|, eps)) and added to the
// last layer's output gradient at the root's local row (roots that are the same node share it: atomics).  One wave per root.
__global__ __launch_bounds__(256) void lp_unpack_scatter_kernel(const float* __restrict__ d_rq, const float* __restrict__ d_cand,
                                                                const int32_t* __restrict__ valid, const float* __restrict__ emb,
                                                                const float* __restrict__ inv,
                                                                const int32_t* __restrict__ root_local, int which, int b, int P,
                                                                int H, int n_rn, int d, int normalize,
                                                                float* __restrict__ dh_last) {
  const int lane = threadIdx.x & 63;
  const int r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int T = 1 + P + H, Q = b * P, R0 = Q + b * H;
  const int n_roots = which == 0 ? b * T : n_rn;
  if (r >= n_roots) return;
  const float iv = inv[r];
  if (iv == 0.f) return;
  const int32_t l = root_local[r];
  if (l < 0) return;
  const float* y = emb + (int64_t)r * d;
  float dot = 0.f;
  // (d <= 64 * 8: a lane keeps up to 8 columns)
  float g[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int c = lane + 64 * u;
    float v = 0.f;
    if (c < d) {
      if (which == 1) {
        v = valid[R0 + r] ? d_cand[(int64_t)(R0 + r) * d + c] : 0.f;
      } else {
        const int i = r / T, t = r - i * T;
        if (t == 0) {
          for (int j = 0; j < P; ++j)
            if (valid[i * P + j]) v += d_rq[(int64_t)(i * P + j) * d + c];
        } else {
          const int col = t <= P ? i * P + t - 1 : Q + i * H + t - 1 - P;
          if (valid[col]) v = d_cand[(int64_t)col * d + c];
        }
      }
      dot += v * y[c];
    }
    g[u] = v;
  }
  for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off, 64);
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int c = lane + 64 * u;
    if (c < d) {
      const float dx = normalize ? (g[u] - y[c] * dot) * iv : g[u];
      if (dx != 0.f) atomicAdd(&dh_last[(int64_t)l * d + c], dx);
    }
  }
}

// an encode's forward and the roots' embeddings; the random negatives' on the forked stream
int32_t lp_forward(gigl_nablp_train_plan* t, int which, bool train) {
  const SageTrainEnc& e = t->enc[which];
  gigl_ctx* ctx = which == 1 && t->fork ? t->actx : t->lctx;
  const int32_t rc = sage_enc_forward(ctx, *t, e, e.base, train, which, t->consts + 2);
  if (rc != GIGL_OK) return rc;
  hipLaunchKernelGGL(lp_take_norm_kernel, dim3((unsigned)((e.b + 3) / 4)), dim3(256), 0, ctx->stream, (const float*)e.h[t->L - 1],
                     (const int32_t*)e.base->un.root_local, e.b, t->dims[t->L], t->normalize, (const int32_t*)e.base->un.meta, e.emb,
                     e.inv);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

// an encode's backward over workspace w: the random negatives' on the forked stream with its own `da`, the main batch's
// weight gradients on the third stream (see wctx)
int32_t lp_backward(gigl_nablp_train_plan* t, int which, int w) {
  const SageTrainEnc& e = t->enc[which];
  const bool alt = which == 1 && t->fork;
  return sage_enc_backward(alt ? t->actx : t->lctx, *t, e, e.base, t->tlists[w][which], alt ? t->da2 : t->da,
                           which == 0 && t->fork ? t->wctx : nullptr, t->ev_w);
}

// every launch of a step, on lctx's stream (the caller's)
int32_t gat_lp_begin(gigl_nablp_train_plan* t);
int32_t gat_lp_forward(gigl_nablp_train_plan* t, int which);
int32_t gat_lp_backward(gigl_nablp_train_plan* t, int which);
int32_t gat_lp_finish(gigl_nablp_train_plan* t);

// sample + union of both root sets of workspace w, on its side stream (bwd_gather is a SAGE encoder's: no lists for the GAT kind)
int32_t lp_enqueue_graph(gigl_nablp_train_plan* t, int w, int32_t sampling_seed, int32_t mode) {
  for (int k = 0; k < 2; ++k) {
    const int32_t rc = sage_enqueue_graph(*t, t->enc[k], &t->ring.slot[w].base[k], t->tlists[w][k], sampling_seed, mode);
    if (rc != GIGL_OK) return rc;
  }
  return GIGL_OK;
}

// the job's task over the plan's scores, ids and validity words (loss.hip)
LpTaskHead lp_task_head(const gigl_nablp_train_plan* t) {
  const bool retrieval = t->task_kind == GIGL_LP_TASK_RETRIEVAL;
  return LpTaskHead{t->task_kind, retrieval ? t->temperature : t->task_param, t->task_weight, t->scores, (int64_t)t->cand_cols(),
                    t->b, t->P, t->H, t->n_rn, t->pos_cnt, t->valid, t->qid, t->remove_hits ? t->cid : nullptr};
}

// the forward half of the layers part over workspace w: both encodes, the head's operands, the scores, the loss rows
// (shared by the training step — train: with the plan's dropout — and gigl_nablp_train_plan_eval, which runs without)
int32_t lp_enqueue_forward(gigl_nablp_train_plan* t, int w, bool train) {
  gigl_ctx* ctx = t->lctx;
  hipStream_t st = ctx->stream;
  const int L = t->L, d = t->dims[L], Q = t->b * t->P, Cn = t->cand_cols();
  int32_t rc = GIGL_OK;
  for (int k = 0; k < 2; ++k) t->enc[k].base = &t->ring.slot[w].base[k];
  gigl_fill_u32(st, t->zero_base, 0u, (int64_t)(t->zero_bytes / 4));
  if (t->kind == 1) {
    rc = gat_lp_begin(t);
    if (rc != GIGL_OK) return rc;
  }
  for (int l = 1; l < L && t->kind == 0; ++l)  // W_l^T for the input gradients of both encodes
    gigl_transpose_f32(st, t->w[l], t->dims[l + 1], 2 * t->dims[l], t->wt_l[l]);
  if (t->fork) {
    GIGL_HIP_CHECK(ctx, hipEventRecord(t->ev_fork[0], st));
    GIGL_HIP_CHECK(ctx, hipStreamWaitEvent(t->actx->stream, t->ev_fork[0], 0));
  }
  for (int k = 0; k < 2; ++k) {
    rc = t->kind == 1 ? gat_lp_forward(t, k) : lp_forward(t, k, train);
    if (rc != GIGL_OK) return rc;
  }
  if (t->fork) {
    GIGL_HIP_CHECK(ctx, hipEventRecord(t->ev_join[0], t->actx->stream));
    GIGL_HIP_CHECK(ctx, hipStreamWaitEvent(st, t->ev_join[0], 0));
  }
  const BatchGraph *pm = t->enc[0].base, *pr = t->enc[1].base;
  hipLaunchKernelGGL(lp_pack_kernel, dim3((unsigned)((Cn + 3) / 4)), dim3(256), 0, st, (const float*)t->enc[0].emb,
                     (const float*)t->enc[1].emb, (const uint32_t*)pm->roots_buf, (const uint32_t*)pr->roots_buf,
                     (const int32_t*)t->pos_cnt, (const float*)t->enc[0].inv, (const float*)t->enc[1].inv, t->b, t->P, t->H,
                     t->n_rn, d, t->rq, t->cand, t->qid, t->cid, t->valid);
  // scores[q][c] = <rq[q], cand[c]>  (decoder.py:64-70: torch.mm(q, c.T))
  rc = gigl_linear(ctx, t->rq, t->cand, nullptr, t->consts + 0, Q, d, Cn, 0, t->scores);
  if (rc != GIGL_OK) return rc;
  gigl_lp_task_rows_enqueue(st, lp_task_head(t), t->row_lse, t->row_loss);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

// everything after the graph part, over workspace w's trees and union graphs, on lctx's stream (the caller's)
int32_t lp_enqueue_layers(gigl_nablp_train_plan* t, int w) {
  gigl_ctx* ctx = t->lctx;
  hipStream_t st = ctx->stream;
  const int L = t->L, d = t->dims[L], Q = t->b * t->P, Cn = t->cand_cols();
  int32_t rc = lp_enqueue_forward(t, w, true);
  if (rc != GIGL_OK) return rc;
  const BatchGraph *pm = t->enc[0].base, *pr = t->enc[1].base;
  const LpTaskHead h = lp_task_head(t);
  gigl_lp_task_sum_enqueue(st, h, t->row_lse, t->row_loss, t->loss, t->consts + 2, (const int32_t*)pm->un.meta,
                           (const int32_t*)pr->un.meta, nullptr, nullptr);
  gigl_lp_task_backward_enqueue(st, h, t->row_lse, t->row_loss, t->loss, t->dscores, (int64_t)Cn);
  // d rq = dscores . cand ;  d cand = dscores^T . rq
  gigl_transpose_f32(st, t->cand, Cn, d, t->cand_t);
  rc = gigl_linear(ctx, t->dscores, t->cand_t, nullptr, t->consts + 0, Q, Cn, d, 0, t->d_rq);
  if (rc != GIGL_OK) return rc;
  gigl_fill_u32(st, t->d_cand, 0u, (int64_t)Cn * d);  // (gigl_linear_weight_grad ADDS its chunks' sums to dw)
  rc = gigl_linear_weight_grad(ctx, t->dscores, t->rq, nullptr, t->consts + 0, Q, Cn, d, t->d_cand, nullptr);
  if (rc != GIGL_OK) return rc;
  for (int k = 0; k < 2; ++k) {
    const SageTrainEnc& e = t->enc[k];
    hipLaunchKernelGGL(lp_unpack_scatter_kernel, dim3((unsigned)((e.b + 3) / 4)), dim3(256), 0, st, (const float*)t->d_rq,
                       (const float*)t->d_cand, (const int32_t*)t->valid, (const float*)e.emb, (const float*)e.inv,
                       (const int32_t*)e.base->un.root_local, k, t->b, t->P, t->H, t->n_rn, d, t->normalize, e.dh[L - 1]);
  }
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  if (t->fork) {
    GIGL_HIP_CHECK(ctx, hipEventRecord(t->ev_fork[1], st));
    GIGL_HIP_CHECK(ctx, hipStreamWaitEvent(t->actx->stream, t->ev_fork[1], 0));
  }
  for (int k = 0; k < 2; ++k) {
    rc = t->kind == 1 ? gat_lp_backward(t, k) : lp_backward(t, k, w);
    if (rc != GIGL_OK) return rc;
  }
  if (t->fork) {
    GIGL_HIP_CHECK(ctx, hipEventRecord(t->ev_join[1], t->actx->stream));
    GIGL_HIP_CHECK(ctx, hipStreamWaitEvent(st, t->ev_join[1], 0));
    if (t->wctx) {
      GIGL_HIP_CHECK(ctx, hipEventRecord(t->ev_wjoin, t->wctx->stream));
      GIGL_HIP_CHECK(ctx, hipStreamWaitEvent(st, t->ev_wjoin, 0));
    }
  }
  if (t->kind == 1) return gat_lp_finish(t);
  AdamPack ap = sage_adam_pack(*t, &t->enc[0], pm, &t->enc[1], pr);
  ap.lr_warm = t->lr_warm;
  ap.warm_iters = t->warm_iters;
  launch_adam(st, 208, ap, (const int32_t*)(t->consts + 2), (const int32_t*)pm->un.meta, (const int32_t*)pr->un.meta,
              (const int32_t*)nullptr, &t->clip);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

// ---- what the two link-prediction plans' creation shares (t->ctx, b, P, n_rn are set)

// the layers' ctx and the ring: per workspace the two root sets' batch graphs (number_every_node: batch_graph_init)
int32_t lp_create_workspaces(gigl_nablp_train_plan* t, gigl_graph* graph, gigl_feat* feat, const int32_t* fanouts, int32_t hops,
                             const int32_t* dims, float* const* w, bool number_every_node) {
  gigl_ctx* ctx = t->ctx;
  t->feat = feat;
  int32_t rc = plan_check_layers(ctx, feat, hops, dims, w);
  if (rc == GIGL_OK) rc = gigl_ctx_create(ctx->device, &t->lctx);
  const int32_t nb[2] = {t->b * (1 + t->P + t->H), t->n_rn > 0 ? t->n_rn : 1};
  for (int k = 0; k < 2; ++k) t->enc[k].b = nb[k];
  if (rc == GIGL_OK) rc = t->ring.create(ctx, gigl_nablp_train_plan::WS, 2, nb, graph, fanouts, hops, number_every_node);
  if (rc == GIGL_OK)
    for (int k = 0; k < 2; ++k) t->enc[k].base = &t->ring.slot[0].base[k];
  return rc;
}

// the head over embeddings of width d: the encodes' root rows, repeated queries, candidates, ids, validity, scores, their
// gradients, the loss words; consts = {Q, C, Adam's step counter}
bool lp_head_alloc(gigl_nablp_train_plan* t, size_t d) {
  auto alloc = [&](size_t bytes) { return plan_alloc(t->owned, bytes); };
  const size_t Q = (size_t)t->b * t->P, Cn = (size_t)t->cand_cols();
  bool ok = true;
  for (SageTrainEnc& e : t->enc) {
    e.emb = (float*)alloc((size_t)e.b * d * 4);
    e.inv = (float*)alloc((size_t)e.b * 4);
    ok = ok && e.emb && e.inv;
  }
  t->rq = (float*)alloc(Q * d * 4);
  t->cand = (float*)alloc(Cn * d * 4);
  t->cand_t = (float*)alloc(Cn * d * 4);
  t->scores = (float*)alloc(Q * Cn * 4);
  t->dscores = (float*)alloc(Q * Cn * 4);
  t->d_rq = (float*)alloc(Q * d * 4);
  t->d_cand = (float*)alloc(Cn * d * 4);
  t->qid = (int64_t*)alloc(Q * 8);
  t->cid = (int64_t*)alloc(Cn * 8);
  t->valid = (int32_t*)alloc(Cn * 4);
  t->pos_cnt = (int32_t*)alloc(t->cnt_words() * 4);
  t->consts = (int32_t*)alloc(64);
  t->row_lse = (float*)alloc(Q * 4);
  t->row_loss = (float*)alloc(Q * 4);
  t->loss = (float*)alloc(64);
  t->rank_part = (double*)alloc((size_t)t->b * (2 + GIGL_LP_EVAL_MAX_KS) * sizeof(double));
  ok = ok && t->rank_part && t->rq && t->cand && t->cand_t && t->scores && t->dscores && t->d_rq && t->d_cand && t->qid && t->cid && t->valid &&
       t->pos_cnt && t->consts && t->row_lse && t->row_loss && t->loss;
  const int32_t c[16] = {(int32_t)Q, (int32_t)Cn, 0 /* Adam's step counter */, 0};
  return ok && hipMemcpy(t->consts, c, sizeof(c), hipMemcpyHostToDevice) == hipSuccess && hipMemset(t->loss, 0, 64) == hipSuccess;
}

// (default on, GIGL_LP_FORK=0 off) the random negatives' encode on a stream of its own
bool lp_fork_wanted(const gigl_nablp_train_plan* t) {
  const char* fork_env = getenv("GIGL_LP_FORK");
  return t->n_rn > 0 && !(fork_env && fork_env[0] == '0');
}

// the forked streams' ctxs and events (the second encode's own scratch is its plan's business); -> t->fork
bool lp_fork_setup(gigl_nablp_train_plan* t) {
  bool ok = gigl_ctx_create(t->ctx->device, &t->actx) == GIGL_OK;
  for (int i = 0; i < 2 && ok; ++i)
    ok = hipEventCreateWithFlags(&t->ev_fork[i], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&t->ev_join[i], hipEventDisableTiming) == hipSuccess;
  // a third stream for the main batch's weight gradients (the GAT plan's 768-wide ones fill the GPU and slow the chain
  // beside them: measured, see gat_lp_backward)
  if (ok && t->kind == 0)
    ok = gigl_ctx_create(t->ctx->device, &t->wctx) == GIGL_OK &&
         hipEventCreateWithFlags(&t->ev_w, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&t->ev_wjoin, hipEventDisableTiming) == hipSuccess;
  t->fork = ok;
  return ok;
}

// a plan of `kind` with what both kinds' creation is handed: batch shape, head, Adam's hyper-parameters (NULL: no memory)
static gigl_nablp_train_plan* lp_plan_new(gigl_ctx* ctx, int kind, int32_t L, int32_t b_anchors, int32_t num_positives,
                                   int32_t n_random_negatives, int32_t act_last, int32_t l2_normalize, float temperature,
                                   int32_t remove_accidental_hits, float lr, float beta1, float beta2, float eps,
                                   float weight_decay) {
  gigl_nablp_train_plan* t = new (std::nothrow) gigl_nablp_train_plan();
  if (!t) return nullptr;
  t->ctx = ctx;
  t->kind = kind;
  t->L = L;
  t->b = b_anchors;
  t->P = num_positives;
  t->H = ctx->lp_hard_negatives;
  t->n_rn = n_random_negatives;
  t->normalize = l2_normalize ? 1 : 0;
  t->remove_hits = remove_accidental_hits ? 1 : 0;
  t->temperature = temperature;
  t->act_last = act_last;
  t->lr = lr;
  t->beta1 = beta1;
  t->beta2 = beta2;
  t->eps = eps;
  t->wd = weight_decay;
  return t;
}

}  // namespace

int32_t gigl_nablp_train_plan_destroy(gigl_nablp_train_plan* t) {
  if (!t) return GIGL_OK;
  if (t->ctx) {
    hipSetDevice(t->ctx->device);
    hipStreamSynchronize(t->ctx->stream);
  }
  t->ring.release();
  if (t->actx) hipStreamSynchronize(t->actx->stream);
  if (t->wctx) hipStreamSynchronize(t->wctx->stream);
  if (t->ev_w) hipEventDestroy(t->ev_w);
  if (t->ev_wjoin) hipEventDestroy(t->ev_wjoin);
  for (int i = 0; i < 2; ++i) {
    if (t->ev_fork[i]) hipEventDestroy(t->ev_fork[i]);
    if (t->ev_join[i]) hipEventDestroy(t->ev_join[i]);
  }
  for (void* q : t->owned) hipFree(q);
  t->ring.destroy_ctxs();
  if (t->actx) gigl_ctx_destroy(t->actx);
  if (t->wctx) gigl_ctx_destroy(t->wctx);
  if (t->lctx) {
    gigl_ctx_set_stream(t->lctx, nullptr);  // (the stream is the caller's)
    gigl_ctx_destroy(t->lctx);
  }
  delete t;
  return GIGL_OK;
}

int32_t gigl_nablp_train_plan_create(gigl_ctx* ctx, gigl_graph* graph, gigl_feat* feat, int32_t b_anchors,
                                     int32_t num_positives, int32_t n_random_negatives, const int32_t* fanouts, int32_t hops,
                                     const int32_t* dims, float* const* w, float* const* bias, int32_t act_last,
                                     int32_t l2_normalize, float temperature, int32_t remove_accidental_hits, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, gigl_nablp_train_plan** out) {
  if (!ctx || !out) return GIGL_E_INVALID_ARG;
  *out = nullptr;
  GIGL_REQUIRE(ctx, graph && feat && fanouts && dims && w, "null argument");
  GIGL_REQUIRE(ctx, hops >= 1 && hops <= GIGL_MAX_HOPS && b_anchors >= 1 && num_positives >= 1 && n_random_negatives >= 0,
               "bad plan shape");
  GIGL_REQUIRE(ctx, dims[hops] <= 512, "embedding width %d: the head keeps a row in 8 registers per lane (<= 512)", dims[hops]);
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  gigl_nablp_train_plan* t = lp_plan_new(ctx, 0, hops, b_anchors, num_positives, n_random_negatives, act_last, l2_normalize,
                                         temperature, remove_accidental_hits, lr, beta1, beta2, eps, weight_decay);
  if (!t) return gigl_fail(ctx, GIGL_E_OOM, "host OOM");
  const int32_t rc = lp_create_workspaces(t, graph, feat, fanouts, hops, dims, w, false);
  if (rc != GIGL_OK) {
    gigl_nablp_train_plan_destroy(t);
    return rc;
  }
  auto alloc = [&](size_t bytes) { return plan_alloc(t->owned, bytes); };
  size_t zero_floats = 0, da_floats = 16;
  bool ok = sage_shared_alloc(*t, t->owned, dims, w, bias);
  // (gw | gb are part of the cleared block: gigl_nablp_train_plan_grads adds the partial sums up into them)
  for (SageTrainEnc& e : t->enc) ok = sage_enc_alloc(*t, e, t->owned, ctx->wide, fanouts, true, &zero_floats, &da_floats) && ok;
  float* z = (float*)alloc(zero_floats * 4);
  t->zero_base = z;
  t->zero_bytes = zero_floats * 4;
  for (int k = 0; k < 2 && z; ++k) z = sage_enc_carve(*t, t->enc[k], true, z);
  for (int wi = 0; wi < gigl_nablp_train_plan::WS; ++wi)
    for (int k = 0; k < 2; ++k)
      ok = sage_tlists_alloc(*t, t->enc[k], t->owned, t->ring.slot[wi].base[k].un.cap_edges, t->tlists[wi][k]) && ok;
  t->da = (float*)alloc(da_floats * 4);
  ok = ok && t->zero_base && t->da && lp_head_alloc(t, (size_t)dims[hops]);
  // (GIGL_LP_FORK=0 off: 1.18 -> 1.07 ms per step, bit-identical results.  The forked step's layers part is
  // launched EAGERLY, not replayed: captured, the two-branch graph brought the whole GPU suite down with a segmentation fault
  // inside a step — ~400 tests into the session, three runs of three — and never in six runs once it was launched eagerly)
  if (ok && lp_fork_wanted(t)) {
    t->da2 = (float*)alloc(da_floats * 4);
    ok = t->da2 != nullptr && lp_fork_setup(t);
  }
  if (!ok) {
    gigl_nablp_train_plan_destroy(t);
    return gigl_fail(ctx, GIGL_E_OOM, "hipMalloc of the link-prediction training workspace failed");
  }
  *out = t;
  return GIGL_OK;
}

namespace {
// the graph part of workspace w for these roots: sample + union of both root sets (no random negatives: one absent root)
int32_t lp_issue_graph(gigl_nablp_train_plan* t, int w, PlanRing::Family fam, const uint32_t* main_roots,
                       const uint32_t* rn_roots, int32_t sampling_seed, int32_t mode) {
  const uint32_t* roots[2] = {main_roots, rn_roots};
  const size_t count[2] = {(size_t)t->enc[0].b, (size_t)t->n_rn};
  return t->ring.issue_graph_part(w, fam, roots, count, train_part_captures(0),
                                  [&]() { return lp_enqueue_graph(t, w, sampling_seed, mode); });
}
}  // namespace

int32_t gigl_nablp_train_plan_step2(gigl_nablp_train_plan* t, const uint32_t* main_roots, const int32_t* pos_cnt,
                                    const uint32_t* rn_roots, const uint32_t* next_main_roots, const uint32_t* next_rn_roots,
                                    int32_t sampling_seed, int32_t mode, float* loss_out) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, main_roots && pos_cnt && (rn_roots || t->n_rn == 0), "null argument");
  GIGL_REQUIRE(ctx, !next_main_roots || next_rn_roots || t->n_rn == 0, "the next step's random negatives are missing");
  if (mode == GIGL_MODE_REPLACE)
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "the training plan needs duplicate-free trees (no with-replacement mode)");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  t->gat.parts_pending = t->kind == 1;  // (this step's gradient buffers will lack the partial sums)
  t->stepped = true;
  hipStream_t st = ctx->stream;
  int32_t rc = train_bind_stream(ctx, t->lctx);
  if (rc != GIGL_OK) return rc;
  PlanRing& ring = t->ring;
  ring.reseed(PlanRing::TRAIN, sampling_seed, mode);
  const int w = ring.cur;
  PlanRing::Slot& wk = ring.slot[w];
  // this step's trees: prefetched by the previous call for exactly these buffers, or sampled now
  if (!ring.holds(w, main_roots, rn_roots)) {
    rc = lp_issue_graph(t, w, PlanRing::TRAIN, main_roots, rn_roots, sampling_seed, mode);
    if (rc != GIGL_OK) return rc;
  }
  ring.consume(w);
  const int wn = (w + 1) % gigl_nablp_train_plan::WS;
  if (next_main_roots) {  // the next step's graph part goes to the other workspace, beside this step's layers
    rc = lp_issue_graph(t, wn, PlanRing::TRAIN, next_main_roots, next_rn_roots, sampling_seed, mode);
    if (rc != GIGL_OK) return rc;
  }
  GIGL_HIP_CHECK(ctx, hipMemcpyAsync(t->pos_cnt, pos_cnt, t->cnt_words() * 4, hipMemcpyDeviceToDevice, st));
  GIGL_HIP_CHECK(ctx, hipStreamWaitEvent(st, wk.ev_graph, 0));
  // (a forked step is launched eagerly: as fast as its replay — 1.07 / 1.71 ms both ways — and no graph with a second branch is
  // ever instantiated; see DESIGN_HISTORY "Round 6" for what those did to a long session)
  if (t->fork) rc = lp_enqueue_layers(t, w);
  else rc = gigl_run_part(t->lctx, t->lctx, &wk.layers, train_part_captures(1), "training step", [&]() { return lp_enqueue_layers(t, w); });
  if (rc != GIGL_OK) return gigl_fail(ctx, rc, "%s", gigl_last_error(t->lctx));
  GIGL_HIP_CHECK(ctx, hipEventRecord(wk.ev_layers, st));
  if (loss_out) GIGL_HIP_CHECK(ctx, hipMemcpyAsync(loss_out, t->loss, 8, hipMemcpyDeviceToDevice, st));
  if (next_main_roots) ring.cur = wn;
  return GIGL_OK;
}

int32_t gigl_nablp_train_plan_step(gigl_nablp_train_plan* t, const uint32_t* main_roots, const int32_t* pos_cnt,
                                   const uint32_t* rn_roots, int32_t sampling_seed, int32_t mode, float* loss_out) {
  return gigl_nablp_train_plan_step2(t, main_roots, pos_cnt, rn_roots, nullptr, nullptr, sampling_seed, mode, loss_out);
}

int32_t gigl_nablp_train_plan_eval(gigl_nablp_train_plan* t, const uint32_t* main_roots, const int32_t* pos_cnt,
                                   const uint32_t* rn_roots, int32_t sampling_seed, int32_t mode, const int32_t* ks,
                                   int32_t n_ks, double* acc, int32_t* overflow_acc) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, main_roots && pos_cnt && (rn_roots || t->n_rn == 0) && ks && acc && overflow_acc, "null argument");
  if (mode == GIGL_MODE_REPLACE)
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "the training plan needs duplicate-free trees (no with-replacement mode)");
  GIGL_REQUIRE(ctx, n_ks >= 1 && n_ks <= GIGL_LP_EVAL_MAX_KS, "n_ks=%d outside [1, %d]", n_ks, GIGL_LP_EVAL_MAX_KS);
  for (int i = 0; i < n_ks; ++i) GIGL_REQUIRE(ctx, ks[i] >= 1, "ks must be greater-or-equal to 1 (got %d)", ks[i]);
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  int32_t rc = train_bind_stream(ctx, t->lctx);
  if (rc != GIGL_OK) return rc;
  PlanRing& ring = t->ring;
  ring.reseed(PlanRing::EVAL, sampling_seed, mode);
  // the workspace that holds no announced batch (a _step2 with next roots left its graph part in slot[cur])
  const int w = ring.slot[ring.cur].fetched ? (ring.cur + 1) % gigl_nablp_train_plan::WS : ring.cur;
  PlanRing::Slot& wk = ring.slot[w];
  GIGL_REQUIRE(ctx, !wk.fetched, "both workspaces hold an announced batch");
  rc = lp_issue_graph(t, w, PlanRing::EVAL, main_roots, rn_roots, sampling_seed, mode);
  if (rc != GIGL_OK) return rc;
  GIGL_HIP_CHECK(ctx, hipMemcpyAsync(t->pos_cnt, pos_cnt, t->cnt_words() * 4, hipMemcpyDeviceToDevice, st));
  GIGL_HIP_CHECK(ctx, hipStreamWaitEvent(st, wk.ev_graph, 0));
  // (eager: no captured layers graph is made or invalidated — and none with a second branch, see gigl_nablp_train_plan_create)
  BatchGraph* const held[2] = {t->enc[0].base, t->enc[1].base};
  rc = lp_enqueue_forward(t, w, false);
  const BatchGraph *pm = &wk.base[0], *pr = &wk.base[1];
  for (int k = 0; k < 2; ++k) t->enc[k].base = held[k];
  if (rc != GIGL_OK) return gigl_fail(ctx, rc, "%s", gigl_last_error(t->lctx));
  const int Q = t->b * t->P;
  gigl_lp_task_sum_enqueue(st, lp_task_head(t), t->row_lse, t->row_loss, nullptr, nullptr, (const int32_t*)pm->un.meta,
                           (const int32_t*)pr->un.meta, acc, overflow_acc);
  const int R0 = Q + t->b * t->H;  // (ranked against the random negatives only, as the reference's validate does)
  rc = gigl_lp_rank_metrics_enqueue(t->lctx, st, t->scores, (int64_t)t->cand_cols(), t->b, t->P, t->pos_cnt, t->n_rn, R0,
                                    t->valid + R0, ks, n_ks, pm->un.meta, pr->un.meta, t->rank_part, acc);
  if (rc != GIGL_OK) return gigl_fail(ctx, rc, "%s", gigl_last_error(t->lctx));
  GIGL_HIP_CHECK(ctx, hipEventRecord(wk.ev_layers, st));
  return GIGL_OK;
}

const float* gigl_nablp_train_plan_loss(gigl_nablp_train_plan* t) { return t ? t->loss : nullptr; }

int32_t gigl_nablp_train_plan_adam_steps(gigl_nablp_train_plan* t, int32_t* out) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, out, "null output");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  GIGL_HIP_CHECK(ctx, hipMemcpyAsync(out, t->consts + 2, 4, hipMemcpyDeviceToDevice, ctx->stream));
  return GIGL_OK;
}

int32_t gigl_nablp_train_plan_set_clip_grad_norm(gigl_nablp_train_plan* t, float max_norm) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, !t->stepped, "gradient clipping is set after create and before the first step (the step is captured)");
  GIGL_REQUIRE(ctx, std::isfinite(max_norm) && max_norm > 0.f, "max_norm must be finite and > 0");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (!t->clip.partials) {
    t->clip.partials = (double*)plan_alloc(t->owned, (size_t)ADAM_MAX * ADAM_GRID_X_MAX * sizeof(double));
    t->clip.out2 = (float*)plan_alloc(t->owned, 16);
    if (!t->clip.partials || !t->clip.out2) {
      t->clip = AdamClip{};
      return gigl_fail(ctx, GIGL_E_OOM, "hipMalloc of the gradient norm's partial sums failed");
    }
    GIGL_HIP_CHECK(ctx, hipMemset(t->clip.out2, 0, 16));
  }
  t->clip.max_norm = max_norm;
  return GIGL_OK;
}

int32_t gigl_nablp_train_plan_set_task(gigl_nablp_train_plan* t, int32_t kind, float param, float weight) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, !t->stepped, "the task is set after create and before the first step (the step is captured)");
  const int32_t rc = gigl_lp_task_check(ctx, kind, param, weight);
  if (rc != GIGL_OK) return rc;
  t->task_kind = kind;
  t->task_param = kind == GIGL_LP_TASK_RETRIEVAL ? 0.f : param;
  t->task_weight = weight;
  return GIGL_OK;
}

int32_t gigl_nablp_train_plan_set_dropout(gigl_nablp_train_plan* t, float p, uint64_t seed) {
  if (!t) return GIGL_E_INVALID_ARG;
  if (t->kind != 0 && p != 0.f)
    return gigl_fail(t->ctx, GIGL_E_UNSUPPORTED, "dropout: the GAT link-prediction plans have none (feature and attention "
                                                 "dropout belong together there)");
  return sage_set_dropout(t->ctx, *t, t->stepped, p, seed);
}

int32_t gigl_nablp_train_plan_set_constant_lr(gigl_nablp_train_plan* t, float factor, int32_t total_iters) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, !t->stepped, "the learning-rate schedule is set after create and before the first step (the step is captured)");
  GIGL_REQUIRE(ctx, factor > 0.f && factor <= 1.f, "ConstantLR: factor must be in (0, 1]");
  GIGL_REQUIRE(ctx, total_iters >= 0, "ConstantLR: total_iters must be >= 0");
  t->lr_warm = t->lr * factor;  // (once, in fp32: a power-of-two factor is exact)
  t->warm_iters = total_iters;
  return GIGL_OK;
}

int32_t gigl_nablp_train_plan_grad_norm(gigl_nablp_train_plan* t, float* out2) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, out2, "null output");
  GIGL_REQUIRE(ctx, t->clip.out2, "the plan does not clip (gigl_nablp_train_plan_set_clip_grad_norm): no norm is computed");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  GIGL_HIP_CHECK(ctx, hipMemcpyAsync(out2, t->clip.out2, 8, hipMemcpyDeviceToDevice, ctx->stream));
  return GIGL_OK;
}

namespace {
__global__ __launch_bounds__(256) void lp_acc_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] += src[i];
}
__global__ __launch_bounds__(256) void lp_add2_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                      float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = a[i] + b[i];
}

// ---- what walks the GAT kind's tensor table, slots [first, last)
// the slots' gradients of one stream — every tensor on the caller's (alt 0), the forking ones on the second (alt 1) — laid
// out from float `at` of a cleared block; -> the next free float.  block == NULL only measures.
static size_t gat_grads_carve(PlanTensor* tb, int first, int last, int alt, float* block, size_t at) {
  for (int s = first; s < last; ++s)
    if (!alt || gat_slot_forks(s)) {
      tb[s].g[alt] = block ? block + at : nullptr;
      at += (size_t)tb[s].n;
    }
  return at;
}
// Adam's m, v: zero
static bool gat_moments_alloc(std::vector<void*>& owned, PlanTensor* tb, int first, int last) {
  for (int s = first; s < last; ++s)
    for (float** q : {&tb[s].m, &tb[s].v}) {
      const size_t bytes = (size_t)(tb[s].n ? tb[s].n : 1) * 4;
      *q = (float*)plan_alloc(owned, bytes);
      if (!*q || hipMemset(*q, 0, bytes) != hipSuccess) return false;
    }
  return true;
}
static int32_t gat_moments_adopt(gigl_ctx* ctx, PlanTensor* dst, const PlanTensor* src, int first, int last, const char* mismatch) {
  for (int s = first; s < last; ++s) {
    GIGL_REQUIRE(ctx, dst[s].n == src[s].n, "%s", mismatch);
    const size_t bytes = (size_t)(dst[s].n ? dst[s].n : 1) * 4;
    GIGL_HIP_CHECK(ctx, hipMemcpyAsync(dst[s].m, src[s].m, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    GIGL_HIP_CHECK(ctx, hipMemcpyAsync(dst[s].v, src[s].v, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  }
  return GIGL_OK;
}
// a tensor's gradient of the last step -> dst (NULL: skipped): both streams' shares, `blocks` workgroups for the second's
static int32_t gat_grad_export(gigl_ctx* ctx, const PlanTensor& x, float* dst, unsigned blocks) {
  if (!dst || !x.n) return GIGL_OK;
  GIGL_HIP_CHECK(ctx, hipMemcpyAsync(dst, x.g[0], (size_t)x.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
  if (x.g[1]) hipLaunchKernelGGL(lp_acc_kernel, dim3(blocks), dim3(256), 0, ctx->stream, dst, (const float*)x.g[1], x.n);
  return GIGL_OK;
}
}  // namespace

int32_t gigl_sage_train_plan_moments(gigl_sage_train_plan* t, int32_t layer, float* m_w, float* v_w, float* m_b, float* v_b) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, layer >= 0 && layer < t->L, "layer %d", layer);
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int32_t rc = sage_moments_copy(ctx, *t, 2 * layer, m_w, v_w);
  return rc != GIGL_OK ? rc : sage_moments_copy(ctx, *t, 2 * layer + 1, m_b, v_b);
}

int32_t gigl_nablp_train_plan_moments(gigl_nablp_train_plan* t, int32_t index, float* m, float* v) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (t->kind == 0) {
    GIGL_REQUIRE(ctx, index >= 0 && index < 2 * t->L, "tensor %d", index);
    return sage_moments_copy(ctx, *t, index, m, v);
  }
  GIGL_REQUIRE(ctx, index >= 0 && index < (t->gat.e.table ? GAT_TENSORS : GAT_CORE), "tensor %d", index);
  const PlanTensor& x = t->gat.tensor[index];  // (gat_slot: the table's index is the published one)
  if (m && x.n) GIGL_HIP_CHECK(ctx, hipMemcpyAsync(m, x.m, (size_t)x.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
  if (v && x.n) GIGL_HIP_CHECK(ctx, hipMemcpyAsync(v, x.v, (size_t)x.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
  return GIGL_OK;
}

int32_t gigl_sage_train_plan_adopt(gigl_sage_train_plan* dst, gigl_sage_train_plan* src) {
  if (!dst || !src) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = dst->ctx;
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  GIGL_HIP_CHECK(ctx, hipStreamSynchronize(src->ctx->stream));
  const int32_t rc = sage_moments_adopt(ctx, *dst, *src);
  return rc != GIGL_OK ? rc : nc_adopt_counter(dst, src);
}

int32_t gigl_nablp_train_plan_adopt(gigl_nablp_train_plan* dst, gigl_nablp_train_plan* src) {
  if (!dst || !src) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = dst->ctx;
  GIGL_REQUIRE(ctx, dst->L == src->L && dst->kind == src->kind && dst->H == src->H, "plans of different kinds");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  GIGL_HIP_CHECK(ctx, hipStreamSynchronize(src->ctx->stream));
  if (dst->kind == 1) {
    int32_t rc = gat_moments_adopt(ctx, dst->gat.tensor, src->gat.tensor, 0, GAT_CORE, "plans of different widths");
    if (rc != GIGL_OK) return rc;
    GIGL_REQUIRE(ctx, (dst->gat.e.table != nullptr) == (src->gat.e.table != nullptr), "plans with / without edge features");
    if (dst->gat.e.table)
      rc = gat_moments_adopt(ctx, dst->gat.tensor, src->gat.tensor, GAT_CORE, GAT_TENSORS, "plans of different edge widths");
    if (rc != GIGL_OK) return rc;
  } else {
    const int32_t rc = sage_moments_adopt(ctx, *dst, *src);
    if (rc != GIGL_OK) return rc;
  }
  if (!dst->stepped) {  // (the job's task: a plan that has stepped keeps its own, its step is captured)
    dst->task_kind = src->task_kind;
    dst->task_param = src->task_param;
    dst->task_weight = src->task_weight;
  } else {
    GIGL_REQUIRE(ctx, dst->task_kind == src->task_kind && dst->task_param == src->task_param && dst->task_weight == src->task_weight,
                 "plans of different tasks");
  }
  // (Adam's step counter: the bias correction and the ConstantLR schedule go on where src stood)
  GIGL_HIP_CHECK(ctx, hipMemcpyAsync(dst->consts + 2, src->consts + 2, 4, hipMemcpyDeviceToDevice, ctx->stream));
  if (dst->clip.out2 && src->clip.out2)
    GIGL_HIP_CHECK(ctx, hipMemcpyAsync(dst->clip.out2, src->clip.out2, 8, hipMemcpyDeviceToDevice, ctx->stream));
  GIGL_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return GIGL_OK;
}

int32_t gigl_nablp_train_plan_grads(gigl_nablp_train_plan* t, int32_t layer, float* gw, float* gb) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, t->kind == 0 && layer >= 0 && layer < t->L && gw, "bad plan / layer / null output");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int64_t nw = (int64_t)t->dims[layer + 1] * 2 * t->dims[layer];
  for (const SageTrainEnc& e : t->enc) {  // the step kept partial sums only: add them up now, into the (cleared) gradient buffers
    gigl_fill_u32(ctx->stream, e.gw[layer], 0u, nw);
    if (t->bias[layer]) gigl_fill_u32(ctx->stream, e.gb[layer], 0u, (int64_t)t->dims[layer + 1]);
    const int32_t rc = gigl_linear_weight_grad_sum(ctx, e.part_w[layer], t->bias[layer] ? e.part_b[layer] : nullptr,
                                                   e.base->un.meta + GIGL_META_LEVEL0 + (t->L - 1 - layer), t->dims[layer + 1],
                                                   2 * t->dims[layer], e.part_rc[layer], e.gw[layer],
                                                   t->bias[layer] ? e.gb[layer] : nullptr);
    if (rc != GIGL_OK) return rc;
  }
  hipLaunchKernelGGL(lp_add2_kernel, dim3(256), dim3(256), 0, ctx->stream, (const float*)t->enc[0].gw[layer],
                     (const float*)t->enc[1].gw[layer], nw, gw);
  if (gb && t->bias[layer])
    hipLaunchKernelGGL(lp_add2_kernel, dim3(4), dim3(256), 0, ctx->stream, (const float*)t->enc[0].gb[layer],
                       (const float*)t->enc[1].gb[layer], (int64_t)t->dims[layer + 1], gb);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

// ------------------------------------------------------------------------------------------
// The same step with the GAT encoder of configs[4] (GAT.init_conv_layers, python/gigl/src/common/models/pyg/
// homogeneous.py:300-343, under node_anchor_based_link_prediction_modeling_task_spec.py:334-451): two GATConv layers,
// `heads` concatenated heads in the first, one in the second, no edge features.  The first layer runs from the INPUT
// side (as models_attn.GAT does when the stored rows are wider than heads * channels): attention-weighted sums of the
// stored rows under the folded vectors u_h = W_h^T att_h (gigl_gat_input_aggregate), then one projection per head — for
// the nodes of level <= 1 only; the second layer for the roots only.  Backward: gigl_gat_aggregate_backward + epilogue,
// the projections' weight / input gradients, gigl_gat_input_aggregate_backward (d u), the fold's own backward.  Both
// encodes ADD into one set of gradients; head, loss, Adam, workspaces and prefetch are gigl_nablp_train_plan's.
namespace {

// the fold's backward, one workgroup per weight row r = hC + c:
//   gw[r][k] += att_src[r] du[h][k] + att_dst[r] du[H + h][k];  g_att_src[r] += <W[r], du[h]>;  g_att_dst[r] += <W[r], du[H + h]>
__global__ __launch_bounds__(256) void gat_fold_backward_kernel(const float* __restrict__ w, const float* __restrict__ att_src,
                                                                const float* __restrict__ att_dst, const float* __restrict__ du,
                                                                int H, int C, int d, float* __restrict__ gw,
                                                                float* __restrict__ g_att_src, float* __restrict__ g_att_dst) {
  __shared__ float s_a[4], s_b[4];
  const int r = blockIdx.x, h = r / C;
  const float as = att_src[r], ad = att_dst[r];
  const float* ds = du + (int64_t)h * d;
  const float* dd = du + (int64_t)(H + h) * d;
  float pa = 0.f, pb = 0.f;
  for (int k = threadIdx.x; k < d; k += blockDim.x) {
    const float wv = w[(int64_t)r * d + k], a = ds[k], b = dd[k];
    gw[(int64_t)r * d + k] += as * a + ad * b;
    pa += wv * a;
    pb += wv * b;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    pa += __shfl_xor(pa, o, 64);
    pb += __shfl_xor(pb, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_a[threadIdx.x >> 6] = pa;
    s_b[threadIdx.x >> 6] = pb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    g_att_src[r] += s_a[0] + s_a[1] + s_a[2] + s_a[3];
    g_att_dst[r] += s_b[0] + s_b[1] + s_b[2] + s_b[3];
  }
}
// out[h][i][c] = y[i][hC + c] > 0 ? dy[i][hC + c] : 0 for i < *n_rows: the heads' slices of the relu'd layer's gradient, each
// contiguous (planes rows_cap * C floats apart)
__global__ __launch_bounds__(256) void gat_split_mask_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                             const int32_t* __restrict__ n_rows_dev, int64_t rows_cap, int H,
                                                             int C, float* __restrict__ out) {
  const int64_t n = (int64_t)*n_rows_dev * H * C;
  const int HC = H * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / HC;
    const int col = (int)(i - row * HC), h = col / C, c = col - h * C;
    out[((int64_t)h * rows_cap + row) * C + c] = y[i] > 0.f ? dy[i] : 0.f;
  }
}
// y[i][c] = x[i][c] + bias[c] for i < *n_rows (x without the bias stays: the attention backward wants it)
__global__ __launch_bounds__(256) void gat_add_bias_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                           const int32_t* __restrict__ n_rows_dev, int C, float* __restrict__ y) {
  const int64_t n = (int64_t)*n_rows_dev * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = x[i] + (bias ? bias[i % C] : 0.f);
}
// gb[c] += sum over the rows i < *n_rows of dy[i][c]: 8 rows per workgroup, one atomic per (workgroup, column)
__global__ __launch_bounds__(256) void gat_bias_grad_kernel(const float* __restrict__ dy, const int32_t* __restrict__ n_rows_dev,
                                                            int C, float* __restrict__ gb) {
  const int n = *n_rows_dev;
  const int r0 = blockIdx.x * 8, r1 = r0 + 8 < n ? r0 + 8 : n;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float acc = 0.f;
    for (int r = r0; r < r1; ++r) acc += dy[(int64_t)r * C + c];
    if (acc != 0.f) atomicAdd(&gb[c], acc);
  }
}

// the edge terms' fold, v[h][k] = sum_c att_edge[hC + c] W_e[hC + c][k] (<lin_edge(e), att_edge_h> = <e, v_h>): one thread
// per (h, k)
__global__ __launch_bounds__(256) void gat_edge_fold_kernel(const float* __restrict__ w_e, const float* __restrict__ att_e, int H,
                                                            int C, int De, float* __restrict__ v) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= H * De) return;
  const int h = t / De, k = t - h * De;
  float acc = 0.f;
  for (int c = 0; c < C; ++c) acc += att_e[h * C + c] * w_e[(int64_t)(h * C + c) * De + k];
  v[t] = acc;
}
// its backward, one wave per weight row r = hC + c, lane k < De (De <= 64):
//   g_w[r][k] += att_edge[r] dv[h][k];  g_att[r] += <W_e[r], dv[h]>
__global__ __launch_bounds__(256) void gat_edge_fold_backward_kernel(const float* __restrict__ w_e, const float* __restrict__ att_e,
                                                                     const float* __restrict__ dv, int H, int C, int De,
                                                                     float* __restrict__ g_w, float* __restrict__ g_att) {
  const int lane = threadIdx.x & 63;
  const int r = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (r >= H * C) return;
  const int h = r / C;
  float p = 0.f;
  if (lane < De) {
    const float dvk = dv[h * De + lane];
    g_w[(int64_t)r * De + lane] += att_e[r] * dvk;
    p = w_e[(int64_t)r * De + lane] * dvk;
  }
  for (int o = 32; o >= 1; o >>= 1) p += __shfl_xor(p, o, 64);
  if (lane == 0) g_att[r] += p;
}

int64_t gat_rows1(const gigl_nablp_train_plan* t, int which) { return t->enc[which].rows_cap[0]; }

// the first layer's edge terms over encode `which`'s batch graph (its eid: the graph part wrote them)
gigl_gat_edge_terms gat_edge_terms0(const gigl_nablp_train_plan* t, int which) {
  const auto& ge = t->gat.e;
  gigl_gat_edge_terms et{};
  et.eid = t->enc[which].base->eid;
  et.table = (const float*)ge.table->rows;
  et.edge_dim = ge.De;
  et.att_edge_folded = ge.v;
  et.w_edge_msg = t->gat.at(GAT_W_MSG, 0).p;
  et.ze = ge.ze[which];
  return et;
}

// once per step: the folded attention vectors of the first layer (both encodes read them)
int32_t gat_lp_begin(gigl_nablp_train_plan* t) {
  const auto& g = t->gat;
  hipStream_t st = t->lctx->stream;
  gigl_gat_fold(st, g.at(GAT_W, 0).p, g.at(GAT_ATT_SRC, 0).p, g.at(GAT_ATT_DST, 0).p, g.heads, g.c0, g.d_in, g.u);
  // W1^T and the heads' W0^T for the input gradients of both encodes
  gigl_transpose_f32(st, g.at(GAT_W, 1).p, g.c1, g.heads * g.c0, g.wt1);
  for (int h = 0; h < g.heads; ++h)
    gigl_transpose_f32(st, g.at(GAT_W, 0).p + (int64_t)h * g.c0 * g.d_in, g.c0, g.d_in, g.wt0[h]);
  if (g.e.table) {  // both layers' folded att_edge (the parameters change every step), the edge gradients' clean slate
    const int De = g.e.De;
    gigl_fill_u32(st, g.e.zero_base, 0u, (int64_t)(g.e.zero_bytes / 4));
    hipLaunchKernelGGL(gat_edge_fold_kernel, dim3((unsigned)((g.heads * De + 255) / 256)), dim3(256), 0, st,
                       (const float*)g.at(GAT_W_EDGE, 0).p, (const float*)g.at(GAT_ATT_EDGE, 0).p, g.heads, g.c0, De, g.e.v);
    hipLaunchKernelGGL(gat_edge_fold_kernel, dim3(1), dim3(256), 0, st, (const float*)g.at(GAT_W_EDGE, 1).p,
                       (const float*)g.at(GAT_ATT_EDGE, 1).p, 1, g.c1, De, g.e.v + g.heads * De);
  }
  GIGL_HIP_CHECK(t->lctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gat_lp_forward(gigl_nablp_train_plan* t, int which) {
  SageTrainEnc& e = t->enc[which];
  const BatchGraph* p = e.base;
  auto& g = t->gat;
  GatScratch& s = g.sc[which == 1 && t->fork];
  gigl_ctx* ctx = s.ctx;
  hipStream_t st = ctx->stream;
  const float *w0 = g.at(GAT_W, 0).p, *b0 = g.at(GAT_BIAS, 0).p, *w1 = g.at(GAT_W, 1).p, *as1 = g.at(GAT_ATT_SRC, 1).p,
              *ad1 = g.at(GAT_ATT_DST, 1).p, *b1 = g.at(GAT_BIAS, 1).p, *wm0 = g.at(GAT_W_MSG, 0).p, *wm1 = g.at(GAT_W_MSG, 1).p;
  const int H = g.heads, C0 = g.c0, C1 = g.c1, d = g.d_in;
  const int64_t rows1 = gat_rows1(t, which);
  const int32_t* n0 = p->un.meta + GIGL_META_LEVEL0;
  const int32_t* n1 = p->un.meta + GIGL_META_LEVEL0 + 1;
  const bool edge = g.e.table != nullptr, msg0 = edge && wm0;
  const gigl_gat_edge_terms et = edge ? gat_edge_terms0(t, which) : gigl_gat_edge_terms{};
  int32_t rc = gigl_gat_input_aggregate_edge(ctx, t->feat->rows, t->feat->dtype, d, p->un.nodes, g.u, H, g.slope, p->un.rowptr,
                                             p->un.rowend, p->un.col, n1, rows1, g.z[which], edge ? &et : nullptr);
  if (rc != GIGL_OK) return rc;
  // h0[:, hC:(h+1)C] = relu(z_h W_h^T (+ W_msg,h ze_h) + b_h): one launch for all heads (the messages' De-wide term, the
  // bias and the relu in one more)
  rc = gigl_linear_batched(ctx, g.z[which], w0, msg0 ? nullptr : b0, n1, rows1, d, C0, msg0 ? 0 : 1, H, rows1 * d,
                           (int64_t)C0 * d, H * C0, e.h[0]);
  if (rc == GIGL_OK && msg0) rc = gigl_gat_edge_msg_add(ctx, g.e.ze[which], wm0, b0, n1, rows1, H, C0, g.e.De, 1, e.h[0]);
  if (rc != GIGL_OK) return rc;
  rc = gigl_linear(ctx, e.h[0], w1, nullptr, n1, rows1, H * C0, C1, 0, g.xw[which]);
  if (rc != GIGL_OK) return rc;
  if (edge)
    rc = gigl_gat_aggregate_edge_indexed(ctx, g.xw[which], as1, ad1, 1, C1, g.slope, 1, p->un.rowptr,
                                         p->un.rowend, p->un.col, n1, rows1, n0, e.rows_cap[1], nullptr, 0,
                                         (const float*)g.e.table->rows, p->eid, g.e.De, p->un.cap_edges, g.e.v + H * g.e.De,
                                         wm1, s.alpha, g.out_pre[which]);
  else
    rc = gigl_gat_aggregate(ctx, g.xw[which], as1, ad1, 1, C1, g.slope, 1, p->un.rowptr, p->un.rowend,
                            p->un.col, n1, rows1, n0, e.rows_cap[1], nullptr, 0, s.alpha, g.out_pre[which]);
  if (rc != GIGL_OK) return rc;
  {
    int64_t blocks = (e.rows_cap[1] * C1 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(gat_add_bias_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)g.out_pre[which],
                       b1, n0, C1, e.h[1]);
  }
  hipLaunchKernelGGL(lp_take_norm_kernel, dim3((unsigned)((e.b + 3) / 4)), dim3(256), 0, st, (const float*)e.h[1],
                     (const int32_t*)p->un.root_local, e.b, C1, t->normalize, (const int32_t*)p->un.meta, e.emb, e.inv);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

int32_t gat_lp_backward(gigl_nablp_train_plan* t, int which) {
  SageTrainEnc& e = t->enc[which];
  const BatchGraph* p = e.base;
  auto& g = t->gat;
  const int alt = which == 1 && t->fork;
  GatScratch& s = g.sc[alt];
  gigl_ctx* ctx = s.ctx;
  hipStream_t st = ctx->stream;
  const float *as1 = g.at(GAT_ATT_SRC, 1).p, *ad1 = g.at(GAT_ATT_DST, 1).p, *wm0 = g.at(GAT_W_MSG, 0).p, *wm1 = g.at(GAT_W_MSG, 1).p;
  const int H = g.heads, C0 = g.c0, C1 = g.c1, d = g.d_in, HC = H * C0;
  const int64_t rows1 = gat_rows1(t, which);
  const int32_t* n0 = p->un.meta + GIGL_META_LEVEL0;
  const int32_t* n1 = p->un.meta + GIGL_META_LEVEL0 + 1;
  // this stream's gradient slots (W0's, its attention vectors', b0's, W1's come from the partial sums and the fold's backward)
  float *gas1 = g.at(GAT_ATT_SRC, 1).g[alt], *gad1 = g.at(GAT_ATT_DST, 1).g[alt], *gb1 = g.at(GAT_BIAS, 1).g[alt];
  // ---- second layer (the roots' rows): e.dh[1] = d loss / d (out before the bias)
  if (g.at(GAT_BIAS, 1).p)
    hipLaunchKernelGGL(gat_bias_grad_kernel, dim3((unsigned)((e.rows_cap[1] + 7) / 8)), dim3(256), 0, st, (const float*)e.dh[1],
                       n0, C1, gb1);
  gigl_fill_u32(st, s.dxw, 0u, rows1 * C1);
  gigl_fill_u32(st, s.ds, 0u, s.dd - s.ds + rows1);  // (ds | dd: dd starts where a ds of the scratch's row capacity ends)
  // (edge features: both layers' d v on this stream's buffer, the message weights' gradients on this stream's slots — a
  // shared weight's slot IS lin_edge.weight's)
  const bool edge = g.e.table != nullptr;
  const int De = g.e.De;
  float *gm0 = g.at(GAT_W_MSG, 0).g[alt], *gm1 = g.at(GAT_W_MSG, 1).g[alt];
  int32_t rc = GIGL_OK;
  if (edge) {
    const bool msg1 = wm1 != nullptr;
    if (msg1)  // dze_i = W_msg^T dout_i
      rc = gigl_gat_edge_msg_backward(ctx, e.dh[1], 0, wm1, nullptr, n0, e.rows_cap[1], 1, C1, De, s.dze, nullptr);
    if (rc == GIGL_OK)
      rc = gigl_gat_aggregate_backward_indexed(ctx, g.xw[which], as1, ad1, C1, g.slope, p->un.rowptr,
                                               p->un.rowend, p->un.col, n1, rows1, n0, e.rows_cap[1], g.out_pre[which], e.dh[1],
                                               (const float*)g.e.table->rows, p->eid, De, g.e.v + H * De,
                                               msg1 ? s.dze : nullptr, s.alpha, s.dxw, s.ds, s.dd, s.dv + H * De,
                                               msg1 ? s.z1 : nullptr);
    if (rc == GIGL_OK && msg1)  // d W_msg += sum_i dout_i (x) z1_i
      rc = gigl_gat_edge_msg_backward(ctx, e.dh[1], 0, nullptr, s.z1, n0, e.rows_cap[1], 1, C1, De, nullptr, gm1);
  } else {
    rc = gigl_gat_aggregate_backward(ctx, g.xw[which], as1, ad1, 1, C1, g.slope, p->un.rowptr,
                                     p->un.rowend, p->un.col, n1, rows1, n0, e.rows_cap[1], g.out_pre[which], e.dh[1],
                                     nullptr, 0, p->un.cap_edges, nullptr, s.alpha, s.dxw, s.ds, s.dd, nullptr, nullptr,
                                     nullptr);
  }
  if (rc != GIGL_OK) return rc;
  rc = gigl_gat_backward_epilogue(ctx, s.dxw, s.ds, s.dd, g.xw[which], as1, ad1, n1, rows1, 1, C1, gas1, gad1);
  if (rc != GIGL_OK) return rc;
  // (measured: the main batch's weight gradients on a third stream, as the GraphSAGE plan runs them — 1.75 against 1.71 ms:
  // these 768-wide ones fill the GPU and slow the chain beside them)
  rc = gigl_linear_weight_grad_parts(ctx, s.dxw, e.h[0], nullptr, n1, rows1, C1, HC, g.part_w1[which], nullptr);
  if (rc != GIGL_OK) return rc;
  rc = gigl_linear(ctx, s.dxw, g.wt1, nullptr, n1, rows1, C1, HC, 0, s.dh0);
  if (rc != GIGL_OK) return rc;
  // ---- first layer: relu mask, the heads' slices, their projections' backward, the attention-weighted sums' backward
  {
    int64_t blocks = (rows1 * HC + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(gat_split_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)s.dh0, (const float*)e.h[0],
                       n1, rows1, H, C0, s.dh0s);
  }
  for (int h = 0; h < H; ++h) {
    const float* dyh = s.dh0s + (int64_t)h * rows1 * C0;
    rc = gigl_linear_weight_grad_parts(ctx, dyh, g.z[which] + (int64_t)h * rows1 * d, nullptr, n1, rows1, C0, d,
                                       g.part_w0[which][h], g.at(GAT_BIAS, 0).p ? g.part_b0[which][h] : nullptr);
    if (rc != GIGL_OK) return rc;
    rc = gigl_linear(ctx, dyh, g.wt0[h], nullptr, n1, rows1, C0, d, 0, s.dz + (int64_t)h * rows1 * d);
    if (rc != GIGL_OK) return rc;
  }
  if (edge) {
    const bool msg0 = wm0 != nullptr;
    const gigl_gat_edge_terms et = gat_edge_terms0(t, which);
    if (msg0) {  // dze_i,h = W_msg,h^T dy_i,h and d W_msg += sum_i dy_i (x) ze_i, from the heads' masked slices
      rc = gigl_gat_edge_msg_backward(ctx, s.dh0s, rows1 * C0, wm0, g.e.ze[which], n1, rows1, H, C0, De, s.dze, gm0);
      if (rc != GIGL_OK) return rc;
    }
    rc = gigl_gat_input_aggregate_backward_edge(ctx, t->feat->rows, t->feat->dtype, d, p->un.nodes, g.u, H, g.slope, p->un.rowptr,
                                                p->un.rowend, p->un.col, n1, rows1, s.dz, s.du, &et, msg0 ? s.dze : nullptr, s.dv);
  } else {
    rc = gigl_gat_input_aggregate_backward(ctx, t->feat->rows, t->feat->dtype, d, p->un.nodes, g.u, H, g.slope, p->un.rowptr,
                                           p->un.rowend, p->un.col, n1, rows1, s.dz, nullptr, s.du);
  }
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return rc;
}

// after both encodes: d u -> the first layer's weights and attention vectors, then Adam over the table
int32_t gat_lp_finish(gigl_nablp_train_plan* t) {
  gigl_ctx* ctx = t->lctx;
  hipStream_t st = ctx->stream;
  auto& g = t->gat;
  const PlanTensor &w0 = g.at(GAT_W, 0), &b0 = g.at(GAT_BIAS, 0), &w1 = g.at(GAT_W, 1);
  if (t->fork)  // the random negatives' share of d u, accumulated on its own stream
    hipLaunchKernelGGL(lp_acc_kernel, dim3(64), dim3(256), 0, st, g.sc[0].du, (const float*)g.sc[1].du, (int64_t)2 * g.heads * g.d_in);
  hipLaunchKernelGGL(gat_fold_backward_kernel, dim3((unsigned)(g.heads * g.c0)), dim3(256), 0, st, (const float*)w0.p,
                     (const float*)g.at(GAT_ATT_SRC, 0).p, (const float*)g.at(GAT_ATT_DST, 0).p, (const float*)g.sc[0].du, g.heads,
                     g.c0, g.d_in, w0.g[0], g.at(GAT_ATT_SRC, 0).g[0], g.at(GAT_ATT_DST, 0).g[0]);
  if (g.e.table) {  // d v of both layers -> lin_edge.weight and att_edge (v = W_e^T att_edge per head)
    const int De = g.e.De;
    float* dv = g.sc[0].dv;
    if (t->fork) hipLaunchKernelGGL(lp_acc_kernel, dim3(1), dim3(256), 0, st, dv, (const float*)g.sc[1].dv, (int64_t)(g.heads + 1) * De);
    hipLaunchKernelGGL(gat_edge_fold_backward_kernel, dim3((unsigned)((g.heads * g.c0 + 3) / 4)), dim3(256), 0, st,
                       (const float*)g.at(GAT_W_EDGE, 0).p, (const float*)g.at(GAT_ATT_EDGE, 0).p, (const float*)dv, g.heads, g.c0,
                       De, g.at(GAT_W_EDGE, 0).g[0], g.at(GAT_ATT_EDGE, 0).g[0]);
    hipLaunchKernelGGL(gat_edge_fold_backward_kernel, dim3((unsigned)((g.c1 + 3) / 4)), dim3(256), 0, st,
                       (const float*)g.at(GAT_W_EDGE, 1).p, (const float*)g.at(GAT_ATT_EDGE, 1).p, (const float*)(dv + g.heads * De), 1,
                       g.c1, De, g.at(GAT_W_EDGE, 1).g[0], g.at(GAT_ATT_EDGE, 1).g[0]);
  }
  AdamPack ap{};
  ap.n_src = 2;
  const int32_t* n1a = t->enc[0].base->un.meta + GIGL_META_LEVEL0 + 1;
  const int32_t* n1b = t->enc[1].base->un.meta + GIGL_META_LEVEL0 + 1;
  auto add = [&](const PlanTensor& x, int64_t at, int64_t n, const float* pa, const float* pb, int32_t rca, int32_t rcb) {
    const int k = ap.count++;
    ap.p[k] = x.p + at;
    ap.g[0][k] = x.g[0] + at;
    ap.g[1][k] = x.g[1];  // (fork: what the second stream accumulated itself; never a sliced tensor's)
    ap.part[0][k] = pa;
    ap.part[1][k] = pb;
    ap.rows[0][k] = n1a;
    ap.rows[1][k] = n1b;
    ap.rc[0][k] = rca;
    ap.rc[1][k] = rcb;
    ap.m[k] = x.m + at;
    ap.v[k] = x.v + at;
    ap.n[k] = n;
  };
  // in table order (the gradient norm's fixed-order sum follows it); a shared message weight has n == 0: no entry of its own
  for (const PlanTensor& x : g.tensor) {
    if (!x.n) continue;
    if (&x == &w0 || &x == &b0) {  // a slice per head, each with its own partial sums of both encodes
      const auto& part = &x == &w0 ? g.part_w0 : g.part_b0;
      for (int h = 0; h < g.heads; ++h) add(x, h * (x.n / g.heads), x.n / g.heads, part[0][h], part[1][h], g.rc_w0[0], g.rc_w0[1]);
    } else if (&x == &w1) {
      add(x, 0, x.n, g.part_w1[0], g.part_w1[1], g.rc_w1[0], g.rc_w1[1]);
    } else {
      add(x, 0, x.n, nullptr, nullptr, 0, 0);
    }
  }
  ap.lr = t->lr;
  ap.beta1 = t->beta1;
  ap.beta2 = t->beta2;
  ap.eps = t->eps;
  ap.wd = t->wd;
  ap.lr_warm = t->lr_warm;
  ap.warm_iters = t->warm_iters;
  launch_adam(st, 104, ap, (const int32_t*)(t->consts + 2), (const int32_t*)t->enc[0].base->un.meta,
              (const int32_t*)t->enc[1].base->un.meta, (const int32_t*)nullptr, &t->clip);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return GIGL_OK;
}

// a stream's backward scratch, for encodes of up to rows1 nodes of level <= 1, cap_edges edges and b roots
static bool gat_scratch_alloc(gigl_nablp_train_plan* t, GatScratch& s, gigl_ctx* stream_ctx, int64_t rows1, int64_t cap_edges, int64_t b) {
  const auto& g = t->gat;
  auto alloc = [&](int64_t floats) { return (float*)plan_alloc(t->owned, (size_t)floats * 4); };
  s.ctx = stream_ctx;
  s.rows1 = rows1;
  s.b = b;
  s.dxw = alloc(rows1 * g.c1);
  s.ds = alloc(2 * rows1);
  s.dd = s.ds ? s.ds + rows1 : nullptr;
  s.alpha = alloc(2 * rows1 + cap_edges);
  s.dh0 = alloc(rows1 * g.heads * g.c0);
  s.dh0s = alloc(rows1 * g.heads * g.c0);
  s.dz = alloc(g.heads * rows1 * g.d_in);
  return s.dxw && s.ds && s.alpha && s.dh0 && s.dh0s && s.dz;
}
// ... and what the message weights' backward adds to it
static bool gat_scratch_alloc_edge(gigl_nablp_train_plan* t, GatScratch& s) {
  const auto& g = t->gat;
  s.dze = (float*)plan_alloc(t->owned, (size_t)s.rows1 * g.heads * g.e.De * 4);
  s.z1 = (float*)plan_alloc(t->owned, (size_t)s.b * g.e.De * 4);
  return s.dze && s.z1;
}

}  // namespace

int32_t gigl_gat_nablp_train_plan_create(gigl_ctx* ctx, gigl_graph* graph, gigl_feat* feat, int32_t b_anchors,
                                         int32_t num_positives, int32_t n_random_negatives, const int32_t* fanouts, int32_t hops,
                                         const int32_t* heads, const int32_t* channels, float* const* w,
                                         float* const* att_src, float* const* att_dst, float* const* bias,
                                         float negative_slope, int32_t l2_normalize, float temperature,
                                         int32_t remove_accidental_hits, float lr, float beta1, float beta2, float eps,
                                         float weight_decay, gigl_nablp_train_plan** out) {
  if (!ctx || !out) return GIGL_E_INVALID_ARG;
  *out = nullptr;
  GIGL_REQUIRE(ctx, graph && feat && fanouts && heads && channels && w && att_src && att_dst, "null argument");
  GIGL_REQUIRE(ctx, b_anchors >= 1 && num_positives >= 1 && n_random_negatives >= 0, "bad batch shape");
  if (hops != 2 || heads[1] != 1)
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "the GAT link-prediction plan runs two layers, one head in the second");
  const int H = heads[0], C0 = channels[0], C1 = channels[1], d = feat->d;
  if ((d & 3) || d > 1024 || (H != 1 && H != 2 && H != 4) || (feat->dtype != GIGL_DTYPE_F32 && feat->dtype != GIGL_DTYPE_F16) ||
      H * C0 > 1024 || (C0 & 3) || (C1 & 3) || C1 > 512)
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "GAT link-prediction plan: feature dim %d / %d heads x %d / %d channels outside "
                     "the built shapes", d, H, C0, C1);
  for (int l = 0; l < 2; ++l) GIGL_REQUIRE(ctx, w[l] && att_src[l] && att_dst[l], "layer %d: null parameter", l);
  if (fanouts[1] > GIGL_FAST_FANOUT) return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "second fan-out beyond %d", GIGL_FAST_FANOUT);
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  gigl_nablp_train_plan* t = lp_plan_new(ctx, 1, 2, b_anchors, num_positives, n_random_negatives, 0, l2_normalize, temperature,
                                         remove_accidental_hits, lr, beta1, beta2, eps, weight_decay);
  if (!t) return gigl_fail(ctx, GIGL_E_OOM, "host OOM");
  auto& g = t->gat;
  g.heads = H;
  g.c0 = C0;
  g.c1 = C1;
  g.d_in = d;
  g.slope = negative_slope;
  const int32_t dims[3] = {d, H * C0, C1};
  for (int l = 0; l <= 2; ++l) t->dims[l] = dims[l];
  for (int l = 0; l < 2; ++l) {
    g.at(GAT_W, l).set(w[l], (int64_t)dims[l + 1] * dims[l]);
    g.at(GAT_ATT_SRC, l).set(att_src[l], dims[l + 1]);
    g.at(GAT_ATT_DST, l).set(att_dst[l], dims[l + 1]);
    g.at(GAT_BIAS, l).set(bias ? bias[l] : nullptr, dims[l + 1]);
  }
  // every node of the batch graphs is numbered: gigl_gat_input_aggregate reads its sources through un.nodes
  const int32_t rc = lp_create_workspaces(t, graph, feat, fanouts, hops, dims, w, true);
  if (rc != GIGL_OK) {
    gigl_nablp_train_plan_destroy(t);
    return rc;
  }
  auto alloc = [&](size_t bytes) { return plan_alloc(t->owned, bytes); };
  bool ok = true;
  // (default on, GIGL_LP_FORK=0 off, as the GraphSAGE plan: the forked step's layers part launched eagerly)
  const bool want_fork = lp_fork_wanted(t);
  int64_t rows1_max = 0, b_max = 0;
  for (int k = 0; k < 2; ++k) {
    SageTrainEnc& e = t->enc[k];
    e.rows_cap[0] = gigl_level_rows(ctx->wide, e.b, fanouts, hops, 1);  // nodes of level <= 1
    e.rows_cap[1] = e.b;
    if (e.rows_cap[0] > rows1_max) rows1_max = e.rows_cap[0];
    if (e.b > b_max) b_max = e.b;
    e.h[0] = (float*)alloc((size_t)e.rows_cap[0] * H * C0 * 4);
    e.h[1] = (float*)alloc((size_t)e.b * C1 * 4);
    g.z[k] = (float*)alloc((size_t)H * e.rows_cap[0] * d * 4);
    g.xw[k] = (float*)alloc((size_t)e.rows_cap[0] * C1 * 4);
    g.out_pre[k] = (float*)alloc((size_t)e.b * C1 * 4);
    ok = ok && e.h[0] && e.h[1] && g.z[k] && g.xw[k] && g.out_pre[k];
  }
  // the block cleared at the start of every step, laid out twice (to measure it, then in the buffer)
  auto lay_out = [&](float* block) {
    size_t at = gat_grads_carve(g.tensor, 0, GAT_CORE, 0, block, 0);
    auto take = [&](float*& q, size_t floats) { q = block ? block + at : nullptr; at += floats; };
    take(g.sc[0].du, (size_t)2 * H * d);
    for (SageTrainEnc& e : t->enc) take(e.dh[1], (size_t)e.b * C1);
    if (want_fork) {
      take(g.sc[1].du, (size_t)2 * H * d);
      at = gat_grads_carve(g.tensor, 0, GAT_CORE, 1, block, at);
    }
    return at;
  };
  t->zero_bytes = lay_out(nullptr) * 4;
  t->zero_base = alloc(t->zero_bytes);
  if (t->zero_base) lay_out((float*)t->zero_base);
  g.u = (float*)alloc((size_t)2 * H * d * 4);
  ok = ok && t->zero_base && g.u && gat_moments_alloc(t->owned, g.tensor, 0, GAT_CORE) &&
       gat_scratch_alloc(t, g.sc[0], t->lctx, rows1_max, t->ring.slot[0].base[0].un.cap_edges, b_max);
  if (want_fork && ok)  // the second stream's ctx and events, its own scratch (the random negatives' rows and edges)
    ok = lp_fork_setup(t) && gat_scratch_alloc(t, g.sc[1], t->actx, t->enc[1].rows_cap[0], t->ring.slot[0].base[1].un.cap_edges, t->enc[1].b);
  if (ok) {
    g.wt1 = (float*)alloc((size_t)C1 * H * C0 * 4);
    ok = g.wt1 != nullptr;
    for (int h = 0; h < H && ok; ++h) {
      g.wt0[h] = (float*)alloc((size_t)C0 * d * 4);
      ok = g.wt0[h] != nullptr;
    }
    for (int k = 0; k < 2 && ok; ++k) {
      const int64_t rows1 = t->enc[k].rows_cap[0];
      const int64_t ch1 = gigl_linear_weight_grad_chunks(rows1, C1, H * C0, &g.rc_w1[k]);
      g.part_w1[k] = (float*)alloc((size_t)ch1 * C1 * H * C0 * 4);
      const int64_t ch0 = gigl_linear_weight_grad_chunks(rows1, C0, d, &g.rc_w0[k]);
      ok = g.part_w1[k] != nullptr;
      for (int h = 0; h < H && ok; ++h) {
        g.part_w0[k][h] = (float*)alloc((size_t)ch0 * C0 * d * 4);
        g.part_b0[k][h] = (float*)alloc((size_t)ch0 * C0 * 4);
        ok = g.part_w0[k][h] && g.part_b0[k][h];
      }
    }
  }
  ok = ok && lp_head_alloc(t, (size_t)C1);
  if (!ok) {
    gigl_nablp_train_plan_destroy(t);
    return gigl_fail(ctx, GIGL_E_OOM, "hipMalloc of the GAT link-prediction training workspace failed");
  }
  *out = t;
  return GIGL_OK;
}

int32_t gigl_gat_nablp_train_plan_grads(gigl_nablp_train_plan* t, int32_t layer, float* gw, float* g_att_src,
                                        float* g_att_dst, float* gb) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, t->kind == 1 && layer >= 0 && layer < 2 && gw && g_att_src && g_att_dst, "bad plan / layer / null output");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (t->gat.parts_pending) {  // the step kept the projections' gradients as partial sums: add them up, once
    auto& g = t->gat;
    float *gw0 = g.at(GAT_W, 0).g[0], *gb0 = g.at(GAT_BIAS, 0).p ? g.at(GAT_BIAS, 0).g[0] : nullptr;
    for (int k = 0; k < 2; ++k) {
      const int32_t* n1 = t->enc[k].base->un.meta + GIGL_META_LEVEL0 + 1;
      int32_t rc = gigl_linear_weight_grad_sum(ctx, g.part_w1[k], nullptr, n1, g.c1, g.heads * g.c0, g.rc_w1[k], g.at(GAT_W, 1).g[0],
                                               nullptr);
      for (int h = 0; h < g.heads && rc == GIGL_OK; ++h)
        rc = gigl_linear_weight_grad_sum(ctx, g.part_w0[k][h], gb0 ? g.part_b0[k][h] : nullptr, n1, g.c0, g.d_in, g.rc_w0[k],
                                         gw0 + (int64_t)h * g.c0 * g.d_in, gb0 ? gb0 + h * g.c0 : nullptr);
      if (rc != GIGL_OK) return rc;
    }
    g.parts_pending = false;
  }
  float* const dst[4] = {gw, g_att_src, g_att_dst, gb};
  const GatPart part[4] = {GAT_W, GAT_ATT_SRC, GAT_ATT_DST, GAT_BIAS};
  int32_t rc = GIGL_OK;
  for (int i = 0; i < 4 && rc == GIGL_OK; ++i) rc = gat_grad_export(ctx, t->gat.at(part[i], layer), dst[i], 4);
  return rc;
}

int32_t gigl_gat_nablp_train_plan_set_edge_features(gigl_nablp_train_plan* t, gigl_feat* edge_table, float* const* w_edge,
                                                    float* const* att_edge, float* const* w_edge_msg) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, t->kind == 1, "edge features apply to the GAT link-prediction plan (gigl_gat_nablp_train_plan_create)");
  GIGL_REQUIRE(ctx, !t->stepped && !t->gat.e.table, "edge features are set once, after create and before the first step");
  GIGL_REQUIRE(ctx, edge_table && w_edge && att_edge, "null argument");
  const gigl_graph* graph = t->ring.slot[0].base[0].graph;
  const int32_t De = edge_table->d;
  if (edge_table->dtype != GIGL_DTYPE_F32 || De < 1 || De > 64)  // (a lane per component of an edge row)
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "GAT link-prediction plan: the edge table must be fp32, 1..64 wide (dtype %d, %d)",
                     edge_table->dtype, De);
  if (t->gat.heads == 4 && t->gat.d_in > 768)  // (the one shape whose edge backward would spill: not built, agg.hip)
    return gigl_fail(ctx, GIGL_E_UNSUPPORTED, "GAT link-prediction plan: edge features with four heads need rows of at most 768 "
                     "floats (%d)", t->gat.d_in);
  GIGL_REQUIRE(ctx, edge_table->n == graph->e, "the edge table holds one row per resident edge (%lld rows, %lld edges)",
               (long long)edge_table->n, (long long)graph->e);
  for (int l = 0; l < 2; ++l) GIGL_REQUIRE(ctx, w_edge[l] && att_edge[l], "layer %d: null edge parameter", l);
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  auto& g = t->gat;
  auto& ge = g.e;
  const int H = g.heads;
  const int64_t hc[2] = {(int64_t)H * g.c0, g.c1};
  ge.De = De;
  for (int l = 0; l < 2; ++l) {
    g.at(GAT_W_EDGE, l).set(w_edge[l], hc[l] * De);
    g.at(GAT_ATT_EDGE, l).set(att_edge[l], hc[l]);
    float* w_msg = w_edge_msg ? w_edge_msg[l] : nullptr;
    g.at(GAT_W_MSG, l).set(w_msg, w_msg != w_edge[l] ? hc[l] * De : 0);  // (shared: n == 0, gradient slots joined below)
  }
  const bool fork = t->fork, any_msg = g.at(GAT_W_MSG, 0).p || g.at(GAT_W_MSG, 1).p;
  const size_t nv = (size_t)(H + 1) * De;
  // the edge block: gradients | dv, and as much again for a forked stream (no att_edge slots there: its tail stays unused)
  auto lay_out = [&](float* block) {
    const size_t half = gat_grads_carve(g.tensor, GAT_CORE, GAT_TENSORS, 0, block, 0) + nv;
    g.sc[0].dv = block ? block + half - nv : nullptr;
    if (!fork) return half;
    g.sc[1].dv = block ? block + gat_grads_carve(g.tensor, GAT_CORE, GAT_TENSORS, 1, block, half) : nullptr;
    return 2 * half;
  };
  ge.zero_bytes = lay_out(nullptr) * 4;
  ge.zero_base = plan_alloc(t->owned, ge.zero_bytes);
  ge.v = (float*)plan_alloc(t->owned, nv * 4);
  bool ok = ge.zero_base && ge.v;
  if (ok) lay_out((float*)ge.zero_base);
  for (int l = 0; l < 2; ++l)  // a shared message weight's gradient joins lin_edge.weight's, on both streams
    if (g.at(GAT_W_MSG, l).p == g.at(GAT_W_EDGE, l).p)
      for (int k = 0; k < 2; ++k) g.at(GAT_W_MSG, l).g[k] = g.at(GAT_W_EDGE, l).g[k];
  ok = ok && gat_moments_alloc(t->owned, g.tensor, GAT_CORE, GAT_TENSORS);
  if (any_msg && ok) {
    for (int k = 0; k < 2; ++k) {
      ge.ze[k] = (float*)plan_alloc(t->owned, (size_t)t->enc[k].rows_cap[0] * H * De * 4);
      ok = ok && ge.ze[k];
    }
    for (int k = 0; k < (fork ? 2 : 1); ++k) ok = ok && gat_scratch_alloc_edge(t, g.sc[k]);
  }
  if (!ok) return gigl_fail(ctx, GIGL_E_OOM, "hipMalloc of the GAT link-prediction plan's edge workspace failed");
  // every workspace's batch graphs get their edge ids from their own graph part (plan_edge_ids_kernel; all rows are numbered)
  for (int wi = 0; wi < gigl_nablp_train_plan::WS; ++wi)
    for (BatchGraph& bg : t->ring.slot[wi].base) {
      const int32_t rc = batch_graph_attach_edge_table(&bg, edge_table);
      if (rc != GIGL_OK) return gigl_fail(ctx, rc, "%s", gigl_last_error(bg.ctx));
    }
  ge.table = edge_table;
  return GIGL_OK;
}

int32_t gigl_gat_nablp_train_plan_edge_grads(gigl_nablp_train_plan* t, int32_t layer, float* g_w_edge, float* g_att_edge,
                                             float* g_w_edge_msg) {
  if (!t) return GIGL_E_INVALID_ARG;
  gigl_ctx* ctx = t->ctx;
  GIGL_REQUIRE(ctx, t->kind == 1 && t->gat.e.table && layer >= 0 && layer < 2, "bad plan / layer");
  GIGL_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  float* const dst[3] = {g_w_edge, g_att_edge, g_w_edge_msg};
  const GatPart part[3] = {GAT_W_EDGE, GAT_ATT_EDGE, GAT_W_MSG};
  int32_t rc = GIGL_OK;
  for (int j = 0; j < 3 && rc == GIGL_OK; ++j) rc = gat_grad_export(ctx, t->gat.at(part[j], layer), dst[j], 16);
  GIGL_HIP_CHECK(ctx, hipGetLastError());
  return rc;
}

}  // extern "C"
