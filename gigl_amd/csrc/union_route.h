// union_route.h — which build serves a union call, and with what shape (host only; nothing from HIP).
//
// The leaf-global two-hop union of the plans has two builds in union.hip: LG3 (a batch's node table in LDS, one dedup
// workgroup per hash partition of a batch) and LG2 (the table in HBM, position-parallel launches).  union_route() is the
// ONE place that decides between them from the batch shape; gigl_union_build_impl dispatches on its answer,
// union_build_lg3 launches with the sizes it returns, and gigl_union_route (gigl_hip.h) hands the same answer to tests,
// so that a test case built for one route says so when a constant moves it to another.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>

constexpr int LG3_CODE_BITS = 20;
constexpr uint32_t LG3_CODE_MASK = (1u << LG3_CODE_BITS) - 1u;
constexpr int LG3_MAX_PARTS = 16;
constexpr int LG3_NT_DEFAULT = 512;      // threads per dedup workgroup (round 5: 512 x 128-KB tables find a CU sooner next to other kernels than 1024 — 7.0 vs 10.7 us/step under three streams; smaller tables lose to their redundant stream scans: profiles/r05d_lg3_shapes.txt)
constexpr int LG3_CAP_DEFAULT = 16384;   // slots of its LDS table (8 bytes each)
constexpr int LG3_TC = 5;  // per-tile counts: level-0 firsts, level-1 firsts, row entries to store, long / tiny rows to sort
constexpr size_t LG3_LDS_LIMIT = 150 * 1024;  // dynamic LDS the dedup kernels opt in to

// (the values of GIGL_ROUTE_* / GIGL_ROUTE_WHY_* in gigl_hip.h)
enum : int32_t { UNION_ROUTE_GENERIC = 0, UNION_ROUTE_LG2 = 1, UNION_ROUTE_LG3 = 2 };
enum : int32_t {
  UNION_WHY_NONE = 0,
  UNION_WHY_CODES = 1,    // the batch's stream does not fit 20-bit codes / the 64-bit root mask / int32 positions
  UNION_WHY_PARTS = 2,    // more than LG3_MAX_PARTS hash partitions per batch
  UNION_WHY_FEW_WGS = 3,  // fewer dedup workgroups than GIGL_LG3_MIN_WGS (32)
  UNION_WHY_LDS = 4,      // table + root set + tile counts past LG3_LDS_LIMIT
  UNION_WHY_ENV = 5,      // GIGL_UNION_LG2 is set
};

struct UnionRoute {
  int32_t route = UNION_ROUTE_GENERIC;
  int32_t why = UNION_WHY_NONE;  // why LG2 and not LG3
  // LG3's shape; filled as far as the decision got (0 beyond the rule that sent the call to LG2)
  int32_t nt = 0;        // threads per dedup workgroup: 512 | 1024
  int32_t rs_log2 = 0;
  int64_t P = 0;         // hash partitions (workgroups) per batch
  int64_t cap = 0;       // LDS table slots
  int64_t rs = 0;        // root set slots
  size_t lds_bytes = 0;
};

// b roots in batches of group_roots (which divides b; b > 0), fan-outs f0, f1 when hops == 2
inline UnionRoute union_route(int32_t b, const int32_t* fanouts, int32_t hops, int32_t group_roots, int32_t leaf_global) {
  UnionRoute r;
  if (!leaf_global || hops != 2) return r;  // the generic build (every public entry point; the one-hop plans)
  r.route = UNION_ROUTE_LG2;
  static const bool keep_lg2 = getenv("GIGL_UNION_LG2") != nullptr;  // (A/B knob)
  if (keep_lg2) {
    r.why = UNION_WHY_ENV;
    return r;
  }
  const int f0 = fanouts[0], f1 = fanouts[1];
  const int64_t S0 = (int64_t)b * f0, S1 = S0 * f1;
  const int64_t n_groups = b / group_roots;
  const int64_t gr = group_roots, Tg = gr * (1 + f0), S1g = gr * f0 * f1;
  // (20-bit stream codes; a thread of the dedup pass keeps one bit per 1024 hop-0 slots of the batch in a 64-bit mask)
  // workgroup shape of the dedup pass (round 5): 512 | 1024 threads, up to LG3_CAP_DEFAULT slots per table
  // (a thread keeps one bit per NT hop-0 slots of its batch in a 64-bit mask: batches of more than 64 * 512 slots — B = 4096
  // at fan-out 15 — take the 1024-thread shape)
  int lg3_nt = gr * f0 <= 64 * (int64_t)LG3_NT_DEFAULT ? LG3_NT_DEFAULT : 1024;
  r.why = UNION_WHY_CODES;
  if (Tg + S1g >= (int64_t)LG3_CODE_MASK || f1 > 64 || b + S0 + S1 >= ((int64_t)1 << 31) || gr * f0 > 64 * (int64_t)lg3_nt) return r;
  // LDS table: 8-byte slots at load <= 1/2 for the nodes a batch may hold (more do not fit the plan's workspace)
  int64_t cap = 1024;
  while (cap < 2 * Tg && cap < LG3_CAP_DEFAULT) cap <<= 1;
  const int64_t P = (2 * Tg + cap - 1) / cap;
  r.cap = cap;
  r.P = P;
  r.why = UNION_WHY_PARTS;
  if (P > LG3_MAX_PARTS) return r;
  // (the 512-thread shape pays when the launch fills the GPU — a workgroup per CU and more, other streams' kernels beside
  // it; a launch of fewer workgroups than CUs is over sooner with 1024 threads each: the sharded plan's 16-batch calls,
  // lg3_dedup 3.6 -> 5.0 us per rank-step with 512, profiles/r05e_emulated_world8_kernel_time.txt)
  if (n_groups * P < 256) lg3_nt = 1024;
  r.nt = lg3_nt;
  // a call of a few batches (a training step: one) leaves most CUs without a workgroup of the dedup pass, whose duration
  // is that of ONE workgroup walking its batch's whole stream (~80 us at [25,10] x 1024): LG2's position-parallel
  // launches finish such a call sooner (training step 0.42 -> 0.39 ms)
  static const int64_t min_wgs = getenv("GIGL_LG3_MIN_WGS") ? atoll(getenv("GIGL_LG3_MIN_WGS")) : 32;
  r.why = UNION_WHY_FEW_WGS;
  if (n_groups * P < min_wgs) return r;
  int64_t rs = 64;
  int rs_log2 = 6;
  while (rs < 2 * gr) {
    rs <<= 1;
    ++rs_log2;
  }
  const int64_t n_tcnt = LG3_TC * ((gr >> 10) + 2 + ((gr * f0) >> 10) + 2);
  r.rs = rs;
  r.rs_log2 = rs_log2;
  r.lds_bytes = (size_t)cap * 8 + (size_t)(rs + rs / 4 + n_tcnt) * 4;
  r.why = UNION_WHY_LDS;
  if (r.lds_bytes > LG3_LDS_LIMIT) return r;
  r.route = UNION_ROUTE_LG3;
  r.why = UNION_WHY_NONE;
  return r;
}
