"""TEST INFRASTRUCTURE ONLY: the reference, the checker, the route table and the graphs of the leaf-global two-hop union
tests (tests/test_union_cases_cpu.py, tests/test_gpu_union_leaf_global.py).

The builds under test are union_build_lg3 / union_build_lg2 of csrc/union.hip, reached through the one-call plans
(GraphSAGE.make_plan -> run -> last_batch_to_host).  Which of them a shape takes is asked of the library
(gigl_union_route, include/gigl_hip.h), never restated here.

Reference.  The grouped union of G batches is the ordinary union of the same trees with every node id of batch g replaced
by id + g*n (tests/test_gpu_groups.py): oracle.union_build on the tagged tree.  reference() translates its answer to the
leaf-global contract of the plans' builds:
  * only nodes of level < 2 are numbered: meta[0] == meta[3] == meta[4] == the oracle's meta[3]
  * level 0 (distinct roots) is numbered exactly as the oracle numbers it; level 1 is the same SET, in an order of the
    build's own (a level-1 node's leaf occurrences are not inserted, so its first position may differ)
  * rows of level-0 nodes hold local ids, rows of level-1 nodes the GLOBAL ids of their sources; every row is strictly
    ascending as int32; the unique-edge count meta[1] and the level counts are exact
  * root_local[i] is the oracle's, also for repeated roots (both entries name the one local id of their batch's copy)
  * an INVALID root (0xFFFFFFFF) is no node: it is not numbered, has no row, and its root_local entry is -1 — what
    lg3_fill_kernel / lg2's fill write for it (`lid = valid ? ... : -1`) and what test_gpu_union_lg3.py pins between the
    two builds.  The oracle numbers the INVALID id like any other root: reference() takes that one node out again.
  * meta[GIGL_META_OVERFLOW] == 0

The tree the reference is built from is the one the DEVICE produced (hb["nbr"], hb["cnt"]), so that a sampler difference
can neither fake nor hide a union failure; check_tree() asserts separately that this tree is the oracle's.

check() works on whole arrays (no Python loop over rows).  Every failure is an AssertionError whose message starts with
the name of the property, which is what the mutation tests match on.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle  # noqa: E402
from helpers import rmat_edges  # noqa: E402

INVALID = 0xFFFFFFFF
META_OVERFLOW = 8
GENERIC, LG2, LG3 = 0, 1, 2  # GIGL_ROUTE_*
WHY_NONE, WHY_CODES, WHY_PARTS, WHY_FEW_WGS, WHY_LDS, WHY_ENV = range(6)  # GIGL_ROUTE_WHY_*


# ------------------------------------------------------------------------------------------------------------- route
def route(gr, fan, G, leaf_global=1):
    """gigl_union_route for G batches of gr roots: dict(build, threads, parts, table_slots, root_slots, lds_bytes, why)"""
    import ctypes as C
    from gigl_amd import _lib
    lib = _lib.load()
    out = (C.c_int32 * 8)()
    fo = (C.c_int32 * len(fan))(*[int(f) for f in fan])
    rc = lib.gigl_union_route(int(gr) * int(G), fo, len(fan), int(gr), int(leaf_global), out)
    assert rc == 0, rc
    return dict(build=out[0], threads=out[1], parts=out[2], table_slots=out[3], root_slots=out[4], lds_bytes=out[5],
                why=out[6])


def route_name(r):
    """'LG3/512 P=2' | 'LG2 (lds)' | 'generic': the route in the words the tests print (`ROUTE <test> <route>`)"""
    if r["build"] == LG3:
        return f"LG3/{r['threads']} P={r['parts']}"
    if r["build"] == LG2:
        return "LG2 (%s)" % ["", "codes", "parts", "few workgroups", "lds", "env"][r["why"]]
    return "generic"


# (label, gr, f0, f1, G) -> what gigl_union_route must say; only the listed keys are compared
ROUTE_TABLE = [
    ("a", 4, 3, 2, 256, dict(build=LG3, threads=512, parts=1)),
    ("b", 4, 3, 2, 255, dict(build=LG3, threads=1024, parts=1)),
    ("c32", 1, 1, 1, 32, dict(build=LG3, threads=1024, parts=1)),
    ("c31", 1, 1, 1, 31, dict(build=LG2, why=WHY_FEW_WGS)),
    ("d40", 37, 7, 5, 40, dict(build=LG3, threads=1024, parts=1)),
    ("d33", 37, 7, 5, 33, dict(build=LG3, threads=1024, parts=1)),
    ("e", 1100, 7, 2, 16, dict(build=LG3, threads=1024, parts=2)),
    ("f", 2048, 8, 2, 11, dict(build=LG3, threads=1024, parts=3)),
    ("g", 2048, 32, 2, 4, dict(build=LG3, threads=1024, parts=9, root_slots=4096, lds_bytes=152952)),
    ("h", 2049, 31, 2, 8, dict(build=LG2, why=WHY_LDS)),
    ("i15", 2048, 32, 15, 4, dict(build=LG2, why=WHY_CODES)),
    ("i14", 2048, 32, 14, 4, dict(build=LG3, threads=1024, parts=9)),
    ("j", 330, 25, 2, 128, dict(build=LG3, threads=512, parts=2)),
    ("k52", 1024, 32, 1, 52, dict(build=LG3, threads=512, parts=5)),
    ("k51", 1024, 32, 1, 51, dict(build=LG3, threads=1024, parts=5)),
    ("l1", 300, 25, 10, 1, dict(build=LG2, why=WHY_FEW_WGS)),
    ("l4", 256, 25, 10, 4, dict(build=LG2, why=WHY_FEW_WGS)),
]
SHAPES = {label: (gr, [f0, f1], G, want) for label, gr, f0, f1, G, want in ROUTE_TABLE}


def assert_route(gr, fan, G, want):
    got = route(gr, fan, G)
    assert {k: got[k] for k in want} == want, f"route of gr={gr} fan={fan} G={G}: {got}, expected {want}"
    return got


# --------------------------------------------------------------------------------------------------------- reference
def tag(arr, per_group, n):
    """arr laid out group-major with `per_group` entries per batch -> ids + g*n (INVALID kept)"""
    a = np.asarray(arr).astype(np.uint64)
    g = np.arange(a.size, dtype=np.uint64) // np.uint64(per_group)
    return np.where(a == INVALID, np.uint64(INVALID), a + g * np.uint64(n)).astype(np.uint32)


def reference(roots, fan, gr, n, nbr):
    """the leaf-global union of G = len(roots) / gr batches over the tree `nbr` (tree layout, the batches one after the
    other at every hop), from oracle.union_build on the tagged tree.  Tagged id = global id + batch * n."""
    roots = np.asarray(roots, dtype=np.uint32)
    f0, f1 = int(fan[0]), int(fan[1])
    b = roots.size
    G = b // gr
    assert G * gr == b and (G * n) < INVALID
    o = oracle.union_build(tag(roots, gr, n), [f0, f1], [tag(nbr[0], gr * f0, n), tag(nbr[1], gr * f0 * f1, n)])
    n0, n1 = int(o["meta"][2]), int(o["meta"][3])
    assert int(o["rowptr"][n1]) == int(o["meta"][1])  # every edge ends in a node of level < 2
    t = o["nodes"][:n1].astype(np.int64)
    keep = t != INVALID  # (the oracle numbers the INVALID id as a root: take it out)
    new_id = np.cumsum(keep) - 1
    new_id[~keep] = -1
    lens = np.diff(o["rowptr"][: n1 + 1]).astype(np.int64)
    assert (lens[~keep] == 0).all()
    dst = np.repeat(t, lens)
    src = o["nodes"].astype(np.int64)[o["col"][: int(o["rowptr"][n1])]]
    dropped0 = int((~keep[:n0]).sum())
    tk = t[keep]
    inner_per_batch = np.bincount(tk // n, minlength=G)
    return dict(G=G, gr=gr, n=n, fan=[f0, f1], b=b, n0=n0 - dropped0, n1=n1 - dropped0, n_edges=int(o["meta"][1]),
                cap_edges=b * f0 + b * f0 * f1,
                nodes0=tk[: n0 - dropped0], level1_sorted=np.sort(tk[n0 - dropped0:]),
                edge_keys=np.sort((dst.astype(np.uint64) << np.uint64(32)) | src.astype(np.uint64)),
                root_local=new_id[o["root_local"]].astype(np.int32), inner_per_batch=inner_per_batch,
                # (for synthesize(): the oracle's rows of the kept nodes, sources as tagged ids)
                _rows=(tk, lens[keep], src))


def fits_workspace(ref):
    """every batch's nodes of level < 2 fit the rows the plan holds for it (gr * (1 + f0)): no overflow may be reported"""
    return bool((ref["inner_per_batch"] <= ref["gr"] * (1 + ref["fan"][0])).all())


def check_tree(hb, rowptr, col, roots, fan):
    """the tree the plan sampled == the oracle's canonical sample"""
    nbr_o, cnt_o = oracle.sample_khop(rowptr, col, np.asarray(roots, dtype=np.uint32), fan, canonical=True)
    for k in range(len(fan)):
        assert np.array_equal(hb["cnt"][k], cnt_o[k]), f"tree: cnt of hop {k}"
        assert np.array_equal(hb["nbr"][k], nbr_o[k]), f"tree: nbr of hop {k}"


def predup_row_lengths(roots, fan, gr, n, nbr, cnt):
    """entries of every row BEFORE deduplication, as the builds count them for a node all of whose contributing
    occurrences are full or that is a root: dict tagged id -> length, over level-0 rows (root occurrences' cnt0, plus
    cnt1 of every hop-0 slot that holds the root) and over rows of hop-0 nodes (cnt1 of every slot that holds the node)"""
    roots = np.asarray(roots, dtype=np.uint32)
    f0, f1 = fan
    tr, t0 = tag(roots, gr, n).astype(np.int64), tag(nbr[0], gr * f0, n).astype(np.int64)
    ids = np.concatenate([tr[tr != INVALID], t0[t0 != INVALID]])
    w = np.concatenate([cnt[0][tr != INVALID], cnt[1][t0 != INVALID]]).astype(np.int64)
    u, inv = np.unique(ids, return_inverse=True)
    return u, np.bincount(inv, weights=w).astype(np.int64)


# ----------------------------------------------------------------------------------------------------------- checker
def check(hb, ref):
    """hb: SagePlan.last_batch_to_host() (or synthesize()); ref: reference().  Raises AssertionError naming the property."""
    G, n, n0, n1 = ref["G"], ref["n"], ref["n0"], ref["n1"]
    meta = np.asarray(hb["meta"])
    assert int(meta[META_OVERFLOW]) == 0, f"overflow: meta[8] = {int(meta[META_OVERFLOW])}"
    want_meta = [n1, ref["n_edges"], n0, n1, n1]
    assert [int(v) for v in meta[:5]] == want_meta, f"meta: {meta[:5].tolist()} != {want_meta}"
    nodes = np.asarray(hb["nodes"]).astype(np.int64)
    assert nodes.size == n1, "nodes: length"
    batch0 = ref["nodes0"] // n
    assert np.array_equal(nodes[:n0], ref["nodes0"] % n), "nodes: level 0 is not the oracle's order"
    assert np.array_equal(np.asarray(hb["root_local"]), ref["root_local"]), "root_local"
    # rows: bounds, storage, order
    col = np.asarray(hb["col"])
    rp = np.asarray(hb["rowptr"])[:n1].astype(np.int64)
    re_ = np.asarray(hb["rowend"])[:n1].astype(np.int64)
    assert rp.size == n1 and re_.size == n1, "row bounds: length"
    assert bool(((0 <= rp) & (rp <= re_) & (re_ <= col.size)).all()), "row bounds: 0 <= rowptr <= rowend <= len(col)"
    lens = re_ - rp
    stored = np.nonzero((lens > 0) & (rp < ref["cap_edges"]))[0]  # (the others may alias tree segments)
    assert bool((re_[stored] <= ref["cap_edges"]).all()), "row storage: a stored row runs past cap_edges"
    by_start = stored[np.argsort(rp[stored], kind="stable")]
    assert bool((re_[by_start][:-1] <= rp[by_start][1:]).all()), "row storage: stored rows overlap"
    total = int(lens.sum())
    row = np.repeat(np.arange(n1, dtype=np.int64), lens)
    first = np.cumsum(lens) - lens
    val = col[np.repeat(rp - first, lens) + np.arange(total, dtype=np.int64)].astype(np.int32).astype(np.int64)
    same = row[1:] == row[:-1]
    assert bool((val[1:][same] > val[:-1][same]).all()), "row order: a row is not strictly ascending"
    is0 = row < n0
    v0, r0 = val[is0], row[is0]
    assert bool(((v0 >= 0) & (v0 < n1)).all()), "edges: a level-0 row holds something that is no local id"
    v1 = val[~is0]
    assert bool(((v1 >= 0) & (v1 < n)).all()), "edges: a level-1 row holds something that is no global id"
    # batch membership, from the oracle's level-0 order alone
    b_row0 = batch0[r0]
    from0 = v0 < n0
    assert np.array_equal(batch0[v0[from0]], b_row0[from0]), "batch membership: a level-0 row names a root of another batch"
    pairs = np.unique((v0[~from0] - n0) * G + b_row0[~from0])
    assert np.array_equal(pairs // G, np.arange(n1 - n0)), \
        "batch membership: a level-1 node is referenced from no batch or from more than one"
    batch = np.concatenate([batch0, pairs % G])
    tagged = nodes + batch * n
    assert np.unique(tagged).size == n1, "nodes: an id twice in one batch"
    assert np.array_equal(np.sort(tagged[n0:]), ref["level1_sorted"]), "nodes: level 1 is not the oracle's set"
    # the edge multiset
    src = np.empty(total, dtype=np.int64)
    src[is0] = tagged[v0]
    src[~is0] = v1 + batch[row[~is0]] * n
    keys = np.sort((tagged[row].astype(np.uint64) << np.uint64(32)) | src.astype(np.uint64))
    assert keys.size == ref["edge_keys"].size and np.array_equal(keys, ref["edge_keys"]), \
        f"edges: the rows hold {keys.size} pairs, not the oracle's {ref['edge_keys'].size} (or other ones)"


# -------------------------------------------------------------------------------------------- a correct union, on the CPU
def synthesize(ref, nbr, cnt, perm0=None, reverse_level1=True, slack=1):
    """a correct leaf-global union for `ref` as last_batch_to_host() would return it, laid out the way the builds lay it
    out: rows keep spare capacity (`slack` words each), level 1 in an order of its own, the row of a level-1 node whose
    first occurrence sampled its whole in-neighbourhood aliasing that tree segment past cap_edges.  perm0 (new local id of
    every level-0 node): a consistently renumbered — and therefore wrong — level 0, for the mutation tests."""
    n, n0, n1, G = ref["n"], ref["n0"], ref["n1"], ref["G"]
    f0, f1 = ref["fan"]
    tk, lens, src_t = ref["_rows"]
    new = np.arange(n1)
    if reverse_level1:
        new[n0:] = n0 + (n1 - n0 - 1 - np.arange(n1 - n0))
    if perm0 is not None:
        new[:n0] = perm0
    local_of = dict(zip(tk.tolist(), new.tolist()))
    first_slot = {}
    t0 = tag(nbr[0], ref["gr"] * f0, n).astype(np.int64)
    for p in np.nonzero(t0 != INVALID)[0][::-1]:
        first_slot[int(t0[p])] = int(p)
    cap_edges = ref["cap_edges"]
    col = np.full(cap_edges + nbr[1].size, -7, dtype=np.int32)
    col[cap_edges:] = nbr[1].view(np.int32)
    nodes = np.zeros(n1, dtype=np.uint32)
    rowptr, rowend = np.zeros(n1 + 1, np.int32), np.zeros(n1 + 1, np.int32)
    e, stored = 0, []
    for i in range(n1):
        s = src_t[e:e + int(lens[i])]
        e += int(lens[i])
        li = new[i]
        nodes[li] = tk[i] % n
        if i < n0:
            r = np.sort(np.array([local_of[int(x)] for x in s], dtype=np.int32))
        else:
            r = np.sort((s % n).astype(np.int32))
            p = first_slot.get(int(tk[i]))
            if p is not None and cnt[1][p] < f1 and np.array_equal(r, nbr[1][p * f1:p * f1 + cnt[1][p]].view(np.int32)):
                rowptr[li], rowend[li] = cap_edges + p * f1, cap_edges + p * f1 + r.size
                continue
        stored.append((li, r))
    spare = cap_edges - sum(r.size for _, r in stored)  # (a build's rows keep their pre-dedup capacity: never more)
    at = 0
    for li, r in stored:
        rowptr[li], rowend[li] = at, at + r.size
        col[at:at + r.size] = r
        give = slack if r.size and spare >= slack else 0
        spare -= give
        at += r.size + give
    assert at <= cap_edges
    meta = np.zeros(16, dtype=np.int32)
    meta[:5] = [n1, ref["n_edges"], n0, n1, n1]
    rl = ref["root_local"].copy()
    rl[rl >= 0] = new[rl[rl >= 0]]
    return dict(nbr=nbr, cnt=cnt, meta=meta, nodes=nodes, rowptr=rowptr, rowend=rowend, col=col, root_local=rl)


# ------------------------------------------------------------------------------------------------------------ graphs
class Graph:
    """a graph as the engine builds it from COO and as the oracle reads it (CSC by destination)"""

    def __init__(self, n, src, dst, directed=False, multi=False):
        self.n, self.directed, self.multi = int(n), directed, multi
        self.src, self.dst = np.asarray(src).astype(np.uint32), np.asarray(dst).astype(np.uint32)
        self.rowptr, self.col = oracle.build_csc(self.n, self.src, self.dst, is_directed=directed, keep_multi_edges=multi)

    def load(self, eng):
        eng.build_from_coo(self.n, self.src, self.dst, is_directed=self.directed, keep_multi_edges=self.multi)


@functools.lru_cache(maxsize=None)
def graph_rmat():
    """the R-MAT graph of test_gpu_union_lg3.py (2^13 nodes, skewed degrees)"""
    s, d = rmat_edges(13, 150000, seed=8)
    return Graph(1 << 13, s, d)


@functools.lru_cache(maxsize=None)
def graph_ring(log2n=16, half_width=16, n_rmat=20000, seed=3):
    """a +-half_width ring plus a few R-MAT edges, undirected: every node has degree >= 2 * half_width and few have more,
    so that the oracle's pass over millions of tree positions stays cheap (the large shapes)"""
    n = 1 << log2n
    s, d = rmat_edges(log2n, n_rmat, seed=seed)
    v = np.arange(n)
    ring_s = np.concatenate([v] * half_width)
    ring_d = np.concatenate([(v + k) % n for k in range(1, half_width + 1)])
    return Graph(n, np.concatenate([s % n, ring_s]), np.concatenate([d % n, ring_d]))


@functools.lru_cache(maxsize=None)
def graph_fan(log2n=16, f=32):
    """directed, for the shapes with millions of hop-1 slots: an even node has f in-neighbours (f - 1 odd ones and one
    even one), an odd node two (both even).  Even roots fill every hop-0 slot up to fan-out f, and nearly every hop-1
    slot costs the oracle a permutation of two ids; hop-0 slots still hold roots of the batch now and then (extras)"""
    n = 1 << log2n
    ev, od = np.arange(0, n, 2), np.arange(1, n, 2)
    src = [(ev + 1 + 2 * t) % n for t in range(f - 1)] + [(ev + 34) % n, (od + 1) % n, (od + 7) % n]
    dst = [ev] * f + [od, od]
    return Graph(n, np.concatenate(src), np.concatenate(dst), directed=True)


@functools.lru_cache(maxsize=None)
def graph_dense(multi=False):
    """300 nodes, ~4000 random edges (test_gpu_union_lg3.py `dense`): most hop-0 nodes of a batch are roots themselves;
    multi: directed, 500 records twice — rows are multisets (the builds' multiset_rows mode)"""
    rng = np.random.default_rng(5)
    ns = 300
    ss, ds = rng.integers(0, ns, 4000), rng.integers(0, ns, 4000)
    if multi:
        return Graph(ns, np.concatenate([ss, ss[:500]]), np.concatenate([ds, ds[:500]]), directed=True, multi=True)
    return Graph(ns, ss, ds)


@functools.lru_cache(maxsize=None)
def graph_small_dense():
    """40 nodes, ~500 random edges, undirected: small enough to make every node a root of each of 256 batches"""
    rng = np.random.default_rng(7)
    return Graph(40, rng.integers(0, 40, 500), rng.integers(0, 40, 500))


@functools.lru_cache(maxsize=None)
def graph_hub():
    """2000 nodes that all point at node 0, plus 6000 random edges, undirected (test_gpu_union_lg3.py `hub`)"""
    rng = np.random.default_rng(6)
    hs = np.concatenate([np.arange(1, 2000), rng.integers(0, 2000, 6000)])
    hd = np.concatenate([np.zeros(1999, np.int64), rng.integers(0, 2000, 6000)])
    return Graph(2000, hs, hd)


# level-0 rows of c sampled in-edges under a root repeated k times, level-1 rows of a node with cnt1 == f1 == 1 under k parents
ROW_CLASS_LENGTHS = (1, 2, 32, 33, 64, 65)
ROW_CLASS_FAN = [13, 1]
_L0 = {1: (1, 1), 2: (2, 1), 32: (8, 4), 33: (11, 3), 64: (8, 8), 65: (13, 5)}  # length -> (in-degree <= f0, repeats)


@functools.lru_cache(maxsize=None)
def graph_row_classes():
    """directed.  For every length L of ROW_CLASS_LENGTHS: a root with c in-neighbours that nothing points at, to be
    repeated k times (c * k == L: its level-0 row), and a middle node with 40 in-neighbours that is the only
    in-neighbour of L parents (fan-out [13, 1]: L occurrences of one sampled child each — its level-1 row; the child
    depends on the parent, so the row keeps several distinct sources).  Returns (graph, roots of one batch, named rows)."""
    src, dst, roots, named0, named1 = [], [], [], {}, {}
    nxt = 0

    def fresh(k):
        nonlocal nxt
        nxt += k
        return np.arange(nxt - k, nxt)
    for L in ROW_CLASS_LENGTHS:
        c, k = _L0[L]
        r = int(fresh(1)[0])
        src.append(fresh(c))
        dst.append(np.full(c, r))
        roots += [r] * k
        named0[L] = r
        m = int(fresh(1)[0])
        src.append(fresh(40))
        dst.append(np.full(40, m))
        parents = fresh(L)
        src.append(np.full(L, m))
        dst.append(parents)
        roots += parents.tolist()
        named1[L] = m
    rng = np.random.default_rng(2)
    roots = np.array(roots, dtype=np.uint32)[rng.permutation(len(roots))]
    return Graph(nxt, np.concatenate(src), np.concatenate(dst), directed=True), roots, named0, named1


@functools.lru_cache(maxsize=None)
def graph_big_row(k, degree):
    """directed: `degree` sources point at hub 0, and hub 0 is the only in-neighbour of parents 1..k.  With fan-out
    [f0, f1] every parent's hop-0 slot holds the hub with f1 sampled children of its own choice: the hub's row has
    k * f1 entries before deduplication"""
    n = 1 + k + degree
    src = np.concatenate([np.arange(1 + k, n), np.zeros(k, np.int64)])
    dst = np.concatenate([np.zeros(degree, np.int64), np.arange(1, 1 + k)])
    return Graph(n, src, dst, directed=True)


@functools.lru_cache(maxsize=None)
def graph_overflow(gr, pool):
    """directed: root r (0 <= r < gr) has every root and `pool` nodes of its own as in-neighbours.  A hop-0 slot that
    holds a root makes that root's sampled children nodes of level 1 (the extras): with a large last fan-out one batch of
    these roots has far more nodes of level < 2 than gr * (1 + f0)"""
    src, dst = [], []
    for r in range(gr):
        own = gr + r * pool + np.arange(pool)
        src.append(np.concatenate([np.arange(gr), own]))
        dst.append(np.full(gr + pool, r))
    return Graph(gr + gr * pool, np.concatenate(src), np.concatenate(dst), directed=True)
