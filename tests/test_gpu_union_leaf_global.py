"""The plans' two-hop union builds (csrc/union.hip union_build_lg3 / union_build_lg2) against the oracle on every route:
both workgroup shapes of lg3_dedup_kernel, one to nine hash partitions, the full root mask, the LDS and code-range
fallbacks to LG2, single and grouped LG2, every row-sort class, and the overflow report.

Each case runs the way production does — GraphSAGE.make_plan(eng, gr, fan, groups=G), one run, last_batch_to_host(), in
this process with the default environment — asks gigl_union_route which build and shape the call takes and asserts it,
then hands the batch to tests/union_cases.py: check_tree (the sampled tree is the oracle's), reference (oracle.union_build
on the device's tree, ids tagged per batch, translated to the leaf-global contract) and check (meta, node order, batch
membership, the edge multiset, row order, bounds and storage, root_local).  Every case but the last asserts on the oracle's
output that each batch fits the plan's workspace, and that no overflow is reported.

Every test prints `ROUTE <test> <route>` (pytest -s shows which test ran which route).

Reference semantics: first-seen numbering per level, edges deduplicated per batch (the oracle's union_build)."""
import numpy as np
import pytest
import torch

import union_cases as uc

pytestmark = pytest.mark.gpu
INVALID = uc.INVALID


_loaded = [None]  # the graph the module's engine holds (graphs are cached objects: compared by identity)


@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    _loaded[0] = None
    yield e
    e.close()


def _run(eng, g, gr, fan, G, roots, d=4):
    """one plan call over G batches of gr roots on graph g -> last_batch_to_host()"""
    from gigl_amd.models import GraphSAGE
    roots = np.ascontiguousarray(roots, dtype=np.uint32)
    assert roots.size == gr * G
    if _loaded[0] is not g:
        g.load(eng)
        eng.load_features(np.random.default_rng(1).standard_normal((g.n, d)).astype(np.float32))
        _loaded[0] = g
    torch.manual_seed(0)
    model = GraphSAGE(d, 8, 4, num_layers=2).to(eng.device)
    plan = model.make_plan(eng, gr, fan, groups=G)
    try:
        plan.run(torch.from_numpy(roots.view(np.int32)).to(eng.device))
        return plan.last_batch_to_host()
    finally:
        plan.close()


def _case(eng, request, g, gr, fan, G, roots, want):
    """the whole check of one call; returns (hb, ref) for what a test asserts on top"""
    r = uc.assert_route(gr, fan, G, want)
    print(f"\nROUTE {request.node.name} {uc.route_name(r)}")
    hb = _run(eng, g, gr, fan, G, roots)
    uc.check_tree(hb, g.rowptr, g.col, roots, fan)
    ref = uc.reference(roots, fan, gr, g.n, hb["nbr"])
    assert uc.fits_workspace(ref), "the case itself does not fit the plan's workspace"
    uc.check(hb, ref)
    return hb, ref


def _mixed_roots(n, gr, G, seed):
    """random roots with the awkward ones in: a root repeated inside batch 0, the same root in batches 0 and 1 (twice
    there), INVALID roots in two batches, and — from four batches on — batch 2 made of INVALID roots only"""
    r = np.random.default_rng(seed).integers(0, n, gr * G).astype(np.uint32)
    if gr >= 4:
        r[3] = r[2]
        r[1] = INVALID
    if G >= 2:
        r[gr] = r[0]
        if gr >= 2:
            r[gr + gr - 1] = r[0]
        if gr >= 3:
            r[gr + 1] = INVALID
    if G >= 4:
        r[2 * gr:3 * gr] = INVALID
    return r


# ------------------------------------------------------------------------------------------------- the route table
# label -> graph; the shapes and the route each must take are union_cases.ROUTE_TABLE: one line per edge of the dispatch
# (both workgroup shapes at the 256-workgroup rule, the fewest-workgroups rule, 1 / 2 / 3 / 5 / 9 partitions, the full
# root mask at 512 and 1024 threads, the LDS limit, the 20-bit code range, the training step's LG2)
_SHAPE_GRAPH = {
    "a": uc.graph_rmat, "b": uc.graph_rmat, "c32": uc.graph_rmat, "c31": uc.graph_rmat, "d40": uc.graph_rmat,
    "d33": uc.graph_rmat, "e": uc.graph_ring, "f": uc.graph_ring, "g": uc.graph_ring, "h": uc.graph_ring,
    "i15": uc.graph_ring, "i14": uc.graph_ring, "j": uc.graph_fan, "k52": uc.graph_fan, "k51": uc.graph_fan,
    "l1": uc.graph_rmat, "l4": uc.graph_rmat,
}


@pytest.mark.parametrize("label", list(_SHAPE_GRAPH))
def test_shape(eng, request, label):
    """every line of the route table: the workgroup shapes, the partition counts, the mask, LDS and code edges"""
    gr, fan, G, want = uc.SHAPES[label]
    g = _SHAPE_GRAPH[label]()
    seed = sum(map(ord, label))
    if label in ("g", "k52", "k51"):  # (every hop-0 slot of every batch holds a node: no INVALID root, full rows)
        roots = (np.random.default_rng(seed).integers(0, g.n // 2, gr * G) * 2).astype(np.uint32)
    else:
        roots = _mixed_roots(g.n, gr, G, seed)
    hb, ref = _case(eng, request, g, gr, fan, G, roots, want)
    assert ref["n1"] > ref["n0"] > 0
    if label == "g":  # every bit of the root mask belongs to a hop-0 slot that holds a node
        assert (hb["nbr"][0] != INVALID).all() and gr * fan[0] == 64 * 1024
    if label == "k52":
        assert (hb["nbr"][0] != INVALID).all() and gr * fan[0] == 64 * 512


# ------------------------------------------------------------------------------------------------- content, per route
_CONTENT_ROUTES = {  # (gr, f0, G): batches of 32 roots at fan-out [10, f1] have one partition and a 1024-slot table;
    # lg3_512_p2 is line j of the route table (330 roots, fan-out [25, f1], 128 batches: two partitions, 512 threads)
    "lg3_1024": (32, 10, 32, dict(build=uc.LG3, threads=1024, parts=1)),
    "lg3_512": (32, 10, 256, dict(build=uc.LG3, threads=512, parts=1)),
    "lg3_512_p2": (330, 25, 128, dict(build=uc.LG3, threads=512, parts=2)),
    "lg2": (32, 10, 4, dict(build=uc.LG2)),
}


# (no hub on lg3_512_p2: 42,000 hop-0 slots would hold the hub, and the oracle permutes its 2,000 in-neighbours for each)
@pytest.mark.parametrize("content,route", [(c, r) for c in ("extras", "multi_edges", "hub") for r in _CONTENT_ROUTES
                                           if (c, r) != ("hub", "lg3_512_p2")])
def test_content(eng, request, content, route):
    """extras: a 300-node graph, most hop-0 nodes of a batch are roots of it (their children become level-1 nodes);
    multi_edges: the same directed with repeated records (multiset_rows); hub: node 0 is a root of every batch and
    everybody's neighbour.  All with repeated, shared and INVALID roots and a batch of INVALID roots only."""
    gr, f0, G, want = _CONTENT_ROUTES[route]
    if content == "hub":
        g, fan = uc.graph_hub(), [f0, 2]
        roots = _mixed_roots(g.n, gr, G, seed=40)
        roots[::gr] = 0
        roots[2 * gr:3 * gr] = INVALID
    else:
        g, fan = uc.graph_dense(multi=content == "multi_edges"), [f0, 5 if f0 == 10 else 2]
        roots = _mixed_roots(g.n, gr, G, seed=30)
    hb, ref = _case(eng, request, g, gr, fan, G, roots, want)
    if content == "extras":  # the case has what it is named for: hop-0 slots that hold a root of their batch, with children
        t0 = uc.tag(hb["nbr"][0], gr * fan[0], g.n)
        assert int((np.isin(t0, ref["nodes0"]) & (hb["cnt"][1] > 0)).sum()) > 2 * G
    if content == "hub":
        hubs = np.nonzero(ref["nodes0"] % g.n == 0)[0]
        assert hubs.size == G - 1 and (hb["rowend"][hubs] - hb["rowptr"][hubs] > 20).all()


@pytest.mark.parametrize("nodes,G,want", [(300, 32, dict(build=uc.LG3, threads=1024, parts=1)),
                                          (40, 256, dict(build=uc.LG3, threads=512, parts=1)), (300, 2, dict(build=uc.LG2))],
                         ids=["lg3_1024", "lg3_512", "lg2"])
def test_every_root_is_also_a_hop0_node(eng, request, nodes, G, want):
    """all nodes of the graph (300, or 40 where the call has 256 batches) are the roots of every batch, in an order of
    its own: no level-1 node at all, every hop-0 slot is root-valued and every child an extra that is a root again"""
    g = uc.graph_dense() if nodes == 300 else uc.graph_small_dense()
    assert g.n == nodes
    roots = np.concatenate([np.random.default_rng(g_).permutation(g.n) for g_ in range(G)])
    hb, ref = _case(eng, request, g, g.n, [10, 5], G, roots, want)
    assert ref["n1"] == ref["n0"] == G * g.n


# ------------------------------------------------------------------------------------------------- row-sort classes
@pytest.mark.parametrize("G,want", [(1, dict(build=uc.LG2)), (32, dict(build=uc.LG3, threads=1024, parts=1)),
                                    (256, dict(build=uc.LG3, threads=512, parts=1))], ids=["lg2", "lg3_1024", "lg3_512"])
def test_row_lengths_at_the_sort_class_edges(eng, request, G, want):
    """rows of 1, 2, 32, 33, 64 and 65 entries before deduplication (the <= 32 and <= 64 classes and their neighbours),
    one level-0 row and one level-1 row each, in every batch — the lengths asserted on the device's own tree"""
    g, roots1, named0, named1 = uc.graph_row_classes()
    gr, fan = roots1.size + 1, uc.ROW_CLASS_FAN
    roots = np.concatenate([np.roll(np.append(roots1, np.uint32(INVALID)), 7 * k) for k in range(G)])
    hb, ref = _case(eng, request, g, gr, fan, G, roots, want)
    ids, lens = uc.predup_row_lengths(roots, fan, gr, g.n, hb["nbr"], hb["cnt"])
    batches = np.arange(G, dtype=np.int64) * g.n
    for L in uc.ROW_CLASS_LENGTHS:
        for node in (named0[L], named1[L]):
            at = np.searchsorted(ids, node + batches)
            assert np.array_equal(ids[at], node + batches) and (lens[at] == L).all(), (L, node)
    # a level-1 row of L entries under L different parents keeps several distinct sources
    m = int(np.nonzero(hb["nodes"][ref["n0"]:] == named1[65])[0][0]) + ref["n0"]
    assert 1 < hb["rowend"][m] - hb["rowptr"][m] <= 40


@pytest.mark.parametrize("G,want", [(32, dict(build=uc.LG3, threads=1024, parts=1)), (1, dict(build=uc.LG2))],
                         ids=["lg3", "lg2"])
def test_rows_of_more_than_32_entries_under_roots_that_occur_once(eng, request, G, want):
    """fan-out [40, 2] on a ring of 48 neighbours per node: a root that nothing else in its batch names owns a row of 40
    local ids that no sort queue sees (it has no duplicates) — the row still has to come out ascending, through the
    in-place path that rows beyond the 32-register network take"""
    g, gr, fan = uc.graph_ring(12, 24, 2000, 4), 64, [40, 2]
    roots = _mixed_roots(g.n, gr, G, seed=50)
    hb, ref = _case(eng, request, g, gr, fan, G, roots, want)
    tr, t0 = uc.tag(roots, gr, g.n), uc.tag(hb["nbr"][0], gr * fan[0], g.n)
    ids, occ = np.unique(np.concatenate([tr, t0]), return_counts=True)
    once = (occ[np.searchsorted(ids, tr)] == 1) & (tr != INVALID) & (hb["cnt"][0] > 32)
    assert once.sum() >= G  # (on the device's own tree)
    rows = hb["root_local"][once]
    assert ((hb["rowend"][rows] - hb["rowptr"][rows]) == hb["cnt"][0][once]).all()


_BIG = {  # hub's row: (k parents, hub in-degree, gr, fan, the hub is a root)
    "level1": (470, 24000, 470, [1, 64], False),
    "level0": (380, 40000, 2048, [8, 60], True),
}


@pytest.mark.parametrize("route", ["lg3", "lg2"])
@pytest.mark.parametrize("level", list(_BIG))
def test_row_beyond_the_lds_sort(eng, request, level, route):
    """one row of more than 16,384 entries with more than 16,384 distinct sources (the global-memory sort): the hub's
    level-1 row under 470 parents of 64 children each, and — the hub a root itself, its parents' children extras — its
    level-0 row.  LG3: one batch carries it, the others hold INVALID roots only"""
    k, degree, gr, fan, hub_is_root = _BIG[level]
    g = uc.graph_big_row(k, degree)
    first = np.full(gr, INVALID, dtype=np.uint32)
    first[:k] = np.arange(1, k + 1)
    if hub_is_root:
        first[k] = 0
    probe = uc.route(gr, fan, 1)
    G = 1 if route == "lg2" else -(-32 // max(probe["parts"], 1))
    want = dict(build=uc.LG2) if route == "lg2" else dict(build=uc.LG3, threads=1024)
    roots = np.concatenate([first, np.full(gr * (G - 1), INVALID, dtype=np.uint32)])
    hb, ref = _case(eng, request, g, gr, fan, G, roots, want)
    ids, lens = uc.predup_row_lengths(roots, fan, gr, g.n, hb["nbr"], hb["cnt"])
    assert ids[0] == 0 and lens[0] == k * fan[1] + (fan[0] if hub_is_root else 0) and lens[0] > 16384
    assert int((ref["edge_keys"] >> np.uint64(32) == 0).sum()) > 16384  # the oracle's row of the hub: distinct sources
    hub = int(np.nonzero(hb["nodes"] == 0)[0][0])
    assert (hub < ref["n0"]) == hub_is_root
    assert hb["rowend"][hub] - hb["rowptr"][hub] > 16384


# ------------------------------------------------------------------------------------------------- overflow (LAST)
def test_a_batch_beyond_the_workspace_is_reported_on_the_lds_route(eng, request):
    """28 roots that are each other's in-neighbours, 272 more in-neighbours each, fan-out [16, 64]: every hop-0 slot
    that holds a root turns 64 sampled children into level-1 nodes — the batch has more nodes of level < 2 than its
    28 * 17 rows, and more than the slots of its LDS table.  The build says so; nothing else is asserted."""
    gr, fan, G = 28, [16, 64], 32
    g = uc.graph_overflow(gr, 272)
    r = uc.assert_route(gr, fan, G, dict(build=uc.LG3, threads=1024, parts=1, table_slots=1024))
    print(f"\nROUTE {request.node.name} {uc.route_name(r)}")
    roots = np.concatenate([np.arange(gr, dtype=np.uint32), np.full(gr * (G - 1), INVALID, dtype=np.uint32)])
    hb = _run(eng, g, gr, fan, G, roots)
    uc.check_tree(hb, g.rowptr, g.col, roots, fan)
    ref = uc.reference(roots, fan, gr, g.n, hb["nbr"])
    assert ref["inner_per_batch"][0] > r["table_slots"] * r["parts"] > gr * (1 + fan[0])
    assert hb["meta"][uc.META_OVERFLOW] != 0
