"""CPU-side checks of tests/union_cases.py: the route table of the leaf-global union tests as gigl_union_route answers it
(host-only query, no device), and the checker's teeth — it accepts a correct leaf-global union synthesized from the
oracle's output, for one batch and for several, and rejects every single-word corruption listed below, each through the
property that is there to catch it."""
import functools

import numpy as np
import pytest

import oracle
import union_cases as uc


@pytest.mark.parametrize("label,gr,f0,f1,G,want", uc.ROUTE_TABLE, ids=[r[0] for r in uc.ROUTE_TABLE])
def test_route_table(label, gr, f0, f1, G, want):
    uc.assert_route(gr, [f0, f1], G, want)


def test_route_query_answers_for_the_other_builds_and_rejects_bad_shapes():
    import ctypes as C
    from gigl_amd import _lib
    assert uc.route(300, [25, 10], 1, leaf_global=0)["build"] == uc.GENERIC  # the public entry points
    assert uc.route(300, [25], 1)["build"] == uc.GENERIC                     # the one-hop plans
    assert uc.route(64, [5, 4, 3], 1, leaf_global=0)["build"] == uc.GENERIC
    # the full 64-bit root mask at both workgroup shapes; one hop-0 slot more leaves LG3
    assert uc.route(1024, [32, 1], 52)["threads"] == 512 and uc.route(1025, [32, 1], 52)["threads"] == 1024
    assert uc.route(2048, [32, 1], 4)["build"] == uc.LG3 and uc.route(2049, [32, 1], 4)["why"] == uc.WHY_CODES
    assert uc.route(64, [25, 65], 64)["why"] == uc.WHY_CODES  # (more than 64 children per slot)
    assert uc.route(65536, [1, 1], 1)["parts"] == 16         # (the root mask bounds a batch before 17 partitions do)
    lib = _lib.load()
    out, fo = (C.c_int32 * 8)(), (C.c_int32 * 2)(3, 2)
    assert lib.gigl_union_route(10, fo, 2, 4, 1, out) == -1   # group_roots does not divide b
    assert lib.gigl_union_route(0, fo, 2, 1, 1, out) == -1
    assert lib.gigl_union_route(8, fo, 2, 4, 1, None) == -1
    assert lib.gigl_union_route(8, None, 2, 4, 1, out) == -1


def _case(grouped):
    """a small dense graph: roots that are each other's neighbours, repeated roots, an INVALID root; grouped: four
    batches, the same root in two of them"""
    g = uc.graph_dense()
    gr, fan = (24, [4, 3]) if grouped else (48, [5, 3])
    G = 4 if grouped else 1
    roots = np.random.default_rng(3).integers(0, g.n, gr * G).astype(np.uint32)
    roots[5] = roots[4]
    roots[9] = uc.INVALID
    if grouped:
        roots[gr + 2] = roots[0]  # the same root in batches 0 and 1
        roots[gr + 3] = roots[gr + 2]
    nbr, cnt = oracle.sample_khop(g.rowptr, g.col, roots, fan, canonical=True)
    return roots, fan, gr, g.n, nbr, cnt


@functools.lru_cache(maxsize=None)
def _good(grouped):
    roots, fan, gr, n, nbr, cnt = _case(grouped)
    ref = uc.reference(roots, fan, gr, n, nbr)
    return roots, ref, uc.synthesize(ref, nbr, cnt), nbr, cnt


@pytest.fixture(scope="module", params=[False, True], ids=["single", "grouped"])
def good(request):
    return _good(request.param)


def _copy(hb):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in hb.items()}


def _row(hb, ref, level, min_len):
    """a stored row of `level` with at least min_len entries"""
    n0, n1 = ref["n0"], ref["n1"]
    lo, hi = (0, n0) if level == 0 else (n0, n1)
    lens = hb["rowend"][lo:hi] - hb["rowptr"][lo:hi]
    ok = np.nonzero((lens >= min_len) & (hb["rowptr"][lo:hi] < ref["cap_edges"]))[0]
    assert ok.size
    return lo + int(ok[0])


def test_checker_accepts_a_correct_union(good):
    roots, ref, hb, nbr, cnt = good
    assert ref["n1"] > ref["n0"] > 0 and (ref["root_local"] == -1).sum() == 1 and uc.fits_workspace(ref)
    assert (hb["rowptr"][:ref["n1"]] >= ref["cap_edges"]).any()  # some rows alias their tree segment
    uc.check(hb, ref)
    # level 1 in any order, rows with or without spare capacity
    uc.check(uc.synthesize(ref, nbr, cnt, reverse_level1=False, slack=0), ref)


def test_checker_rejects_a_dropped_edge(good):
    _, ref, hb, _, _ = good
    for level in (0, 1):
        m = _copy(hb)
        m["rowend"][_row(m, ref, level, 2)] -= 1
        with pytest.raises(AssertionError, match="^edges"):
            uc.check(m, ref)


def test_checker_rejects_an_entry_twice_in_a_row(good):
    _, ref, hb, _, _ = good
    for level in (0, 1):
        m = _copy(hb)
        p = m["rowptr"][_row(m, ref, level, 2)]
        m["col"][p + 1] = m["col"][p]
        with pytest.raises(AssertionError, match="^row order"):
            uc.check(m, ref)


def test_checker_rejects_two_entries_swapped(good):
    _, ref, hb, _, _ = good
    for level in (0, 1):
        m = _copy(hb)
        p = m["rowptr"][_row(m, ref, level, 2)]
        m["col"][[p, p + 1]] = m["col"][[p + 1, p]]
        with pytest.raises(AssertionError, match="^row order"):
            uc.check(m, ref)


def test_checker_rejects_level0_ids_exchanged(good):
    """a CONSISTENT renumbering — nodes, rows, row contents and root_local all follow — is still not the oracle's order"""
    _, ref, hb, nbr, cnt = good
    perm = np.arange(ref["n0"])
    perm[[1, 2]] = perm[[2, 1]]
    m = uc.synthesize(ref, nbr, cnt, perm0=perm)
    with pytest.raises(AssertionError, match="^nodes: level 0"):
        uc.check(m, ref)
    # and exchanged in the rows alone: the edges are other ones
    m = _copy(hb)
    c = m["col"][:ref["cap_edges"]]
    stored0 = np.zeros(c.size, bool)
    for i in range(ref["n0"]):
        stored0[m["rowptr"][i]:m["rowend"][i]] = True
    a, b = stored0 & (c == 1), stored0 & (c == 2)
    assert a.any() or b.any()
    c[a], c[b] = 2, 1
    with pytest.raises(AssertionError, match="^(edges|row order|batch membership)"):
        uc.check(m, ref)


def test_checker_rejects_a_level1_node_referenced_from_two_batches():
    """(the grouped case only: one batch has no second batch to reference a node from)"""
    _, ref, hb, _, _ = _good(True)
    n0 = ref["n0"]
    m = _copy(hb)
    batch0 = ref["nodes0"] // ref["n"]
    # level 1 is numbered in reverse here, so the last batch's level-1 ids are the smallest: a level-1 id named by a row
    # of another batch goes behind the last entry of one of its rows (into the row's spare word: still ascending)
    last = ref["G"] - 1
    others = np.concatenate([m["col"][m["rowptr"][k]:m["rowend"][k]] for k in np.nonzero(batch0 != last)[0]])
    j = int(others.max())
    spare = [k for k in np.nonzero(batch0 == last)[0] if m["rowend"][k] > m["rowptr"][k] and m["col"][m["rowend"][k]] == -7]
    i = int(spare[0])
    assert j >= n0 and j > m["col"][m["rowend"][i] - 1]
    m["col"][m["rowend"][i]] = j
    m["rowend"][i] += 1
    with pytest.raises(AssertionError, match="^batch membership"):
        uc.check(m, ref)


def test_checker_rejects_a_repeated_roots_entry_at_the_wrong_copy(good):
    roots, ref, hb, _, _ = good
    m = _copy(hb)
    if ref["G"] == 1:
        assert roots[5] == roots[4] and m["root_local"][5] == m["root_local"][4]
        m["root_local"][5] = (m["root_local"][5] + 1) % ref["n0"]
    else:
        gr = ref["gr"]
        assert roots[gr + 3] == roots[gr + 2] == roots[0] and m["root_local"][gr + 3] == m["root_local"][gr + 2]
        assert m["root_local"][gr + 3] != m["root_local"][0]
        m["root_local"][gr + 3] = m["root_local"][0]  # batch 0's copy of the same global id
    with pytest.raises(AssertionError, match="^root_local"):
        uc.check(m, ref)


def test_checker_rejects_an_edge_count_off_by_one(good):
    _, ref, hb, _, _ = good
    for d in (-1, 1):
        m = _copy(hb)
        m["meta"][1] += d
        with pytest.raises(AssertionError, match="^meta"):
            uc.check(m, ref)
    m = _copy(hb)
    m["meta"][uc.META_OVERFLOW] = 1
    with pytest.raises(AssertionError, match="^overflow"):
        uc.check(m, ref)


def test_checker_rejects_a_stored_row_overlapping_its_neighbour(good):
    """a row moved down so that its first word lies on the last word of the row stored before it"""
    _, ref, hb, _, _ = good
    m = _copy(hb)
    n1 = ref["n1"]
    rp, re_ = m["rowptr"][:n1], m["rowend"][:n1]
    stored = np.nonzero((re_ > rp) & (rp < ref["cap_edges"]))[0]
    order = stored[np.argsort(rp[stored])]
    prev, i = int(order[2]), int(order[3])
    row = m["col"][rp[i]:re_[i]].copy()
    start = re_[prev] - 1
    m["col"][start:start + row.size] = row
    m["rowptr"][i], m["rowend"][i] = start, start + row.size
    with pytest.raises(AssertionError, match="^row storage: stored rows overlap"):
        uc.check(m, ref)


def test_checker_rejects_a_row_out_of_bounds(good):
    _, ref, hb, _, _ = good
    m = _copy(hb)
    i = _row(m, ref, 1, 1)
    m["rowend"][i] = m["col"].size + 1
    with pytest.raises(AssertionError, match="^row bounds"):
        uc.check(m, ref)


def test_row_class_and_overflow_graphs_are_what_the_gpu_tests_need():
    """the degree-forced graphs hit the lengths they name, on the oracle's tree (the GPU tests assert it again on the
    device's)"""
    g, roots, named0, named1 = uc.graph_row_classes()
    fan = uc.ROW_CLASS_FAN
    nbr, cnt = oracle.sample_khop(g.rowptr, g.col, roots, fan, canonical=True)
    ids, lens = uc.predup_row_lengths(roots, fan, roots.size, g.n, nbr, cnt)
    for L in uc.ROW_CLASS_LENGTHS:
        assert lens[np.searchsorted(ids, named0[L])] == L and lens[np.searchsorted(ids, named1[L])] == L
    ref = uc.reference(roots, fan, roots.size, g.n, nbr)
    assert uc.fits_workspace(ref)
    uc.check(uc.synthesize(ref, nbr, cnt), ref)
