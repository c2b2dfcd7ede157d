"""expand_rows_kernel walks its work lists as a software pipeline: a step's candidates, the next step's descriptors and
the items of the step after that are in flight together, a pair's items are one 8-byte load, and the partner of an odd
last row is chosen by a select.  Only the time a load is issued changed, so every case below is the sampler against the
CPU oracle, bit-exact on ids and counts, at the shapes where the pipeline can go wrong: lists of 0, 1, 2 and an odd
number of rows, waves of exactly 1, 2 and 3 steps (prologue only, prologue + last step, steady state), a hop of more
than one copy of the grid, pairs of rows of different kinds, and the plan's captured replay.

Shapes follow from run_expand (sample.hip): parent slots go to 64 lists in blocks of 256, the grid is min(2048, about
n_parents / 8) workgroups of four waves, wave g walks list g % 64 from pair g / 64 in strides of waves / 64, and a copy of
the grid is 16 steps of a wave."""
import numpy as np
import pytest
import torch

import oracle
from helpers import rmat_edges

pytestmark = pytest.mark.gpu

N_RING = 1 << 13


@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _check_tree(eng, rowptr, col, roots, fanouts, **kw):
    tree = eng.sample_khop(roots, fanouts, **kw)
    nbr_o, cnt_o = oracle.sample_khop(rowptr, col, roots, fanouts, canonical=True, **kw)
    for k in range(len(fanouts)):
        assert np.array_equal(tree.cnt[k].cpu().numpy(), cnt_o[k]), f"cnt hop {k}"
        assert np.array_equal(_u32(tree.nbr[k]), nbr_o[k]), f"nbr hop {k}"
    return cnt_o


def _ring_rmat(n_rmat_edges, seed):
    """R-MAT edges plus a +-3 ring, undirected: every node has degree >= 6, so with a last fanout of 5 every valid slot of
    the last hop is a row the expansion pass has to select from"""
    s, d = rmat_edges(13, n_rmat_edges, seed=seed)
    v = np.arange(N_RING)
    ring_s = np.concatenate([v, v, v])
    ring_d = np.concatenate([(v + 1) % N_RING, (v + 2) % N_RING, (v + 3) % N_RING])
    src = np.concatenate([s % N_RING, ring_s]).astype(np.uint32)
    dst = np.concatenate([d % N_RING, ring_d]).astype(np.uint32)
    rowptr, col = oracle.build_csc(N_RING, src, dst, is_directed=False)
    deg = np.diff(rowptr)
    assert deg.min() >= 6
    return rowptr, col, np.nonzero(deg >= 10)[0].astype(np.uint32)


@pytest.fixture(scope="module")
def ring_rmat():
    return _ring_rmat(120000, 21)


# roots of degree >= 10 under [10, 5]: the last hop has exactly 10 real rows per root.  16,384 rows are one step of every
# wave of the full grid (64 lists x 128 waves x 2 rows); one block of 256 slots more puts a second / third step on a list.
@pytest.mark.parametrize("n_roots", [1638, 1639, 3276, 3277, 4915, 4916])
def test_waves_of_one_two_and_three_steps(eng, ring_rmat, n_roots):
    rowptr, col, wide = ring_rmat
    eng.load_csc(rowptr, col)
    roots = wide[np.random.default_rng(n_roots).integers(0, wide.size, size=n_roots)]
    cnt_o = _check_tree(eng, rowptr, col, roots, [10, 5])
    assert int((cnt_o[0] == 10).sum()) == n_roots and int((cnt_o[1] == 5).sum()) == 10 * n_roots


def test_a_hop_of_more_than_one_copy_of_the_grid(eng):
    """40,000 roots x [10, 5]: more than 262,144 real rows in the last hop (2,048 workgroups x 4 waves x 16 steps x 2
    rows): the second copy of the grid runs its own prologue, and the last copy is partly empty.  (Fewer R-MAT edges
    than the other cases' graph: the oracle's time goes with the rows' lengths.)"""
    rowptr, col, _ = _ring_rmat(16000, 22)
    eng.load_csc(rowptr, col)
    roots = np.random.default_rng(3).integers(0, N_RING, size=40000).astype(np.uint32)
    cnt_o = _check_tree(eng, rowptr, col, roots, [10, 5])
    assert int((cnt_o[1] == 5).sum()) > 262144


def _hub_graph(hubs, n=4096, hub_deg=40):
    """directed, simple: the nodes in `hubs` have hub_deg in-neighbours, every other node exactly two"""
    v = np.arange(n)
    src = [(v + 1) % n, (v + 2) % n]
    dst = [v, v]
    for h in hubs:
        src.append((h + 3 + np.arange(hub_deg - 2)) % n)
        dst.append(np.full(hub_deg - 2, h))
    src, dst = np.concatenate(src).astype(np.uint32), np.concatenate(dst).astype(np.uint32)
    return oracle.build_csc(n, src, dst, is_directed=True)


def test_lists_of_zero_one_two_and_three_rows(eng):
    """rows of degree <= f are finished by the planning pass: only the hubs reach a work list.  Parent slot p goes to list
    (p / 256) % 64, so the hubs' places among the roots decide each list's length"""
    hubs = np.array([100, 200, 300, 400, 500, 600, 700, 800, 900])
    rowptr, col = _hub_graph(hubs)
    eng.load_csc(rowptr, col)
    plain = np.arange(1000, 1000 + 1024, dtype=np.uint32)  # degree 2
    # every list empty: copy-through rows, and INVALID parents behind roots without in-edges at the second hop
    _check_tree(eng, rowptr, col, plain, [3, 3])
    _check_tree(eng, rowptr, col, np.full(300, 0xFFFFFFFF, np.uint32), [3, 3])
    # exactly one row of degree > f in the whole hop
    roots = plain.copy()
    roots[5] = hubs[0]
    _check_tree(eng, rowptr, col, roots, [3])
    # lists of 3, 2, 1 and 4 rows next to each other (blocks of 256 roots): an odd list between even ones reads the word
    # past its end and pairs its last row with the ROW_SKIP slot
    roots = plain.copy()
    roots[[3, 77, 255]] = hubs[:3]
    roots[[256, 511]] = hubs[3:5]
    roots[[600]] = hubs[5:6]
    roots[[768, 769, 1000, 1023]] = hubs[[6, 7, 8, 0]]
    _check_tree(eng, rowptr, col, roots, [3])
    _check_tree(eng, rowptr, col, roots, [3, 2])  # (hop 1: the hubs' sampled neighbours have degree 2)


@pytest.mark.parametrize("seed", [42, 2**31 - 1, -(2**31), 1234567891])
def test_pairs_of_rows_of_different_kinds(eng, seed):
    """a hub of 3,000 neighbours (a run of one of the table's levels) next to rows of 12 and 100 (the flat array), rows
    shorter than the fanout and INVALID parents in between; the extreme seeds move windows out of the table (hashed on
    the spot), as test_int32_wraparound_of_key_sum does"""
    rng = np.random.default_rng(8)
    n = 6000
    src = [rng.choice(n, size=3000, replace=False), rng.choice(n, size=700, replace=False),
           rng.choice(n, size=100, replace=False), rng.choice(n, size=12, replace=False),
           rng.choice(n, size=129, replace=False), rng.choice(n, size=3, replace=False)]
    dst = [np.full(m.size, i) for i, m in enumerate(src)]
    s, d = rmat_edges(12, 40000, seed=5)
    src, dst = np.concatenate(src + [s]).astype(np.uint32), np.concatenate(dst + [d]).astype(np.uint32)
    rowptr, col = oracle.build_csc(n, src, dst, is_directed=True)
    eng.load_csc(rowptr, col)
    roots = np.array([0, 3, 1, 2, 0xFFFFFFFF, 5, 4, 0, 0xFFFFFFFF, 0xFFFFFFFF, 3, 4, 1, 5999, 2, 0, 3], dtype=np.uint32)
    roots = np.concatenate([roots, rng.integers(0, n, size=300).astype(np.uint32)])
    _check_tree(eng, rowptr, col, roots, [10, 5], sampling_seed=seed)
    _check_tree(eng, rowptr, col, roots, [4, 3, 2], sampling_seed=seed)


def test_multi_edge_rows_share_pairs_with_fast_rows(eng):
    """directed multi-edge graph: every row takes the general path (short rows are ROW_COPY and still need their
    repeated ids removed), one after the other behind the step's prefetches"""
    rng = np.random.default_rng(14)
    n = 2000
    src = rng.integers(0, 300, size=30000).astype(np.uint32)
    dst = rng.integers(0, n, size=30000).astype(np.uint32)
    src = np.concatenate([src, np.full(300, 9, np.uint32), np.arange(50, 250, dtype=np.uint32)])
    dst = np.concatenate([dst, np.full(500, 4, np.uint32)])
    rowptr, col = oracle.build_csc(n, src, dst, is_directed=True, keep_multi_edges=True)
    eng.build_from_coo(n, src, dst, is_directed=True, keep_multi_edges=True)
    rp, cl = eng.graph_to_host()
    assert np.array_equal(rp, rowptr) and np.array_equal(cl, col)
    roots = np.concatenate([np.array([4, 4, 0], np.uint32), rng.integers(0, n, size=350).astype(np.uint32)])
    for fan in ([10, 5], [20], [3, 3]):
        _check_tree(eng, rowptr, col, roots, fan)


def test_plan_replay_rows_equal_eager_single_batch_rows(eng, ring_rmat):
    """gigl_sage_plan_run with groups under hipGraph replay: the second (replayed) call's rows equal those of eager
    single-batch calls, bit for bit"""
    from gigl_amd.models import GraphSAGE
    rowptr, col, _ = ring_rmat
    x = (np.random.default_rng(0).standard_normal((N_RING, 32)) / 8).astype(np.float32)
    eng.load_csc(rowptr, col)
    eng.load_features(x)
    torch.manual_seed(4)
    model = GraphSAGE(32, 24, 12, num_layers=2).to(eng.device)
    b, fan, G = 48, [10, 5], 3
    roots = torch.from_numpy(np.random.default_rng(5).integers(0, N_RING, size=(2, G * b)).astype(np.int32)).to(eng.device)
    single = model.make_plan(eng, b, fan)
    grouped = model.make_plan(eng, b, fan, groups=G)
    want = [torch.cat([single.run(roots[i, g * b:(g + 1) * b].contiguous()).clone() for g in range(G)]) for i in range(2)]
    st = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    torch.cuda.set_stream(st)
    try:
        grouped.use_graph(True)
        first = grouped.run(roots[0]).clone()  # (call 0 captures)
        second = grouped.run(roots[1]).clone()
        st.synchronize()
        assert torch.equal(first, want[0])
        assert torch.equal(second, want[1])
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream(eng.device))
        eng.bind_stream(None)
        grouped.close()
        single.close()
