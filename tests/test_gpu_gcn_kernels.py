"""The GCN training plan's kernels through the C ABI (gigl_gcn_dinv, gigl_gcn_gather, gigl_gcn_gather_backward_lists:
csrc/agg.hip gcn_dinv_kernel, gcn_gather_rows_kernel<T, LPR, VPL>, gcn_gather_scalar_kernel<T>, gcn_gather_bwd_kernel<LPR,
VEC>) on hand-built CSRs, against an explicit dense float64 A_hat and its transpose.  No sampler is involved.

Graph A (N_ROWS_CAP row slots, N_ROWS live rows, N_SRC live sources of N_SRC_CAP): rows of 0, 1, 63, 64, 65 and 130 edges, a
row that stores only its self loop, a row with a stored self loop among others, a row that stores one source twice, the rest
0..12 random edges; sources that nobody reads below and above N_ROWS; a source read only by itself.  Graph B: 300 rows that
all read one source (a reader list of 300) beside a few random ones.  Buffers hold a sentinel beyond the live rows / sources
that must survive.

Reference: A_hat[i][j] = dinv_i dinv_j per stored edge j != i (a source stored twice counts twice), A_hat[i][i] = dinv_i^2,
dinv = 1 / sqrt(1 + non-self in-edges) in float64; forward = A_hat x, backward = A_hat^T y.  The same products in float32 on
the CPU are the yardstick: a bound is the larger of 1e-5 x the tensor's largest magnitude (the project's bar for fp32 rows) and
4 x the float32 CPU computation's error against float64.  The device results must also satisfy <A_hat x, y> = <x, A_hat^T y>,
and the forward run twice must give the same bits.  Nothing reads a device result to form an expectation.

Measured on an MI355X (worst over the cases of a row; err and fp32 relative to the tensor's largest magnitude):

    quantity                                          err       fp32
    dinv                                          2.4e-08    2.4e-08
    forward fp32 rows, vector paths               2.2e-07    1.7e-07
    forward fp32 rows, element paths              2.1e-07    1.4e-07
    forward fp16 rows, vector paths               1.6e-07    2.4e-07
    forward fp16 rows, element paths              2.0e-07    1.5e-07
    backward graph A, vector paths                1.7e-07    1.1e-07
    backward graph A, element paths               1.4e-07    1.8e-07
    backward reader list of 300, vector paths     5.5e-07    9.2e-07
    backward reader list of 300, element paths    6.3e-07    5.1e-07
    adjoint identity, |lhs - rhs| / scale         1.4e-08          -
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
N_ROWS_CAP, N_ROWS, N_SRC_CAP, N_SRC = 308, 300, 324, 316
SPECIAL_DEGREES = [0, 1, 63, 64, 65, 130]  # rows 0..5
ONLY_SELF, SELF_AMONG, TWICE = 6, 7, 8      # rows
UNREAD_LOW, UNREAD_HIGH = 11, N_ROWS + 5    # sources nobody reads, below / above the live rows
HOT = 9                                      # graph B: the source every row reads
WIDEST_VECTOR_D = 1024                       # gcn_gather_rows_kernel<T, 64, 4>
# (the second line: widths for the instantiations the first leaves out — see test_graphs_hold_what_the_cases_claim)
WIDTHS = [1, 3, 4, 20, 64, 256, 260, WIDEST_VECTOR_D + 4,
          18, 37, 70, 72, 132, WIDEST_VECTOR_D]
SENTINEL = 7.0
BAR = 1e-5


# ---- graphs (CPU) -------------------------------------------------------------------------------------------------------
def _pool(rng, forbidden):
    return np.array([j for j in range(N_SRC) if j not in forbidden], dtype=np.int64)


@functools.lru_cache(None)
def graph(which: str):
    """-> rows (list of int64 arrays, one per live row), rowptr / rowend int32 [N_SRC_CAP + 1] (rows at and beyond N_ROWS
    are empty), col int32"""
    rng = np.random.default_rng(5 if which == "A" else 6)
    rows = []
    if which == "A":
        pool = _pool(rng, {ONLY_SELF, UNREAD_LOW, UNREAD_HIGH})
        for i, deg in enumerate(SPECIAL_DEGREES):  # (no stored self loop: every entry of these rows is an edge to add)
            rows.append(rng.choice(pool[pool != i], deg, replace=False))
        rows.append(np.array([ONLY_SELF]))
        r = rng.choice(pool[pool != SELF_AMONG], 5, replace=False)
        rows.append(np.concatenate([r[:2], [SELF_AMONG], r[2:]]))
        r = rng.choice(pool[pool != TWICE], 4, replace=False)
        rows.append(np.concatenate([r, r[1:2]]))
        for i in range(len(rows), N_ROWS):
            deg = int(rng.integers(0, 13))
            r = rng.choice(pool, deg, replace=False)
            if i % 7 == 0 and deg:  # more stored self loops, at any position
                r[int(rng.integers(0, deg))] = i
            rows.append(r)
    else:
        pool = _pool(rng, set())
        for i in range(N_ROWS):
            r = rng.choice(pool[pool != HOT], int(rng.integers(0, 4)), replace=False)
            rows.append(np.concatenate([r[:1], [HOT], r[1:]]))
    deg = np.array([r.size for r in rows] + [0] * (N_SRC_CAP - N_ROWS), dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(deg)])
    return types.SimpleNamespace(rows=rows, rowptr=rp[:-1].astype(np.int32), rowend=rp[1:].astype(np.int32),
                                 col=np.concatenate(rows).astype(np.int32))


def a_hat(which: str, dtype):
    """-> (dense A_hat [N_ROWS, N_SRC], dinv [N_SRC]) in `dtype`, every product and sum in that precision"""
    gr = graph(which)
    deg = np.ones(N_SRC, dtype=dtype)
    for i, r in enumerate(gr.rows):
        deg[i] += dtype((r != i).sum())
    dinv = (dtype(1.0) / np.sqrt(deg)).astype(dtype)
    a = np.zeros((N_ROWS, N_SRC), dtype=dtype)
    for i, r in enumerate(gr.rows):
        a[i, i] += dinv[i] * dinv[i]
        for j in r[r != i]:
            a[i, j] += dinv[i] * dinv[j]
    return a, dinv


def _exact(rng, shape, half=False):
    """random values that float32 (float16) holds exactly, as float32 / float16"""
    x = rng.standard_normal(shape).astype(np.float32)
    return x.astype(np.float16) if half else x


def _bound(want, e32):
    return max(BAR * float(np.abs(want).max()), 4.0 * e32)


def _report(label, got, want, want32):
    err = float(np.abs(got.astype(np.float64) - want).max())
    e32 = float(np.abs(want32.astype(np.float64) - want).max())
    big = max(float(np.abs(want).max()), 1e-300)
    print(f"{label}: err={err / big:.3e} fp32={e32 / big:.3e}")
    assert np.isfinite(got).all(), label
    assert err <= _bound(want, e32), (label, err, e32, big)


# ---- device side --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _count(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def _csr(which):
    gr = graph(which)
    return types.SimpleNamespace(rowptr=_dev(gr.rowptr), rowend=_dev(gr.rowend), col=_dev(gr.col), n_edges=int(gr.col.size))


def _dinv(eng, csr, n_nodes=N_SRC):
    from gigl_amd._lib import check
    dinv, nn = torch.full((N_SRC_CAP,), SENTINEL, dtype=torch.float32, device="cuda"), _count(n_nodes)
    torch.cuda.synchronize()
    check(eng._lib.gigl_gcn_dinv(eng._ctx, _p(csr.rowptr), _p(csr.rowend), _p(csr.col), _p(nn), N_SRC_CAP, _p(dinv)), eng._ctx)
    eng.synchronize()
    return dinv


def _gather(eng, csr, dinv, h, d, gid, n_rows, out=None):
    from gigl_amd._lib import DTYPE_F16, DTYPE_F32, check
    if out is None:
        out = torch.full((N_ROWS_CAP, d), SENTINEL, dtype=torch.float32, device="cuda")
    nr = _count(n_rows)
    torch.cuda.synchronize()
    check(eng._lib.gigl_gcn_gather(eng._ctx, _p(h), DTYPE_F16 if h.dtype == torch.float16 else DTYPE_F32, d, _p(gid), _p(dinv),
                                   _p(csr.rowptr), _p(csr.rowend), _p(csr.col), _p(nr), N_ROWS_CAP, _p(out)), eng._ctx)
    eng.synchronize()
    return out


def _backward(eng, csr, dinv, dout, d, n_rows, n_src):
    from gigl_amd._lib import check
    lib = eng._lib
    words = int(lib.gigl_transposed_rows_words(N_SRC_CAP, csr.n_edges))
    lists = torch.zeros(words, dtype=torch.int32, device="cuda")
    dsrc = torch.full((N_SRC_CAP, d), SENTINEL, dtype=torch.float32, device="cuda")
    nr, ns = _count(n_rows), _count(n_src)
    torch.cuda.synchronize()
    check(lib.gigl_transposed_rows_build(eng._ctx, _p(csr.rowptr), _p(csr.rowend), _p(csr.col), _p(nr), N_ROWS_CAP, _p(ns),
                                         N_SRC_CAP, csr.n_edges, _p(lists)), eng._ctx)
    check(lib.gigl_gcn_gather_backward_lists(eng._ctx, _p(dout), d, _p(dinv), _p(csr.rowptr), _p(csr.rowend), _p(nr), _p(ns),
                                             N_SRC_CAP, _p(lists), _p(dsrc)), eng._ctx)
    eng.synchronize()
    return dsrc


def _source(rng, d, half, ids):
    """-> (x float64 [N_SRC, d], what the kernel reads, gather_ids): local rows, or rows of a wider table through ids; the
    rows no live source names are NaN"""
    x = _exact(rng, (N_SRC, d), half)
    if not ids:
        h = np.full((N_SRC_CAP, d), np.nan, dtype=x.dtype)
        h[:N_SRC] = x
        return x.astype(np.float64), _dev(h), None
    n_tab = 400
    gid = rng.permutation(n_tab)[:N_SRC]
    table = np.full((n_tab, d), np.nan, dtype=x.dtype)
    table[gid] = x
    gids = np.zeros(N_SRC_CAP, dtype=np.int32)
    gids[:N_SRC] = gid
    return x.astype(np.float64), _dev(table), _dev(gids)


# ---- tests --------------------------------------------------------------------------------------------------------------
@gpu
def test_dinv_against_float64(eng):
    for which in ("A", "B"):
        _, want = a_hat(which, np.float64)
        _, want32 = a_hat(which, np.float32)
        got = _dinv(eng, _csr(which)).cpu().numpy()
        _report(f"dinv {which}", got[:N_SRC], want, want32)
        assert (got[N_SRC:] == SENTINEL).all()
        assert float(want[ONLY_SELF]) == 1.0 or which == "B"  # (a row that stores only its self loop has degree 1)


@gpu
@pytest.mark.parametrize("ids", [False, True], ids=["local", "ids"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("d", WIDTHS)
def test_gather_against_dense_float64(eng, d, half, ids):
    rng = np.random.default_rng(1000 + 8 * d + 2 * half + ids)
    a64, _ = a_hat("A", np.float64)
    a32, _ = a_hat("A", np.float32)
    x, h, gid = _source(rng, d, half, ids)
    want, want32 = a64 @ x, a32 @ x.astype(np.float32)
    csr = _csr("A")
    dinv = _dinv(eng, csr)
    out = _gather(eng, csr, dinv, h, d, gid, N_ROWS)
    got = out.cpu().numpy()
    _report(f"gather d={d} {'fp16' if half else 'fp32'} {'ids' if ids else 'local'}", got[:N_ROWS], want, want32)
    assert (got[N_ROWS:] == SENTINEL).all(), "rows at and beyond *n_rows_dev were touched"
    again = _gather(eng, csr, dinv, h, d, gid, N_ROWS)
    assert torch.equal(out, again), "two runs differ"
    # fewer live rows than the capacity, and none
    short = _gather(eng, csr, dinv, h, d, gid, 5).cpu().numpy()
    assert np.array_equal(short[:5], got[:5]) and (short[5:] == SENTINEL).all()
    assert (_gather(eng, csr, dinv, h, d, gid, 0).cpu().numpy() == SENTINEL).all()


@gpu
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("d", WIDTHS)
def test_backward_against_dense_float64_transpose(eng, d, which):
    rng = np.random.default_rng(2000 + 8 * d + (which == "B"))
    a64, _ = a_hat(which, np.float64)
    a32, _ = a_hat(which, np.float32)
    y = _exact(rng, (N_ROWS, d))
    want, want32 = a64.T @ y.astype(np.float64), a32.T @ y
    dout = np.full((N_ROWS_CAP, d), np.nan, dtype=np.float32)
    dout[:N_ROWS] = y
    csr = _csr(which)
    dinv = _dinv(eng, csr)
    got = _backward(eng, csr, dinv, _dev(dout), d, N_ROWS, N_SRC).cpu().numpy()
    _report(f"backward {which} d={d}", got[:N_SRC], want, want32)
    assert (got[N_SRC:] == SENTINEL).all(), "rows at and beyond *n_src_dev were touched"
    if which == "A":
        dv = a_hat("A", np.float64)[1]
        # a source nobody reads: its own term below the live rows, zeros above; a source read only by itself
        assert np.abs(got[UNREAD_LOW] - dv[UNREAD_LOW] ** 2 * y[UNREAD_LOW]).max() <= _bound(want, 0.0)
        assert (got[UNREAD_HIGH] == 0.0).all()
        assert np.abs(got[ONLY_SELF] - y[ONLY_SELF]).max() <= _bound(want, 0.0)
    # the adjoint identity on the device results: <A_hat x, y> = <x, A_hat^T y>
    x = _exact(rng, (N_SRC, d))
    h = np.zeros((N_SRC_CAP, d), dtype=np.float32)
    h[:N_SRC] = x
    fwd = _gather(eng, csr, dinv, _dev(h), d, None, N_ROWS).cpu().numpy()[:N_ROWS].astype(np.float64)
    lhs, rhs = float((fwd * y).sum()), float((x.astype(np.float64) * got[:N_SRC]).sum())
    scale = float(np.abs(fwd * y).sum()) + float(np.abs(x * got[:N_SRC]).sum())
    print(f"adjoint {which} d={d}: |lhs - rhs| / scale = {abs(lhs - rhs) / scale:.3e}")
    assert abs(lhs - rhs) <= BAR * scale


@gpu
def test_backward_with_no_live_row_or_source(eng):
    csr = _csr("A")
    dinv = _dinv(eng, csr)
    dout = torch.zeros(N_ROWS_CAP, 8, device="cuda")
    assert (_backward(eng, csr, dinv, dout, 8, 0, 0).cpu().numpy() == SENTINEL).all()
    # no live row: every live source gets zeros (nobody reads it, it has no row of its own)
    got = _backward(eng, csr, dinv, dout + 1.0, 8, 0, N_SRC).cpu().numpy()
    assert (got[:N_SRC] == 0.0).all() and (got[N_SRC:] == SENTINEL).all()


# ---- the CPU self-check -------------------------------------------------------------------------------------------------
def test_graphs_hold_what_the_cases_claim():
    gr = graph("A")
    assert [gr.rows[i].size for i in range(6)] == SPECIAL_DEGREES
    assert gr.rows[ONLY_SELF].tolist() == [ONLY_SELF]
    assert (gr.rows[SELF_AMONG] == SELF_AMONG).sum() == 1 and gr.rows[SELF_AMONG].size > 1
    vals, cnt = np.unique(gr.rows[TWICE], return_counts=True)
    assert cnt.max() == 2 and TWICE not in vals
    read = np.concatenate([r[r != i] for i, r in enumerate(gr.rows)])
    assert UNREAD_LOW not in read and UNREAD_HIGH not in read and ONLY_SELF not in read
    assert UNREAD_LOW < N_ROWS <= UNREAD_HIGH < N_SRC < N_SRC_CAP and N_ROWS < N_ROWS_CAP
    assert sum(int((r == i).any()) for i, r in enumerate(gr.rows)) >= 20  # stored self loops
    assert read.max() >= N_ROWS  # sources that are no row
    a, dinv = a_hat("A", np.float64)
    assert a[TWICE, gr.rows[TWICE][1]] == 2 * dinv[TWICE] * dinv[gr.rows[TWICE][1]]
    assert a[ONLY_SELF].sum() == 1.0 and dinv[N_ROWS:].max() == 1.0
    assert all(HOT in r for r in graph("B").rows) and len(graph("B").rows) == 300
    # which kernel a width takes (csrc/agg.hip gigl_gcn_gather / gigl_gcn_gather_backward_lists): every path is run
    fwd = {d: ("scalar" if d % 4 or d // 4 > WIDEST_VECTOR_D // 4 else
               next(p for v, p in ((8, (8, 1)), (16, (16, 1)), (32, (32, 1)), (64, (64, 1)), (128, (64, 2)), (256, (64, 4)))
                    if d // 4 <= v)) for d in WIDTHS}
    assert set(fwd.values()) == {"scalar", (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4)}, fwd
    assert fwd[WIDEST_VECTOR_D + 4] == "scalar" and fwd[WIDEST_VECTOR_D] == (64, 4) and fwd[260] == (64, 2)
    units = {d: (d // 4 if d % 4 == 0 else d) for d in WIDTHS}
    lanes = {d: (64 if u >= 64 else 32 if u >= 32 else 16 if u >= 16 else 8, d % 4 == 0) for d, u in units.items()}
    assert set(lanes.values()) == {(w, v) for w in (8, 16, 32, 64) for v in (False, True)}, lanes
