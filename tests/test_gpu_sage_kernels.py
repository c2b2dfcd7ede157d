"""The kernels every GraphSAGE / GCN / link-prediction training step runs — csrc/agg.hip's segmented reduce (forward,
scatter backward, transposed-gather backward), GCN aggregation and weight gradient, csrc/loss.hip's retrieval loss —
called directly through the HipEngine wrappers against float64 references computed on the CPU, at the shapes where the
dispatch code changes path.

References: a few lines each, written here (segment mean / sum / amax, the masked weight gradient, the retrieval loss
with its masks) plus oracle/gnn_ref.py's gcn_conv; backward references are torch autograd through the float64 forward
formula.  The CPU test at the end pins them at 1e-12 against gnn_ref.sage_conv / gcn_conv / retrieval_loss_rows and
against independent torch autograd formulas, and asserts from the parametrisation that every kernel instantiation is run.

Inputs that a comparison decides on (max and its ties, relu_y > 0) lie on the grid of multiples of 1/64 in [-2, 2], so
the kernel's and the reference's masks agree by construction; everything else is random float32 (or float16) values,
widened exactly.

Graph: one CSR by destination, 195 rows over 260 sources; in-degrees 0..129 around every 4 G step (G = 1, 2, 4, 8
source rows per wave instruction) and the 64-entry index chunk, a row of 300, a source read by ~100 rows, sources nobody
reads, a row that lists itself, a row with a duplicated source; packed (rowend = rowptr[1:]) and windowed (a third of
the rows end early; the skipped col entries name a padding row of NaN).  *n_rows_dev = 190 < rows_cap = 195: the output
rows >= 190 keep a sentinel.  Rows of dy / a / relu_y past *m_dev, of dout past *n_rows_dev and the padding columns of
the score matrix are NaN.

Tolerances: forward rtol = atol = 1e-5; gradients rtol = 1e-4, atol = 1e-4 * max|want| per tensor (the project's own).
Per tensor the bound is the larger of that and 4 x the maximum error of the SAME reference formula evaluated in float32
on the CPU (the factor covers summation order, atomics and expf).  The weight gradient's figure is the scaled error
max |got - ref| / (|dy_masked|^T |a|) (db: / sum |dy_masked|) with the project's 4e-7 as the floor; its float32
reference is taken twice — one product, and per-chunk products added in chunk order — and the larger error counts.
Exact: the self half, sentinels, the selection check, excluded columns of the masked logits and of dscores.  Nothing is
derived from the kernel's output.  Every case prints `label tensor: err=<kernel> fp32=<float32 reference>`.

Measured on an MI355X (maximum |kernel - float64|, the scaled figure for the weight gradient, next to the float32
reference's own error; worst case of the class):

    kernel, cases                        tensor     kernel    float32 reference
    weight gradient, rc = 32             dW         1.9e-07   3.1e-07   (scaled figures; bound 4e-7 or 4 x fp32)
                                         db         9.6e-08   9.6e-08
    weight gradient, rc = 128            dW         3.2e-07   1.6e-06
                                         db         1.3e-07   1.9e-07
    weight gradient, rc = 256            dW         1.6e-07   7.0e-07
                                         db         4.7e-08   4.0e-08
    weight gradient, rc = 512 (70 000)   dW         1.8e-07   2.5e-07
                                         db         7.0e-08   1.3e-07
    gather mean, fp32 / fp16 source      reduce     2.4e-07   2.4e-07
    gather sum, fp32 / fp16 source       reduce     4.6e-05   5.3e-05   (max|reduce| ~ 70)
    gather max, fp32 / fp16 source       reduce     0         0
    scatter backward, mean               dsrc       7.2e-06   6.6e-06   (every rows_cap)
    scatter backward, sum                dsrc       1.4e-05   1.3e-05
    scatter backward, max                dsrc       1.1e-05   7.0e-06
    transposed backward, mean            dsrc       6.1e-06   6.4e-06
    transposed backward, sum             dsrc       1.3e-05   1.1e-05
    gcn, fp32 / fp16 source              out        1.9e-06   1.8e-06
    retrieval loss, unit scores          loss       9.1e-04   8.5e-04   (a sum over up to 300 rows)
                                         row_lse    6.3e-06   5.1e-06
                                         logits     6.6e-06   4.9e-06
                                         dscores    3.6e-05   3.6e-05
    retrieval loss, only the diagonal    loss / dscores 0     0
    retrieval loss, scores +-80, no T    loss       9.7e-05   9.6e-04
                                         row_lse    3.7e-06   3.7e-06
                                         dscores    3.6e-06   3.6e-06
    retrieval loss, scores +-80, T 0.07  loss       2.6e-03   1.8e-02   (logits up to +-1143: an ulp is 1.2e-4)
                                         row_lse    1.0e-04   1.0e-04
                                         logits     1.2e-04   1.2e-04
                                         dscores    4.1e-04   4.1e-04
"""
import functools
import types

import pytest
import torch

from oracle import gnn_ref

gpu = pytest.mark.gpu
N_ROWS, N_SRC, N_LIVE = 195, 260, 190  # rows_cap, sources, *n_rows_dev
N_READ = 250  # the sources >= N_READ are read by nobody
DEGREES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300]  # rows 0..21
SELF_ROW, DUP_ROW, HOT = 23, 24, 200  # (neither row is windowed: i % 3 != 1); HOT: the source ~100 rows read
OOB = N_SRC  # what the skipped col entries of a windowed row name: a padding row of NaN after the last source
SENTINEL = 7.0
FLT_MAX = torch.finfo(torch.float32).max


# ---- the graph (CPU int64) ------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _base_rows():
    g = torch.Generator().manual_seed(23)
    rows = [torch.randint(0, N_READ, (d,), generator=g) for d in DEGREES]
    rows.append(torch.randint(0, N_READ, (3,), generator=g))  # row 22
    s = torch.randint(0, N_READ, (4,), generator=g)
    rows.append(torch.cat([s[:1], torch.tensor([SELF_ROW]), s[1:]]))  # row 23 lists itself
    s = torch.randperm(N_READ, generator=g)[:4]
    s = s[s != HOT]
    rows.append(torch.cat([s, s[1:2]]))  # row 24: source s[1] twice
    for i in range(len(rows), N_ROWS):  # the rest: degree 0..6 (the rows a window shortens: 1..6); rows 60..159 read HOT
        deg = max(int(torch.randint(0, 7, (1,), generator=g)), int(i % 3 == 1))
        r = torch.randint(0, N_READ, (deg,), generator=g)
        if 60 <= i < 160:
            r = torch.cat([torch.tensor([HOT]), r[1:]])
        rows.append(r)
    assert len(rows) == N_ROWS
    return rows


def _csr_of(rows, window):
    """-> rowptr [n], rowend [n], col, the rows' effective sources: with `window` every row i % 3 == 1 ends 1 or 2
    entries early and the skipped entries are OOB"""
    deg = torch.tensor([r.numel() for r in rows])
    rp = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(deg, 0)])
    col, rowend, eff = torch.cat(rows).clone(), rp[1:].clone(), list(rows)
    if window:
        for i in range(1, len(rows), 3):
            skip = min(int(deg[i]), 1 + (i // 3) % 2)
            rowend[i] -= skip
            col[int(rowend[i]):int(rp[i + 1])] = OOB
            eff[i] = rows[i][:rows[i].numel() - skip]
    return rp, rowend, col, eff


def _edges(eff, n):
    deg = torch.tensor([r.numel() for r in eff[:n]])
    return torch.stack([torch.cat(eff[:n]), torch.repeat_interleave(torch.arange(n), deg)])


@functools.lru_cache(None)
def sage_graph(window):
    rp, rowend, col, eff = _csr_of(_base_rows(), window)
    return types.SimpleNamespace(rp=rp, rowend=rowend, col=col, rows=eff, window=window,
                                 deg=torch.tensor([r.numel() for r in eff]), ei=_edges(eff, N_LIVE))


@functools.lru_cache(None)
def gcn_graph():
    """the windowed rows, then rows 195..259 (degree 0..3) of the sources that are no destination: a square graph over
    N_SRC nodes, as the union graph is"""
    g = torch.Generator().manual_seed(29)
    rows = list(_base_rows())
    for _ in range(N_ROWS, N_SRC):
        rows.append(torch.randint(0, N_SRC, (int(torch.randint(0, 4, (1,), generator=g)),), generator=g))
    rp, rowend, col, eff = _csr_of(rows, True)
    return types.SimpleNamespace(rp=rp, rowend=rowend, col=col, rows=eff, window=True, ei=_edges(eff, N_SRC))


def _grid(g, *shape):
    return torch.randint(-128, 129, shape, generator=g).double() / 64


def _free(g, *shape, half=False):
    """random values that float32 (float16) holds exactly, as float64"""
    t = torch.randn(*shape, generator=g, dtype=torch.float32)
    return (t.half() if half else t).double()


# ---- references (dtype follows the inputs) --------------------------------------------------------------------------
def reduce_ref(x, gr, aggr):
    """[reduce | self] of the rows < N_LIVE over the local source matrix x [N_SRC, d]; an empty row reduces to 0"""
    d = x.shape[1]
    if aggr == "max":
        red = torch.stack([x[r].amax(0) if r.numel() else x.new_zeros(d) for r in gr.rows[:N_LIVE]])
    else:
        red = x.new_zeros(N_LIVE, d).index_add(0, gr.ei[1], x[gr.ei[0]])
        if aggr == "mean":
            red = red / gr.deg[:N_LIVE].clamp(min=1).to(x.dtype)[:, None]
    return torch.cat([red, x[:N_LIVE]], 1)


def reduce_backward_ref(x, dout, gr, aggr):
    """gradient of sum(dout * reduce_ref(x)) w.r.t. x (amax shares the gradient evenly among ties)"""
    x = x.clone().requires_grad_(True)
    return torch.autograd.grad((reduce_ref(x, gr, aggr) * dout).sum(), x)[0]


def wgrad_ref(dy, a, relu_y, m, rc=None):
    """(dW, db) = ((dy * [y > 0])^T a, column sums of the masked dy) over the first m rows; rc: as per-chunk products of
    rc rows added in chunk order"""
    dym = dy[:m] if relu_y is None else torch.where(relu_y[:m] > 0, dy[:m], torch.zeros_like(dy[:m]))
    if rc is None:
        return dym.T @ a[:m], dym.sum(0)
    dw, db = dy.new_zeros(dy.shape[1], a.shape[1]), dy.new_zeros(dy.shape[1])
    for r0 in range(0, m, rc):
        r1 = min(m, r0 + rc)
        dw, db = dw + dym[r0:r1].T @ a[r0:r1], db + dym[r0:r1].sum(0)
    return dw, db


def loss_ref(scores, temperature, prob, qid, cid):
    """-> (loss, row_lse, logits, excluded): s_ij = scores_ij / T - log(max(p_j, 1e-10)); column j != i is excluded when
    j < Q and qid[j] == qid[i], or when cid[j] == cid[i]; loss = sum_i (logsumexp over the kept j of s_ij) - s_ii"""
    q, c = scores.shape
    s = scores / temperature if temperature else scores
    if prob is not None:
        s = s - torch.log(prob.to(s.dtype).clamp(min=torch.tensor(1e-10, dtype=torch.float32).to(s.dtype)))
    ex = torch.zeros(q, c, dtype=torch.bool)
    if qid is not None:
        ex[:, :q] |= qid[None, :] == qid[:, None]
    if cid is not None:
        ex |= cid[None, :] == cid[:q, None]
    ex[torch.arange(q), torch.arange(q)] = False
    lse = torch.logsumexp(s.masked_fill(ex, float("-inf")), 1)
    return (lse - s.diagonal()).sum(), lse, s, ex


def check(label, name, got, want, e32, grad=False):
    got, want = got.detach().double().cpu(), want.detach().double()
    assert got.shape == want.shape, (label, name, got.shape, want.shape)
    rtol = 1e-4 if grad else 1e-5
    atol = 1e-4 * float(want.abs().max()) if grad and want.numel() else 1e-5
    tol = torch.clamp(atol + rtol * want.abs(), min=4.0 * e32)
    err = (got - want).abs()
    print(f"{label} {name}: err={float(err.max()) if err.numel() else 0.0:.3e} fp32={e32:.3e}")
    assert bool(torch.isfinite(got).all()), f"{label} {name}: non-finite values"
    bad = err > tol
    assert not bool(bad.any()), (f"{label} {name}: {int(bad.sum())} of {bad.numel()} beyond the bound, max err "
                                 f"{float(err.max()):.3e} (float32 reference {e32:.3e})")
    return tol


def _err(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


# ---- which code a shape takes (restated from the launch code; the CPU test asserts that every one is run) ----------
def gather_instantiation(d):
    """launch_gather: (lanes per source row, float4 vectors per lane), or "generic" """
    if d % 4 or d // 4 > 512:
        return "generic"
    for vecs, inst in ((8, (8, 1)), (16, (16, 1)), (32, (32, 1)), (64, (64, 1)), (128, (64, 2)), (256, (64, 4))):
        if d // 4 <= vecs:
            return inst
    return (64, 8)


def backward_wpr(rows_cap):
    """gigl_gather_reduce_backward: waves per destination row"""
    return 1 if rows_cap >= 32768 else 2 if rows_cap >= 8192 else 4 if rows_cap >= 2048 else 8


def backward_path(d):
    return "registers" if d % 4 == 0 and d <= 1024 else "scalar"


def gmt_lanes(d):
    """gigl_gather_mean_backward_lists: lanes per source row of gmt_gather_kernel"""
    return 64 if d >= 256 else 32 if d >= 128 else 16 if d >= 64 else 8


def wgrad_rows_per_chunk(m_cap, n, k):
    """agg.hip's wgrad_rows_per_chunk (not exported): 256 rows, halved down to 32 while m_cap gives fewer than 32 chunks,
    then doubled while chunks x (64 x 64 tiles of dW) exceeds 4096 workgroups"""
    rc = 256
    while rc > 32 and m_cap // rc < 32:
        rc >>= 1
    tiles = ((n + 63) // 64) * ((k + 63) // 64)
    while rc < 8192 and ((m_cap + rc - 1) // rc) * tiles > 4096:
        rc <<= 1
    return rc


# ---- device side ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _i32(t):
    return t.to(torch.int32).cuda()


def _csr(gr):
    """packed: rowptr with its n + 1 entries and rowend None (the wrappers then pass rowptr[1:]); windowed: n + n"""
    if not gr.window:
        return types.SimpleNamespace(rowptr=_i32(gr.rp), rowend=None, col=_i32(gr.col))
    return types.SimpleNamespace(rowptr=_i32(gr.rp[:-1]), rowend=_i32(gr.rowend), col=_i32(gr.col))


def _count(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def _table(x, half, ids, g):
    """the source as the kernel gets it: x's rows and a NaN row that OOB names — directly, or as rows of a wider table
    through gather_ids"""
    dt = torch.float16 if half else torch.float32
    nan = torch.full((1, x.shape[1]), float("nan"), dtype=torch.float64)
    if not ids:
        return torch.cat([x, nan]).to(dt).cuda(), None
    n_tab = 300
    gid = torch.randperm(n_tab, generator=g)[:N_SRC]
    table = nan.repeat(n_tab + 1, 1)
    table[gid] = x
    return table.to(dt).cuda(), _i32(torch.cat([gid, torch.tensor([n_tab])]))


# ---- 1. weight gradient ---------------------------------------------------------------------------------------------
WGRAD_SHAPES = [(1000, 1000, 64, 64), (1000, 937, 47, 30), (1000, 1, 5, 3), (1000, 0, 16, 8), (8192, 8000, 130, 200),
                (4100, 4097, 256, 68), (70000, 69000, 256, 256)]  # (m_cap, m, N, K)
WGRAD_SELECT = [(1000, 937, 47, 30), (8192, 8000, 130, 200)]
WGRAD_FLOOR = 4e-7


@functools.lru_cache(2)
def wgrad_inputs(m_cap, m, n, k):
    g = torch.Generator().manual_seed(m_cap + 3 * m + 5 * n + 7 * k)
    dy = torch.randn(m_cap, n, generator=g) * torch.exp(torch.randn(m_cap, 1, generator=g) * 2)  # rows of very different scale
    dy[:, 0] *= 1e-4
    a = torch.randn(m_cap, k, generator=g)
    y = torch.randint(-128, 129, (m_cap, n), generator=g).float() / 64  # exact 0.0 among them
    y[torch.rand(m_cap, n, generator=g) < 0.05] = -0.0
    for t in (dy, a, y):
        t[m:] = float("nan")
    return dy, a, y


@functools.lru_cache(None)
def wgrad_case(m_cap, m, n, k, relu):
    """-> (dW, db, their scales, the float32 reference's scaled errors) of the shape"""
    dy, a, y = wgrad_inputs(m_cap, m, n, k)
    y = y if relu else None
    y64 = y.double() if relu else None
    dw, db = wgrad_ref(dy.double(), a.double(), y64, m)
    dym = dy[:m].double().abs() if not relu else torch.where(y64[:m] > 0, dy[:m].double().abs(), torch.zeros(()).double())
    sw, sb = dym.T @ a[:m].double().abs(), dym.sum(0)
    ew = eb = 0.0
    for rc in (None, wgrad_rows_per_chunk(m_cap, n, k)):
        lw, lb = wgrad_ref(dy, a, y, m, rc)
        ew, eb = max(ew, _scaled(lw, dw, sw)), max(eb, _scaled(lb, db, sb))
    return dw, db, sw, sb, ew, eb


def _scaled(got, want, scale):
    got = got.double().cpu()
    assert not bool(got[scale == 0].any()), "a gradient entry without any contribution is not 0"
    live = scale > 0
    return float(((got - want).abs()[live] / scale[live]).max()) if bool(live.any()) else 0.0


@gpu
@pytest.mark.parametrize("want_bias", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("m_cap,m,n,k", WGRAD_SHAPES)
def test_weight_grad(eng, m_cap, m, n, k, relu, want_bias):
    dy, a, y = wgrad_inputs(m_cap, m, n, k)
    dw, db, sw, sb, ew, eb = wgrad_case(m_cap, m, n, k, relu)
    got_w, got_b = eng.linear_weight_grad(dy.cuda(), a.cuda(), _count(m), y.cuda() if relu else None, want_bias)
    label = f"wgrad {m_cap}/{m}x{n}x{k} rc={wgrad_rows_per_chunk(m_cap, n, k)} relu={relu}"
    assert tuple(got_w.shape) == (n, k) and bool(torch.isfinite(got_w).all())
    err = _scaled(got_w, dw, sw)
    print(f"{label} dW: err={err:.3e} fp32={ew:.3e}")
    assert err <= max(WGRAD_FLOOR, 4.0 * ew), (label, err, ew)
    if not want_bias:
        assert got_b is None
        return
    assert tuple(got_b.shape) == (n,) and bool(torch.isfinite(got_b).all())
    err = _scaled(got_b, db, sb)
    print(f"{label} db: err={err:.3e} fp32={eb:.3e}")
    assert err <= max(WGRAD_FLOOR, 4.0 * eb), (label, err, eb)
    if m == 0:
        assert not bool(got_w.any()) and not bool(got_b.any())


def selection_rows(m, n, rc):
    """rho(n): column n's single row — chunk n % chunks, and inside it a position that runs over 0..31 of a 32-row block
    (and over the chunk's blocks), folded into the rows the last chunk really has"""
    chunks = (m + rc - 1) // rc
    rho = []
    for c in range(n):
        ch = c % chunks
        p = (c + 5) % 32 + 32 * ((c // 32) % (rc // 32))
        rho.append(ch * rc + p % min(rc, m - ch * rc))
    rho = torch.tensor(rho)
    assert set((rho // rc).tolist()) == set(range(chunks)) and set((rho % 32).tolist()) == set(range(32))
    assert int(rho.max()) < m
    return rho


@gpu
@pytest.mark.parametrize("m_cap,m,n,k", WGRAD_SELECT)
def test_weight_grad_selects_rows_exactly(eng, m_cap, m, n, k):
    """dy = one 1.0 per column, at row rho(n): dW[n] is row rho(n) of a, bit for bit (the three planes of a sum exactly,
    smallest first) — a transposed or mis-swizzled tile, or a row of the wrong chunk, cannot pass"""
    _, a, _ = wgrad_inputs(m_cap, m, n, k)
    rho = selection_rows(m, n, wgrad_rows_per_chunk(m_cap, n, k))
    dy = torch.zeros(m_cap, n)
    dy[rho, torch.arange(n)] = 1.0
    dy[m:] = float("nan")
    got_w, got_b = eng.linear_weight_grad(dy.cuda(), a.cuda(), _count(m), None, True)
    assert torch.equal(got_w.cpu(), a[rho])
    assert torch.equal(got_b.cpu(), torch.ones(n))


# ---- 2. forward reduce ----------------------------------------------------------------------------------------------
GATHER_WIDTHS = [4, 32, 36, 64, 68, 128, 256, 260, 512, 516, 1024, 1028, 2048, 2, 30, 2052]
GATHER_SUBSET = [4, 36, 128, 256, 260, 1024, 2048, 30, 2052]  # one width per instantiation, and the generic kernel
GATHER_CASES = [("mean", False, d, w, i) for d in GATHER_WIDTHS for w in (False, True) for i in (False, True)] + \
               [(aggr, half, d, w, w) for aggr, half in (("mean", True), ("sum", False), ("sum", True), ("max", False),
                                                         ("max", True))
                for d in GATHER_SUBSET for w in (False, True)]  # (aggr, fp16, d, windowed, through gather_ids)


def reduce_source(d, half, aggr, seed=0):
    """the local source matrix [N_SRC, d]: for max on the grid, column 1 strictly negative (an identity of 0 instead of
    -inf would show) and the duplicated source of DUP_ROW at the grid's top in column 0 (a tie of the row's maximum)"""
    g = torch.Generator().manual_seed(100 * d + 10 * len(aggr) + half + seed)
    if aggr != "max":
        return _free(g, N_SRC, d, half=half), g
    x = _grid(g, N_SRC, d)
    x[:, 1] = -x[:, 1].abs() - 1.0 / 64
    x[_base_rows()[DUP_ROW][1], 0] = 2.0
    return x, g


@gpu
@pytest.mark.parametrize("aggr,half,d,window,ids", GATHER_CASES)
def test_gather_reduce(eng, aggr, half, d, window, ids):
    gr = sage_graph(window)
    x, g = reduce_source(d, half, aggr)
    want = reduce_ref(x, gr, aggr)
    e32 = _err(reduce_ref(x.float(), gr, aggr), want)
    table, gid = _table(x, half, ids, g)
    u = _csr(gr)
    out = torch.full((N_ROWS, 2 * d), SENTINEL, dtype=torch.float32, device="cuda")
    eng.gather_mean(table, d, gid, u.rowptr, u.rowend, u.col, _count(N_LIVE), N_ROWS, out=out, aggr=aggr)
    got = out.cpu()
    label = f"gather {aggr} {'fp16' if half else 'fp32'} d={d} {gather_instantiation(d)} window={window} ids={ids}"
    check(label, "reduce", got[:N_LIVE, :d], want[:, :d], e32)
    assert torch.equal(got[:N_LIVE, d:].double(), want[:, d:]), f"{label}: the self half is the source row itself"
    assert bool((got[N_LIVE:] == SENTINEL).all()), f"{label}: rows past *n_rows_dev were written"
    if aggr == "max":
        assert not bool(got[:N_LIVE, :d][gr.deg[:N_LIVE] == 0].any()), f"{label}: an empty row reduces to 0"
        assert bool((got[:N_LIVE, 1][gr.deg[:N_LIVE] > 0] < 0).all())


# ---- 3. backward reduce ---------------------------------------------------------------------------------------------
BACKWARD_WIDTHS = [4, 20, 30, 256, 1024, 1028]
ROWS_CAPS = [N_ROWS, 2048, 8192, 32768]  # only the host-side waves-per-row and the grid change
GMT_WIDTHS = [4, 8, 60, 64, 124, 128, 252, 256, 300]


@functools.lru_cache(None)
def backward_case(aggr, d, window):
    gr = sage_graph(window)
    x, g = reduce_source(d, False, aggr, seed=1)
    dout = _free(g, N_ROWS, 2 * d)
    want = reduce_backward_ref(x, dout[:N_LIVE], gr, aggr)
    e32 = _err(reduce_backward_ref(x.float(), dout[:N_LIVE].float(), gr, aggr), want)
    dout[N_LIVE:] = float("nan")
    return gr, x, dout, want, e32


@gpu
@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("d", BACKWARD_WIDTHS)
@pytest.mark.parametrize("aggr", ["mean", "sum", "max"])
def test_gather_reduce_backward(eng, aggr, d, window):
    gr, x, dout, want, e32 = backward_case(aggr, d, window)
    u, do, nd = _csr(gr), dout.float().cuda(), _count(N_LIVE)
    src = _table(x, False, False, None)[0] if aggr == "max" else None
    for rows_cap in ROWS_CAPS:
        dsrc = torch.zeros((N_SRC + 1, d), dtype=torch.float32, device="cuda")
        eng.gather_mean_backward(do, d, u.rowptr, u.rowend, u.col, nd, rows_cap, dsrc, aggr=aggr, src=src)
        got = dsrc.cpu()
        label = f"scatter bwd {aggr} d={d} {backward_path(d)} window={window} rows_cap={rows_cap} wpr={backward_wpr(rows_cap)}"
        check(label, "dsrc", got[:N_SRC], want, e32, grad=True)
        assert not bool(got[N_SRC:].any()), f"{label}: a skipped col entry was followed"
        assert not bool(got[N_READ:N_SRC].any()), f"{label}: the sources nobody reads have no gradient"


@gpu
@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("d", GMT_WIDTHS)
@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_gather_backward_transposed(eng, aggr, d, window):
    gr, x, dout, want, e32 = backward_case(aggr, d, window)
    u, do, nd = _csr(gr), dout.float().cuda(), _count(N_LIVE)
    dsrc = torch.full((N_SRC + 4, d), SENTINEL, dtype=torch.float32, device="cuda")
    eng.gather_mean_backward_transposed(do, d, u.rowptr, u.rowend, u.col, nd, N_ROWS, _count(N_SRC), dsrc, aggr=aggr)
    scat = torch.zeros((N_SRC + 4, d), dtype=torch.float32, device="cuda")
    eng.gather_mean_backward(do, d, u.rowptr, u.rowend, u.col, nd, N_ROWS, scat, aggr=aggr)
    got, scat = dsrc.cpu(), scat.cpu()
    label = f"transposed bwd {aggr} d={d} lanes={gmt_lanes(d)} window={window}"
    tol = check(label, "dsrc", got[:N_SRC], want, e32, grad=True)
    assert bool((got[N_SRC:] == SENTINEL).all()), f"{label}: rows past *n_src_dev were written"
    # both kernels are within `tol` of the float64 result, so within 2 tol of each other
    assert bool(((got[:N_SRC] - scat[:N_SRC]).abs().double() <= 2 * tol).all()), f"{label}: differs from the scatter kernel"


# ---- 4. GCN ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("d", [3, 64, 200])
def test_gcn_aggregate(eng, d, half, ids, bias):
    """D^-1/2 (A + I) D^-1/2 h (+ bias, relu) of the rows < N_LIVE; every node's degree counts its listed in-edges
    except self loops, the rows >= N_LIVE included"""
    gr = gcn_graph()
    g = torch.Generator().manual_seed(7000 + 10 * d + half)
    x = _free(g, N_SRC, d, half=half)
    b = _free(g, d) if bias else None

    def ref(dt):
        out = gnn_ref.gcn_conv(x.to(dt), gr.ei, torch.eye(d, dtype=dt), b.to(dt) if bias else None)
        return (torch.relu(out) if bias else out)[:N_LIVE]

    want = ref(torch.float64)
    e32 = _err(ref(torch.float32), want)
    table, gid = _table(x, half, ids, g)
    u = types.SimpleNamespace(nodes=torch.empty(N_SRC, dtype=torch.int32, device="cuda"), rowptr=_i32(gr.rp[:-1]),
                              rowend=_i32(gr.rowend), col=_i32(gr.col),
                              meta=torch.tensor([N_SRC, gr.col.numel()], dtype=torch.int32, device="cuda"))
    out = torch.full((N_SRC, d), SENTINEL, dtype=torch.float32, device="cuda")
    eng.gcn_aggregate(table, d, gid, u, _count(N_LIVE), b.float().cuda() if bias else None, 1 if bias else 0, out=out)
    got = out.cpu()
    label = f"gcn d={d} {'fp16' if half else 'fp32'} ids={ids} bias+relu={bias}"
    check(label, "out", got[:N_LIVE], want, e32)
    assert bool((got[N_LIVE:] == SENTINEL).all()), f"{label}: rows past *n_rows_dev were written"


# ---- 5. retrieval loss ----------------------------------------------------------------------------------------------
LOSS_SHAPES = [(1, 1), (3, 255), (5, 256), (5, 257), (64, 513), (300, 300)]
LOSS_VARIANTS = [(t, p, m, "unit") for t in (None, 0.07) for p in (False, True) for m in ("query", "cand", "both")] + \
                [(None, False, "both", "same"), (0.07, True, "both", "same"),  # only the diagonal survives
                 (None, False, "both", "large"), (0.07, True, "query", "large")]  # scores up to +-80


def loss_inputs(q, c, prob, mask, kind):
    g = torch.Generator().manual_seed(1000 * q + c + len(mask) + len(kind))
    scores = _free(g, q, c)
    if kind == "large":
        scores = (scores * (80.0 / float(scores.abs().max()))).float().double()
    p = None
    if prob:
        p = torch.rand(c, generator=g, dtype=torch.float32) * 0.99 + 0.01
        p[0], p[c // 2] = 0.0, 1e-20  # both below the 1e-10 clamp
        p = p.double()
    if kind == "same":
        qid, cid = torch.full((q,), 5), torch.full((c,), 9)
    else:
        qid, cid = torch.randint(0, q // 2 + 1, (q,), generator=g), torch.randint(0, c // 2 + 1, (c,), generator=g)
    return scores, p, (qid if mask != "cand" else None), (cid if mask != "query" else None)


@gpu
@pytest.mark.parametrize("temperature,prob,mask,kind", LOSS_VARIANTS)
@pytest.mark.parametrize("q,c", LOSS_SHAPES)
def test_retrieval_loss(eng, q, c, temperature, prob, mask, kind):
    scores, p, qid, cid = loss_inputs(q, c, prob, mask, kind)

    def ref(dt, grad_loss):
        s = scores.to(dt).clone().requires_grad_(True)
        loss, lse, logits, ex = loss_ref(s, temperature, p.to(dt) if prob else None, qid, cid)
        ds = torch.autograd.grad(loss * grad_loss, s)[0]
        return {"loss": loss.detach().reshape(1), "row_lse": lse.detach(), "logits": logits.detach(), "dscores": ds}, ex

    buf = torch.full((q, c + 3), float("nan"), dtype=torch.float32)  # ld = c + 3: the padding is never read
    buf[:, :c] = scores.float()
    view = buf.cuda()[:, :c]
    dev = lambda t, dt: None if t is None else t.to(dt).cuda()
    pd, qd, cd = dev(p, torch.float32), dev(qid, torch.int64), dev(cid, torch.int64)
    loss, lse, masked = eng.retrieval_loss(view, temperature, pd, qd, cd, want_masked=True)
    label = f"loss {q}x{c} T={temperature} prob={prob} mask={mask} {kind}"
    want, ex = ref(torch.float64, 1.0)
    lo, _ = ref(torch.float32, 1.0)
    e32 = {k: _err(lo[k], want[k]) for k in want}
    check(label, "loss", loss.reshape(1), want["loss"], e32["loss"])
    check(label, "row_lse", lse, want["row_lse"], e32["row_lse"])
    masked = masked.cpu()
    assert torch.equal(masked == -FLT_MAX, ex), f"{label}: the excluded logits are exactly -FLT_MAX, and only they"
    if temperature is None and not prob:
        assert torch.equal(masked[~ex], scores.float()[~ex]), f"{label}: a kept logit without T and p is the score"
    check(label, "logits", masked.masked_fill(ex, 0.0), want["logits"].masked_fill(ex, 0.0), e32["logits"])
    for grad_loss in (None, 0.5):
        gl = torch.tensor(grad_loss, dtype=torch.float32, device="cuda") if grad_loss else None
        ds = eng.retrieval_loss_backward(view, temperature, pd, qd, cd, lse, gl).cpu()
        want, _ = ref(torch.float64, grad_loss or 1.0)
        lo, _ = ref(torch.float32, grad_loss or 1.0)
        check(f"{label} g={grad_loss}", "dscores", ds, want["dscores"], _err(lo["dscores"], want["dscores"]), grad=True)
        assert not bool(ds[ex].any()), f"{label}: excluded columns have no gradient"
        if kind == "same":
            assert not bool(ds.any())
    if kind == "same":
        assert float(loss) == 0.0 and bool(ex.sum(1).eq(c - 1).all())


# ---- CPU: the formulas above against gnn_ref and torch autograd (float64), the graph, the coverage -----------------
def test_references_graph_and_coverage():
    rows, packed, win = _base_rows(), sage_graph(False), sage_graph(True)
    # the graph delivers what the cases rely on
    assert len(rows) == N_ROWS and packed.deg[:len(DEGREES)].tolist() == DEGREES
    assert all(r.numel() <= 6 for r in rows[len(DEGREES):]) and N_ROWS < N_SRC
    assert int((packed.rp[1:] != packed.rowend).sum()) == 0
    assert int((rows[SELF_ROW] == SELF_ROW).sum()) == 1
    dup = rows[DUP_ROW]
    assert dup.numel() - dup.unique().numel() == 1 and int((dup == dup[1]).sum()) == 2
    assert sum(int((r == HOT).any()) for r in rows[:N_LIVE]) >= 100
    assert set(range(N_READ, N_SRC)).isdisjoint(packed.col.tolist()) and int(packed.col.max()) < N_READ
    short = win.rp[1:] - win.rowend
    assert int((short > 0).sum()) == N_ROWS // 3 and set(short[short > 0].tolist()) == {1, 2}
    assert short[SELF_ROW] == 0 and short[DUP_ROW] == 0 and short[len(DEGREES) - 1] == 0
    skipped = torch.cat([win.col[int(win.rowend[i]):int(win.rp[i + 1])] for i in range(N_ROWS)])
    assert skipped.numel() == int(short.sum()) and bool((skipped == OOB).all())
    assert int((win.col == OOB).sum()) == skipped.numel()
    assert torch.equal(torch.cat(win.rows), win.col[win.col != OOB])
    gg = gcn_graph()
    assert len(gg.rows) == N_SRC and any(r.numel() for r in gg.rows[N_ROWS:])
    assert int((gg.ei[0] == gg.ei[1]).sum()) >= 1 and int(gg.ei[0].max()) < N_SRC
    # max: real ties, the duplicated source among them; a strictly negative column
    x, _ = reduce_source(4, False, "max")
    ties = [(x[r] == x[r].amax(0)).sum(0) for r in packed.rows[:N_LIVE] if r.numel()]
    assert int((torch.stack(ties) > 1).sum()) >= 10
    assert int((x[dup] == x[dup].amax(0)).sum(0)[0]) >= 2 and bool((x[:, 1] < 0).all())

    # reduce: mean against SAGEConv with identity weights; sum / max and their gradients against other torch formulas
    g = torch.Generator().manual_seed(3)
    d = 6
    eye = torch.eye(d, dtype=torch.float64)
    for gr in (packed, win):
        x, w = _grid(g, N_SRC, d), _free(g, N_LIVE, 2 * d)
        conv = gnn_ref.sage_conv(x, gr.ei, eye, None, None)[:N_LIVE]
        assert _err(reduce_ref(x, gr, "mean")[:, :d], conv) <= 1e-12
        idx = gr.ei[1][:, None].expand(-1, d)

        def other(x, aggr):
            if aggr == "max":
                red = torch.full((N_LIVE, d), float("-inf"), dtype=x.dtype).scatter_reduce(0, idx, x[gr.ei[0]], "amax")
                red = torch.where(torch.isinf(red), torch.zeros_like(red), red)
            else:
                red = torch.stack([x[r].sum(0) / (max(r.numel(), 1) if aggr == "mean" else 1) for r in gr.rows[:N_LIVE]])
            return torch.cat([red, x[:N_LIVE]], 1)

        for aggr in ("mean", "sum", "max"):
            xo = x.clone().requires_grad_(True)
            fwd = other(xo, aggr)
            assert _err(reduce_ref(x, gr, aggr), fwd.detach()) <= 1e-12
            assert _err(reduce_backward_ref(x, w, gr, aggr), torch.autograd.grad((fwd * w).sum(), xo)[0]) <= 1e-12

    # GCN: the edge list handed to gcn_conv against the dense D^-1/2 (A + I) D^-1/2 of the rows as the kernel reads them
    adj = torch.zeros(N_SRC, N_SRC, dtype=torch.float64)
    for i, r in enumerate(gg.rows):
        for j in r.tolist():
            adj[i, j] += j != i
    adj += torch.eye(N_SRC, dtype=torch.float64)
    dinv = adj.sum(1).pow(-0.5)
    x, b = _free(g, N_SRC, d), _free(g, d)
    assert _err(dinv[:, None] * (adj @ (dinv[:, None] * x)) + b, gnn_ref.gcn_conv(x, gg.ei, eye, b)) <= 1e-12

    # retrieval loss against the row-by-row restatement (no candidate probabilities there)
    for q, c in ((1, 1), (5, 9), (12, 12)):
        scores, _, qid, cid = loss_inputs(q, c, False, "both", "unit")
        rows_ = gnn_ref.retrieval_loss_rows(scores, qid.tolist(), cid.tolist(), temperature=0.07)
        assert _err(loss_ref(scores, 0.07, None, qid, cid)[0], rows_) <= 1e-12 * max(1.0, float(rows_.abs()))
        rows_ = gnn_ref.retrieval_loss_rows(scores, qid.tolist(), cid.tolist(), temperature=1.0, remove_accidental_hits=False)
        assert _err(loss_ref(scores, None, None, qid, None)[0], rows_) <= 1e-12 * max(1.0, float(rows_.abs()))
    _, lse, s, ex = loss_ref(torch.zeros(2, 3, dtype=torch.float64), None, torch.tensor([0.0, 1e-20, 1.0]).double(), None, None)
    assert _err(s[0, :2], torch.full((2,), 23.025850929940457)) <= 1e-6 and float(s[0, 2]) == 0.0 and not bool(ex.any())

    # weight gradient against autograd through relu(a W^T + b), in one product and in chunks
    m, n, k = 37, 5, 7
    a, wt, bias, w = _free(g, m + 3, k), _free(g, n, k).requires_grad_(True), _free(g, n).requires_grad_(True), _free(g, m + 3, n)
    y = (a[:m] @ wt.T + bias).relu()
    gw, gb = torch.autograd.grad((y * w[:m]).sum(), [wt, bias])
    for rc in (None, 8):
        dw, db = wgrad_ref(w, a, torch.cat([y.detach(), torch.ones(3, n).double()]), m, rc)
        assert _err(dw, gw) <= 1e-12 and _err(db, gb) <= 1e-12
    dw, db = wgrad_ref(w, a, None, m)
    assert _err(dw, w[:m].T @ a[:m]) <= 1e-12 and _err(db, w[:m].sum(0)) <= 1e-12

    # the parametrisation runs every instantiation
    every = {(8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 8), "generic"}
    for aggr in ("mean", "sum", "max"):
        for half in (False, True):
            for ids in (False, True):
                seen = {gather_instantiation(c[2]) for c in GATHER_CASES if c[:2] == (aggr, half) and c[4] == ids}
                assert seen == every, (aggr, half, ids, every - seen)
    assert {gather_instantiation(d) for d in GATHER_SUBSET} == every
    assert [gather_instantiation(d) for d in (32, 36, 64, 68, 128, 132, 256, 260, 512, 516, 1024, 1028, 2048, 2052)] == \
        [(8, 1), (16, 1), (16, 1), (32, 1), (32, 1), (64, 1), (64, 1), (64, 2), (64, 2), (64, 4), (64, 4), (64, 8), (64, 8),
         "generic"]
    assert {gmt_lanes(d) for d in GMT_WIDTHS} == {8, 16, 32, 64} and all(d % 4 == 0 for d in GMT_WIDTHS)
    assert [gmt_lanes(d) for d in (60, 64, 124, 128, 252, 256)] == [8, 16, 16, 32, 32, 64]
    assert {backward_wpr(r) for r in ROWS_CAPS} == {8, 4, 2, 1}
    assert {backward_path(d) for d in BACKWARD_WIDTHS} == {"registers", "scalar"}
    assert backward_path(1024) == "registers" and backward_path(1028) == "scalar"
    rcs = {s: wgrad_rows_per_chunk(s[0], s[2], s[3]) for s in WGRAD_SHAPES}
    assert {32, 256, 512} <= set(rcs.values()) and rcs[(70000, 69000, 256, 256)] == 512 and rcs[(8192, 8000, 130, 200)] == 256
    assert rcs[(1000, 937, 47, 30)] == 32 and (4097 - 1) % rcs[(4100, 4097, 256, 68)] == 0
    for s in WGRAD_SELECT:
        assert s in WGRAD_SHAPES
        selection_rows(s[1], s[2], rcs[s])
