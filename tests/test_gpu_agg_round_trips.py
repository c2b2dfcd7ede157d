"""The aggregation kernels of csrc/agg.hip where a wave owns SEVERAL rows and where the fused last layer's rows have every
length class: gather_mean_kernel's row loop is a software pipeline (row i's source rows, row i + W's first `col` chunk
and row i + 2 W's bounds in flight together, W = waves of the grid), sage_fused_out_kernel reads a root's first 64 `col`
entries in one load and issues up to 32 edges' p rows before the first add.  The other gather tests have 195 rows — at
most one per wave, so the pipeline's steady state never runs there.

1. HipEngine.gather_mean, rows_cap = 70 000.  The grid is min(ceil(rows_cap / 4), 4096) blocks of four waves = 16 384 waves
   and wave w takes rows w, w + 16 384, ...: *n_rows_dev = 0, 1, 5, 16 384, 16 385, 49 153, 69 997 give waves that own 0, 1,
   2, 3, 4 and 5 rows, and a last row (49 152, 69 996) on a wave that has others.  In-degree of row i:
   DEG[(i + i // 16384) % 16] over 0, 0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 130 — a wave's consecutive rows differ,
   empty rows sit between long ones, 65 and 130 take a second and third 64-entry chunk.  Sources: the first 4 096 local
   rows.  Every third row ends 1 or 2 entries early (windowed rowend) and the skipped `col` entries name a row of NaN.
   gather_ids present (a 4 097-row table behind 70 001 local ids) and absent (the local matrix is the table); mean, sum,
   max; d = 8 (LPR 8) and 260 (LPR 64, VPL 2) over fp32, d = 8 over fp16, d = 100 (LPR 32) once.  Rows >= *n_rows_dev keep a
   sentinel; the self half is the source row bit for bit.
2. The GraphSAGE plan's tiled `no_self` first layer and its *n_local_dev switch (the roots' rows go through gather_ids,
   the rows behind them hold global ids) with 4 to 5 rows per wave: one fused-path plan — 2 layers, hidden 256, out 47,
   fp32 table d = 100, 20 000 nodes, B = 512, fan-outs [25, 10], groups = 8 — asserted to give more than 65 536 layer-0
   rows.
3. sage_fused_out_kernel through the same kind of plan at fan-outs [3, 2], [25, 10] and [70, 2] on a graph with isolated
   roots, roots of in-degree 1 .. 5, a root adjacent to itself and hubs of 24, 25, 80 and 200 in-edges: root rows of 0,
   1 .. 5, 24, 25 and 70 (a second chunk) entries, asserted from the plan's own union graph; output widths 1, 5, 47, 48,
   mean and sum, bias on and off; a batch with a root slot that holds no node (id 0xFFFFFFFF >= N: a zero row); a call that overflows its workspace (NaN rows).

References and bounds.  1: a float64 segment reduce over the effective edge list, written here; the bound is
tests/test_gpu_sage_kernels.py::check (rtol = atol = 1e-5, floored at 4 x the error of the same formula in float32).
2 and 3: tests/sage_plan_cases.py's float64 forward over the plan's OWN union graph with its per-element bounds (as
tests/test_gpu_sage_plan_layers.py), and `check` on top with the float32 forward's error as the floor.  relu is
1-Lipschitz, so the bounds hold whatever side of zero a hidden pre-activation falls on.  Nothing comes from a kernel's
output.

Time on an MI355X: 29 GPU tests, 19 s in all — the 20 000-node plan 4.8 s (its float64 forwards), the d = 260 gathers 2.7 ..
3.0 s each (eight calls and comparisons of up to 70 000 x 260), d = 100 1.2 s, everything else under 0.1 s.
"""
import functools

import numpy as np
import pytest
import torch

import sage_plan_cases as sc
import test_gpu_sage_kernels as sk

gpu = pytest.mark.gpu

ROWS_CAP, N_SRC = 70_000, 4096
WAVES = 16_384  # min(ceil(ROWS_CAP / 4), 256 * 16) blocks of four waves (launch_gather in csrc/agg.hip)
LIVE = [0, 1, 5, 16_384, 16_385, 49_153, 69_997]
DEG = [0, 0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 130]
OOB = ROWS_CAP  # the local id the skipped entries of a windowed row name: a row of NaN behind the last row


# ---- 1. gather_mean with several rows per wave ----------------------------------------------------------------------
@functools.lru_cache(None)
def big_graph():
    """-> rowptr [n], rowend [n], col, and the effective (windowed) edge list: sources, row lengths"""
    i = np.arange(ROWS_CAP)
    deg = np.array(DEG)[(i + i // WAVES) % len(DEG)]
    rp = np.concatenate([[0], np.cumsum(deg)])
    col = np.random.default_rng(41).integers(0, N_SRC, rp[-1])
    rowend = rp[1:].copy()
    w = np.arange(1, ROWS_CAP, 3)
    rowend[w] -= np.minimum(deg[w], 1 + (w // 3) % 2)
    keep = np.arange(rp[-1]) < np.repeat(rowend, deg)
    col[~keep] = OOB
    return rp[:-1], rowend, col, col[keep], rowend - rp[:-1]


def segment_reduce(x, src, lens, aggr):
    """reduce_{e in row i} x[src[e]] in x's dtype, 0 for an empty row; mean = sum / length"""
    out = np.zeros((lens.size, x.shape[1]), x.dtype)
    start = np.concatenate([[0], np.cumsum(lens)])
    op = np.maximum if aggr == "max" else np.add
    for lo in range(0, lens.size, 4096):
        hi = min(lo + 4096, lens.size)
        rows = lo + np.nonzero(lens[lo:hi])[0]
        if rows.size:
            out[rows] = op.reduceat(x[src[start[lo]:start[hi]]], start[rows] - start[lo], axis=0)
    if aggr == "mean":
        out /= np.maximum(lens, 1).astype(x.dtype)[:, None]
    return out


@functools.lru_cache(None)
def big_inputs(d, half, for_max):
    """the 4 097-row table (its last row NaN), the ids of the 70 001 local rows in it, the local matrix (float64)"""
    g = torch.Generator().manual_seed(1000 * d + 10 * half + for_max)
    t = torch.randn(N_SRC, d, generator=g, dtype=torch.float32)
    if for_max:
        t[:, 1] = -t[:, 1].abs() - 1.0 / 64  # (an identity of 0 instead of -inf would show)
    t = torch.cat([t.half().float() if half else t, torch.full((1, d), float("nan"))])
    gid = torch.cat([torch.randperm(N_SRC, generator=g), torch.randint(0, N_SRC, (ROWS_CAP - N_SRC,), generator=g),
                     torch.tensor([N_SRC])])
    return t, gid, t[gid].double().numpy()


@functools.lru_cache(None)
def big_reference(d, half, aggr):
    """(float64 reduce over every row, the float32 formula's largest error)"""
    _, _, _, src, lens = big_graph()
    xl = big_inputs(d, half, aggr == "max")[2]
    want = segment_reduce(xl, src, lens, aggr)
    e32 = float(np.abs(segment_reduce(xl.astype(np.float32), src, lens, aggr) - want).max())
    return torch.from_numpy(want), e32


@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def test_segment_reduce_is_the_plain_loop():
    """the reference of part 1 against a loop over rows, on the graph's first and last rows (CPU)"""
    _, _, _, src, lens = big_graph()
    x = np.random.default_rng(0).standard_normal((N_SRC, 3))
    start = np.concatenate([[0], np.cumsum(lens)])
    rows = list(range(40)) + list(range(ROWS_CAP - 40, ROWS_CAP))
    for aggr, f in (("sum", np.sum), ("mean", np.mean), ("max", np.max)):
        got = segment_reduce(x, src, lens, aggr)
        for i in rows:
            v = x[src[start[i]:start[i + 1]]]
            np.testing.assert_allclose(got[i], f(v, 0) if v.size else 0.0, rtol=0, atol=1e-12)
    i = np.arange(ROWS_CAP)
    deg = np.array(DEG)[(i + i // WAVES) % len(DEG)]
    assert set(lens[i % 3 != 1].tolist()) == set(DEG) and (lens <= deg).all()
    assert set((deg - lens)[1::3].tolist()) == {0, 1, 2}  # the windowed rows end up to two entries early
    assert all(len(set(deg[w::WAVES].tolist())) >= 4 for w in range(16))  # a wave's five rows differ (DEG has 0 twice)


GATHER_BIG = [(100, False, "mean")] + [(d, half, aggr) for d, half in ((8, False), (260, False), (8, True))
                                       for aggr in ("mean", "sum", "max")]


@gpu
@pytest.mark.parametrize("d,half,aggr", GATHER_BIG)
def test_gather_reduce_with_several_rows_per_wave(eng, d, half, aggr):
    rp, rowend, col, _, lens = big_graph()
    table, gid, xl = big_inputs(d, half, aggr == "max")
    want, e32 = big_reference(d, half, aggr)
    self_rows = torch.from_numpy(xl[:ROWS_CAP]).float()
    dt = torch.float16 if half else torch.float32
    dev = dict(rowptr=sk._i32(torch.from_numpy(rp)), rowend=sk._i32(torch.from_numpy(rowend)), col=sk._i32(torch.from_numpy(col)))
    tables = {True: (table.to(dt).cuda(), gid.to(torch.int32).cuda()), False: (torch.from_numpy(xl).to(dt).cuda(), None)}
    # gather_ids present and absent in turn over the row counts, both at the largest
    runs = [(n, bool(k % 2)) for k, n in enumerate(LIVE)] + [(LIVE[-1], False)]
    for n, ids in runs:
        src, g_ids = tables[ids]
        out = torch.full((ROWS_CAP, 2 * d), sk.SENTINEL, dtype=torch.float32, device="cuda")
        eng.gather_mean(src, d, g_ids, dev["rowptr"], dev["rowend"], dev["col"], sk._count(n), ROWS_CAP, out=out, aggr=aggr)
        label = f"gather {aggr} {'fp16' if half else 'fp32'} d={d} rows={n} of {ROWS_CAP} ids={ids}"
        assert bool((out[n:] == sk.SENTINEL).all()), f"{label}: rows past *n_rows_dev were written"
        got = out[:n].cpu()
        sk.check(label, "reduce", got[:, :d], want[:n], e32)
        assert torch.equal(got[:, d:], self_rows[:n]), f"{label}: the self half is the source row itself"
        if aggr == "max" and n:
            assert not bool(got[:, :d][torch.from_numpy(lens[:n] == 0)].any()), f"{label}: an empty row reduces to 0"


# ---- 2 and 3: the plan's first-layer gather and sage_fused_out ------------------------------------------------------
def _csc(n, src, dst):
    import oracle
    return oracle.build_csc(n, np.asarray(src, np.uint32), np.asarray(dst, np.uint32), is_directed=True)


@functools.lru_cache(None)
def wide_graph():
    """20 000 nodes: the 4 096 roots have 30 in-neighbours each among the other nodes, the other nodes 0 .. 12 among
    themselves — no root is a sampled neighbour, so a batch of 512 roots at fan-outs [25, 10] has ~9 000 layer-0 rows"""
    n, n_roots = 20_000, 4096
    rng = np.random.default_rng(7)
    deg = np.where(np.arange(n) < n_roots, 30, np.array([0, 1, 1, 2, 2, 3, 12, 1])[np.arange(n) % 8])
    dst = np.repeat(np.arange(n), deg)
    src = rng.integers(n_roots, n, dst.size)
    return (n,) + tuple(_csc(n, src, dst))


SPECIAL = dict(isolated=[0, 1, 2, 3], deg=[4, 5, 6, 7, 8, 9, 10, 11, 12, 13], self_adjacent=20, hubs={40: 24, 41: 25, 42: 80, 43: 200})
N_SMALL = 2048


@functools.lru_cache(None)
def root_graph():
    """2 048 nodes.  Isolated nodes 0 .. 3; nodes 4 .. 13 of in-degree 1, 1, 2, 2, .., 5, 5; node 20 adjacent to itself (and to
    two more); hubs 40 .. 43 of 24, 25, 80 and 200 in-edges; every node >= 64 has 0 .. 30 in-edges.  All sources >= 64"""
    n = N_SMALL
    rng = np.random.default_rng(11)
    src, dst = [], []

    def add(v, k):
        src.extend(rng.choice(np.arange(64, n), k, replace=False).tolist())
        dst.extend([v] * k)
    for j, v in enumerate(SPECIAL["deg"]):
        add(v, 1 + j // 2)
    add(SPECIAL["self_adjacent"], 2)
    src.append(SPECIAL["self_adjacent"])
    dst.append(SPECIAL["self_adjacent"])
    for v, k in SPECIAL["hubs"].items():
        add(v, k)
    for v in range(64, n):
        add(v, [0, 1, 2, 3, 5, 9, 14, 30][v % 8])
    return (n,) + tuple(_csc(n, src, dst))


def small_roots(b, groups=1):
    special = SPECIAL["isolated"] + SPECIAL["deg"] + [SPECIAL["self_adjacent"]] + list(SPECIAL["hubs"])
    r = np.concatenate([special, 64 + 5 * np.arange(b * groups - len(special))])
    return np.ascontiguousarray(r, dtype=np.uint32)


class PlanBench:
    """one engine per graph; a case = (case dict of sage_plan_cases, table, weights, roots)"""

    def __init__(self):
        self._e = {}

    def engine(self, name, graph):
        from gigl_amd.engine import HipEngine
        if name not in self._e:
            self._e[name] = HipEngine(0)
            self._e[name].load_csc(graph[1], graph[2])
        return self._e[name]

    def close(self):
        for e in self._e.values():
            e.close()


@pytest.fixture(scope="module")
def bench():
    b = PlanBench()
    yield b
    b.close()


def run_fused_plan(eng, case, x, roots):
    """-> (rows [b * groups, n_out], the plan's union graph on the host, weights, biases, dispatch)"""
    ws, bs = sc.make_weights(case, sc._rng(case, 2))
    disp = sc.dispatch(case, x)
    assert disp["fused"], "the case is meant for the fused pair of layers"
    eng.load_features(x)
    plan = sc.make_plan(eng, case, dict(weights=ws, biases=bs, roots=roots), roots)
    try:
        assert plan.fused_layers() and plan.half_split()
        out = plan.run(sc._dev_roots(eng, roots)).cpu().numpy()
        hb = plan.last_batch_to_host()
    finally:
        plan.close()
    return out, hb, ws, bs, disp


def check_against_float64(case, x, out, hb, ws, bs, disp, present=None):
    """the rows of the roots in `present` (all) against the float64 forward over the plan's own union graph"""
    ext = sc.plan_ext(case, hb)
    assert hb["meta"][sc.META_OVERFLOW] == 0 and ext is not None, "the plan's union graph is not a graph over the table"
    x64 = x.float().numpy().astype(np.float64)
    # (the scales of layer_params take the reduced operand's largest magnitude under a sum only: no extra forward for a mean)
    params = sc.params_of(case, disp, x, ws, bs, ext) if case["aggr"] == "sum" else sc.layer_params(case, disp, x, ws, bs, [0.0, 0.0])
    res = sc.forward(case, x64, ext, ws, bs, params)
    f32 = sc.forward(case, x.float().numpy(), ext, ws, bs, None, np.float32)
    keep = slice(None) if present is None else present
    got, want, bound = out[keep], res["y"][keep], res["bound"][keep]
    e32 = float(np.abs(f32["y"][keep].astype(np.float64) - want).max())
    err = np.abs(got.astype(np.float64) - want)
    print(f"{case['label']}: err/bound={float((err / bound).max()):.3g} fp32={e32:.3e}")
    assert np.isfinite(got).all() and (err <= bound).all(), (case["label"], float((err / bound).max()))
    sk.check(case["label"], "rows", torch.from_numpy(got), torch.from_numpy(want), e32)
    return ext


@gpu
def test_plan_first_layer_gather_with_several_rows_per_wave(bench, monkeypatch):
    n, rowptr, col = wide_graph()
    monkeypatch.setattr(sc, "N_NODES", n)  # (plan_ext: the leaves stand as global ids behind the local nodes)
    case = sc._case("round trips wide", d_in=100, hidden=[256], n_out=47, groups=8, fan=[25, 10])
    x = torch.from_numpy((np.random.default_rng(3).standard_normal((n, 100)) / 4).astype(np.float32))
    roots = np.random.default_rng(5).permutation(4096).astype(np.uint32)  # 8 batches of 512 distinct roots
    out, hb, ws, bs, disp = run_fused_plan(bench.engine("wide", (n, rowptr, col)), case, x, roots)
    ext = check_against_float64(case, x, out, hb, ws, bs, disp)
    # rows of the first layer: 16 384 waves (the plan provisions 8 * 512 * 26 rows) own 4 to 5 of them each, the first
    # 4 096 (the roots: local sources through gather_ids) on the same waves as rows of global ids
    assert ext["n_roots"] == 4096 and ext["n_rows"] > 65_536, (ext["n_roots"], ext["n_rows"])


FUSED_OUT = [(fan, n_out, aggr, bias) for fan, combos in (([3, 2], "msms"), ([25, 10], "smsm"), ([70, 2], "mssm"))
             for (n_out, bias), a in zip(((1, True), (5, False), (47, True), (48, False)), combos)
             for aggr in [{"m": "mean", "s": "sum"}[a]]] + \
            [([25, 10], 47, "mean", False), ([25, 10], 5, "sum", True), ([3, 2], 48, "sum", True), ([70, 2], 1, "mean", False)]


@gpu
@pytest.mark.parametrize("fan,n_out,aggr,bias", FUSED_OUT, ids=lambda v: str(v).replace(" ", ""))
def test_fused_out_over_every_root_row_length(bench, monkeypatch, fan, n_out, aggr, bias):
    n, rowptr, col = root_graph()
    monkeypatch.setattr(sc, "N_NODES", n)
    case = sc._case(f"round trips out{n_out} {aggr} fan{fan[0]} bias{int(bias)}", d_in=36, hidden=[256], n_out=n_out,
                    aggr=aggr, bias=bias, fan=fan, act_last=(n_out == 5))
    x = torch.from_numpy((np.random.default_rng(13).standard_normal((n, 36)) / 4).astype(np.float32))
    roots = small_roots(64)
    out, hb, ws, bs, disp = run_fused_plan(bench.engine("roots", (n, rowptr, col)), case, x, roots)
    check_against_float64(case, x, out, hb, ws, bs, disp)
    lens = (hb["rowend"] - hb["rowptr"])[hb["root_local"]]
    want = {0, 1, 2, 3} | ({4, 5, 24, 25} if fan[0] >= 25 else set()) | ({70} if fan[0] == 70 else set())
    assert want <= set(lens.tolist()), (sorted(set(lens.tolist())), "the roots' rows miss a length class")


@gpu
def test_fused_out_absent_root_gives_a_zero_row(bench, monkeypatch):
    n, rowptr, col = root_graph()
    monkeypatch.setattr(sc, "N_NODES", n)
    case = sc._case("round trips absent root", d_in=36, hidden=[256], n_out=47, fan=[25, 10], groups=2)
    x = torch.from_numpy((np.random.default_rng(13).standard_normal((n, 36)) / 4).astype(np.float32))
    roots = small_roots(32, 2)
    gone = 32 + 9  # a slot of the second batch
    roots[gone] = 0xFFFFFFFF  # (GIGL_INVALID, the id of a slot that holds no node; the plan does not range-check other ids)
    out, hb, ws, bs, disp = run_fused_plan(bench.engine("roots", (n, rowptr, col)), case, x, roots)
    assert hb["root_local"][gone] < 0 and not out[gone].any(), "an absent root's row is zero (no bias, no activation)"
    present = np.arange(roots.size) != gone
    assert (hb["root_local"][present] >= 0).all()
    hb["root_local"] = np.where(present, hb["root_local"], 0)  # (the reference reads a row for every slot)
    check_against_float64(case, x, out, hb, ws, bs, disp, present)


@gpu
def test_fused_out_writes_nan_rows_when_the_call_overflows(bench):
    """eight roots whose only in-neighbour is the hub root: the hub's sampled neighbours move up to level 1 under every
    one of them — more inner rows than the b * (1 + f0) the plan provisions (tests/test_gpu_overflow.py)"""
    n, hub, b, fan = 512, 0, 8, [2, 50]
    src = list(range(100, 300)) + [hub] * (b - 1)
    dst = [hub] * 200 + list(range(1, b))
    rowptr, col = _csc(n, src, dst)
    case = sc._case("round trips overflow", d_in=36, hidden=[256], n_out=47, fan=fan)
    x = torch.from_numpy((np.random.default_rng(17).standard_normal((n, 36)) / 4).astype(np.float32))
    out, hb, *_ = run_fused_plan(bench.engine("overflow", (n, rowptr, col)), case, x, np.arange(b, dtype=np.uint32))
    assert hb["meta"][sc.META_OVERFLOW] != 0, "the call no longer overflows: the test graph does not exercise the failed batch"
    assert np.isnan(out).all()
