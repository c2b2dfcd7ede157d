"""The per-edge attention kernels of csrc/gatv2.hip and csrc/hetero.hip, called directly through the HipEngine wrappers,
against float64 references: forward outputs and every returned gradient (torch autograd through the reference with
loss = sum(w * out), w fixed), at the shapes where the kernels change path.

References: oracle/gnn_ref.py's gatv2_conv / transformer_conv with float64 tensors and selection-matrix projections
(x = [xl | xr], lin_l = [I | 0], ...), its _segment_softmax for the SimpleHGN alpha, and three few-line edge-list
formulas written here (HGT reduce with edge types, GINE aggregation, weighted reduce) which the CPU test at the end pins
against gnn_ref.hgt_conv / transformer_conv / gine_conv / simplehgn_conv at 1e-12.

Inputs that are ADDED before a leaky_relu / relu (xl, xr, xe, x, ee, k, v) lie on the grid of multiples of 1/64 in
[-2, 2]: the sums are exact in fp32, so the kernel's and the reference's masks agree by construction.

Graphs: "rows" (195 rows = 3 mod 32: in-degrees 0..33 around every unroll / chunk boundary, a hub of 300, a row whose
only edge is a self loop, a self loop among other edges, a duplicated edge) and "long" (more rows than the capped grids
have waves: 16 400, and 4 200 for the GATv2 backward).

Tolerances: forward rtol = atol = 1e-5; gradients rtol = 1e-4, atol = 1e-4 * max|want| per tensor (the project's own).
On the rows graph (a 300-edge hub in every case, logits up to +-60 in the large-logit cases) the bound per tensor is the
larger of that and 4 x the maximum error of the SAME reference formula evaluated in float32 on the CPU (the factor
covers the kernel's summation order, its atomics and __expf); nothing is derived from the kernel's output.  Every case
prints `label err=<kernel> fp32=<float32 reference>`.

Measured on an MI355X (maximum |kernel - float64| next to the float32 reference's own error, worst tensor of the case):

    kernel, cases                      tensor     kernel    float32 reference
    gatv2, unit scale                  out        6.6e-07   6.2e-07
                                       dxl/dxr/dxe 1.9e-06  1.3e-06
                                       datt       1.3e-04   9.4e-05
    gatv2, hub logits +-60             out        5.0e-06   5.3e-06
                                       dxl/dxr/dxe 5.7e-05  1.4e-04
                                       datt       1.4e-04   1.8e-04
    transformer-edge, unit scale       out        1.6e-06   1.4e-06
                                       dq/dk/dv/dxe 3.0e-06 4.0e-06
    transformer-edge, hub logits +-60  out        3.6e-06   9.1e-06
                                       dq/dk/dv/dxe 2.6e-05 3.0e-05
    gine                               out        6.1e-06   6.1e-06   (max|out| ~ 250)
                                       dx / dee   1.8e-06   2.3e-06
                                       deps       5.1e-05   4.0e-05
    hgt reduce, unit scale             out        2.0e-06   2.2e-06
                                       dq/dk/dv   1.5e-06   1.6e-06
                                       dp_rel     7.8e-05   4.3e-05
    hgt reduce, hub logits +-60        out        3.4e-06   6.5e-06
                                       dq/dk/dv   2.9e-05   2.4e-05
                                       dp_rel     4.7e-04   2.2e-04
    weighted reduce                    out        3.2e-05   3.5e-05   (max|out| ~ 60)
                                       dalpha/dv  6.7e-06   1.1e-05
    simplehgn_alpha                    alpha      5.6e-08   5.6e-08
    long graphs (project tolerance only): out 1.2e-06, row gradients 3.6e-06, gine deps 2.4e-04
"""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import gnn_ref

gpu = pytest.mark.gpu
SLOPE = 0.2
HUB = 15
DEGREES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 300]  # rows 0..15 (the hub last)
SHAPES = [(1, 8), (3, 16), (2, 128), (1, 256), (3, 128), (8, 64), (10, 64), (3, 256), (4, 256)]
SHAPES_HGT = SHAPES + [(1, 4), (2, 16), (1, 64), (4, 32), (2, 64), (1, 128)]
REFUSED = [(33, 32), (1, 12), (1, 6)]
LARGE = [(3, 128), (2, 16)]


# ---- graphs (CSR by destination, CPU int64) -------------------------------------------------------------------------
def _graph(rows):
    deg = torch.tensor([r.numel() for r in rows])
    rp = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(deg, 0)])
    col = torch.cat(rows)
    return types.SimpleNamespace(n=len(rows), rp=rp, col=col, ei=gnn_ref.union_edge_index(rp, col))


@functools.lru_cache(None)
def rows_graph():
    g = torch.Generator().manual_seed(11)
    n = 195

    def others(i, d):  # d sources, none of them i
        s = torch.randint(0, n - 1, (d,), generator=g)
        return s + (s >= i).long()

    rows = [others(i, d) for i, d in enumerate(DEGREES)]
    rows.append(torch.tensor([16]))  # row 16: its only listed edge is a self loop
    s = others(17, 6)
    rows.append(torch.cat([s[:2], torch.tensor([17]), s[2:]]))  # row 17: a self loop among other edges
    s = others(18, 4)
    rows.append(torch.cat([s, s[1:2]]))  # row 18: a duplicated (src, dst) pair
    for i in range(19, n):  # the rest: degree 0..6, self loops allowed
        rows.append(torch.randint(0, n, (int(torch.randint(0, 7, (1,), generator=g)),), generator=g))
    gr = _graph(rows)
    assert gr.n % 32 == 3 and int(gr.rp[HUB + 1] - gr.rp[HUB]) == 300
    return gr


@functools.lru_cache(None)
def long_graph(n):
    g = torch.Generator().manual_seed(n)
    deg = torch.randint(0, 7, (n,), generator=g)  # average 3
    return _graph(list(torch.split(torch.randint(0, n, (int(deg.sum()),), generator=g), deg.tolist())))


def _grid(g, *shape):
    return torch.randint(-128, 129, shape, generator=g).double() / 64


def _free(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


# ---- references (dtype follows the inputs) --------------------------------------------------------------------------
def _sel(hc, parts, which, dt):
    """[0 | .. | I | .. | 0]: picks block `which` of `parts` blocks of hc columns"""
    w = torch.zeros(hc, parts * hc, dtype=dt)
    w[:, which * hc:(which + 1) * hc] = torch.eye(hc, dtype=dt)
    return w


def gatv2_ref(ei, heads, ch, xl, xr, att, xe=None):
    hc, dt = heads * ch, xl.dtype
    z = torch.zeros(hc, dtype=dt)
    p = {"lin_l.weight": _sel(hc, 2, 0, dt), "lin_l.bias": z, "lin_r.weight": _sel(hc, 2, 1, dt), "lin_r.bias": z,
         "att": att.view(1, heads, ch), "bias": z, "lin_edge.weight": torch.eye(hc, dtype=dt)}
    return gnn_ref.gatv2_conv(torch.cat([xl, xr], 1), ei, p, heads, ch, SLOPE, edge_attr=xe)


def transformer_ref(ei, heads, ch, q, k, v, xe=None):
    hc, dt = heads * ch, q.dtype
    z = torch.zeros(hc, dtype=dt)
    p = {"lin_query.weight": _sel(hc, 3, 0, dt), "lin_key.weight": _sel(hc, 3, 1, dt),
         "lin_value.weight": _sel(hc, 3, 2, dt), "lin_query.bias": z, "lin_key.bias": z, "lin_value.bias": z,
         "lin_edge.weight": torch.eye(hc, dtype=dt)}
    return gnn_ref.transformer_conv(torch.cat([q, k, v], 1), ei, p, heads, ch, root_weight=False, edge_attr=xe)


def hgt_ref(ei, heads, dim, etype, q, k, v, p_rel=None):
    """out_i = sum_e softmax_e(<q_i, k_j> p_rel[type(e)] / sqrt(D)) v_j over the in-edges of i, per head"""
    n, (src, dst) = q.shape[0], ei
    logit = (q[dst] * k[src]).view(-1, heads, dim).sum(-1) / dim ** 0.5
    if p_rel is not None:
        logit = logit * p_rel[etype]
    alpha = gnn_ref._segment_softmax(logit, dst, n)
    out = torch.zeros((n, heads, dim), dtype=q.dtype).index_add_(0, dst, v[src].view(-1, heads, dim) * alpha[:, :, None])
    return out.reshape(n, heads * dim)


def gine_ref(ei, x, ee, eps):
    return (1.0 + eps) * x + torch.zeros_like(x).index_add(0, ei[1], torch.relu(x[ei[0]] + ee))


def weighted_ref(ei, heads, dim, alpha, v):
    n = v.shape[0]
    out = torch.zeros((n, heads, dim), dtype=v.dtype).index_add_(0, ei[1], v[ei[0]].view(-1, heads, dim) * alpha[:, :, None])
    return out.reshape(n, heads * dim)


def shgn_alpha_ref(src, dst, etype, n, hl, hr, het, hef=None):
    logit = hl[src] + hr[dst] + het[etype]
    if hef is not None:
        logit = logit + hef
    return gnn_ref._segment_softmax(F.leaky_relu(logit, SLOPE), src, n)


def _run(fn, inputs, w, dt):
    leaves = {k: t.to(dt).clone().requires_grad_(True) for k, t in inputs.items() if t is not None}
    out = fn(**leaves)
    grads = torch.autograd.grad((out * w.to(dt)).sum(), list(leaves.values()))
    res = {"out": out.detach().double()}
    res.update({"d" + k: gr.double() for k, gr in zip(leaves, grads)})
    return res


def reference(fn, inputs, w, fp32=True):
    """-> (want: float64 output "out" and gradients "d<name>", e32: the float32 evaluation's maximum error per tensor)"""
    want = _run(fn, inputs, w, torch.float64)
    if not fp32:
        return want, None
    lo = _run(fn, inputs, w, torch.float32)
    return want, {k: float((lo[k] - want[k]).abs().max()) for k in want}


def check(label, got, want, e32, name, rows=None):
    grad = name != "out"
    got, want = got.detach().double().cpu(), want[name]
    if rows is not None:
        got, want = got[:rows], want[:rows]
    assert got.shape == want.shape, (label, name, got.shape, want.shape)
    rtol = 1e-4 if grad else 1e-5
    atol = 1e-4 * float(want.abs().max()) if grad and want.numel() else 1e-5
    tol = atol + rtol * want.abs()
    f32 = e32[name] if e32 is not None else 0.0
    tol = torch.clamp(tol, min=4.0 * f32)
    err = (got - want).abs()
    print(f"{label} {name}: err={float(err.max()) if err.numel() else 0.0:.3e} fp32={f32:.3e}")
    assert bool(torch.isfinite(got).all()), f"{label} {name}: non-finite values"
    bad = err > tol
    assert not bool(bad.any()), (f"{label} {name}: {int(bad.sum())} of {bad.numel()} beyond the bound, max err "
                                 f"{float(err.max()):.3e} (float32 reference {f32:.3e})")


# ---- device side ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _f(t):
    return None if t is None else t.float().contiguous().cuda()


def _csr(gr, col=None):
    rp = gr.rp.to(torch.int32).cuda()
    return types.SimpleNamespace(rp=rp, rowptr=rp[:-1], rowend=rp[1:], col=(gr.col if col is None else col).to(torch.int32).cuda())


def _count(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def _hub_sort(gr, col, z, descending, per_edge):
    """reorder the hub row's edges by the logit z[:, 0] (the order inside a CSR row is free)"""
    sl = slice(int(gr.rp[HUB]), int(gr.rp[HUB + 1]))
    order = torch.argsort(z[:, 0], descending=descending)
    col[sl] = col[sl][order]
    for t in per_edge:
        if t is not None:
            t[sl] = t[sl][order]
    return sl


def _graph_with(gr, col):
    return types.SimpleNamespace(n=gr.n, rp=gr.rp, col=col, ei=gnn_ref.union_edge_index(gr.rp, col))


# ---- GATv2 ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def gatv2_case(heads, ch, edge, large=None, rows=None):
    """large: None | "asc" | "desc" (hub logits +-60, ordered); rows: None = the rows graph, else a long graph"""
    gr = rows_graph() if rows is None else long_graph(rows)
    g = torch.Generator().manual_seed(1000 * heads + ch + (7 if edge else 0))
    hc, ne = heads * ch, gr.col.numel()
    xl, xr = _grid(g, gr.n, hc), _grid(g, gr.n, hc)
    xe = _grid(g, ne, hc) if edge else None
    att, w = _free(g, hc) / ch ** 0.5, _free(g, gr.n, hc)
    col = gr.col.clone()
    if large:
        sl = slice(int(gr.rp[HUB]), int(gr.rp[HUB + 1]))
        s = xl[col[sl]] + xr[HUB] + (xe[sl] if edge else 0)
        z = (F.leaky_relu(s, SLOPE) * att).view(-1, heads, ch).sum(-1)
        att = att * (60.0 / float(z.abs().max()))
        _hub_sort(gr, col, z, large == "desc", [xe])
        gr = _graph_with(gr, col)
    inputs = {"xl": xl, "xr": xr, "att": att, "xe": xe}
    want, e32 = reference(functools.partial(gatv2_ref, gr.ei, heads, ch), inputs, w, fp32=rows is None)
    return gr, inputs, w, want, e32


def _gatv2_run(eng, case, heads, ch, backward, n_rows=None):
    gr, inp, w, want, e32 = case
    u, nd = _csr(gr), _count(gr.n if n_rows is None else n_rows)
    xl, xr, att, xe = (_f(inp[k]) for k in ("xl", "xr", "att", "xe"))
    out = eng.gatv2_aggregate(xl, xr, att, heads, ch, u, nd, None, SLOPE, 0, xe)
    if not backward:
        return {"out": out}
    dxl, dxr, datt, dxe = eng.gatv2_aggregate_backward(xl, xr, att, heads, ch, u, nd, out, _f(w), SLOPE, xe)
    return {"out": out, "dxl": dxl, "dxr": dxr, "datt": datt, "dxe": dxe}


GATV2_CASES = [(h, c, e, None) for (h, c) in SHAPES for e in (False, True)] + \
              [(h, c, True, o) for (h, c) in LARGE for o in ("asc", "desc")]


@gpu
@pytest.mark.parametrize("heads,ch,edge,large", GATV2_CASES)
def test_gatv2_forward(eng, heads, ch, edge, large):
    case = gatv2_case(heads, ch, edge, large)
    got = _gatv2_run(eng, case, heads, ch, False)
    check(f"gatv2 fwd {heads}x{ch} edge={edge} {large}", got["out"], case[3], case[4], "out")


@gpu
@pytest.mark.parametrize("heads,ch,edge,large", GATV2_CASES)
def test_gatv2_backward(eng, heads, ch, edge, large):
    case = gatv2_case(heads, ch, edge, large)
    got = _gatv2_run(eng, case, heads, ch, True)
    for name in ("dxl", "dxr", "datt") + (("dxe",) if edge else ()):
        check(f"gatv2 bwd {heads}x{ch} edge={edge} {large}", got[name], case[3], case[4], name)
    if not edge:
        assert got["dxe"] is None


@gpu
def test_gatv2_forward_takes_a_second_grid_stride_step(eng):
    case = gatv2_case(1, 8, True, None, 16400)  # 16 400 rows > 4096 blocks x 4 waves
    check("gatv2 fwd long", _gatv2_run(eng, case, 1, 8, False)["out"], case[3], None, "out")


@gpu
def test_gatv2_backward_takes_a_second_grid_stride_step(eng):
    case = gatv2_case(1, 8, True, None, 4200)  # 4 200 rows > 1024 blocks x 4 waves; datt is summed per wave
    got = _gatv2_run(eng, case, 1, 8, True)
    for name in ("out", "dxl", "dxr", "datt", "dxe"):
        check("gatv2 bwd long", got[name], case[3], None, name)


def _prefix_reference(fn, inputs, w, keep):
    """the reference restricted to the destination rows < keep: only they enter the loss (their outputs do not depend
    on the other rows' edges), so every gradient of the other rows' edges and rows is exactly 0"""
    wm = w.clone()
    wm[keep:] = 0
    return reference(fn, inputs, wm)


@gpu
@pytest.mark.parametrize("edge", [False, True])
def test_gatv2_row_prefix(eng, edge):
    heads, ch = 3, 16
    gr, inp, w, _, _ = gatv2_case(heads, ch, edge)
    keep = gr.n - 37
    want, e32 = _prefix_reference(functools.partial(gatv2_ref, gr.ei, heads, ch), inp, w, keep)
    got = _gatv2_run(eng, (gr, inp, w, want, e32), heads, ch, True, n_rows=keep)  # (dout is NOT masked for the kernel)
    label = f"gatv2 prefix edge={edge}"
    check(label, got["out"], want, e32, "out", rows=keep)  # (the forward output buffer is not initialised past keep)
    for name in ("dxl", "dxr", "datt") + (("dxe",) if edge else ()):
        check(label, got[name], want, e32, name)
    assert not bool(got["dxr"][keep:].any())
    if edge:
        assert not bool(got["dxe"][int(gr.rp[keep]):].any())


# ---- TransformerConv with edge rows ---------------------------------------------------------------------------------
@functools.lru_cache(None)
def transformer_case(heads, ch, large=None, rows=None):
    gr = rows_graph() if rows is None else long_graph(rows)
    g = torch.Generator().manual_seed(2000 * heads + ch)
    hc, ne = heads * ch, gr.col.numel()
    q, k, v, xe, w = _grid(g, gr.n, hc), _grid(g, gr.n, hc), _grid(g, gr.n, hc), _grid(g, ne, hc), _free(g, gr.n, hc)
    col = gr.col.clone()
    if large:
        sl = slice(int(gr.rp[HUB]), int(gr.rp[HUB + 1]))
        z = (q[HUB] * (k[col[sl]] + xe[sl])).view(-1, heads, ch).sum(-1) / ch ** 0.5
        q = q * (60.0 / float(z.abs().max()))
        _hub_sort(gr, col, z, large == "desc", [xe])
        gr = _graph_with(gr, col)
    inputs = {"q": q, "k": k, "v": v, "xe": xe}
    want, e32 = reference(functools.partial(transformer_ref, gr.ei, heads, ch), inputs, w, fp32=rows is None)
    return gr, inputs, w, want, e32


def _transformer_run(eng, case, heads, ch, backward, n_rows=None):
    gr, inp, w, want, e32 = case
    u, nd = _csr(gr), _count(gr.n if n_rows is None else n_rows)
    q, k, v, xe = (_f(inp[n]) for n in ("q", "k", "v", "xe"))
    out = eng.transformer_aggregate_edge(q, k, v, xe, heads, ch, u, nd)
    if not backward:
        return {"out": out}
    dq, dk, dv, dxe = eng.transformer_aggregate_edge_backward(q, k, v, xe, heads, ch, u, nd, out, _f(w))
    return {"out": out, "dq": dq, "dk": dk, "dv": dv, "dxe": dxe}


TRANSFORMER_CASES = [(h, c, None) for (h, c) in SHAPES] + [(h, c, o) for (h, c) in LARGE for o in ("asc", "desc")]


@gpu
@pytest.mark.parametrize("heads,ch,large", TRANSFORMER_CASES)
def test_transformer_edge_forward(eng, heads, ch, large):
    case = transformer_case(heads, ch, large)
    check(f"transformer fwd {heads}x{ch} {large}", _transformer_run(eng, case, heads, ch, False)["out"], case[3], case[4],
          "out")


@gpu
@pytest.mark.parametrize("heads,ch,large", TRANSFORMER_CASES)
def test_transformer_edge_backward(eng, heads, ch, large):
    case = transformer_case(heads, ch, large)
    got = _transformer_run(eng, case, heads, ch, True)
    for name in ("dq", "dk", "dv", "dxe"):
        check(f"transformer bwd {heads}x{ch} {large}", got[name], case[3], case[4], name)


@gpu
def test_transformer_edge_takes_a_second_grid_stride_step(eng):
    case = transformer_case(1, 8, None, 16400)
    got = _transformer_run(eng, case, 1, 8, True)
    for name in ("out", "dq", "dk", "dv", "dxe"):
        check("transformer long", got[name], case[3], None, name)


@gpu
def test_transformer_edge_row_prefix(eng):
    heads, ch = 3, 16
    gr, inp, w, _, _ = transformer_case(heads, ch)
    keep = gr.n - 37
    want, e32 = _prefix_reference(functools.partial(transformer_ref, gr.ei, heads, ch), inp, w, keep)
    got = _transformer_run(eng, (gr, inp, w, want, e32), heads, ch, True, n_rows=keep)
    check("transformer prefix", got["out"], want, e32, "out", rows=keep)
    for name in ("dq", "dk", "dv", "dxe"):
        check("transformer prefix", got[name], want, e32, name)
    assert not bool(got["out"][keep:].any()) and not bool(got["dq"][keep:].any())
    assert not bool(got["dxe"][int(gr.rp[keep]):].any())


# ---- GINE -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def gine_case(d, eps, rows=None):
    gr = rows_graph() if rows is None else long_graph(rows)
    g = torch.Generator().manual_seed(3000 + d)
    x, ee, w = _grid(g, gr.n, d), _grid(g, gr.col.numel(), d), _free(g, gr.n, d)
    inputs = {"x": x, "ee": ee, "eps": torch.tensor([eps], dtype=torch.float64)}
    want, e32 = reference(functools.partial(gine_ref, gr.ei), inputs, w, fp32=rows is None)
    return gr, inputs, w, want, e32


def _gine_run(eng, case, n_rows=None):
    gr, inp, w, want, e32 = case
    u, nd = _csr(gr), _count(gr.n if n_rows is None else n_rows)
    x, ee, eps = _f(inp["x"]), _f(inp["ee"]), _f(inp["eps"])
    out = eng.gine_aggregate(x, ee, eps, u, nd)
    dx, dee, deps = eng.gine_aggregate_backward(x, ee, eps, u, nd, _f(w))
    return {"out": out, "dx": dx, "dee": dee, "deps": deps}


@gpu
@pytest.mark.parametrize("eps", [0.0, -0.3])
@pytest.mark.parametrize("d", [1, 5, 64, 65, 200])
def test_gine_forward_and_backward(eng, d, eps):
    case = gine_case(d, eps)
    got = _gine_run(eng, case)
    for name in ("out", "dx", "dee", "deps"):
        check(f"gine d={d} eps={eps}", got[name], case[3], case[4], name)


@gpu
def test_gine_takes_a_second_grid_stride_step(eng):
    case = gine_case(8, -0.3, 16400)
    got = _gine_run(eng, case)
    for name in ("out", "dx", "dee", "deps"):
        check("gine long", got[name], case[3], None, name)


@gpu
def test_gine_row_prefix(eng):
    gr, inp, w, _, _ = gine_case(65, -0.3)
    keep = gr.n - 37
    want, e32 = _prefix_reference(functools.partial(gine_ref, gr.ei), inp, w, keep)
    got = _gine_run(eng, (gr, inp, w, want, e32), n_rows=keep)
    check("gine prefix", got["out"], want, e32, "out", rows=keep)
    for name in ("dx", "dee", "deps"):
        check("gine prefix", got[name], want, e32, name)
    assert not bool(got["out"][keep:].any()) and not bool(got["dee"][int(gr.rp[keep]):].any())


# ---- HGT reduce -----------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def hgt_case(heads, dim, typed, large=None):
    gr = rows_graph()
    g = torch.Generator().manual_seed(4000 * heads + dim + (3 if typed else 0))
    hd, ne = heads * dim, gr.col.numel()
    q, k, v, w = _grid(g, gr.n, hd), _grid(g, gr.n, hd), _grid(g, gr.n, hd), _free(g, gr.n, hd)
    etype = torch.randint(0, 3, (ne,), generator=g) if typed else None
    p_rel = 0.5 + torch.rand(3, heads, generator=g, dtype=torch.float64) if typed else None
    col = gr.col.clone()
    if large:
        sl = slice(int(gr.rp[HUB]), int(gr.rp[HUB + 1]))
        z = (q[HUB] * k[col[sl]]).view(-1, heads, dim).sum(-1) / dim ** 0.5
        if typed:
            z = z * p_rel[etype[sl]]
        q = q * (60.0 / float(z.abs().max()))
        _hub_sort(gr, col, z, large == "desc", [etype])
        gr = _graph_with(gr, col)
    inputs = {"q": q, "k": k, "v": v, "p_rel": p_rel}
    want, e32 = reference(functools.partial(hgt_ref, gr.ei, heads, dim, etype), inputs, w)
    return gr, inputs, w, want, e32, etype


def _hgt_run(eng, case, heads, dim, backward):
    gr, inp, w, want, e32, etype = case
    u = _csr(gr)
    q, k, v, p_rel = (_f(inp[n]) for n in ("q", "k", "v", "p_rel"))
    et = etype.to(torch.int32).cuda() if etype is not None else None
    out = torch.zeros_like(q)
    eng.hgt_aggregate(q, k, v, heads, dim, u.rp, u.col, et, p_rel, gr.n, out)
    if not backward:
        return {"out": out}
    dq, dk, dv, dp = eng.hgt_aggregate_backward(q, k, v, heads, dim, u.rp, u.col, et, p_rel, gr.n, out, _f(w))
    return {"out": out, "dq": dq, "dk": dk, "dv": dv, "dp_rel": dp}


HGT_CASES = [(h, d, t, None) for (h, d) in SHAPES_HGT for t in (False, True)] + \
            [(h, d, True, o) for (h, d) in LARGE for o in ("asc", "desc")]


@gpu
@pytest.mark.parametrize("heads,dim,typed,large", HGT_CASES)
def test_hgt_reduce_forward(eng, heads, dim, typed, large):
    case = hgt_case(heads, dim, typed, large)
    check(f"hgt fwd {heads}x{dim} typed={typed} {large}", _hgt_run(eng, case, heads, dim, False)["out"], case[3], case[4],
          "out")


@gpu
@pytest.mark.parametrize("heads,dim,typed,large", HGT_CASES)
def test_hgt_reduce_backward(eng, heads, dim, typed, large):
    case = hgt_case(heads, dim, typed, large)
    got = _hgt_run(eng, case, heads, dim, True)
    for name in ("dq", "dk", "dv") + (("dp_rel",) if typed else ()):
        check(f"hgt bwd {heads}x{dim} typed={typed} {large}", got[name], case[3], case[4], name)
    if not typed:
        assert got["dp_rel"] is None


# ---- weighted reduce ------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def weighted_case(heads, dim):
    gr = rows_graph()
    g = torch.Generator().manual_seed(5000 * heads + dim)
    hd = heads * dim
    inputs = {"alpha": torch.rand(gr.col.numel(), heads, generator=g, dtype=torch.float64), "v": _grid(g, gr.n, hd)}
    w = _free(g, gr.n, hd)
    want, e32 = reference(functools.partial(weighted_ref, gr.ei, heads, dim), inputs, w)
    return gr, inputs, w, want, e32


@gpu
@pytest.mark.parametrize("heads,dim", SHAPES_HGT)
def test_weighted_reduce_forward_and_backward(eng, heads, dim):
    gr, inp, w, want, e32 = weighted_case(heads, dim)
    u, alpha, v = _csr(gr), _f(inp["alpha"]), _f(inp["v"])
    out = torch.zeros_like(v)
    eng.weighted_aggregate(alpha, v, heads, dim, u.rp, u.col, gr.n, out)
    dalpha, dv = eng.weighted_aggregate_backward(alpha, v, heads, dim, u.rp, u.col, gr.n, _f(w))
    for name, got in (("out", out), ("dalpha", dalpha), ("dv", dv)):
        check(f"weighted {heads}x{dim}", got, want, e32, name)


# ---- shapes outside the built set -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("heads,ch", REFUSED)
def test_unbuilt_shapes_are_refused(eng, heads, ch):
    from gigl_amd._lib import GiglError
    gr = rows_graph()
    u, nd, hc, ne = _csr(gr), _count(gr.n), heads * ch, gr.col.numel()
    x, xe, att = torch.zeros(gr.n, hc, device="cuda"), torch.zeros(ne, hc, device="cuda"), torch.zeros(hc, device="cuda")
    alpha = torch.zeros(ne, heads, device="cuda")
    calls = [
        lambda: eng.gatv2_aggregate(x, x, att, heads, ch, u, nd, None),
        lambda: eng.gatv2_aggregate(x, x, att, heads, ch, u, nd, None, edge_rows=xe),
        lambda: eng.gatv2_aggregate_backward(x, x, att, heads, ch, u, nd, x, x),
        lambda: eng.gatv2_aggregate_backward(x, x, att, heads, ch, u, nd, x, x, edge_rows=xe),
        lambda: eng.transformer_aggregate_edge(x, x, x, xe, heads, ch, u, nd),
        lambda: eng.transformer_aggregate_edge_backward(x, x, x, xe, heads, ch, u, nd, x, x),
        lambda: eng.hgt_aggregate(x, x, x, heads, ch, u.rp, u.col, None, None, gr.n, torch.zeros_like(x)),
        lambda: eng.hgt_aggregate_backward(x, x, x, heads, ch, u.rp, u.col, None, None, gr.n, x, x),
        lambda: eng.weighted_aggregate(alpha, x, heads, ch, u.rp, u.col, gr.n, torch.zeros_like(x)),
        lambda: eng.weighted_aggregate_backward(alpha, x, heads, ch, u.rp, u.col, gr.n, x),
    ]
    for call in calls:
        with pytest.raises(GiglError):
            call()


# ---- SimpleHGN alpha (softmax over the edges that share a SOURCE node) ---------------------------------------------
N_SHGN = 64
G_EMPTY, G_ONE, G_TWO, G_BIG, G_WIDE, G_NEGZERO, G_MIX = 0, 1, 2, 3, 4, 5, 6  # the source nodes of the groups


@functools.lru_cache(None)
def shgn_case(heads, with_ef):
    """groups of 0, 1, 2 and 300 edges at unit scale (destinations 0..19, types 0 / 1); G_WIDE: 40 edges whose logits
    span +-60 after the leaky_relu (raw -300..60: through hr of its destinations 20..59, or through hef); G_NEGZERO: 5
    edges whose hl, hr, het (type 2) and hef are all -0.0; G_MIX: -0.0 and negative logits"""
    g = torch.Generator().manual_seed(6000 + heads + (5 if with_ef else 0))
    src = [G_ONE] + [G_TWO] * 2 + [G_BIG] * 300
    dst = torch.randint(0, 20, (len(src),), generator=g).tolist()
    et = torch.randint(0, 2, (len(src),), generator=g).tolist()
    src += [G_WIDE] * 40 + [G_NEGZERO] * 5 + [G_MIX] * 6
    dst += list(range(20, 60)) + [60, 61, 60, 61, 60] + [60, 62, 61, 63, 62, 60]
    et += [0] * 40 + [2] * 11
    order = torch.randperm(len(src), generator=g)  # the groups interleaved in the edge list
    src, dst, et = (torch.tensor(t)[order] for t in (src, dst, et))
    hl, hr, het = _free(g, N_SHGN, heads), _free(g, N_SHGN, heads), _free(g, 3, heads)
    hef = _free(g, src.numel(), heads) if with_ef else None
    ramp = torch.linspace(-300.0, 60.0, 40, dtype=torch.float64)[:, None].expand(40, heads)
    hl[G_WIDE] = 0.0
    if with_ef:
        hr[20:60] = 0.0
        hef[src == G_WIDE] = ramp[dst[src == G_WIDE] - 20] - het[0]
    else:
        hr[20:60] = ramp - het[0]
    hl[G_NEGZERO], hl[G_MIX], het[2] = -0.0, -0.0, -0.0
    hr[60], hr[61], hr[62], hr[63] = -0.0, -0.0, -1.5, -4.0
    if with_ef:
        hef[(src == G_NEGZERO) | (src == G_MIX)] = -0.0
    want = shgn_alpha_ref(src, dst, et, N_SHGN, hl, hr, het, hef)
    lo = shgn_alpha_ref(src, dst, et, N_SHGN, hl.float(), hr.float(), het.float(), hef.float() if with_ef else None)
    return src, dst, et, hl, hr, het, hef, want, float((lo.double() - want).abs().max())


@gpu
@pytest.mark.parametrize("with_ef", [False, True])
@pytest.mark.parametrize("heads", [1, 3])
def test_simplehgn_alpha(eng, heads, with_ef):
    src, dst, et, hl, hr, het, hef, want, e32 = shgn_case(heads, with_ef)
    i32 = lambda t: t.to(torch.int32).cuda()
    for t in (hl[G_NEGZERO], het[2], hr[60]):  # the -0.0 inputs reach the device as -0.0
        assert bool(torch.signbit(_f(t)).all())
    got = eng.simplehgn_alpha(_f(hl), _f(hr), _f(het), _f(hef), i32(src), i32(dst), i32(et), N_SHGN, heads, SLOPE)
    check(f"simplehgn_alpha heads={heads} ef={with_ef}", got, {"out": want}, {"out": e32}, "out")
    nz = got.cpu()[src == G_NEGZERO]
    assert nz.shape == (5, heads) and torch.allclose(nz, torch.full_like(nz, 0.2), rtol=1e-6, atol=0)
    sums = torch.zeros(N_SHGN, heads, dtype=torch.float64).index_add_(0, src, got.double().cpu())
    for grp in (G_ONE, G_TWO, G_BIG, G_WIDE, G_NEGZERO, G_MIX):
        assert torch.allclose(sums[grp], torch.ones(heads, dtype=torch.float64), rtol=1e-5, atol=0)


# ---- CPU: the formulas written above against the gnn_ref layers (float64, 30 nodes) --------------------------------
def test_reference_helpers_match_gnn_ref():
    g = torch.Generator().manual_seed(5)
    n, heads, dim, T = 30, 3, 8, 3
    hd = heads * dim
    deg = torch.randint(0, 6, (n,), generator=g)
    gr = _graph(list(torch.split(torch.randint(0, n, (int(deg.sum()),), generator=g), deg.tolist())))
    src, dst = gr.ei
    ne = src.numel()
    etype = torch.randint(0, T, (ne,), generator=g)
    q, k, v = _grid(g, n, hd), _grid(g, n, hd), _grid(g, n, hd)
    p_rel = 0.5 + torch.rand(T, heads, generator=g, dtype=torch.float64)
    eye = lambda m: torch.eye(m, dtype=torch.float64)
    zeros = lambda *s: torch.zeros(*s, dtype=torch.float64)

    # HGT reduce with edge types: HGTConv with identity projections / relation transforms is gelu(reduce)
    ets = [("n", f"r{t}", "n") for t in range(T)]
    p = {"kqv": {"n": (eye(3 * hd), zeros(3 * hd))}, "out": {"n": (eye(hd), zeros(hd))},
         "k_rel": [eye(dim)] * (heads * T), "v_rel": [eye(dim)] * (heads * T), "skip": {"n": zeros(())},
         "p_rel": {et: p_rel[t] for t, et in enumerate(ets)}, "edge_types": ets}
    conv = gnn_ref.hgt_conv({"n": torch.cat([k, q, v], 1)}, {et: gr.ei[:, etype == t] for t, et in enumerate(ets)}, p,
                            heads)["n"]
    mine = hgt_ref(gr.ei, heads, dim, etype, q, k, v, p_rel)
    assert float((F.gelu(mine) - conv).abs().max()) <= 1e-12
    # ... and without types: TransformerConv without edge features
    assert float((hgt_ref(gr.ei, heads, dim, None, q, k, v) - transformer_ref(gr.ei, heads, dim, q, k, v)).abs().max()) \
        <= 1e-12

    # GINE: identity edge projection, MLP = [I; -I] -> relu -> [I | -I] (relu(a) - relu(-a) = a)
    d, eps = 7, -0.3
    x, ee = _grid(g, n, d), _grid(g, ne, d)
    conv = gnn_ref.gine_conv(x, gr.ei, ee, eye(d), zeros(d), torch.cat([eye(d), -eye(d)]), zeros(2 * d),
                             torch.cat([eye(d), -eye(d)], 1), zeros(d), eps=eps)
    assert float((gine_ref(gr.ei, x, ee, eps) - conv).abs().max()) <= 1e-12

    # SimpleHGN: alpha over the SOURCE groups, then the weighted reduce at the destinations
    fin, out_dim, te, ein = 6, 8, 4, 5
    for with_ef in (False, True):
        p = {"W_nfeat": _free(g, fin, heads * out_dim), "a_l": _free(g, 1, heads, out_dim), "a_r": _free(g, 1, heads, out_dim),
             "a_etype": _free(g, 1, heads, te), "edge_type_emb": _free(g, T, te),
             "W_etype": (_free(g, T, te, heads * te), _free(g, T, heads * te)), "residual": None,
             "W_efeat": _free(g, ein, heads * ein), "a_efeat": _free(g, 1, heads, ein)}
        feat, ef = _free(g, n, fin), (_free(g, ne, ein) if with_ef else None)
        conv = gnn_ref.simplehgn_conv(gr.ei, feat, etype, p, heads, out_dim, SLOPE, edge_feat=ef)
        emb = (feat @ p["W_nfeat"]).reshape(n, heads, out_dim)
        w_et, b_et = p["W_etype"]
        et_vec = torch.stack([p["edge_type_emb"][t] @ w_et[t] + b_et[t] for t in range(T)]).reshape(T, heads, te)
        hef = (p["a_efeat"] * (ef @ p["W_efeat"]).reshape(-1, heads, ein)).sum(-1) if with_ef else None
        alpha = shgn_alpha_ref(src, dst, etype, n, (p["a_l"] * emb).sum(-1), (p["a_r"] * emb).sum(-1),
                               (p["a_etype"] * et_vec).sum(-1), hef)
        mine = weighted_ref(gr.ei, heads, out_dim, alpha, emb.reshape(n, heads * out_dim))
        assert float((mine - conv).abs().max()) <= 1e-12
