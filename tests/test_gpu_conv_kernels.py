"""The per-edge convolutions of csrc/gatv2.hip — gatv2_forward_kernel<1|2|4> and gatv2_backward_kernel<1|2|4>,
gine_forward_kernel and gine_backward_kernel, transformer_edge_forward_kernel<1|2|4> and
transformer_edge_backward_kernel<1|2|4> — called directly through HipEngine.gatv2_aggregate / gatv2_aggregate_backward /
gine_aggregate / gine_aggregate_backward / transformer_aggregate_edge / transformer_aggregate_edge_backward against
float64 references computed on the CPU, at the shapes where the dispatch code changes path.  The conventions are those of
tests/test_gpu_gat_kernels.py; the graphs, inputs, references, case lists and the restated dispatch live in
tests/attn_cases.py.

References: gatv2_ref, gine_ref, trans_ref — edge-list formulas whose leaves are the kernels' own inputs (xl, xr, att, xe;
x, ee, eps; q, k, v, xe), so torch autograd gives exactly what the backward kernels return (d xe with the self loop's
ds_self / cnt share).  The CPU test at the end pins them at 1e-12 against oracle/gnn_ref.py's gatv2_conv and
transformer_conv (selector weights, with and without edge features) and gine_conv (identity edge map, an MLP that is the
identity): outputs and an input gradient.  out / out_pre handed to a backward is the float64 reference output rounded to
fp32 (the pre-bias one for GATv2).

Inputs: GATv2's xl, xr, xe and GINE's x, ee sit on multiples of 1/8 in [-1, 1], zeros included: xl_j + xr_i + xe_e and
x_j + ee_e are exact in fp32 and the `> 0` masks of kernel and reference agree by construction.  The one inexact sum is
the GATv2 self loop's, through its mean edge row: a channel of xr[i] is drawn again where the float64 |s_self| is below
1e-3 (for the packed and the windowed graph at once); the CPU test asserts the condition for every case.  The edge-
Transformer has no masks: random fp32 values, q times 30 in the large-logit case; att times 4 does the same for GATv2.
dout is random fp32, every 7th row all zero.  NaN: the node past the last referenced one (and every later row of xl / x /
k / v), xr / q / dout / out past the live rows, the edge rows of the entries a window skips, of the rows past the live
ones and, for GATv2, of the listed self loops.

Graph "rows" (attn_cases.rows_graph): 131 rows, *n_rows_dev = 127, capacity 136; in-degrees 0, 1, 2, 3, 4, 5, 7, 8, 9, 15,
16, 17, 31, 32, 33, 63, 64, 65 and a hub of 300, a duplicated edge, a row listing itself twice, a row whose only edge is a
self loop; packed and windowed (every row i % 3 == 1 ends 1 or 2 entries early, the skipped entries name the NaN node).
The nodes 128 and 129 are read by nobody.  "long": 16 400 rows of degree 0..3, more rows than the capped grids have waves
(forwards and the other backwards 16 384, GATv2 backward 4 096), at heads x channels = 1 x 4 and d = 3.

Tolerances: forward rtol = atol = 1e-5; gradients rtol = 1e-4, atol = 1e-4 * max|want| per tensor (the project's own).  On
the rows graph the bound per tensor is the larger of that and 4 x the maximum error of the SAME formula evaluated in
float32 on the CPU; the long graph gets the project tolerance only.  Exact: sentinels past *n_rows_dev, the gradient rows
of the nodes nobody reads, d xe / d ee at the skipped entries and at GATv2's dropped self loops, everything row-owned of
a row whose dout is zero, empty rows of the edge-Transformer (0), buffers after a refused call.  Every case prints
`label tensor: err=<kernel> fp32=<float32 reference>`.

Measured on an MI355X (maximum |kernel - float64| next to the float32 reference's own error; worst case of the class):

    kernels, cases                          tensor        kernel    float32 reference
    GATv2 forward <1|2|4>                   out           1.4e-06   1.9e-06
    GATv2 forward, edge rows                out           1.3e-06   1.5e-06
    GATv2 backward <1|2|4>                  dxl           8.2e-06   7.9e-06
                                            dxr           1.4e-05   9.3e-06
                                            datt          3.3e-05   2.5e-05
    GATv2 backward, edge rows               dxl           1.2e-05   1.1e-05
                                            dxr           1.6e-05   1.0e-05
                                            datt          5.2e-05   4.3e-05
                                            dxe           1.0e-05   9.9e-06
    GATv2, att times 4 (with / without xe)  out           3.6e-06   4.9e-06
                                            dxl           8.6e-05   6.6e-05
                                            dxr / dxe     1.2e-04   3.6e-05
                                            datt          7.6e-05   3.0e-05
    GINE forward                            out           4.9e-06   4.9e-06
    GINE backward                           dx            1.1e-06   1.1e-06
                                            dee           0         0         (a masked copy of dout)
                                            deps          1.9e-05   2.0e-05
    edge-Transformer forward <1|2|4>        out           1.4e-06   1.4e-06
    edge-Transformer backward <1|2|4>       dq            2.0e-06   2.4e-06
                                            dk / dv       1.8e-06   1.4e-06
                                            dxe           1.7e-06   1.5e-06
    edge-Transformer, q times 30            out           1.7e-05   1.5e-05
                                            dq            4.1e-05   1.1e-05
                                            dk / dxe      8.1e-04   1.2e-04   (max|dk| ~ 140)
                                            dv            6.1e-06   8.5e-06
    long graph (project tolerance only): GATv2 out 1.9e-07, dxl / dxr / dxe 6.2e-07, datt 6.3e-05; GINE out 3.4e-07,
    dx 5.4e-07, deps 1.2e-04; edge-Transformer out 7.8e-07, dq / dk / dv / dxe 2.2e-06

No defect of gatv2.hip was found.
"""
import pytest
import torch

import attn_cases as ac
from attn_cases import check, count, f32
from oracle import gnn_ref

gpu = pytest.mark.gpu
GATV2 = [(s, edge, CASE % 3) for CASE, (s, edge) in enumerate((s, e) for s in ac.CONV_ALL for e in (False, True))]
GINE = [(d, ac.GINE_EPS[i % 2]) for i, d in enumerate(ac.GINE_D)] + [(65, 0.0), (64, 0.37)]


def _id(x):
    if isinstance(x, tuple) and len(x) == 3:
        return "%dx%d" % x[0] + ("-xe" if x[1] else "") + "-mode%d" % x[2]
    return "%dx%d" % x if isinstance(x, tuple) and isinstance(x[1], int) else str(x)


def _label(kind, heads, c, gr):
    return f"{kind} {heads}x{c} (V, <V>, lph)={ac.conv_shape(heads, c)} {gr.kind} window={gr.window}"


@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _read(gr, rows, live_too):
    """the nodes somebody reads: the sources of the live windows, and (self loop / self term) the live rows"""
    read = torch.zeros(rows, dtype=torch.bool)
    read[gr.raw_src] = True
    if live_too:
        read[:gr.n_live] = True
    return read


def check_forward(label, via_engine, own, want, e32, gr):
    """via_engine: what the HipEngine method returned; own: the same entry point on a sentinel-filled buffer of ours"""
    n = gr.n_live
    check(label, "out", via_engine[:n].cpu(), want, e32)
    assert torch.equal(via_engine[:n].cpu(), own[:n].cpu()), f"{label}: two calls of a forward differ"
    assert bool((own[n:] == ac.SENTINEL).all()), f"{label}: rows past *n_rows_dev were written"


def _dout(t, gr):
    d = t.dout.clone()
    d[gr.n_live:] = ac.NAN
    return f32(d)


def check_row_owned(label, name, x, t, gr, mask_unused):
    """x [entries, width]: 0 at the entries that do not count and at those of the rows whose dout is zero"""
    assert not bool(x[mask_unused].any()), f"{label} {name}: written at an entry that does not count"
    assert not bool(x[gr.raw[t.zero_rows[gr.raw_dst]]].any()), f"{label} {name}: of a row whose dout is zero"


# ---- 1. GATv2 --------------------------------------------------------------------------------------------------------
def run_gatv2(eng, t, gr, mode):
    u, nr, hc = ac.dev_graph(gr), count(gr.n_live), t.heads * t.c
    xl, xr, att, bias = f32(t.xl), f32(t.xr), f32(t.att), f32(t.bias) if mode else None
    xe = ac.nan_where(t.xe, ~gr.keep) if t.edge else None
    got = eng.gatv2_aggregate(xl, xr, att, t.heads, t.c, u, nr, bias, ac.SLOPE, int(mode == 2), xe)
    own = ac.full(gr.cap, hc)
    rc = ac.raw_call(eng, "gigl_gatv2_aggregate_edge", xl, xr, att, t.heads, t.c, ac.SLOPE, u.rowptr, u.rowend, u.col, nr,
                     gr.cap, bias, int(mode == 2), xe, own)
    assert rc == 0
    return got, own


def run_gatv2_backward(eng, t, gr, want):
    xe = ac.nan_where(t.xe, ~gr.keep) if t.edge else None
    return eng.gatv2_aggregate_backward(f32(t.xl), f32(t.xr), f32(t.att), t.heads, t.c, ac.dev_graph(gr), count(gr.n_live),
                                        ac.padded(want["out"], gr.cap), _dout(t, gr), ac.SLOPE, xe)


def check_gatv2_backward(label, got, t, gr, want, e32):
    dxl, dxr, datt, dxe = (None if x is None else x.cpu() for x in got)
    n = gr.n_live
    for name, x in (("dxl", dxl), ("dxr", dxr), ("datt", datt)):
        check(label, name, x, want[name], e32[name], grad=True)
    assert not bool(dxl[~_read(gr, gr.cap, True)].any()), f"{label}: dxl of a node nobody reads"
    assert not bool(dxr[n:].any()) and not bool(dxr[:n][t.zero_rows].any()), f"{label}: dxr of a row without dout"
    assert (dxe is None) == (not t.edge)
    if dxe is not None:
        check(label, "dxe", dxe, want["dxe"], e32["dxe"], grad=True)
        check_row_owned(label, "dxe", dxe, t, gr, ~gr.keep)


@gpu
@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("case", GATV2, ids=_id)
def test_gatv2_forward(eng, case, window):
    (heads, c), edge, mode = case
    t, gr, want, e32 = ac.gatv2_case("rows", heads, c, edge, window)
    got, own = run_gatv2(eng, t, gr, mode)
    check_forward(_label("gatv2", heads, c, gr) + f" xe={edge} mode={mode}", got, own, ac.finish(want["out"], t.bias, mode),
                  e32["out"], gr)


@gpu
@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("case", GATV2, ids=_id)
def test_gatv2_backward(eng, case, window):
    (heads, c), edge, _ = case
    t, gr, want, e32 = ac.gatv2_case("rows", heads, c, edge, window)
    label = _label("gatv2 bwd", heads, c, gr) + f" xe={edge}"
    check_gatv2_backward(label, run_gatv2_backward(eng, t, gr, want), t, gr, want, e32)


@gpu
@pytest.mark.parametrize("edge", [False, True])
def test_gatv2_large_logits(eng, edge):
    """att times 4: logits beyond +-50 on the hub row, forward and backward"""
    heads, c = ac.CONV_LARGE
    t, gr, want, e32 = ac.gatv2_case("rows", heads, c, edge, True, 4)
    label = _label("gatv2 x4", heads, c, gr) + f" xe={edge}"
    got, own = run_gatv2(eng, t, gr, 0)
    check_forward(label, got, own, want["out"], e32["out"], gr)
    check_gatv2_backward(label, run_gatv2_backward(eng, t, gr, want), t, gr, want, e32)


@gpu
@pytest.mark.parametrize("edge", [False, True])
def test_gatv2_long_graph(eng, edge):
    heads, c = ac.LONG_SHAPE
    t, gr, want, e32 = ac.gatv2_case("long", heads, c, edge)
    label = _label("gatv2", heads, c, gr) + f" xe={edge}"
    got, own = run_gatv2(eng, t, gr, 2)
    check_forward(label, got, own, ac.finish(want["out"], t.bias, 2), e32["out"], gr)
    check_gatv2_backward(label, run_gatv2_backward(eng, t, gr, want), t, gr, want, e32)


# ---- 2. GINE ---------------------------------------------------------------------------------------------------------
def run_gine(eng, t, gr, eps):
    u, nr = ac.dev_graph(gr), count(gr.n_live)
    x, ee, ep = f32(t.x), ac.nan_where(t.ee, ~gr.used), torch.tensor([eps], dtype=torch.float32, device="cuda")
    got = eng.gine_aggregate(x, ee, ep, u, nr)
    own = ac.full(gr.cap, t.d)
    assert ac.raw_call(eng, "gigl_gine_aggregate", x, ee, ep, t.d, u.rowptr, u.rowend, u.col, nr, gr.cap, own) == 0
    return got, own, eng.gine_aggregate_backward(x, ee, ep, u, nr, _dout(t, gr))


def check_gine(label, res, t, gr, want, e32):
    got, own, (dx, dee, deps) = res
    check_forward(label, got, own, want["out"], e32["out"], gr)
    dx, dee, deps = dx.cpu(), dee.cpu(), deps.cpu()
    check(label, "dx", dx, want["dx"], e32["dx"], grad=True)
    check(label, "dee", dee, want["dee"], e32["dee"], grad=True)
    check(label, "deps", deps.reshape(()), want["deps"], e32["deps"], grad=True)
    assert not bool(dx[~_read(gr, gr.cap, True)].any()), f"{label}: dx of a node nobody reads"
    check_row_owned(label, "dee", dee, t, gr, ~gr.used)


@gpu
@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("d,eps", GINE)
def test_gine(eng, d, eps, window):
    t, gr, want, e32 = ac.gine_case("rows", d, eps, window)
    check_gine(f"gine d={d} eps={eps} window={window}", run_gine(eng, t, gr, eps), t, gr, want, e32)


@gpu
def test_gine_long_graph(eng):
    t, gr, want, e32 = ac.gine_case("long", ac.LONG_D, 0.37)
    check_gine(f"gine d={ac.LONG_D} long", run_gine(eng, t, gr, 0.37), t, gr, want, e32)


# ---- 3. edge-Transformer ---------------------------------------------------------------------------------------------
def run_trans(eng, t, gr, want):
    u, nr, hc = ac.dev_graph(gr), count(gr.n_live), t.heads * t.c
    q, k, v, xe = f32(t.q), f32(t.k), f32(t.v), ac.nan_where(t.xe, ~gr.used)
    got = eng.transformer_aggregate_edge(q, k, v, xe, t.heads, t.c, u, nr)
    own = ac.full(gr.cap, hc)
    assert ac.raw_call(eng, "gigl_transformer_aggregate_edge", q, k, v, xe, t.heads, t.c, u.rowptr, u.rowend, u.col, nr,
                       gr.cap, own) == 0
    back = eng.transformer_aggregate_edge_backward(q, k, v, xe, t.heads, t.c, u, nr, ac.padded(want["out"], gr.cap),
                                                   _dout(t, gr))
    return got, own, back


def check_trans(label, res, t, gr, want, e32):
    got, own, back = res
    n = gr.n_live
    check_forward(label, got, own, want["out"], e32["out"], gr)
    assert not bool(own[:n][gr.m[:n] == 0].any().cpu()), f"{label}: an empty row is not exactly 0"
    dq, dk, dv, dxe = (x.cpu() for x in back)
    for name, x in (("dq", dq), ("dk", dk), ("dv", dv), ("dxe", dxe)):
        check(label, name, x, want[name], e32[name], grad=True)
    assert not bool(dq[n:].any()) and not bool(dq[:n][t.zero_rows].any()), f"{label}: dq of a row without dout"
    unread = ~_read(gr, gr.cap, False)
    assert not bool(dk[unread].any()) and not bool(dv[unread].any()), f"{label}: dk / dv of a node nobody reads"
    check_row_owned(label, "dxe", dxe, t, gr, ~gr.used)


@gpu
@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("shape", ac.CONV_ALL, ids=_id)
def test_transformer_edge(eng, shape, window):
    t, gr, want, e32 = ac.trans_case("rows", *shape, window)
    check_trans(_label("trans", *shape, gr), run_trans(eng, t, gr, want), t, gr, want, e32)


@gpu
def test_transformer_edge_large_logits(eng):
    """q times 30: logits beyond +-50 on the hub row"""
    heads, c = ac.CONV_LARGE
    t, gr, want, e32 = ac.trans_case("rows", heads, c, True, 30)
    check_trans(_label("trans x30", heads, c, gr), run_trans(eng, t, gr, want), t, gr, want, e32)


@gpu
def test_transformer_edge_long_graph(eng):
    t, gr, want, e32 = ac.trans_case("long", *ac.LONG_SHAPE)
    check_trans(_label("trans", *ac.LONG_SHAPE, gr), run_trans(eng, t, gr, want), t, gr, want, e32)


# ---- 4. refused shapes -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", ac.REFUSED, ids=_id)
def test_refused_shapes_write_nothing(eng, shape):
    from gigl_amd._lib import GiglError
    heads, c = shape
    assert ac.conv_shape(heads, c) is None
    gr = ac.rows_graph(True)
    hc, ce, cap = heads * c, gr.col.numel(), gr.cap
    g = torch.Generator().manual_seed(hc)
    a, b, d, dout = (f32(ac.free(g, cap, hc)) for _ in range(4))
    att, xe = f32(ac.free(g, hc)), f32(ac.free(g, ce, hc))
    u, nr = ac.dev_graph(gr), count(gr.n_live)
    calls = [lambda: eng.gatv2_aggregate(a, b, att, heads, c, u, nr, None),
             lambda: eng.gatv2_aggregate(a, b, att, heads, c, u, nr, att, ac.SLOPE, 1, xe),
             lambda: eng.gatv2_aggregate_backward(a, b, att, heads, c, u, nr, d, dout),
             lambda: eng.gatv2_aggregate_backward(a, b, att, heads, c, u, nr, d, dout, ac.SLOPE, xe),
             lambda: eng.transformer_aggregate_edge(a, b, d, xe, heads, c, u, nr),
             lambda: eng.transformer_aggregate_edge_backward(a, b, d, xe, heads, c, u, nr, d, dout)]
    for call in calls:
        with pytest.raises(GiglError) as info:
            call()
        assert info.value.code == ac.E_UNSUPPORTED
    s = [ac.full(cap, hc) for _ in range(7)] + [ac.full(hc), ac.full(ce, hc), ac.full(ce, hc)]
    g3 = (u.rowptr, u.rowend, u.col, nr, cap)
    rcs = [ac.raw_call(eng, "gigl_gatv2_aggregate_edge", a, b, att, heads, c, ac.SLOPE, *g3, att, 1, xe, s[0]),
           ac.raw_call(eng, "gigl_gatv2_aggregate_edge_backward", a, b, att, heads, c, ac.SLOPE, *g3, d, dout, xe, s[1], s[2],
                       s[7], s[8]),
           ac.raw_call(eng, "gigl_transformer_aggregate_edge", a, b, d, xe, heads, c, *g3, s[3]),
           ac.raw_call(eng, "gigl_transformer_aggregate_edge_backward", a, b, d, xe, heads, c, *g3, d, dout, s[4], s[5], s[6],
                       s[9])]
    assert rcs == [ac.E_UNSUPPORTED] * 4
    assert all(bool((x == ac.SENTINEL).all()) for x in s), "a refused call wrote its outputs"


# ---- CPU: the formulas against oracle/gnn_ref.py, the inputs' conditions, the coverage, the bounds -------------------
DD = torch.float64


def _selector(hc, parts, which):
    """[hc, parts * hc]: takes block `which` of a row of `parts` blocks"""
    w = torch.zeros(hc, parts * hc, dtype=DD)
    w[:, which * hc:(which + 1) * hc] = torch.eye(hc, dtype=DD)
    return w


def _pin_gatv2(heads, c, edge, window):
    t, gr = ac.gatv2_inputs("rows", heads, c, edge), ac.rows_graph(window)
    hc, n, nn = heads * c, gr.n_live, ac.N_NODES
    xl0, xr0 = torch.nan_to_num(t.xl), torch.nan_to_num(t.xr)
    x = torch.cat([xl0[:nn], xr0[:nn]], 1).requires_grad_(True)
    p = {"lin_l.weight": _selector(hc, 2, 0), "lin_r.weight": _selector(hc, 2, 1), "lin_l.bias": torch.zeros(hc, dtype=DD),
         "lin_r.bias": torch.zeros(hc, dtype=DD), "att": t.att.view(1, heads, c), "bias": t.bias,
         "lin_edge.weight": torch.eye(hc, dtype=DD)}
    ei = torch.stack([gr.raw_src, gr.raw_dst])  # the live windows, listed self loops included
    assert int((ei[0] == ei[1]).sum()) >= 3
    conv = gnn_ref.gatv2_conv(x, ei, p, heads, c, ac.SLOPE, False, t.xe[gr.raw] if edge else None)[:n]
    w = ac.free(torch.Generator().manual_seed(3), n, hc)
    gx = torch.autograd.grad((conv * w).sum(), x)[0]
    xl, xr = xl0.clone().requires_grad_(True), xr0.clone().requires_grad_(True)
    out = ac.gatv2_ref(gr, heads, c, xl, xr, t.att, t.xe)[0] + t.bias
    dxl, dxr = torch.autograd.grad((out * w).sum(), [xl, xr])
    assert ac.err(out, conv) <= 1e-12, (heads, c, edge, window)
    assert ac.err(dxl[:nn], gx[:, :hc]) <= 1e-12 and ac.err(dxr[:nn], gx[:, hc:]) <= 1e-12


def _pin_trans(heads, c, edge, window):
    t, gr = ac.trans_inputs("rows", heads, c), ac.rows_graph(window)
    hc, n, nn = heads * c, gr.n_live, ac.N_NODES
    q0, k0, v0 = (torch.nan_to_num(z) for z in (t.q, t.k, t.v))
    x = torch.cat([q0[:nn], k0[:nn], v0[:nn]], 1).requires_grad_(True)
    p = {"lin_edge.weight": torch.eye(hc, dtype=DD)}
    for i, name in enumerate(("lin_query", "lin_key", "lin_value")):
        p[name + ".weight"], p[name + ".bias"] = _selector(hc, 3, i), torch.zeros(hc, dtype=DD)
    conv = gnn_ref.transformer_conv(x, torch.stack([gr.raw_src, gr.raw_dst]), p, heads, c, True, False, False,
                                    t.xe[gr.raw] if edge else None)[:n]
    w = ac.free(torch.Generator().manual_seed(4), n, hc)
    gx = torch.autograd.grad((conv * w).sum(), x)[0]
    q, k, v = (z.clone().requires_grad_(True) for z in (q0, k0, v0))
    out = ac.trans_ref(gr, heads, c, q, k, v, t.xe if edge else None)
    dq, dk, dv = torch.autograd.grad((out * w).sum(), [q, k, v])
    assert ac.err(out, conv) <= 1e-12, (heads, c, edge, window)
    assert max(ac.err(dq[:nn], gx[:, :hc]), ac.err(dk[:nn], gx[:, hc:2 * hc]), ac.err(dv[:nn], gx[:, 2 * hc:])) <= 1e-12


def _pin_gine(d, eps, window):
    t, gr = ac.gine_inputs("rows", d), ac.rows_graph(window)
    n, nn = gr.n_live, ac.N_NODES
    x0 = torch.nan_to_num(t.x)
    eye, zero = torch.eye(d, dtype=DD), torch.zeros(d, dtype=DD)
    x = x0[:nn].clone().requires_grad_(True)
    # nn = lin0 -> relu -> lin1 with identity weights and biases +-4096 is the identity, smooth everywhere: |a| < 4096, and
    # the shift costs at most half an ulp of 8192 (4.5e-13)
    conv = gnn_ref.gine_conv(x, torch.stack([gr.raw_src, gr.raw_dst]), t.ee[gr.raw], eye, zero, eye, zero + 4096.0, eye,
                             zero - 4096.0, eps)[:n]
    w = ac.free(torch.Generator().manual_seed(5), n, d)
    x2 = x0.clone().requires_grad_(True)
    out = ac.gine_ref(gr, x2, t.ee, eps)
    assert ac.err(out, conv) <= 1e-12, (d, eps, window)
    assert ac.err(torch.autograd.grad((out * w).sum(), x2)[0][:nn], torch.autograd.grad((conv * w).sum(), x)[0]) <= 1e-12


def test_references_inputs_and_coverage():
    rows, where = ac.base_rows()
    packed, win = ac.rows_graph(False), ac.rows_graph(True)
    # the graphs deliver what the cases rely on
    assert ac.N_LIVE < ac.N_ROWS < ac.CAP and ac.N_ROWS % 8 != 0
    for gr in (packed, win):
        assert [int(gr.m[where["deg%d" % d]]) for d in ac.DEGREES] == ac.DEGREES and int(gr.m[where["hub"]]) == ac.HUB
        assert int(gr.cnt[where["self_only"]]) == 0 and int(gr.m[where["self_only"]]) == 1
        assert int(gr.cnt[where["self_twice"]]) == 4 and int(gr.m[where["self_twice"]]) == 6
        assert int(gr.raw_src.max()) < ac.N_READ and int((gr.cnt == 0).sum()) >= 3 and int((gr.m[:ac.N_LIVE] == 0).sum()) >= 2
        assert int((~gr.keep & gr.used).sum()) >= 3  # listed self loops
        # kept counts that are no power of two (an inexact mean) and that are one
        pow2 = (gr.cnt & (gr.cnt - 1)) == 0
        assert int(pow2.sum()) >= 20 and int((~pow2).sum()) >= 20
    short = win.rp[1:] - win.rowend
    assert int((short > 0).sum()) == ac.N_ROWS // 3 + (ac.N_ROWS % 3 == 2) and set(short[short > 0].tolist()) == {1, 2}
    skipped = win.col[torch.arange(win.col.numel()) >= win.rowend[torch.repeat_interleave(torch.arange(ac.N_ROWS),
                                                                                          win.rp[1:] - win.rp[:-1])]]
    assert skipped.numel() == int(short.sum()) and bool((skipped == ac.NAN_NODE).all())
    assert int((win.col == ac.NAN_NODE).sum()) == skipped.numel() and not bool((packed.col == ac.NAN_NODE).any())
    lg = ac.long_graph()
    assert lg.n_rows == 16400 and lg.n_live > ac.FWD_WAVES > ac.GATV2_BWD_WAVES and lg.n_live < lg.n_rows < lg.cap
    assert int(lg.m.max()) == 3 and int((lg.m == 0).sum()) > 1000 and int((~lg.keep & lg.used).sum()) >= 1
    assert ac.FWD_WAVES == 16384 and ac.GATV2_BWD_WAVES == 4096

    # the formulas against gnn_ref (float64): outputs and input gradients
    for window in (False, True):
        for heads, c in ((2, 4), (1, 8)):
            for edge in (False, True):
                _pin_gatv2(heads, c, edge, window)
                _pin_trans(heads, c, edge, window)
        _pin_gine(3, 0.37, window)
        _pin_gine(5, 0.0, window)

    # the inputs: exact sums, zeros among them, the self loops' margin, the large logits
    for (heads, c), edge, sc in [(s, e, 1) for s, e, _ in GATV2] + [(ac.CONV_LARGE, e, 4) for e in (False, True)]:
        t = ac.gatv2_inputs("rows", heads, c, edge, sc)
        for gr in (packed, win):
            s = torch.nan_to_num(t.xl)[gr.src] + torch.nan_to_num(t.xr)[gr.dst] + (t.xe[gr.pos] if edge else 0)
            assert bool((s * 8 == (s * 8).round()).all()) and float(s.abs().max()) <= 3 and bool((s == 0).any())
            if edge:
                assert float(ac._self_s(t, gr).abs().min()) >= 1e-3, (heads, c, sc)
        assert int(t.zero_rows.sum()) >= 15 and not bool(t.dout[:ac.N_LIVE][t.zero_rows].any())
    for edge in (False, True):
        t = ac.gatv2_inputs("long", *ac.LONG_SHAPE, edge)
        assert not edge or float(ac._self_s(t, lg).abs().min()) >= 1e-3
        t = ac.gatv2_inputs("rows", *ac.CONV_LARGE, edge, 4)
        heads, c = ac.CONV_LARGE
        s = torch.nan_to_num(t.xl)[win.src] + torch.nan_to_num(t.xr)[win.dst] + (t.xe[win.pos] if edge else 0)
        z = (torch.nn.functional.leaky_relu(s, ac.SLOPE).view(-1, heads, c) * t.att.view(1, heads, c)).sum(-1)
        hub = z[win.dst == where["hub"]]  # (a row's logits share xr_i: its centre moves, its spread is what rescales)
        assert float(z.max()) >= 50 and float(z.min()) <= -50, (edge, float(z.max()), float(z.min()))
        assert float((hub.max(0).values - hub.min(0).values).min()) >= 80
    t = ac.trans_inputs("rows", *ac.CONV_LARGE, 30)
    z = ac.trans_logits(t, win)[win.raw_dst == where["hub"]]
    assert float(z.max()) >= 50 and float(z.min()) <= -50
    for d in ac.GINE_D:
        t = ac.gine_inputs("rows", d)
        msg = torch.nan_to_num(t.x)[packed.raw_src] + t.ee[packed.raw]
        assert bool((msg == 0).any()) and bool((msg > 0).any()) and bool((msg < 0).any())

    # coverage, from the case lists and the restated dispatch
    for v in (1, 2, 3, 4):
        assert all(ac.conv_shape(*s)[:2] == (v, ac.instantiation(v)) for s in ac.CONV_SHAPES[v])
    assert {ac.conv_shape(*s)[1] for s in ac.CONV_ALL} == {1, 2, 4} and ac.conv_shape(3, 256) == (3, 4, 64)
    assert {ac.conv_shape(*s)[2] for s in ac.CONV_ALL} == {1, 4, 16, 32, 64}
    assert ac.conv_shape(3, 128) == (2, 2, 32) and (3 * 128 // 4) % 64 != 0  # a partially filled last chunk row
    assert any((h * c // 4) % 64 for h, c in ac.CONV_SHAPES[1]) and ac.conv_shape(6, 128) == (3, 4, 32)
    assert {(e, m) for _, e, m in GATV2} == {(e, m) for e in (False, True) for m in (0, 1, 2)}
    assert all(ac.conv_shape(*s) is None for s in ac.REFUSED) and ac.conv_shape(*ac.LONG_SHAPE) == (1, 1, 1)
    assert {d for d, _ in GINE} == set(ac.GINE_D) and {e for _, e in GINE} == set(ac.GINE_EPS)
    assert {d % 64 for d in ac.GINE_D} >= {0, 1, 63, 2, 3} and {(d + 63) // 64 for d in ac.GINE_D} == {1, 2, 3, 4}

    # the bounds can fail: a deliberately wrong float64 variant against the right one, through the tests' own bound
    for window in (False, True):
        t, gr, want, e32 = ac.gatv2_case("rows", 4, 64, True, window)
        xl, xr = torch.nan_to_num(t.xl), torch.nan_to_num(t.xr)
        assert ac.beyond(want["out"], want["out"], e32["out"], False) == 0
        for wrong in ("self_zero", "self_sum", "keep_self"):
            bad = ac.gatv2_ref(gr, 4, 64, xl, xr, t.att, t.xe, wrong=wrong)[0]
            assert ac.beyond(bad, want["out"], e32["out"], False) > 0, wrong
        t, gr, want, e32 = ac.gatv2_case("rows", 2, 16, False, window)
        bad = ac.gatv2_ref(gr, 2, 16, torch.nan_to_num(t.xl), torch.nan_to_num(t.xr), t.att, None, wrong="keep_self")[0]
        assert ac.beyond(bad, want["out"], e32["out"], False) > 0
        t, gr, want, e32 = ac.trans_case("rows", 2, 16, window)
        for wrong in ("no_xe_values", "no_scale"):
            bad = ac.trans_ref(gr, 2, 16, t.q, torch.nan_to_num(t.k), torch.nan_to_num(t.v), t.xe, wrong=wrong)
            assert ac.beyond(bad[gr.m[:gr.n_live] > 0], want["out"][gr.m[:gr.n_live] > 0], e32["out"], False) > 0, wrong
