"""The hidden-layer GAT aggregation of csrc/agg.hip — gat_alpha / gat_gather (generic), gat_alpha_fast / gat_gather_fast /
gat_gather_heavy (the fast pair and the hub kernel), gat_edge_alpha / gat_edge_gather and the fast kernels' edge and
message terms, gat_backward<V> at 8 / 4 / 2 / 1 waves per row, gat_backward_epilogue — called directly through
HipEngine.gat_aggregate / gat_aggregate_backward / gat_backward_epilogue against float64 references computed on the CPU,
at the shapes where the dispatch code changes path.

Reference: gat_ref below, a few-line edge-list formula whose leaves are h, a_src, a_dst and the per-position a_edge (the
self loop's a_edge and edge attribute are the MEAN over the row's non-self positions inside the formula), so that torch
autograd gives exactly what the backward kernel returns: d_alpha_src, d_alpha_dst, d_alpha_edge (with the dpre_self / cnt
share) and dh through the messages only; z_out is its sum_e alpha_e e_e + alpha_self * mean e.  The CPU test at the end
pins it at 1e-12 against oracle/gnn_ref.py's gat_conv (identity weight, folded edge vector, concat both ways, with and
without w_edge_msg; outputs and the gradient w.r.t. h).  out_pre handed to the backward is the float64 reference output
rounded to fp32, u_msg is W_msg^T dout formed in float64 and rounded.

Inputs: h on multiples of 1/64 in [-2, 2]; att_src, att_dst, edge_attr, att_edge_folded on multiples of 1/8 in [-1, 1]
(the att_* times 4 in the large-logit cases): a_src, a_dst, a_edge and every non-self logit are exact in fp32 in any
summation order, so the kernel's and the reference's leaky_relu masks agree by construction.  The self loop's logit holds
a mean and is not exact: with edge features a node whose float64 |pre_self| would be below 1e-3 for some head gets a
fresh h row (pre_self of row i depends on h[i] only); the CPU test asserts the condition.  dout, bias and w_edge_msg are
random fp32 values; every 7th dout row is all zero (the backward skips it).

Graphs: "rows" — 195 rows (= 3 mod 32), *n_rows_dev = 190, 196 nodes of which the last is a row of NaN, capacity 200; in-
degrees 0..127 around the 4-edge unroll and the 64-lane loops, a row whose only edge is a self loop, a row listing itself
twice, a duplicated edge, hubs of 128 / 129 / 177 / 192 / 300 / 250 in-edges (slices of the hub kernel: all full; five
empty; one empty; exactly full at 12; fifteen of 20 and one empty; a last slice of 10) and three hubs of 140 whose first
(wave 0's) / sixth / first two slices of 12 are all self loops; packed and windowed (every row i % 3 == 1 ends 1 or 2
entries early; the skipped col entries name the NaN node, their edge attributes are NaN, as are those of the self-loop
positions).
Nodes 193..195 are read by nobody.  "long": 16 400 / 20 000 / 33 000 rows of degree 0..6, more rows than the capped grids
have waves (generic gather 16 384; backward at 2 waves per row 16 384; fast gather, gat_alpha_fast and the backward at 1
wave per row 32 768).

Tolerances: forward rtol = atol = 1e-5; gradients and z_out rtol = 1e-4, atol = 1e-4 * max|want| per tensor (the
project's own).  On the rows graph the bound per tensor is the larger of that and 4 x the maximum error of the SAME
formula evaluated in float32 on the CPU (the factor covers summation order, atomics and __expf); the long graphs get the
project tolerance only.  Exact: sentinels past *n_rows_dev, zeros of the nodes nobody reads, of the skipped / self-loop
positions of d_alpha_edge and of everything belonging to a row whose dout is zero, buffers after a refused call.  Nothing
is derived from the kernel's output.  Every case prints `label tensor: err=<kernel> fp32=<float32 reference>`.

Measured on an MI355X (maximum |kernel - float64| next to the float32 reference's own error; worst case of the class):

    kernels, cases                          tensor        kernel    float32 reference
    forward, fast pair + hub kernel         out           2.1e-06   4.1e-06
    forward, fast, edge term                out           2.4e-06   5.0e-06
    forward, fast, message term             out           2.4e-05   1.4e-05   (max|out| ~ 40 at De = 256)
    forward, generic                        out           1.9e-06   2.8e-06
    forward, generic, edge term             out           1.4e-06   2.3e-06
    forward, generic, message term          out           5.9e-06   1.7e-05
    forward, hub logits beyond +-50         out           4.5e-06   4.5e-06   (fast; plain, edge and message term)
    backward, 8 waves per row               dh            5.4e-06   5.6e-06
                                            d_alpha_src/dst 2.0e-05 5.9e-05
    backward, edge term                     dh            5.9e-06   6.4e-06
                                            d_alpha_src/dst 1.5e-05 5.1e-05
                                            d_alpha_edge  1.4e-05   4.5e-05
    backward, message term (1 wave per row) dh            4.8e-06   4.8e-06
                                            d_alpha_src/dst 7.9e-05 8.6e-05
                                            d_alpha_edge  3.9e-05   8.4e-05
                                            z_out         1.6e-06   1.6e-06
    backward, hub logits beyond +-50        dh            2.4e-06   1.8e-06
                                            d_alpha_*     1.1e-05   6.5e-06
                                            z_out         3.8e-07   3.8e-07
    backward, 8 / 4 / 2 / 1 waves per row   dh            2.2e-06   2.4e-06   (capacity 200 .. 32768, same rows)
                                            d_alpha_*     1.2e-05   7.8e-06
    epilogue                                dxw           1.2e-06   1.2e-06
                                            d_att_src/dst 6.1e-05   1.4e-05   (bound 1e-4 * max|want| ~ 9e-3)
    long graphs (project tolerance only): out 7.8e-07, dh 1.2e-06, d_alpha_src/dst/edge 3.6e-06
"""
import functools
import types

import pytest
import torch

from oracle import gnn_ref

gpu = pytest.mark.gpu
SLOPE = 0.2
N_ROWS, N_LIVE, N_NODES, CAP = 195, 190, 196, 200  # rows of the CSR, *n_rows_dev, meta[0], nodes.numel()
N_READ = 193  # sources are < N_READ: the nodes 193, 194 and the NaN node are read by nobody and are no live row
NAN_NODE = N_NODES - 1
SENTINEL = 7.0
E_UNSUPPORTED = -4
LIST_DEGREES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127]
HUBS = [128, 129, 177, 192, 300, 250]
GAT_ZR, HEAVY_MIN, HEAVY_WAVES, MAX_EDGE_DIM = 4, 128, 16, 256  # agg.hip's constants
CAPS = [CAP, 2048, 8192, 32768]  # only the capacity grows: the backward takes 8, 4, 2, 1 waves per row


# ---- the dispatch, restated from agg.hip (the CPU test asserts that every path is run) ------------------------------
def fast_shape(heads, c):
    """gat_fast_shape: (V float4 chunks per lane, lanes per head, chunk rows per head), or None"""
    hc = heads * c
    if c % 4 or hc % 4:
        return None
    chunks = hc // 4
    v = (chunks + 63) // 64
    if v not in (1, 2, 4):
        return None
    if c % 256 == 0:
        return (v, 64, c // 256) if chunks % 64 == 0 else None
    gl = c // 4
    if gl > 64 or gl & (gl - 1):
        return None
    return v, gl, 1


def _msg_fits(heads, c, de):
    g = fast_shape(heads, c)
    return g is not None and de <= GAT_ZR * g[1] and (heads * c // 4) % 64 == 0


def forward_path(heads, c, concat, de=0, msg=False, aligned=True):
    """launch_gat_fast: "fast" or "generic" """
    if not (concat or heads == 1) or fast_shape(heads, c) is None or not aligned:
        return "generic"
    return "fast" if not msg or _msg_fits(heads, c, de) else "generic"


def backward_supported(heads, c, de=0, msg=False, aligned=True):
    return fast_shape(heads, c) is not None and aligned and (not msg or _msg_fits(heads, c, de))


def backward_wpr(cap, msg=False):
    return 1 if msg or cap >= 32768 else 2 if cap >= 8192 else 4 if cap >= 2048 else 8


def heavy_slices(m):
    """gat_gather_heavy_kernel: (edges per wave, waves with a non-empty slice)"""
    per = ((m + HEAVY_WAVES - 1) // HEAVY_WAVES + 3) & ~3
    return per, min(HEAVY_WAVES, (m + per - 1) // per)


# ---- graphs (CSR by destination, CPU int64) -------------------------------------------------------------------------
def _others(g, i, n, hi):
    """n sources in [0, hi) that are not i"""
    r = torch.randint(0, hi - 1, (n,), generator=g)
    return r + (r >= i)


@functools.lru_cache(None)
def _base_rows():
    """-> (rows, index of every special row by name); the special rows sit at i % 3 != 1, which no window shortens"""
    g = torch.Generator().manual_seed(41)
    specs = [("deg%d" % d, d) for d in LIST_DEGREES] + [("self_only", 0), ("self_twice", 0), ("dup", 0)] + \
            [("hub%d" % m, m) for m in HUBS] + [("hub_head", 0), ("hub_mid", 0), ("hub_head2", 0)]
    free = [i for i in range(N_ROWS) if i % 3 != 1]
    rows, where = [None] * N_ROWS, {}
    for (name, m), i in zip(specs, free):
        where[name] = i
        me = torch.tensor([i])
        if name == "self_only":
            rows[i] = me
        elif name == "self_twice":
            o = _others(g, i, 4, N_READ)
            rows[i] = torch.cat([o[:1], me, o[1:3], me, o[3:]])
        elif name == "dup":
            o = torch.randperm(N_READ - 1, generator=g)[:4]
            o = o + (o >= i)
            rows[i] = torch.cat([o, o[1:2]])
        elif name == "hub_head":  # wave 0's slice of 12 holds self loops only
            rows[i] = torch.cat([me.repeat(12), _others(g, i, 128, N_READ)])
        elif name == "hub_head2":  # the slices of wave 0 and wave 1: the merge starts from two empty states
            rows[i] = torch.cat([me.repeat(24), _others(g, i, 116, N_READ)])
        elif name == "hub_mid":  # the sixth slice of 12 (entries 60..71) holds self loops only
            o = _others(g, i, 128, N_READ)
            rows[i] = torch.cat([o[:60], me.repeat(12), o[60:]])
        else:
            rows[i] = _others(g, i, m, N_READ)
    for i in range(N_ROWS):
        if rows[i] is None:  # the rest: degree 0..6 (the rows a window shortens: 1..6)
            rows[i] = _others(g, i, max(int(torch.randint(0, 7, (1,), generator=g)), int(i % 3 == 1)), N_READ)
    return rows, where


def _graph_of(rows, window, n_live, n_nodes, cap):
    """with `window` every row i % 3 == 1 ends 1 or 2 entries early and the skipped entries name the NaN node.  pos / src
    / dst: the col positions of the live rows that count (inside the window, no self loop), their sources and rows"""
    deg = torch.tensor([r.numel() for r in rows])
    rp = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(deg, 0)])
    col, rowend = torch.cat(rows).clone(), rp[1:].clone()
    if window:
        short = torch.arange(len(rows)) % 3 == 1
        skip = torch.minimum(deg, 1 + (torch.arange(len(rows)) // 3) % 2) * short
        rowend = rowend - skip
        p = torch.arange(col.numel())
        row_of = torch.repeat_interleave(torch.arange(len(rows)), deg)
        col[p >= rowend[row_of]] = n_nodes - 1
    p = torch.arange(col.numel())
    row_of = torch.repeat_interleave(torch.arange(len(rows)), deg)
    used = (p < rowend[row_of]) & (row_of < n_live)
    keep = used & (col != row_of)
    pos = p[keep]
    cnt = torch.zeros(n_live, dtype=torch.int64).index_add_(0, row_of[keep], torch.ones_like(pos))
    return types.SimpleNamespace(rp=rp, rowend=rowend, col=col, window=window, m=rowend - rp[:-1], pos=pos, src=col[pos],
                                 dst=row_of[pos], cnt=cnt, raw=p[used], raw_dst=row_of[used], n_rows=len(rows),
                                 n_live=n_live, n_nodes=n_nodes, cap=cap, unused=~keep)


@functools.lru_cache(None)
def rows_graph(window):
    return _graph_of(_base_rows()[0], window, N_LIVE, N_NODES, CAP)


@functools.lru_cache(None)
def long_graph(n):
    """n rows of degree 0..6 over n sources (self loops as they fall), n - 5 live, node n a row of NaN"""
    g = torch.Generator().manual_seed(n)
    deg = torch.randint(0, 7, (n,), generator=g)
    col = torch.randint(0, n, (int(deg.sum()),), generator=g)
    return _graph_of(list(torch.split(col, deg.tolist())), False, n - 5, n + 1, n + 8)


# ---- the reference (dtype follows the inputs) -----------------------------------------------------------------------
def gat_ref(gr, heads, c, h, a_src, a_dst, a_edge=None, ea=None, w_msg=None):
    """-> (out [n_live, H*C] before bias and activation, z [n_live, H, De] | None, the logits before leaky_relu of the
    edges gr.pos and of the n_live self loops).  a_edge [positions, H] and ea [positions, De] are indexed at gr.pos only"""
    n, dt = gr.n_live, h.dtype
    loops = torch.arange(n)
    src, dst = torch.cat([gr.src, loops]), torch.cat([gr.dst, loops])
    inv_cnt = (1.0 / gr.cnt.clamp(min=1).to(dt))[:, None]
    pre = a_src[src] + a_dst[dst]
    if a_edge is not None:
        ae = a_edge[gr.pos]
        pre = pre + torch.cat([ae, torch.zeros(n, heads, dtype=dt).index_add(0, gr.dst, ae) * inv_cnt])
    e = torch.nn.functional.leaky_relu(pre, SLOPE)
    emax = torch.full((n, heads), float("-inf"), dtype=dt).scatter_reduce(0, dst[:, None].expand(-1, heads), e.detach(),
                                                                          reduce="amax")
    ex = torch.exp(e - emax[dst])
    alpha = ex / (torch.zeros(n, heads, dtype=dt).index_add(0, dst, ex)[dst] + 1e-16)
    out = torch.zeros(n, heads, c, dtype=dt).index_add(0, dst, h[src].view(-1, heads, c) * alpha[:, :, None])
    z = None
    if ea is not None:
        ek = ea[gr.pos]
        ek = torch.cat([ek, torch.zeros(n, ek.shape[1], dtype=dt).index_add(0, gr.dst, ek) * inv_cnt])
        z = torch.zeros(n, heads, ek.shape[1], dtype=dt).index_add(0, dst, alpha[:, :, None] * ek[:, None, :])
        if w_msg is not None:
            out = out + torch.einsum("nhk,hck->nhc", z, w_msg.view(heads, c, -1))
    return out.reshape(n, heads * c), z, pre


def _alphas(h, att, heads, c):
    return (h.view(-1, heads, c) * att.view(1, heads, c)).sum(-1)


def _grid(g, den, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double() / den


def _free(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32).double()


@functools.lru_cache(None)
def gat_inputs(kind, heads, c, de, msg, scale):
    """the inputs of a shape as float64, shared by the packed and the windowed graph (kind "rows") or of one long graph
    (kind = its row count); rows of h from the NaN node on are NaN"""
    graphs = [rows_graph(False), rows_graph(True)] if kind == "rows" else [long_graph(kind)]
    n_nodes, cap, ce = graphs[0].n_nodes, graphs[0].cap, graphs[0].col.numel()
    g = torch.Generator().manual_seed(1000 * heads + 7 * c + 13 * de + msg + 100 * scale)
    hc = heads * c
    t = types.SimpleNamespace(heads=heads, c=c, de=de, msg=msg, scale=scale, redrawn=0)
    t.h = _grid(g, 64, -128, 128, cap, hc)
    t.att_src, t.att_dst = scale * _grid(g, 8, -8, 8, hc), scale * _grid(g, 8, -8, 8, hc)
    t.ea = t.v = t.w_msg = None
    if de:
        t.ea, t.v = _grid(g, 8, -8, 8, ce, de), scale * _grid(g, 8, -8, 8, heads, de)
        for _ in range(100):  # |pre_self| >= 1e-3 (float64) for every live row and head: a fresh h row where it is not
            bad = torch.zeros(cap, dtype=torch.bool)
            for gr in graphs:
                bad[:gr.n_live] |= (self_logits(t, gr).abs() < 1e-3).any(1)
            if not bool(bad.any()):
                break
            t.h[bad] = _grid(g, 64, -128, 128, int(bad.sum()), hc)
            t.redrawn += int(bad.sum())
    if msg:
        t.w_msg = _free(g, hc, de)
    t.h[n_nodes - 1:] = float("nan")
    t.bias = {True: _free(g, hc), False: _free(g, c)}  # by concat
    t.dout = _free(g, cap, hc)
    t.dout[torch.arange(cap) % 7 == 3] = 0.0
    t.zero_rows = (torch.arange(graphs[0].n_live) % 7 == 3)
    return t


def self_logits(t, gr):
    """the self loops' logits before leaky_relu, float64: [n_live, H]"""
    n = gr.n_live
    pre = (_alphas(t.h, t.att_src, t.heads, t.c) + _alphas(t.h, t.att_dst, t.heads, t.c))[:n]
    if t.de:
        ae = (t.ea @ t.v.T)[gr.pos]
        pre = pre + torch.zeros(n, t.heads, dtype=ae.dtype).index_add(0, gr.dst, ae) / gr.cnt.clamp(min=1)[:, None]
    return pre


def _leaves(t, dt):
    h = t.h.to(dt)
    a_src, a_dst = _alphas(h, t.att_src.to(dt), t.heads, t.c), _alphas(h, t.att_dst.to(dt), t.heads, t.c)
    a_edge = t.ea.to(dt) @ t.v.to(dt).T if t.de else None
    return h, a_src, a_dst, a_edge, (t.ea.to(dt) if t.de else None), (t.w_msg.to(dt) if t.msg else None)


def forward_ref(t, gr, concat, mode, dt):
    """mode 0: no bias; 1: bias; 2: bias and relu"""
    out, _, pre = gat_ref(gr, t.heads, t.c, *_leaves(t, dt))
    if not concat:
        out = out.view(-1, t.heads, t.c).mean(1)
    if mode:
        out = out + t.bias[bool(concat)].to(dt)
    return (torch.relu(out) if mode == 2 else out), pre


def backward_ref(t, gr, dt):
    """-> out_pre, and what gigl_gat_aggregate_backward returns for dout = t.dout: dh [n_nodes, H*C] through the messages
    only, d_alpha_src / d_alpha_dst [n_nodes, H], d_alpha_edge [positions, H] (0 where no edge counts), z [n_live, H, De]
    (0 for the rows whose dout is zero)"""
    h, a_src, a_dst, a_edge, ea, w_msg = _leaves(t, dt)
    n_nodes = gr.n_nodes
    h = torch.nan_to_num(h[:n_nodes]).requires_grad_(True)  # (the NaN node is read by nobody; a NaN leaf has a NaN gradient)
    a_src = torch.nan_to_num(a_src[:n_nodes]).requires_grad_(True)
    a_dst = torch.nan_to_num(a_dst[:n_nodes]).requires_grad_(True)
    leaves = [h, a_src, a_dst]
    if a_edge is not None:
        a_edge = a_edge.requires_grad_(True)
        leaves.append(a_edge)
    out, z, _ = gat_ref(gr, t.heads, t.c, h, a_src, a_dst, a_edge, ea if t.msg else None, w_msg)
    grads = torch.autograd.grad((out * t.dout[:gr.n_live].to(dt)).sum(), leaves)
    r = {"out_pre": out.detach(), "dh": grads[0], "d_alpha_src": grads[1], "d_alpha_dst": grads[2]}
    if a_edge is not None:
        r["d_alpha_edge"] = grads[3]
    if t.msg:
        r["z_out"] = z.detach().masked_fill(t.zero_rows[:, None, None], 0.0)
    return r


def _err(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max()) if a.numel() else 0.0


@functools.lru_cache(None)
def forward_case(kind, heads, c, concat, de, msg, scale, window, mode):
    t = gat_inputs(kind, heads, c, de, msg, scale)
    gr = rows_graph(window) if kind == "rows" else long_graph(kind)
    want, _ = forward_ref(t, gr, concat, mode, torch.float64)
    e32 = _err(forward_ref(t, gr, concat, mode, torch.float32)[0], want) if kind == "rows" else 0.0
    return t, gr, want, e32


@functools.lru_cache(None)
def backward_case(kind, heads, c, de, msg, scale, window):
    t = gat_inputs(kind, heads, c, de, msg, scale)
    gr = rows_graph(window) if kind == "rows" else long_graph(kind)
    want = backward_ref(t, gr, torch.float64)
    lo = backward_ref(t, gr, torch.float32) if kind == "rows" else want
    return t, gr, want, {k: _err(lo[k], want[k]) for k in want}


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


# ---- the cases: (heads, channels, concat, De, message term, scale of att_*) -----------------------------------------
FAST = {1: [(1, 4), (3, 4), (1, 8), (3, 16), (4, 64), (2, 128), (1, 256)],
        2: [(5, 64), (3, 128), (4, 128), (2, 256), (1, 512)],
        4: [(8, 128), (7, 128), (4, 256), (2, 512), (1, 1024)]}
GENERIC = [(1, 6), (3, 7), (2, 12), (1, 100), (1, 260), (3, 256), (1, 768), (2, 1024)]
CONCAT0 = [(4, 16), (2, 6), (1, 64)]
PLAIN = [(h, c, 1, 0, False, 1) for v in (1, 2, 4) for h, c in FAST[v]] + [(h, c, 1, 0, False, 1) for h, c in GENERIC] + \
        [(h, c, 0, 0, False, 1) for h, c in CONCAT0]
EDGE_SHAPES = [(3, 4, 1), (4, 64, 1), (3, 128, 1), (1, 512, 1), (8, 128, 1), (2, 12, 1), (3, 256, 1), (4, 16, 0)]
EDGE = [(h, c, cc, de, False, 1) for h, c, cc in EDGE_SHAPES for de in (1, 3, 256)]
MSG_TABLE = [(4, 64, 1, "fast"), (4, 64, 5, "fast"), (4, 64, 16, "fast"), (4, 64, 17, "fast"), (4, 64, 64, "fast"),
             (4, 64, 65, "generic"), (1, 256, 3, "fast"), (1, 256, 64, "fast"), (1, 256, 65, "fast"),
             (1, 256, 256, "fast"), (8, 32, 32, "fast"), (8, 32, 33, "generic"), (2, 512, 70, "fast"),
             (4, 16, 5, "generic")]
MSG = [(h, c, 1, de, True, 1) for h, c, de, _ in MSG_TABLE]
EDGE_GENERIC_MSGLESS = [(4, 64, 1, 5, False, 1)]  # gat_edge_gather_kernel without W_msg on a fast shape: misaligned h only
LARGE = [(3, 128, 1, 0, False, 4), (2, 16, 1, 256, False, 4), (8, 128, 1, 3, False, 4), (4, 64, 1, 16, True, 4)]
CASES = PLAIN + EDGE + MSG + LARGE
SWEEP = [(4, 64, 1, 0, False, 1), (3, 128, 1, 3, False, 1), (8, 128, 1, 3, False, 4)]  # one shape per V, over CAPS
MSG_CAPS = [(4, 64, 1, 17, True, 1), (2, 512, 1, 70, True, 1), (4, 64, 1, 16, True, 4)]  # over CAP and 2048: 1 wave per row
LONG = [(16400, (3, 7, 1, 0, False, 1)), (16400, (2, 12, 1, 3, False, 1)), (16400, (2, 6, 0, 0, False, 1)),
        (20000, (2, 16, 1, 0, False, 1)), (33000, (2, 16, 1, 0, False, 1)), (33000, (2, 16, 1, 3, False, 1))]


def _id(case):
    h, c, concat, de, msg, scale = case
    return f"{h}x{c}" + ("" if concat else "-mean") + (f"-De{de}" if de else "") + ("-msg" if msg else "") + \
        (f"-x{scale}" if scale != 1 else "")


def _mode(case):
    return CASES.index(case) % 3 if case in CASES else 2


def has_backward(case):
    return bool(case[2]) or case[0] == 1  # the backward is that of concatenated heads (or of one head)


# ---- device side ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _i32(t):
    return t.to(torch.int32).cuda()


def _f32(t):
    return None if t is None else t.float().cuda()


def _count(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def _dev_graph(gr, cap=None):
    return types.SimpleNamespace(nodes=torch.empty(cap or gr.cap, dtype=torch.int32, device="cuda"),
                                 rowptr=_i32(gr.rp[:-1]), rowend=_i32(gr.rowend), col=_i32(gr.col),
                                 meta=torch.tensor([gr.n_nodes, gr.col.numel()], dtype=torch.int32, device="cuda"))


def _edge_attr(t, gr):
    """the attributes as the kernel gets them: NaN at the positions that do not count"""
    if not t.de:
        return None
    ea = t.ea.clone()
    ea[gr.unused] = float("nan")
    return _f32(ea)


def run_forward(eng, t, gr, concat, mode, cap=None, h=None):
    cap = cap or gr.cap
    bias = _f32(t.bias[bool(concat)]) if mode else None
    out = torch.full((cap, t.heads * t.c if concat else t.c), SENTINEL, dtype=torch.float32, device="cuda")
    eng.gat_aggregate(_f32(t.h) if h is None else h, _f32(t.att_src), _f32(t.att_dst), t.heads, t.c, _dev_graph(gr, cap),
                      _count(gr.n_live), bias, concat=bool(concat), negative_slope=SLOPE, act=int(mode == 2), out=out,
                      edge_attr=_edge_attr(t, gr), att_edge_folded=_f32(t.v), w_edge_msg=_f32(t.w_msg))
    return out.cpu()


def check_forward(label, got, want, e32, gr):
    check(label, "out", got[:gr.n_live], want, e32)
    assert bool((got[gr.n_live:] == SENTINEL).all()), f"{label}: rows past *n_rows_dev were written"


def _backward_args(t, gr, want, cap):
    """(out_pre, dout, u_msg): NaN past the live rows, which nothing may read"""
    n, hc = gr.n_live, t.heads * t.c
    out_pre = torch.full((gr.cap, hc), float("nan"), dtype=torch.float64)
    out_pre[:n] = want["out_pre"]
    dout = t.dout.clone()
    dout[n:] = float("nan")
    u = None
    if t.msg:
        u = torch.full((cap, t.heads, t.de), float("nan"), dtype=torch.float64)
        u[:n] = torch.einsum("nhc,hck->nhk", t.dout[:n].view(n, t.heads, t.c), t.w_msg.view(t.heads, t.c, t.de))
    return _f32(out_pre), _f32(dout), _f32(u)


def run_backward(eng, t, gr, want, cap=None, h=None):
    cap = cap or gr.cap
    out_pre, dout, u = _backward_args(t, gr, want, cap)
    return eng.gat_aggregate_backward(_f32(t.h) if h is None else h, _f32(t.att_src), _f32(t.att_dst), t.heads, t.c,
                                      _dev_graph(gr, cap), _count(gr.n_live), out_pre, dout, negative_slope=SLOPE,
                                      edge_attr=_edge_attr(t, gr), att_edge_folded=_f32(t.v), u_msg=u)


def check_backward(label, got, t, gr, want, e32):
    dh, ds, dd, dae, z = (None if x is None else x.cpu() for x in got)
    nn = gr.n_nodes
    for name, x in (("dh", dh), ("d_alpha_src", ds), ("d_alpha_dst", dd)):
        check(label, name, x[:nn], want[name], e32[name], grad=True)
        assert not bool(x[nn:].any()), f"{label} {name}: rows past the live nodes were written"
        read = torch.zeros(nn, dtype=torch.bool)
        read[gr.src] = True
        read[:gr.n_live] = True
        assert not bool(x[:nn][~read].any()), f"{label} {name}: a node nobody reads has a gradient"
    if gr.n_rows == N_ROWS:
        assert not bool(read[N_READ:].any())
    assert not bool(dd[gr.n_live:].any()) and not bool(dd[:gr.n_live][t.zero_rows].any())
    assert (dae is None) == (t.de == 0) and (z is None) == (not t.msg)
    if dae is not None:
        check(label, "d_alpha_edge", dae, want["d_alpha_edge"], e32["d_alpha_edge"], grad=True)
        assert not bool(dae[gr.unused].any()), f"{label}: d_alpha_edge at a position that does not count"
        assert not bool(dae[gr.pos[t.zero_rows[gr.dst]]].any()), f"{label}: d_alpha_edge of a row whose dout is zero"
    if z is not None:
        check(label, "z_out", z[:gr.n_live], want["z_out"], e32["z_out"], grad=True)
        assert not bool(z[gr.n_live:].any()) and not bool(z[:gr.n_live][t.zero_rows].any()), f"{label}: z_out of a skipped row"


def check_backward_refused(eng, t, gr, label, h=None):
    """the wrapper raises GIGL_E_UNSUPPORTED; called on buffers of our own, the entry point writes nothing"""
    import ctypes as C

    from gigl_amd._lib import GiglError
    want = {"out_pre": torch.zeros(gr.n_live, t.heads * t.c, dtype=torch.float64)}
    with pytest.raises(GiglError) as info:
        run_backward(eng, t, gr, want, h=h)
    assert info.value.code == E_UNSUPPORTED, label
    cap, ce, hc = gr.cap, gr.col.numel(), t.heads * t.c
    out_pre, dout, u = _backward_args(t, gr, want, cap)
    full = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device="cuda")
    outs = [full(cap, hc), full(cap, t.heads), full(cap, t.heads), full(ce, t.heads) if t.de else None,
            full(cap, t.heads, t.de) if t.msg else None]
    scratch = torch.empty(2 * cap * t.heads + ce * t.heads, dtype=torch.float32, device="cuda")
    dg, ea, nr = _dev_graph(gr), _edge_attr(t, gr), _count(gr.n_live)
    hh, a_s, a_d, v = (_f32(t.h) if h is None else h), _f32(t.att_src), _f32(t.att_dst), _f32(t.v)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    rc = eng._lib.gigl_gat_aggregate_backward(
        eng._ctx, p(hh), p(a_s), p(a_d), t.heads, t.c, SLOPE, p(dg.rowptr), p(dg.rowend), p(dg.col), p(dg.meta), cap,
        p(nr), cap, p(out_pre), p(dout), p(ea), t.de, ce, p(v), p(scratch), *[p(x) for x in outs[:4]], p(u), p(outs[4]))
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED, (label, rc)
    assert all(bool((x == SENTINEL).all()) for x in outs if x is not None), f"{label}: a refused backward wrote its outputs"


# ---- 1. forward -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gat_forward(eng, case, window):
    heads, c, concat, de, msg, scale = case
    mode = _mode(case)
    t, gr, want, e32 = forward_case("rows", *case, window, mode)
    label = f"fwd {_id(case)} {forward_path(heads, c, concat, de, msg)} {fast_shape(heads, c)} window={window} mode={mode}"
    check_forward(label, run_forward(eng, t, gr, concat, mode), want, e32, gr)


@gpu
@pytest.mark.parametrize("case", [PLAIN[4], EDGE_GENERIC_MSGLESS[0], MSG[2]], ids=_id)
def test_gat_misaligned_rows_take_the_generic_kernels(eng, case):
    """h at a 4-byte offset into a larger buffer: contiguous, not 16-byte aligned — launch_gat_fast declines, the generic
    kernels give the same answer, the backward refuses"""
    heads, c, concat, de, msg, scale = case
    t, gr, want, e32 = forward_case("rows", *case, True, 2)
    buf = torch.zeros(gr.cap * heads * c + 4, dtype=torch.float32, device="cuda")
    h = buf[1:1 + gr.cap * heads * c].view(gr.cap, heads * c)
    h.copy_(_f32(t.h))
    assert h.is_contiguous() and h.data_ptr() % 16 == 4
    assert forward_path(heads, c, concat, de, msg) == "fast"
    assert forward_path(heads, c, concat, de, msg, aligned=False) == "generic"
    label = f"fwd {_id(case)} misaligned"
    check_forward(label, run_forward(eng, t, gr, concat, 2, h=h), want, e32, gr)
    check_backward_refused(eng, t, gr, label, h=h)


@gpu
def test_gat_edge_dim_beyond_256_is_refused(eng):
    from gigl_amd._lib import GiglError
    gr = rows_graph(False)
    t = gat_inputs("rows", 4, 64, 3, False, 1)
    wide = types.SimpleNamespace(**vars(t))
    g = torch.Generator().manual_seed(5)
    wide.de = MAX_EDGE_DIM + 1
    wide.ea, wide.v = _grid(g, 8, -8, 8, gr.col.numel(), wide.de), _grid(g, 8, -8, 8, 4, wide.de)
    out = torch.full((gr.cap, 256), SENTINEL, dtype=torch.float32, device="cuda")
    with pytest.raises(GiglError):
        eng.gat_aggregate(_f32(wide.h), _f32(wide.att_src), _f32(wide.att_dst), 4, 64, _dev_graph(gr), _count(gr.n_live), None,
                          out=out, edge_attr=_edge_attr(wide, gr), att_edge_folded=_f32(wide.v))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused forward wrote its output"


# ---- 2. backward ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("case", [x for x in CASES if has_backward(x)], ids=_id)
def test_gat_backward(eng, case, window):
    heads, c, concat, de, msg, scale = case
    label = f"bwd {_id(case)} {fast_shape(heads, c)} window={window} wpr={backward_wpr(CAP, msg)}"
    if not backward_supported(heads, c, de, msg):
        t = gat_inputs("rows", heads, c, de, msg, scale)
        check_backward_refused(eng, t, rows_graph(window), label)
        return
    t, gr, want, e32 = backward_case("rows", heads, c, de, msg, scale, window)
    check_backward(label, run_backward(eng, t, gr, want), t, gr, want, e32)


@gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("case", SWEEP, ids=_id)
def test_gat_backward_waves_per_row(eng, case, cap):
    """only the capacity grows: 8, 4, 2, 1 waves share a row, and each result meets the reference"""
    heads, c, concat, de, msg, scale = case
    t, gr, want, e32 = backward_case("rows", heads, c, de, msg, scale, True)
    label = f"bwd {_id(case)} {fast_shape(heads, c)} cap={cap} wpr={backward_wpr(cap)}"
    check_backward(label, run_backward(eng, t, gr, want, cap=cap), t, gr, want, e32)


@gpu
@pytest.mark.parametrize("cap", CAPS[:2])
@pytest.mark.parametrize("case", MSG_CAPS, ids=_id)
def test_gat_backward_message_term_keeps_one_wave_per_row(eng, case, cap):
    heads, c, concat, de, msg, scale = case
    t, gr, want, e32 = backward_case("rows", heads, c, de, msg, scale, True)
    label = f"bwd {_id(case)} {fast_shape(heads, c)} cap={cap} wpr={backward_wpr(cap, True)}"
    check_backward(label, run_backward(eng, t, gr, want, cap=cap), t, gr, want, e32)
    check_forward(label, run_forward(eng, t, gr, 1, 0, cap=cap), want["out_pre"], e32["out_pre"], gr)


# ---- 3. long graphs: a second pass of every capped grid (project tolerance only) ------------------------------------
@gpu
@pytest.mark.parametrize("n,case", LONG, ids=lambda x: _id(x) if isinstance(x, tuple) else str(x))
def test_gat_long_graph(eng, n, case):
    heads, c, concat, de, msg, scale = case
    t, gr, want, e32 = forward_case(n, *case, False, 2)
    label = f"long {n} {_id(case)} {forward_path(heads, c, concat, de, msg)}"
    check_forward(label, run_forward(eng, t, gr, concat, 2), want, e32, gr)
    if backward_supported(heads, c, de, msg) and has_backward(case):
        t, gr, want, e32 = backward_case(n, heads, c, de, msg, scale, False)
        check_backward(f"{label} wpr={backward_wpr(gr.cap)}", run_backward(eng, t, gr, want), t, gr, want, e32)


# ---- 4. the dense tail ----------------------------------------------------------------------------------------------
EPILOGUE_ROWS = [(1, 1), (2, 1), (511, 509), (513, 510), (1200, 1100)]  # (capacity: the grid is min(capacity, 512); live)
EPILOGUE_SHAPES = [(1, 4), (3, 20), (3, 128), (4, 256)]  # H*C = 4, 60 (64 threads), 384, 1024


def epilogue_inputs(cap, live, heads, c):
    g = torch.Generator().manual_seed(10 * cap + heads * c)
    hc = heads * c
    t = types.SimpleNamespace(dh=_free(g, cap, hc), xw=_free(g, cap, hc), ds=_free(g, cap, heads), dd=_free(g, cap, heads),
                              att_src=_free(g, hc), att_dst=_free(g, hc))
    zero = torch.rand(cap, heads, generator=g) < 1 / 3  # (row, head) pairs that are zero in both: not read
    t.ds[zero], t.dd[zero] = 0.0, 0.0
    for x in (t.xw, t.ds, t.dd):
        x[live:] = float("nan")
    return t


def epilogue_ref(t, live, c, dt):
    ds, dd = t.ds[:live].to(dt).repeat_interleave(c, 1), t.dd[:live].to(dt).repeat_interleave(c, 1)
    xw = t.xw[:live].to(dt)
    return t.dh[:live].to(dt) + ds * t.att_src.to(dt) + dd * t.att_dst.to(dt), (ds * xw).sum(0), (dd * xw).sum(0)


@gpu
@pytest.mark.parametrize("heads,c", EPILOGUE_SHAPES)
@pytest.mark.parametrize("cap,live", EPILOGUE_ROWS)
def test_gat_backward_epilogue(eng, cap, live, heads, c):
    t = epilogue_inputs(cap, live, heads, c)
    want = epilogue_ref(t, live, c, torch.float64)
    lo = epilogue_ref(t, live, c, torch.float32)
    dh = _f32(t.dh)
    got, g_s, g_d = eng.gat_backward_epilogue(dh, _f32(t.ds), _f32(t.dd), _f32(t.xw), _f32(t.att_src), _f32(t.att_dst),
                                              heads, c, _count(live))
    assert got.data_ptr() == dh.data_ptr()
    label = f"epilogue {cap}/{live} x {heads}x{c}"
    check(label, "dxw", got[:live], want[0], _err(lo[0], want[0]))
    assert torch.equal(got[live:].cpu(), t.dh[live:].float()), f"{label}: rows past *n_nodes_dev were touched"
    check(label, "d_att_src", g_s, want[1], _err(lo[1], want[1]), grad=True)
    check(label, "d_att_dst", g_d, want[2], _err(lo[2], want[2]), grad=True)


@gpu
def test_gat_backward_epilogue_refuses_more_than_1024_columns(eng):
    from gigl_amd._lib import GiglError
    t = epilogue_inputs(8, 8, 257, 4)
    dh = _f32(t.dh)
    with pytest.raises(GiglError) as info:
        eng.gat_backward_epilogue(dh, _f32(t.ds), _f32(t.dd), _f32(t.xw), _f32(t.att_src), _f32(t.att_dst), 257, 4, _count(8))
    torch.cuda.synchronize()
    assert info.value.code == E_UNSUPPORTED and torch.equal(dh.cpu(), t.dh.float())


# ---- CPU: the formula against gnn_ref.gat_conv (float64), the inputs' conditions, the graph, the coverage ----------
def test_references_inputs_and_coverage():
    rows, where = _base_rows()
    packed, win = rows_graph(False), rows_graph(True)
    # the graph delivers what the cases rely on
    assert N_ROWS % 32 == 3 and N_LIVE == N_ROWS - 5 and N_NODES == N_ROWS + 1 and CAP > N_NODES
    assert all(i % 3 != 1 and i < N_LIVE for i in where.values()) and len(set(where.values())) == len(where)
    for gr in (packed, win):
        assert [int(gr.m[where["deg%d" % d]]) for d in LIST_DEGREES] == LIST_DEGREES
        assert [int(gr.cnt[where["deg%d" % d]]) for d in LIST_DEGREES] == LIST_DEGREES
        assert int(gr.m[where["self_only"]]) == 1 and int(gr.cnt[where["self_only"]]) == 0
        assert int(gr.m[where["self_twice"]]) == 6 and int(gr.cnt[where["self_twice"]]) == 4
        assert [int(gr.m[where["hub%d" % m]]) for m in HUBS] == HUBS
        assert int(gr.col.max()) <= NAN_NODE and int(gr.src.max()) < N_READ and gr.col.numel() == packed.col.numel()
        assert int((gr.cnt == 0).sum()) >= 2
        assert torch.equal(gr.unused, ~torch.isin(torch.arange(gr.col.numel()), gr.pos))
    assert max(LIST_DEGREES) == HEAVY_MIN - 1 and min(HUBS) == HEAVY_MIN
    i = where["dup"]
    dup = rows[i]
    assert dup.numel() - dup.unique().numel() == 1 and i not in dup.tolist()
    assert [heavy_slices(m) for m in HUBS] == [(8, 16), (12, 11), (12, 15), (12, 16), (20, 15), (16, 16)]
    assert 192 == 16 * 12 and 300 == 15 * 20 and 250 % 16 == 10  # exactly full; fifteen full and one empty; ragged
    for name, lo, k in (("hub_head", 0, 12), ("hub_mid", 60, 12), ("hub_head2", 0, 24)):
        r, i = rows[where[name]], where[name]
        assert r.numel() == 140 and heavy_slices(140) == (12, 12) and lo % 12 == 0
        assert bool((r[lo:lo + k] == i).all()) and int((r == i).sum()) == k and int(packed.cnt[i]) == 140 - k
    assert bool((packed.rp[1:] == packed.rowend).all())
    short = win.rp[1:] - win.rowend
    assert int((short > 0).sum()) == N_ROWS // 3 and set(short[short > 0].tolist()) == {1, 2}
    row_of = torch.repeat_interleave(torch.arange(N_ROWS), win.rp[1:] - win.rp[:-1])
    skipped = win.col[torch.arange(win.col.numel()) >= win.rowend[row_of]]
    assert skipped.numel() == int(short.sum()) and bool((skipped == NAN_NODE).all())
    assert int((win.col == NAN_NODE).sum()) == skipped.numel()
    for n in (16400, 20000, 33000):
        gr = long_graph(n)
        assert 2.9 < gr.col.numel() / n < 3.1 and int((gr.m == 0).sum()) > 100
        assert int((gr.col == torch.repeat_interleave(torch.arange(n), gr.m)).sum()) > 0  # self loops among them

    # the formula against gnn_ref.gat_conv: identity weight, folded edge vector, both concat, with and without W_msg
    for gr in (packed, win):
        for heads, c, de, msg in ((2, 6, 0, False), (3, 4, 5, False), (3, 4, 5, True), (1, 8, 3, True)):
            t = gat_inputs("rows", heads, c, de, msg, 1)
            hc, n = heads * c, gr.n_live
            eye = torch.eye(hc, dtype=torch.float64)
            h0 = torch.nan_to_num(t.h[:N_NODES])
            ei = torch.stack([gr.col[gr.raw], gr.raw_dst])  # the live rows' windows, self loops included
            assert int((ei[0] == ei[1]).sum()) >= 50
            w_edge = att_edge = None
            if de:
                w_edge, att_edge = torch.zeros(hc, de, dtype=torch.float64), torch.zeros(heads, c, dtype=torch.float64)
                w_edge[torch.arange(heads) * c], att_edge[:, 0] = t.v, 1.0
            w = _free(torch.Generator().manual_seed(1), n, hc)
            for concat in (False, True):
                wo = w if concat else w[:, :c]
                x = h0.clone().requires_grad_(True)
                conv = gnn_ref.gat_conv(x, ei, eye, t.att_src, t.att_dst, None, heads, concat, SLOPE,
                                        t.ea[gr.raw] if de else None, w_edge, att_edge, t.w_msg)[:n]
                g_conv = torch.autograd.grad((conv * wo).sum(), x)[0]
                hh = h0.clone().requires_grad_(True)
                a_s, a_d = _alphas(hh, t.att_src, heads, c), _alphas(hh, t.att_dst, heads, c)
                out, _, _ = gat_ref(gr, heads, c, hh, a_s, a_d, t.ea @ t.v.T if de else None, t.ea if msg else None, t.w_msg)
                out = out if concat else out.view(n, heads, c).mean(1)
                assert _err(out, conv) <= 1e-12, (heads, c, de, msg, concat)
                assert _err(torch.autograd.grad((out * wo).sum(), hh)[0], g_conv) <= 1e-12
            # the leaves' gradients add up to the whole one: dh + d_alpha_src (x) att_src + d_alpha_dst (x) att_dst
            saved, t.dout = t.dout, torch.cat([w, torch.zeros(CAP - n, hc, dtype=torch.float64)])
            r = backward_ref(t, gr, torch.float64)
            t.dout = saved
            whole = r["dh"] + r["d_alpha_src"].repeat_interleave(c, 1) * t.att_src + \
                r["d_alpha_dst"].repeat_interleave(c, 1) * t.att_dst
            assert _err(whole, g_conv) <= 1e-12
            if msg:  # z_out: d W_msg = sum_i dout_i (x) z_i
                wm = t.w_msg.clone().requires_grad_(True)
                o2 = gnn_ref.gat_conv(h0, ei, eye, t.att_src, t.att_dst, None, heads, True, SLOPE,
                                      t.ea[gr.raw], w_edge, att_edge, wm)[:n]
                z = gat_ref(gr, heads, c, *_leaves(t, torch.float64))[1]
                dw = torch.einsum("nhc,nhk->hck", w.view(n, heads, c), z).reshape(hc, de)
                assert _err(dw, torch.autograd.grad((o2 * w).sum(), wm)[0]) <= 1e-11

    # the inputs: exact scalars in fp32, |pre_self| >= 1e-3 with edge features, logits of +-50 on the hub rows
    hubs = torch.tensor([where["hub%d" % m] for m in HUBS] + [where["hub_head"], where["hub_mid"], where["hub_head2"]])
    for case in CASES + SWEEP + MSG_CAPS + EDGE_GENERIC_MSGLESS:
        heads, c, concat, de, msg, scale = case
        t = gat_inputs("rows", heads, c, de, msg, scale)
        h64 = torch.nan_to_num(t.h)
        for att in (t.att_src, t.att_dst):
            a32 = (h64.float().view(-1, heads, c) * att.float().view(1, heads, c)).flip(-1).cumsum(-1)[..., -1]
            assert torch.equal(a32.double(), _alphas(h64, att, heads, c)), case
        if de:
            assert torch.equal((t.ea.float() @ t.v.float().T).double(), t.ea @ t.v.T), case
        for gr in (packed, win):
            if de:
                assert float(self_logits(t, gr).abs().min()) >= 1e-3, case
            if scale > 1:
                pre = gat_ref(gr, heads, c, *_leaves(t, torch.float64)[:4])[2][:gr.pos.numel()]
                on_hub = torch.isin(gr.dst, hubs)
                hi, lo = float(pre[on_hub].max()), float(pre[on_hub].min())
                assert hi >= 50 and lo <= -50, (case, hi, lo)
        assert int(t.zero_rows.sum()) >= 25 and not bool(t.dout[:N_LIVE][t.zero_rows].any())
    for n, case in LONG:
        if case[3]:
            assert float(self_logits(gat_inputs(n, *case[:2], *case[3:]), long_graph(n)).abs().min()) >= 1e-3

    # coverage, from the parametrisation and the restated dispatch
    shapes = {v: [fast_shape(h, c) for h, c in FAST[v]] for v in FAST}
    assert all(s is not None and s[0] == v for v in FAST for s in shapes[v])
    partial = lambda h, c: (h * c // 4) % 64 != 0
    for v in (1, 2, 4):  # a full and a partially filled last chunk row for every V
        assert any(not partial(h, c) for h, c in FAST[v]) and any(partial(h, c) for h, c in FAST[v])
    assert partial(5, 64) and partial(3, 128) and partial(7, 128)
    assert fast_shape(5, 64) == (2, 16, 1) and fast_shape(3, 128) == (2, 32, 1) and fast_shape(7, 128) == (4, 32, 1)
    assert any(partial(h, c) for h, c in FAST[1]) and not partial(4, 64) and not partial(2, 128) and not partial(8, 128)
    fast_cases = [x for x in CASES if forward_path(*x[:5]) == "fast"]
    assert {fast_shape(x[0], x[1])[1] for x in fast_cases} >= {1, 2, 4, 8, 16, 32, 64}
    assert {fast_shape(x[0], x[1])[2] for x in fast_cases if has_backward(x)} == {1, 2, 4}
    assert fast_shape(1, 256) == (1, 64, 1) and fast_shape(1, 512) == (2, 64, 2) and fast_shape(2, 512) == (4, 64, 2)
    assert fast_shape(1, 1024) == (4, 64, 4) and fast_shape(8, 128) == (4, 32, 1) and fast_shape(1, 4) == (1, 1, 1)
    assert all(fast_shape(h, c) is None for h, c in GENERIC)
    assert all(forward_path(h, c, 1) == "generic" and not backward_supported(h, c) for h, c in GENERIC)
    assert (3 * 256 // 4 + 63) // 64 == 3 and (768 // 4 + 63) // 64 == 3 and (2 * 1024 // 4 + 63) // 64 == 8
    assert [forward_path(h, c, 0) for h, c in CONCAT0] == ["generic", "generic", "fast"] and fast_shape(4, 16) is not None
    assert {forward_path(h, c, cc, de) for h, c, cc in EDGE_SHAPES for de in (1, 3, 256)} == {"fast", "generic"}
    assert {fast_shape(h, c)[0] for h, c, cc in EDGE_SHAPES if forward_path(h, c, cc, 1) == "fast"} == {1, 2, 4}
    for h, c, de, path in MSG_TABLE:
        assert forward_path(h, c, 1, de, True) == path and backward_supported(h, c, de, True) == (path == "fast"), (h, c, de)
    lim = {(h, c): GAT_ZR * fast_shape(h, c)[1] for h, c, _, _ in MSG_TABLE}
    assert lim[(4, 64)] == 64 and lim[(8, 32)] == 32 and lim[(1, 256)] == MAX_EDGE_DIM and (4 * 16 // 4) % 64 != 0
    assert {(4, 64, 64), (4, 64, 65), (8, 32, 32), (8, 32, 33), (1, 256, 256)} <= {x[:3] for x in MSG_TABLE}
    assert [backward_wpr(cap) for cap in CAPS] == [8, 4, 2, 1] and {backward_wpr(cap, True) for cap in CAPS[:2]} == {1}
    assert sorted(fast_shape(x[0], x[1])[0] for x in SWEEP) == [1, 2, 4]
    assert all(backward_supported(*x[:2], *x[3:5]) for x in SWEEP + MSG_CAPS)
    assert all(forward_path(*x[:5]) == "fast" for x in LARGE) and {x[5] for x in LARGE} == {4}
    assert any(x[4] for x in LARGE) and any(fast_shape(x[0], x[1])[0] == 4 for x in LARGE)
    assert (3, 128) in {x[:2] for x in LARGE} and any(x[1] <= 16 for x in LARGE)
    for gr in (packed, win):
        assert int((gr.m[:N_LIVE] >= HEAVY_MIN).sum()) == len(HUBS) + 3
    modes = {(forward_path(*x[:5]), _mode(x)) for x in CASES}
    assert modes == {(p, m) for p in ("fast", "generic") for m in (0, 1, 2)}
    # every long graph exceeds the grid of the kernels it is there for
    assert backward_wpr(long_graph(20000).cap) == 2 and long_graph(20000).n_live > 256 * 32 * 4 // 2
    assert backward_wpr(long_graph(33000).cap) == 1 and long_graph(33000).n_live > 256 * 32 * 4
    assert {forward_path(*case[:5]) for n, case in LONG if n == 16400} == {"generic"} and long_graph(16400).n_live > 16384
    assert any(case[3] for n, case in LONG if n == 16400) and any(not case[2] for n, case in LONG if n == 16400)
    assert {forward_path(*case[:5]) for n, case in LONG if n == 33000} == {"fast"}
    assert [h * c for h, c in EPILOGUE_SHAPES] == [4, 60, 384, 1024]
    assert {min(cap, 512) for cap, _ in EPILOGUE_ROWS} == {1, 2, 511, 512}
