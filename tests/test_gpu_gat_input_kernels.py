"""The input-side and edge-table GAT kernels of csrc/agg.hip — gat_input_online_kernel<T,V,H,EDGE>,
gat_input_backward_onepass_kernel<T,V,H,EDGE>, the two-pass trio gat_score / gat_edge_weight / gat_input_gather, gat_fold,
gat_edge_msg_epilogue / _dze / _wgrad, gat_backward_indexed<V>, gat_edge_alpha_rows and the eid path of the hidden-layer
gathers — called directly through their entry points (ctypes; the edge-term ones have C linkage for this) against float64
references computed on the CPU, at the shapes where the kernels change path.

Reference: input_ref below, a few-line edge-list formula per head: s_j = <x_j, us>, t_i = <x_i, ud>, a_e = <e_e, v>; row
i's kept edges are the stored positions in [rowptr, rowend) whose source is not i; pre_e = s_j + t_i + a_e; the added self
loop has pre = s_i + t_i + mean a_e (0 without a kept edge) and carries the mean attribute; alpha = softmax(leaky_relu(pre)),
z_i = sum alpha x, ze_i = sum alpha e.  Gradients: torch autograd through that formula in float64 with loss = sum dz z +
sum dze ze, which gives du (source and destination halves) and dv as the backward defines them.  The layers: act(W_h z_h +
W_msg ze_h + b) with us = W_h^T att_src formed in float64.  The indexed backward and the indexed forward use gat_ref /
backward_ref of test_gpu_gat_kernels.py with one head (more heads for the forward).  The CPU test pins input_ref at 1e-12
against oracle/gnn_ref.gat_conv: outputs and the gradients w.r.t. att_src, att_dst and att_edge, with and without edge terms
and messages.

Inputs: feature rows on multiples of 1/8 in [-1, 1] (exact in fp16), folded vectors on multiples of 1/64 in [-1/8, 1/8],
edge rows and v on multiples of 1/8 in [-1, 1]: every non-self logit is exact in fp32 in any summation order (the CPU test
asserts that each logit times 512 is an integer below 2^24), so the leaky masks agree by construction.  Large-logit cases
scale u by 8 and give the hub a source aligned with us.  The layers fold on the device: W on multiples of 1/8, att with one
entry of +-1/8 per head, so that u = W^T att is on the same grid.  With edge terms the self logit holds a mean: a node whose
float64 |pre_self| is below 1e-3 for some head gets a fresh feature row (the CPU test asserts none is left).  dz / dout /
dze are random fp32, every 7th row all zero in dz AND dze (the one-pass backward skips a row by its dz alone: dze = W_msg^T dy
is zero wherever dz = W^T dy is, csrc/common.h says so).  One engine serves every case: the entry points take the feature
table by pointer, so each (d, type) table is a tensor of the test's, not an engine's.  Every output buffer is the test's own: a sentinel
past *n_rows_dev, exact zeros where nothing may be added, untouched after a refused call.

Graphs: "rows" — 195 rows (= 3 mod 32), *n_rows_dev = 190, 196 nodes of which the last is a row of NaN that every skipped
col entry names (as every skipped eid entry names the NaN row of the edge table), capacity 200; in-degrees 0 .. 129 around
the groups of U, the 64-edge chunks and the 63-edge groups of the two-pass gather, a hub of 300, rows whose only edge is a
self loop, self loops among other edges, a duplicated edge, windowed rows (every row i % 3 == 1 ends 1 or 2 entries early),
every 5th kept edge with eid = -1; for the fused layer *n_local_dev = 97 and the rows from there on hold global ids in col
(self loops by global id among them).  "long": rows of degree 0..6, more rows than each capped grid has waves (online
forward and edge weight 16 384, two-pass gather and indexed backward 8 192, one-pass backward 2 048, score 2 048 workgroups
x 64 sources with *n_src_dev = 1, 7, 9, 15 mod 16).

Tolerances: forward rtol = atol = 1e-5; gradients, ze and z_out rtol = 1e-4, atol = 1e-4 * max|want| per tensor (the
project's own).  On the rows graph the bound per tensor is the larger of that and 4 x the maximum error of the SAME formula
evaluated in float32 on the CPU (as in test_gpu_gat_kernels.py); the long graphs get the project tolerance only.  Nothing is
derived from the kernel's output.  Every case prints `label tensor: err=<kernel> fp32=<float32 reference>`.

Measured on an MI355X (maximum |kernel - float64| next to the float32 reference's own error; worst case of the class):

    kernels, cases                          tensor        kernel    float32 reference
    online forward (plain rows)             z             3.8e-07   3.3e-07
    online forward, edge terms              z             1.1e-06   1.2e-06
                                            ze            8.8e-07   7.5e-07
    one-pass backward                       du            4.5e-05   6.7e-05
    one-pass backward, edge terms           du            4.8e-05   7.7e-05
                                            dv            2.5e-05   6.1e-05
    both, u x 8 (hub logits beyond 20)      z / ze        1.3e-06   1.4e-06
                                            du / dv       3.5e-05   3.6e-05
    fused layer (fold, tiled z, n_local)    out           2.1e-05   2.2e-05
                                            ze            5.0e-07   4.7e-07
    two-pass layer (score, weight, gather)  out           1.9e-05   1.3e-05
    message epilogue                        out           1.2e-05   1.2e-05
    message backward                        dze           1.3e-05   1.3e-05
                                            g_w_msg       8.3e-05   7.6e-05
    indexed backward                        dh            2.6e-06   1.9e-06
                                            d_alpha_src/dst 7.1e-05 3.9e-05
                                            dv            2.4e-04   1.2e-04
                                            z_out         2.8e-07   4.0e-07
    indexed forward, fast / generic         out           8.7e-06   8.7e-06   (eid against dense: no element differs)
    long graphs (project tolerance only): z 1.9e-07, ze 1.6e-07, du 5.3e-05, dv 2.7e-05, two-pass out 4.7e-07,
    indexed backward dh 5.6e-07, d_alpha_src/dst 1.5e-06, dv 6.2e-05, z_out 1.6e-07

The whole file takes 5.3 s on the machine on which test_gpu_gat_kernels.py takes 4.8 s.  Seeded one-line errors in agg.hip
(scratch builds) and the tests of this file that fail: second 64-edge chunk dropped 61; `take = j != i` removed 65; wself
not rescaled 21; esum * inv_cnt -> esum 21; `lane < ed.De` widened (the ze store) 15; the nkc tile index one row tile off
9; the n_local comparison flipped 65; the S term omitted in the one-pass backward 54; c0 += 63 -> 64 in the two-pass gather
18; dze ignored in the indexed backward 6.  `e + t < mm` -> `<=` in the online forward changes nothing a test could see:
lane mm of the chunk holds no edge, so its bit of the keep mask is 0 and live[t] is false either way.
"""
import ctypes as C
import functools
import types

import pytest
import torch

import test_gpu_gat_kernels as gk
from oracle import gnn_ref

gpu = pytest.mark.gpu
SLOPE, SENTINEL, E_UNSUPPORTED = gk.SLOPE, gk.SENTINEL, gk.E_UNSUPPORTED
N_ROWS, N_LIVE, N_NODES, CAP, N_READ = 195, 190, 196, 200, 193
NAN_NODE, N_LOCAL = N_NODES - 1, 97
DEGREES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 62, 63, 64, 65, 126, 127, 128, 129]
HUB = 300
MAX_DE, MSG_ROWS = 64, 64  # agg.hip's GAT_INPUT_MAX_EDGE_DIM, GAT_MSG_ROWS
F32, F16 = "f32", "f16"
vp, i32, i64, f32_t = C.c_void_p, C.c_int32, C.c_int64, C.c_float


class EdgeTerms(C.Structure):
    """struct gigl_gat_edge_terms (csrc/common.h, static_assert'ed there: 48 bytes, ze at 40)"""
    _fields_ = [("eid", vp), ("table", vp), ("edge_dim", i32), ("att_edge_folded", vp), ("w_edge_msg", vp), ("ze", vp)]


PROTOS = {
    "gigl_gat_input_aggregate_edge": [vp, vp, i32, i32, vp, vp, i32, f32_t, vp, vp, vp, vp, i64, vp, vp],
    "gigl_gat_input_aggregate_backward_edge": [vp, vp, i32, i32, vp, vp, i32, f32_t, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp],
    "gigl_gat_input_layer_fused_hs": [vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, f32_t, vp, vp, vp, vp, i64, vp, i32, vp,
                                      vp, vp, vp],
    "gigl_gat_edge_msg_add": [vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp],
    "gigl_gat_edge_msg_backward": [vp, vp, i64, vp, vp, vp, i64, i32, i32, i32, vp, vp],
    "gigl_gat_aggregate_backward_indexed": [vp] * 4 + [i32, f32_t] + [vp] * 4 + [i64, vp, i64] + [vp] * 4 + [i32] + [vp] * 8,
    "gigl_gat_aggregate_edge_indexed": [vp] * 4 + [i32, i32, f32_t, i32] + [vp] * 4 + [i64, vp, i64, vp, i32, vp, vp, i32, i64] +
                                       [vp] * 4,
}


# ---- the dispatch, restated from agg.hip (the CPU test asserts that every instantiation is run) ---------------------
def chunks_of(d):
    return (d + 255) // 256


def forward_u(dt, v, heads, edge):
    """gat_input_online_kernel: feature rows in flight"""
    if edge and v == 3 and heads == 4:
        return 2
    return 4 if v * heads * (2 if dt == F16 else 4) > 12 else 8


def input_shape_ok(d, heads):
    return d % 4 == 0 and heads in (1, 2, 4) and d <= 1024


def backward_ok(d, heads, edge):
    return input_shape_ok(d, heads) and not (edge and heads == 4 and d > 768)


WAVE_CAPS = {"online": 16384, "edge_weight": 16384, "gather_items": 8192, "indexed": 8192, "onepass": 2048}
SCORE_SOURCES = 2048 * 4 * 16  # workgroups x waves x RB sources a pass


# ---- graphs ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def base_rows():
    """-> (rows, index of every special row by name): the special rows are spread over the live rows at i % 3 != 1 (no
    window shortens them), self-loop rows on both sides of N_LOCAL"""
    g = torch.Generator().manual_seed(43)
    specs = [("self_only", 0), ("self_among", 0), ("dup", 0)] + [("deg%d" % m, m) for m in DEGREES] + [("hub", HUB)] + \
            [("self_only_hi", 0), ("self_among_hi", 0)]
    free = [i for i in range(N_LIVE) if i % 3 != 1]
    slots = free[::len(free) // len(specs)][:len(specs)]
    rows, where = [None] * N_ROWS, {}
    for (name, m), i in zip(specs, slots):
        where[name] = i
        me = torch.tensor([i])
        if name.startswith("self_only"):
            rows[i] = me
        elif name.startswith("self_among"):
            o = gk._others(g, i, 4, N_READ)
            rows[i] = torch.cat([o[:1], me, o[1:3], me, o[3:]])
        elif name == "dup":
            o = torch.randperm(N_READ - 1, generator=g)[:4]
            o = o + (o >= i)
            rows[i] = torch.cat([o, o[1:2]])
        else:
            rows[i] = gk._others(g, i, m, N_READ)
    for i in range(N_ROWS):
        if rows[i] is None:
            rows[i] = gk._others(g, i, max(int(torch.randint(0, 7, (1,), generator=g)), int(i % 3 == 1)), N_READ)
    return rows, where


@functools.lru_cache(None)
def rows_graph(window):
    return gk._graph_of(base_rows()[0], window, N_LIVE, N_NODES, CAP)


def graph_of(kind, window=False):
    return rows_graph(window) if kind == "rows" else gk.long_graph(kind)


@functools.lru_cache(None)
def edge_ids(kind, window):
    """eid per col position: a row of the edge table, -1 for every 5th kept edge, the table's NaN row (its last) where the
    position does not count"""
    gr = graph_of(kind, window)
    ce = gr.col.numel()
    eid = torch.randperm(ce, generator=torch.Generator().manual_seed(ce))
    eid[gr.pos[::5]] = -1
    eid[gr.unused] = ce
    return eid


def edge_rows(tab, kind, window):
    """the attribute per col position as the formula takes it: zero where eid < 0 (and where the position does not count)"""
    eid = edge_ids(kind, window)
    ok = (eid >= 0) & (eid < tab.shape[0] - 1)
    return torch.where(ok[:, None], torch.nan_to_num(tab)[eid.clamp(min=0)], torch.zeros((), dtype=tab.dtype))


# ---- the reference (dtype follows the inputs) -----------------------------------------------------------------------
def input_ref(gr, x, us, ud, ea=None, v=None):
    """x [nodes, d] in the graph's numbering, us / ud [H, d], ea [positions, De] (indexed at gr.pos only), v [H, De] ->
    (z [n_live, H, d], ze [n_live, H, De] | None, the logits before leaky_relu of the edges gr.pos, then of the self loops)"""
    n, heads, dt = gr.n_live, us.shape[0], x.dtype
    loops = torch.arange(n)
    src, dst = torch.cat([gr.src, loops]), torch.cat([gr.dst, loops])
    pre = (x @ us.T)[src] + (x @ ud.T)[dst]
    ek = None
    if ea is not None:
        ek = ea[gr.pos]
        inv_cnt = (1.0 / gr.cnt.clamp(min=1).to(dt))[:, None]
        ek = torch.cat([ek, torch.zeros(n, ek.shape[1], dtype=dt).index_add(0, gr.dst, ek) * inv_cnt])
        pre = pre + ek @ v.T
    e = torch.nn.functional.leaky_relu(pre, SLOPE)
    emax = torch.full((n, heads), float("-inf"), dtype=dt).scatter_reduce(0, dst[:, None].expand(-1, heads), e.detach(),
                                                                          reduce="amax")
    ex = torch.exp(e - emax[dst])
    alpha = ex / torch.zeros(n, heads, dtype=dt).index_add(0, dst, ex)[dst]
    xs = x[src]
    z = torch.stack([torch.zeros(n, x.shape[1], dtype=dt).index_add(0, dst, alpha[:, h:h + 1] * xs) for h in range(heads)], 1)
    ze = None if ek is None else torch.zeros(n, heads, ek.shape[1], dtype=dt).index_add(0, dst, alpha[:, :, None] * ek[:, None])
    return z, ze, pre


def layer_ref(gr, x, w, att_src, att_dst, heads, c, bias, act, ea=None, v=None, w_msg=None):
    """act(W_h z_h + W_msg ze_h + b) -> [n_live, H*C], the logits, and ze [n_live, H, De] | None"""
    wh = w.view(heads, c, -1)
    us = torch.einsum("hc,hcd->hd", att_src.view(heads, c), wh)
    ud = torch.einsum("hc,hcd->hd", att_dst.view(heads, c), wh)
    z, ze, pre = input_ref(gr, x, us, ud, ea, v)
    out = torch.einsum("nhd,hcd->nhc", z, wh)
    if w_msg is not None:
        out = out + torch.einsum("nhk,hck->nhc", ze, w_msg.view(heads, c, -1))
    out = out.reshape(gr.n_live, heads * c)
    if bias is not None:
        out = out + bias
    return (torch.relu(out) if act else out), pre.detach(), ze


def _self_logits(t, gr, window):
    n = gr.n_live
    x = torch.nan_to_num(t.x)
    pre = (x @ t.us.T + x @ t.ud.T)[:n]
    if t.de:
        a = (edge_rows(t.tab, t.kind, window) @ t.v.T)[gr.pos]
        pre = pre + torch.zeros(n, t.heads, dtype=a.dtype).index_add(0, gr.dst, a) / gr.cnt.clamp(min=1)[:, None]
    return pre


@functools.lru_cache(None)
def agg_inputs(kind, d, heads, de, scale):
    """the inputs of a shape as float64, shared by both tables' types and by the packed and the windowed graph"""
    windows = [False, True] if kind == "rows" else [False]
    gr = graph_of(kind)
    cap, nn, ce = gr.cap, gr.n_nodes, gr.col.numel()
    g = torch.Generator().manual_seed(1000 * heads + 7 * d + 13 * de + 100 * scale + (0 if kind == "rows" else kind))
    t = types.SimpleNamespace(kind=kind, d=d, heads=heads, de=de, scale=scale, redrawn=0)
    t.x = gk._grid(g, 8, -8, 8, cap, d)
    t.us, t.ud = scale * gk._grid(g, 64, -8, 8, heads, d), scale * gk._grid(g, 64, -8, 8, heads, d)
    if scale > 1 and kind == "rows":  # the extreme on the hub: its first source points along us[0] in the first 64 columns
        j = int(base_rows()[0][base_rows()[1]["hub"]][0])
        k = min(d, 64)
        t.x[j, :k] = torch.where(t.us[0, :k] >= 0, 1.0, -1.0).double()
    t.tab = t.v = None
    if de:
        t.tab, t.v = gk._grid(g, 8, -8, 8, ce + 1, de), gk._grid(g, 8, -8, 8, heads, de)
        t.tab[ce] = float("nan")
        for _ in range(100):  # |pre_self| >= 1e-3 (float64) for every live row and head: a fresh x row where it is not
            bad = torch.zeros(cap, dtype=torch.bool)
            for w in windows:
                bad[:gr.n_live] |= (_self_logits(t, graph_of(kind, w), w).abs() < 1e-3).any(1)
            if not bool(bad.any()):
                break
            t.x[bad] = gk._grid(g, 8, -8, 8, int(bad.sum()), d)
            t.redrawn += int(bad.sum())
    t.x[nn - 1:] = float("nan")
    t.perm = torch.randperm(cap, generator=g)  # the table row of every node: gather_ids
    t.table = torch.zeros(cap, d, dtype=torch.float64)
    t.table[t.perm] = t.x
    t.zero_rows = torch.arange(gr.n_live) % 7 == 3
    t.dz = gk._free(g, heads, cap, d)
    t.dz[:, torch.arange(cap) % 7 == 3] = 0.0
    t.dz[:, gr.n_live:] = float("nan")
    t.dze = None
    if de:
        t.dze = gk._free(g, cap, heads, de)
        t.dze[torch.arange(cap) % 7 == 3] = 0.0
        t.dze[gr.n_live:] = float("nan")
    return t


def agg_ref(t, gr, window, edge, msg, dt):
    """-> {z [H, n_live, d], ze, du [2H, d], dv [H, De], pre}"""
    n = gr.n_live
    x = torch.nan_to_num(t.x[:gr.n_nodes]).to(dt)
    us, ud = t.us.to(dt).requires_grad_(True), t.ud.to(dt).requires_grad_(True)
    ea = v = None
    leaves = [us, ud]
    if edge:
        ea, v = edge_rows(t.tab, t.kind, window).to(dt), t.v.to(dt).requires_grad_(True)
        leaves.append(v)
    z, ze, pre = input_ref(gr, x, us, ud, ea, v)
    loss = (z * t.dz[:, :n].to(dt).permute(1, 0, 2)).sum()
    if msg:
        loss = loss + (ze * t.dze[:n].to(dt)).sum()
    grads = torch.autograd.grad(loss, leaves)
    r = {"z": z.detach().permute(1, 0, 2), "du": torch.cat([grads[0], grads[1]]), "pre": pre.detach()}
    if edge:
        r["dv"] = grads[2]
    if msg:
        r["ze"] = ze.detach()
    return r


@functools.lru_cache(None)
def agg_case(kind, d, heads, de, msg, scale, window):
    t = agg_inputs(kind, d, heads, de, scale)
    gr = graph_of(kind, window)
    want = agg_ref(t, gr, window, de > 0, msg, torch.float64)
    lo = agg_ref(t, gr, window, de > 0, msg, torch.float32) if kind == "rows" else want
    return t, gr, want, {k: gk._err(lo[k], want[k]) for k in want}


# ---- the cases: (table type, d, heads, De, messages, scale of u, windowed) ------------------------------------------
D_BY_V = {1: [4, 256], 2: [260], 3: [516, 768], 4: [772, 1000, 1024]}
DES = [1, 3, 63, 64]


def _agg_cases():
    out = []
    for combo, (dt, heads, edge) in enumerate((dt, h, e) for dt in (F32, F16) for h in (1, 2, 4) for e in (False, True)):
        for v in (1, 2, 3, 4):
            ds = D_BY_V[v]
            de = DES[(combo // 2 + v) % 4] if edge else 0
            out.append((dt, ds[(combo // 2) % len(ds)], heads, de, bool(edge and (combo // 2 + (v > 2)) % 2), 1,
                        bool((combo + (v > 2)) % 2)))
    return out


AGG = _agg_cases()
LARGE = [(F32, 1024, 1, 0, False, 8, True), (F16, 768, 2, 3, True, 8, False), (F32, 260, 4, 64, True, 8, True),
         (F16, 256, 4, 1, False, 8, False)]
LONG_FWD = [(16400, (F32, 4, 2, 3, True, 1, False)), (16400, (F16, 8, 1, 0, False, 1, False))]
LONG_BWD = [(2100, (F32, 8, 2, 3, True, 1, False)), (2100, (F16, 4, 4, 0, False, 1, False))]


def _id(case):
    dt, d, heads, de, msg, scale, window = case
    return f"{dt}-d{d}-H{heads}" + (f"-De{de}" if de else "") + ("-msg" if msg else "") + (f"-x{scale}" if scale != 1 else "") + \
        ("-win" if window else "")


# ---- device side ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    for name, args in PROTOS.items():
        fn = getattr(e._lib, name)
        fn.argtypes, fn.restype = args, i32
    yield e
    e.close()


def p(x):
    return None if x is None else x.data_ptr()


def full(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")


def _table(t, dt):
    return t.table.to(torch.float16 if dt == F16 else torch.float32).cuda()


def _dev_graph(gr, col=None):
    return types.SimpleNamespace(rowptr=gk._i32(gr.rp[:-1]), rowend=gk._i32(gr.rowend), col=gk._i32(gr.col if col is None else col),
                                 n_rows=gk._count(gr.n_live),
                                 meta=torch.tensor([gr.n_nodes, gr.col.numel()], dtype=torch.int32, device="cuda"))


def edge_terms(tab, eid, v, w_msg, ze, told_de=None):
    """-> (address of a gigl_gat_edge_terms, what must stay alive); told_de: the edge_dim the call is TOLD (the refusals)"""
    keep = [gk._f32(tab), gk._i32(eid), gk._f32(v), gk._f32(w_msg)]
    et = EdgeTerms(p(keep[1]), p(keep[0]), int(tab.shape[1]) if told_de is None else told_de, p(keep[2]), p(keep[3]), p(ze))
    keep.append(et)
    return C.addressof(et), keep


def _agg_edge(t, gr, window, msg, ze, de=None):
    """(the aggregation only asks whether w_edge_msg is there)"""
    if not t.de:
        return None, None
    return edge_terms(t.tab, edge_ids(t.kind, window), t.v, torch.ones(4, dtype=torch.float64) if msg else None, ze, de)


def run_agg_forward(eng, t, gr, dt, window, msg, d=None, heads=None, de=None):
    """-> (rc, z [H, cap, d], ze [cap, H, De] | None); d / heads / de override what the call is TOLD (the refusals)"""
    dg = _dev_graph(gr)
    z = full(t.heads, gr.cap, t.d)
    ze = full(gr.cap, t.heads, t.de) if msg else None
    et, keep = _agg_edge(t, gr, window, msg, ze, de)
    table, ids, u = _table(t, dt), gk._i32(t.perm), gk._f32(torch.cat([t.us, t.ud]))
    rc = eng._lib.gigl_gat_input_aggregate_edge(eng._ctx, p(table), int(dt == F16), d or t.d, p(ids), p(u), heads or t.heads, SLOPE,
                                                p(dg.rowptr), p(dg.rowend), p(dg.col), p(dg.n_rows), gr.cap, p(z), et)
    torch.cuda.synchronize()
    return rc, z.cpu(), None if ze is None else ze.cpu()


def run_agg_backward(eng, t, gr, dt, window, msg, d=None, heads=None, de=None, prefill=0.0):
    """-> (rc, du [2H, d], dv [H, De] | None)"""
    dg = _dev_graph(gr)
    du = torch.full((2 * t.heads, t.d), prefill, dtype=torch.float32, device="cuda")
    dv = torch.full((t.heads, t.de), prefill, dtype=torch.float32, device="cuda") if t.de else None
    ze = torch.zeros(1, dtype=torch.float32, device="cuda") if msg else None  # (one float, neither read nor written: the
    # edge terms are checked as the forward's, which wants ze wherever w_edge_msg is)
    et, keep = _agg_edge(t, gr, window, msg, ze, de)
    table, ids, u = _table(t, dt), gk._i32(t.perm), gk._f32(torch.cat([t.us, t.ud]))
    dz, dze = gk._f32(t.dz), gk._f32(t.dze) if msg else None
    rc = eng._lib.gigl_gat_input_aggregate_backward_edge(
        eng._ctx, p(table), int(dt == F16), d or t.d, p(ids), p(u), heads or t.heads, SLOPE, p(dg.rowptr), p(dg.rowend), p(dg.col),
        p(dg.n_rows), gr.cap, p(dz), p(du), et, p(dze), p(dv))
    torch.cuda.synchronize()
    return rc, du.cpu(), None if dv is None else dv.cpu()


def check_agg_forward(label, got, t, gr, want, e32, msg):
    rc, z, ze = got
    assert rc == 0, (label, rc)
    gk.check(label, "z", z[:, :gr.n_live], want["z"], e32["z"])
    assert bool((z[:, gr.n_live:] == SENTINEL).all()), f"{label}: z rows past *n_rows_dev were written"
    if msg:
        gk.check(label, "ze", ze[:gr.n_live], want["ze"], e32["ze"], grad=True)
        assert bool((ze[gr.n_live:] == SENTINEL).all()), f"{label}: ze rows past *n_rows_dev were written"


def check_agg_backward(label, got, t, want, e32):
    rc, du, dv = got
    assert rc == 0, (label, rc)
    gk.check(label, "du", du, want["du"], e32["du"], grad=True)
    if t.de:
        gk.check(label, "dv", dv, want["dv"], e32["dv"], grad=True)


# ---- 1. the aggregation over folded vectors: gat_input_online_kernel (plain rows out) and its one-pass backward ------
@gpu
@pytest.mark.parametrize("case", AGG + LARGE, ids=_id)
def test_input_aggregate(eng, case):
    dt, d, heads, de, msg, scale, window = case
    t, gr, want, e32 = agg_case("rows", d, heads, de, msg, scale, window)
    label = f"agg {_id(case)} V={chunks_of(d)} U={forward_u(dt, chunks_of(d), heads, de > 0)}"
    check_agg_forward("fwd " + label, run_agg_forward(eng, t, gr, dt, window, msg), t, gr, want, e32, msg)
    if backward_ok(d, heads, de > 0):
        check_agg_backward("bwd " + label, run_agg_backward(eng, t, gr, dt, window, msg), t, want, e32)
    else:
        rc, du, dv = run_agg_backward(eng, t, gr, dt, window, msg, prefill=SENTINEL)
        assert rc == E_UNSUPPORTED and bool((du == SENTINEL).all()) and bool((dv == SENTINEL).all()), (label, rc)


@gpu
@pytest.mark.parametrize("n,case", LONG_FWD + LONG_BWD, ids=lambda x: _id(x) if isinstance(x, tuple) else str(x))
def test_input_aggregate_long_graph(eng, n, case):
    dt, d, heads, de, msg, scale, window = case
    t, gr, want, e32 = agg_case(n, d, heads, de, msg, scale, window)
    label = f"long {n} {_id(case)}"
    check_agg_forward("fwd " + label, run_agg_forward(eng, t, gr, dt, window, msg), t, gr, want, e32, msg)
    check_agg_backward("bwd " + label, run_agg_backward(eng, t, gr, dt, window, msg), t, want, e32)


REFUSED = [("d=1028", dict(d=1028)), ("d=6", dict(d=6)), ("heads=3", dict(heads=3)), ("De=0", dict(de=0)), ("De=65", dict(de=65))]


@gpu
@pytest.mark.parametrize("name,told", REFUSED, ids=[x[0] for x in REFUSED])
def test_input_aggregate_refuses(eng, name, told):
    """the buffers are those of a served shape, the call is told another: nothing may be launched, nothing written"""
    t, gr, _, _ = agg_case("rows", 256, 2, 3, True, 1, False)
    rc, z, ze = run_agg_forward(eng, t, gr, F32, False, True, **told)
    assert rc == E_UNSUPPORTED and bool((z == SENTINEL).all()) and bool((ze == SENTINEL).all()), (name, rc)
    rc, du, dv = run_agg_backward(eng, t, gr, F32, False, True, prefill=SENTINEL, **told)
    assert rc == E_UNSUPPORTED and bool((du == SENTINEL).all()) and bool((dv == SENTINEL).all()), (name, rc)


# ---- 2. the layers: fold + one pass (tiled z, *n_local_dev, edge terms, messages) and fold + two passes -------------
LAYER_C = 8
#         (table type, d, heads, De, messages, act, windowed)
FUSED = [(F32, 4, 1, 0, False, 0, False), (F16, 256, 2, 3, True, 1, True), (F32, 260, 4, 64, False, 1, True),
         (F16, 516, 4, 1, True, 0, False), (F32, 768, 2, 63, True, 1, False), (F16, 772, 1, 0, False, 1, True),
         (F32, 1000, 4, 3, True, 0, True), (F16, 1024, 2, 64, True, 1, False), (F32, 1024, 1, 1, False, 0, True)]
TWOPASS = [(F32, 4, 1), (F16, 256, 2), (F32, 260, 4), (F16, 516, 1), (F32, 768, 4), (F16, 772, 2), (F32, 1000, 1), (F16, 1024, 4),
           (F32, 1028, 2)]
SCORE_LONG = [(131089, F32, 4, 1), (131095, F16, 8, 2), (131097, F32, 4, 4), (131103, F16, 4, 2)]  # (sources, type, d, heads)


@functools.lru_cache(None)
def layer_inputs(kind, d, heads, de, msg):
    """W on multiples of 1/8, att with one entry of +-1/8 per head: u = W^T att on multiples of 1/64 in [-1/8, 1/8]"""
    t = types.SimpleNamespace(**vars(agg_inputs(kind, d, heads, de, 1)))
    g = torch.Generator().manual_seed(31 * d + heads + 5 * de)
    c = LAYER_C
    t.c, t.w = c, gk._grid(g, 8, -8, 8, heads * c, d)
    t.att_src, t.att_dst = torch.zeros(heads * c, dtype=torch.float64), torch.zeros(heads * c, dtype=torch.float64)
    for h in range(heads):  # (two different channels: us + ud, the self loop's vector, is never zero)
        for att, k in zip((t.att_src, t.att_dst), torch.randperm(c, generator=g)[:2].tolist()):
            att[h * c + k] = float(torch.randint(0, 2, (1,), generator=g) * 2 - 1) / 8
    wh = t.w.view(heads, c, d)
    t.us = torch.einsum("hc,hcd->hd", t.att_src.view(heads, c), wh)
    t.ud = torch.einsum("hc,hcd->hd", t.att_dst.view(heads, c), wh)
    gr = graph_of(kind)
    if de:  # (the margin again: these folded vectors are not those of agg_inputs)
        t.x = t.x.clone()
        for _ in range(100):
            bad = torch.zeros(gr.cap, dtype=torch.bool)
            for w in ([False, True] if kind == "rows" else [False]):
                bad[:gr.n_live] |= (_self_logits(t, graph_of(kind, w), w).abs() < 1e-3).any(1)
            if not bool(bad.any()):
                break
            t.x[bad] = gk._grid(g, 8, -8, 8, int(bad.sum()), d)
        t.x[gr.n_nodes - 1:] = float("nan")
        t.table = torch.zeros(gr.cap, d, dtype=torch.float64)
        t.table[t.perm] = t.x
    t.bias = gk._free(g, heads * c)
    t.w_msg = gk._free(g, heads * c, de) if msg else None
    return t


@functools.lru_cache(None)
def layer_case(kind, d, heads, de, msg, act, window):
    t = layer_inputs(kind, d, heads, de, msg)
    gr = graph_of(kind, window)

    def ref(dt):
        f = lambda a: None if a is None else a.to(dt)
        ea = edge_rows(t.tab, kind, window).to(dt) if de else None
        return layer_ref(gr, torch.nan_to_num(t.x[:gr.n_nodes]).to(dt), f(t.w), f(t.att_src), f(t.att_dst), heads, t.c, f(t.bias),
                         act, ea, f(t.v), f(t.w_msg))
    want, pre, ze = ref(torch.float64)
    lo = ref(torch.float32) if kind == "rows" else (want, pre, ze)
    return t, gr, want, gk._err(lo[0], want), pre, ((ze, gk._err(lo[2], ze)) if msg else None)


def global_col(t, gr, n_local):
    """the rows from n_local on name their sources by table row (the leaf-global union of the plan)"""
    col = gr.col.clone()
    row_of = torch.repeat_interleave(torch.arange(gr.n_rows), gr.rp[1:] - gr.rp[:-1])
    far = row_of >= n_local
    col[far] = t.perm[col[far]]
    return col


@gpu
@pytest.mark.parametrize("case", FUSED, ids=lambda c: f"{c[0]}-d{c[1]}-H{c[2]}-De{c[3]}" + ("-msg" if c[4] else "") + f"-act{c[5]}")
def test_input_layer_fused(eng, case):
    dt, d, heads, de, msg, act, window = case
    t, gr, want, e32, _, want_ze = layer_case("rows", d, heads, de, msg, act, window)
    dg = _dev_graph(gr, global_col(t, gr, N_LOCAL))
    out = full(gr.cap, heads * t.c)
    ze = full(gr.cap, heads, de) if msg else None
    et = keep = None
    if de:
        et, keep = edge_terms(t.tab, edge_ids("rows", window), t.v, t.w_msg, ze)
    scratch = torch.full((int(eng._lib.gigl_gat_input_layer_fused_scratch(d, heads, gr.cap)),), float("nan"), dtype=torch.float32,
                         device="cuda")
    table, ids, n_local = _table(t, dt), gk._i32(t.perm), gk._count(N_LOCAL)
    w, a_s, a_d, bias = gk._f32(t.w), gk._f32(t.att_src), gk._f32(t.att_dst), gk._f32(t.bias)
    rc = eng._lib.gigl_gat_input_layer_fused_hs(
        eng._ctx, p(table), int(dt == F16), d, p(ids), p(n_local), p(w), p(a_s), p(a_d), heads, t.c, SLOPE, p(dg.rowptr), p(dg.rowend),
        p(dg.col), p(dg.n_rows), gr.cap, p(bias), act, p(scratch), p(out), None, et)
    torch.cuda.synchronize()
    label = f"fused {_id((dt, d, heads, de, msg, 1, window))} act={act}"
    assert rc == 0, (label, rc)
    out = out.cpu()
    gk.check(label, "out", out[:gr.n_live], want, e32)
    assert bool((out[gr.n_live:] == SENTINEL).all()), f"{label}: rows past *n_rows_dev were written"
    if msg:
        ze = ze.cpu()
        gk.check(label, "ze", ze[:gr.n_live], want_ze[0], want_ze[1], grad=True)
        assert bool((ze[gr.n_live:] == SENTINEL).all()), f"{label}: ze rows past *n_rows_dev were written"


def run_two_pass(eng, t, gr, dt, d, heads, act, n_src, told_d=None, told_heads=None):
    dg = _dev_graph(gr)
    out = full(gr.cap, heads * t.c)
    ce = gr.col.numel()
    scratch = torch.full((int(eng._lib.gigl_gat_input_layer_scratch(d, heads, gr.cap, gr.cap, ce)),), float("nan"),
                         dtype=torch.float32, device="cuda")
    table, ids, n_src_dev = _table(t, dt), gk._i32(t.perm), gk._count(n_src)
    w, a_s, a_d, bias = gk._f32(t.w), gk._f32(t.att_src), gk._f32(t.att_dst), gk._f32(t.bias)
    rc = eng._lib.gigl_gat_input_layer(eng._ctx, p(table), int(dt == F16), told_d or d, p(ids), p(w), p(a_s), p(a_d),
                                       told_heads or heads, t.c, SLOPE, p(dg.rowptr), p(dg.rowend), p(dg.col), ce, p(n_src_dev), gr.cap,
                                       p(dg.n_rows), gr.cap, p(bias), act, p(scratch), p(out))
    torch.cuda.synchronize()
    return rc, out.cpu()


@gpu
@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("dt,d,heads", TWOPASS)
def test_input_layer_two_pass(eng, dt, d, heads, window):
    act = int(d % 8 == 0)
    t, gr, want, e32, _, _ = layer_case("rows", d, heads, 0, False, act, window)
    rc, out = run_two_pass(eng, t, gr, dt, d, heads, act, NAN_NODE)
    label = f"two-pass {dt}-d{d}-H{heads} window={window}"
    assert rc == 0, (label, rc)
    gk.check(label, "out", out[:gr.n_live], want, e32)
    assert bool((out[gr.n_live:] == SENTINEL).all()), f"{label}: rows past *n_rows_dev were written"


@gpu
@pytest.mark.parametrize("n,dt,d,heads", SCORE_LONG)
def test_input_layer_two_pass_long_graph(eng, n, dt, d, heads):
    """more sources than a pass of gat_score_kernel's grid takes, *n_src_dev = 1, 7, 9, 15 mod 16; more rows than the
    edge-weight and the gather grids have waves"""
    t, gr, want, e32, _, _ = layer_case(n, d, heads, 0, False, 1, False)
    rc, out = run_two_pass(eng, t, gr, dt, d, heads, 1, n)
    assert rc == 0, rc
    gk.check(f"two-pass long {n} {dt}-d{d}-H{heads}", "out", out[:gr.n_live], want, e32)
    assert bool((out[gr.n_live:] == SENTINEL).all())


@gpu
def test_input_layers_refuse(eng):
    t, gr, _, _, _, _ = layer_case("rows", 256, 2, 0, False, 0, False)
    for told in (dict(told_d=6), dict(told_heads=3)):
        rc, out = run_two_pass(eng, t, gr, F32, 256, 2, 0, NAN_NODE, **told)
        assert rc == E_UNSUPPORTED and bool((out == SENTINEL).all()), (told, rc)
    dg, out = _dev_graph(gr), full(gr.cap, 2 * t.c)
    scratch = torch.empty(int(eng._lib.gigl_gat_input_layer_fused_scratch(1028, 4, gr.cap)), dtype=torch.float32, device="cuda")
    table, ids = _table(t, F32), gk._i32(t.perm)
    w, a_s, a_d = gk._f32(t.w), gk._f32(t.att_src), gk._f32(t.att_dst)
    for d, heads in ((1028, 2), (6, 2), (256, 3)):
        rc = eng._lib.gigl_gat_input_layer_fused_hs(eng._ctx, p(table), 0, d, p(ids), None, p(w), p(a_s), p(a_d), heads, t.c, SLOPE,
                                                    p(dg.rowptr), p(dg.rowend), p(dg.col), p(dg.n_rows), gr.cap, None, 0, p(scratch),
                                                    p(out), None, None)
        torch.cuda.synchronize()
        assert rc == E_UNSUPPORTED and bool((out == SENTINEL).all()), (d, heads, rc)


# ---- 3. the message kernels ------------------------------------------------------------------------------------------
#      (rows capacity, live rows, heads, channels, De)
MSG = [(63, 63, 1, 4, 1), (64, 64, 2, 8, 3), (65, 65, 4, 4, 63), (130, 127, 2, 12, 64), (200, 129, 1, 16, 3),
       (4100, 4097, 4, 64, 64)]  # the last: rows * H * C and rows * H * De beyond the 4096 x 256 threads of a pass


@functools.lru_cache(None)
def msg_inputs(cap, live, heads, c, de):
    g = torch.Generator().manual_seed(cap + 3 * heads + c + de)
    t = types.SimpleNamespace(plane=cap * c + 20)
    t.ze, t.w_msg, t.bias = gk._free(g, cap, heads, de), gk._free(g, heads * c, de), gk._free(g, heads * c)
    t.out0 = gk._free(g, cap, heads * c)
    t.dy = gk._free(g, heads, t.plane)  # dy[h][i][c] at h * plane + i * c + c
    t.dy[:, live * c:] = float("nan")
    t.ze_nan = t.ze.clone()
    t.ze_nan[live:] = float("nan")
    return t


def msg_ref(t, live, heads, c, de, dt):
    ze, w = t.ze[:live].to(dt), t.w_msg.to(dt).view(heads, c, de)
    out = torch.relu(t.out0[:live].to(dt) + torch.einsum("nhk,hck->nhc", ze, w).reshape(live, heads * c) + t.bias.to(dt))
    dy = t.dy[:, :live * c].to(dt).view(heads, live, c)
    return out, torch.einsum("hnc,hck->nhk", dy, w), torch.einsum("hnc,nhk->hck", dy, ze).reshape(heads * c, de)


@gpu
@pytest.mark.parametrize("cap,live,heads,c,de", MSG)
def test_edge_message_kernels(eng, cap, live, heads, c, de):
    t = msg_inputs(cap, live, heads, c, de)
    want, lo = msg_ref(t, live, heads, c, de, torch.float64), msg_ref(t, live, heads, c, de, torch.float32)
    label = f"msg {cap}/{live} {heads}x{c} De{de}"
    n, ze, w_msg, out = gk._count(live), gk._f32(t.ze_nan), gk._f32(t.w_msg), gk._f32(t.out0)
    assert eng._lib.gigl_gat_edge_msg_add(eng._ctx, p(ze), p(w_msg), p(gk._f32(t.bias)), p(n), cap, heads, c, de, 1, p(out)) == 0
    torch.cuda.synchronize()
    gk.check(label, "out", out[:live], want[0], gk._err(lo[0], want[0]))
    assert torch.equal(out[live:].cpu(), t.out0[live:].float()), f"{label}: rows past *n_rows_dev were touched"
    dze, g_w = full(cap, heads, de), torch.zeros(heads * c, de, dtype=torch.float32, device="cuda")
    dy = gk._f32(t.dy)
    assert eng._lib.gigl_gat_edge_msg_backward(eng._ctx, p(dy), t.plane, p(w_msg), p(ze), p(n), cap, heads, c, de, p(dze), p(g_w)) == 0
    torch.cuda.synchronize()
    gk.check(label, "dze", dze[:live], want[1], gk._err(lo[1], want[1]), grad=True)
    assert bool((dze[live:] == SENTINEL).all()), f"{label}: dze rows past *n_rows_dev were written"
    gk.check(label, "g_w_msg", g_w, want[2], gk._err(lo[2], want[2]), grad=True)


# ---- 4. the hidden layer over the resident edge table: indexed backward, indexed forward ----------------------------
#            (channels, De, messages, scale)
INDEXED = [(4, 1, False, 1), (4, 3, True, 1), (252, 63, True, 1), (256, 64, False, 1), (256, 3, True, 4), (260, 1, True, 1),
           (512, 64, True, 1), (512, 3, False, 1)]
INDEXED_LONG = (8200, (4, 3, True, 1))


@functools.lru_cache(None)
def indexed_inputs(kind, c, de, msg, scale, heads=1):
    """gat_inputs of test_gpu_gat_kernels.py (a copy: its tensors stay as they are), the attributes moved into an edge
    table of shuffled rows behind eid, every 5th kept edge of the windowed graph without one (eid = -1: a zero attribute)"""
    base = gk.gat_inputs(kind, heads, c, de, msg, scale)
    t = types.SimpleNamespace(**vars(base))
    gr = gk.rows_graph(True) if kind == "rows" else gk.long_graph(kind)
    ce = gr.col.numel()
    g = torch.Generator().manual_seed(c + de + 1000 * (heads - 1))
    t.eid = torch.randperm(ce, generator=g)
    t.eid[gr.pos[::5]] = -1
    t.eid[gr.unused] = ce
    t.ea = base.ea.clone()
    t.ea[gr.pos[::5]] = 0.0
    t.tab = torch.full((ce + 1, de), float("nan"), dtype=torch.float64)
    ok = t.eid >= 0
    t.tab[t.eid[ok]] = torch.where(gr.unused[ok][:, None], torch.full((), float("nan"), dtype=torch.float64), t.ea[ok])
    t.h = base.h.clone()
    for _ in range(100):
        bad = torch.zeros(gr.cap, dtype=torch.bool)
        bad[:gr.n_live] = (gk.self_logits(t, gr).abs() < 1e-3).any(1)
        if not bool(bad.any()):
            break
        t.h[bad] = gk._grid(g, 64, -128, 128, int(bad.sum()), heads * c)
    t.h[gr.n_nodes - 1:] = float("nan")
    return t, gr


@functools.lru_cache(None)
def indexed_case(kind, c, de, msg, scale):
    t, gr = indexed_inputs(kind, c, de, msg, scale)

    def ref(dt):
        r = gk.backward_ref(t, gr, dt)
        r["dv"] = r.pop("d_alpha_edge").T @ t.ea.to(dt)
        return r
    want = ref(torch.float64)
    lo = ref(torch.float32) if kind == "rows" else want
    return t, gr, want, {k: gk._err(lo[k], want[k]) for k in want}


def run_indexed_backward(eng, t, gr, want, told_c=None, told_de=None, h=None, sentinel=False):
    cap, n, c = gr.cap, gr.n_live, t.c
    out_pre, dout, _ = gk._backward_args(t, gr, want, cap)
    dze = None
    if t.msg:
        dze = torch.full((cap, t.de), float("nan"), dtype=torch.float64)
        dze[:n] = t.dout[:n] @ t.w_msg
        dze = gk._f32(dze)
    new = (lambda *s: full(*s)) if sentinel else (lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda"))
    dh, ds, dd, dv = new(cap, c), new(cap), new(cap), new(t.de)
    z = full(cap, t.de) if t.msg else None
    scratch = torch.empty(2 * cap, dtype=torch.float32, device="cuda")
    dg = gk._dev_graph(gr)
    hh, a_s, a_d, tab, eid, v = (gk._f32(t.h) if h is None else h), gk._f32(t.att_src), gk._f32(t.att_dst), gk._f32(t.tab), \
        gk._i32(t.eid), gk._f32(t.v)
    nr = gk._count(n)
    rc = eng._lib.gigl_gat_aggregate_backward_indexed(
        eng._ctx, p(hh), p(a_s), p(a_d), told_c or c, SLOPE, p(dg.rowptr), p(dg.rowend), p(dg.col), p(dg.meta), cap, p(nr), cap,
        p(out_pre), p(dout), p(tab), p(eid), t.de if told_de is None else told_de, p(v), p(dze), p(scratch), p(dh), p(ds), p(dd), p(dv), p(z))
    torch.cuda.synchronize()
    return rc, [x if x is None else x.cpu() for x in (dh, ds, dd, dv, z)]


def check_indexed_backward(label, got, t, gr, want, e32):
    rc, (dh, ds, dd, dv, z) = got
    assert rc == 0, (label, rc)
    nn = gr.n_nodes
    read = torch.zeros(nn, dtype=torch.bool)
    read[gr.src] = True
    read[:gr.n_live] = True
    for name, x in (("dh", dh), ("d_alpha_src", ds[:, None]), ("d_alpha_dst", dd[:, None])):
        gk.check(label, name, x[:nn], want[name], e32[name], grad=True)
        assert not bool(x[nn:].any()) and not bool(x[:nn][~read].any()), f"{label} {name}: a node nobody reads has a gradient"
    assert not bool(dd[gr.n_live:].any()) and not bool(dd[:gr.n_live][t.zero_rows].any())
    gk.check(label, "dv", dv[None], want["dv"], e32["dv"], grad=True)
    if t.msg:
        gk.check(label, "z_out", z[:gr.n_live, None], want["z_out"], e32["z_out"], grad=True)
        assert bool((z[gr.n_live:] == SENTINEL).all()) and not bool(z[:gr.n_live][t.zero_rows].any()), f"{label}: z_out of a skipped row"


@gpu
@pytest.mark.parametrize("c,de,msg,scale", INDEXED)
def test_indexed_backward(eng, c, de, msg, scale):
    t, gr, want, e32 = indexed_case("rows", c, de, msg, scale)
    check_indexed_backward(f"indexed bwd C{c} De{de} msg={msg} x{scale} V={1 if c <= 256 else 2}",
                           run_indexed_backward(eng, t, gr, want), t, gr, want, e32)


@gpu
def test_indexed_backward_long_graph(eng):
    n, (c, de, msg, scale) = INDEXED_LONG
    t, gr, want, e32 = indexed_case(n, c, de, msg, scale)
    check_indexed_backward(f"indexed bwd long {n}", run_indexed_backward(eng, t, gr, want), t, gr, want, e32)


@gpu
def test_indexed_backward_refuses(eng):
    """C = 516 (told to a call over the buffers of C = 512), De = 0 / 65 likewise, a matrix off the 16-byte grid"""
    t, gr, want, _ = indexed_case("rows", 512, 3, False, 1)
    rc, outs = run_indexed_backward(eng, t, gr, want, told_c=516, sentinel=True)
    assert rc == E_UNSUPPORTED and all(bool((x == SENTINEL).all()) for x in outs if x is not None), rc
    buf = torch.zeros(gr.cap * 512 + 4, dtype=torch.float32, device="cuda")
    h = buf[1:1 + gr.cap * 512].view(gr.cap, 512)
    h.copy_(gk._f32(t.h))
    assert h.data_ptr() % 16 == 4
    rc, outs = run_indexed_backward(eng, t, gr, want, h=h, sentinel=True)
    assert rc == E_UNSUPPORTED and all(bool((x == SENTINEL).all()) for x in outs if x is not None), rc
    for de in (0, 65):
        rc, outs = run_indexed_backward(eng, t, gr, want, told_de=de, sentinel=True)
        assert rc == E_UNSUPPORTED and all(bool((x == SENTINEL).all()) for x in outs if x is not None), (de, rc)


#                 (heads, channels, concat, De, messages): the fast pair and the generic kernels
INDEXED_FWD = [(4, 64, 1, 3, False), (4, 64, 1, 16, True), (1, 256, 1, 64, True), (2, 12, 1, 3, False), (4, 16, 1, 5, True), (4, 16, 0, 5, False),
               (3, 256, 1, 1, False)]


@functools.lru_cache(None)
def indexed_forward_case(heads, c, concat, de, msg):
    t, gr = indexed_inputs("rows", c, de, msg, 1, heads)
    want = gk.forward_ref(t, gr, concat, 2, torch.float64)[0]
    return t, gr, want, gk._err(gk.forward_ref(t, gr, concat, 2, torch.float32)[0], want)


@gpu
@pytest.mark.parametrize("heads,c,concat,de,msg", INDEXED_FWD)
def test_indexed_forward(eng, heads, c, concat, de, msg):
    """gigl_gat_aggregate_edge_indexed with eid (gat_edge_alpha_rows_kernel, the gathers' eid path; every 5th kept edge has
    eid = -1) against the float64 reference, and EQUAL to the dense call over the same attributes gathered into
    [positions][De] (zero rows where eid = -1): both calls run the same gather over the same values — a missing attribute
    is 0.f on the eid path and a sum of 0.f * v in the dense array's a_edge, the same float"""
    t, gr, want, e32 = indexed_forward_case(heads, c, concat, de, msg)
    ce, cap = gr.col.numel(), gr.cap
    dg, nr = gk._dev_graph(gr), gk._count(gr.n_live)
    hh, a_s, a_d, v, bias, w_msg = gk._f32(t.h), gk._f32(t.att_src), gk._f32(t.att_dst), gk._f32(t.v), gk._f32(t.bias[bool(concat)]), \
        gk._f32(t.w_msg)
    outs = []
    for attr, ids in ((gk._f32(t.tab), gk._i32(t.eid)), (gk._edge_attr(t, gr), None)):
        out = full(cap, heads * c if concat else c)
        scratch = torch.empty(2 * cap * heads + ce * heads, dtype=torch.float32, device="cuda")
        rc = eng._lib.gigl_gat_aggregate_edge_indexed(
            eng._ctx, p(hh), p(a_s), p(a_d), heads, c, SLOPE, concat, p(dg.rowptr), p(dg.rowend), p(dg.col), p(dg.meta), cap, p(nr), cap,
            p(bias), 1, p(attr), p(ids), de, ce, p(v), p(w_msg), p(scratch), p(out))
        torch.cuda.synchronize()
        assert rc == 0, rc
        outs.append(out.cpu())
    label = f"indexed fwd {heads}x{c} concat={concat} De{de} msg={msg} {gk.forward_path(heads, c, concat, de, msg)}"
    gk.check_forward(label + " eid", outs[0], want, e32, gr)
    gk.check_forward(label + " dense", outs[1], want, e32, gr)
    differ = outs[0][:gr.n_live] != outs[1][:gr.n_live]
    print(f"{label} eid against dense: {int(differ.sum())} of {differ.numel()} elements differ")
    assert torch.equal(outs[0][:gr.n_live], outs[1][:gr.n_live]), f"{label}: the eid call and the dense call differ"


# ---- CPU: the struct, the formula against gnn_ref.gat_conv, the inputs' conditions, the graph, the coverage ---------
def test_edge_terms_layout():
    assert C.sizeof(EdgeTerms) == 48 and EdgeTerms.ze.offset == 40 and EdgeTerms.edge_dim.offset == 16


def test_formula_against_gnn_ref():
    for window in (False, True):
        gr = rows_graph(window)
        n = gr.n_live
        ei = torch.stack([gr.col[gr.raw], gr.raw_dst])  # the live rows' windows, self loops included
        assert int((ei[0] == ei[1]).sum()) >= 4
        for d, heads, de, msg in ((12, 2, 0, False), (8, 1, 3, False), (12, 4, 5, True), (4, 2, 1, True)):
            t = layer_inputs("rows", d, heads, de, msg)
            c = t.c
            x = torch.nan_to_num(t.x[:N_NODES])
            g = torch.Generator().manual_seed(d)
            w, a_s0, a_d0 = gk._free(g, heads * c, d), gk._free(g, heads * c), gk._free(g, heads * c)
            wo = gk._free(g, n, heads * c)
            ea = w_edge = None
            leaves = [a_s0.clone().requires_grad_(True), a_d0.clone().requires_grad_(True)]
            leaves2 = [a_s0.clone().requires_grad_(True), a_d0.clone().requires_grad_(True)]
            att_e2 = v = None
            if de:
                ea, w_edge = edge_rows(t.tab, "rows", window), gk._free(g, heads * c, de)
                att_e = gk._free(g, heads, c).requires_grad_(True)
                att_e2 = att_e.detach().clone().requires_grad_(True)
                leaves.append(att_e)
                leaves2.append(att_e2)
                v = torch.einsum("hc,hck->hk", att_e, w_edge.view(heads, c, de))
            conv = gnn_ref.gat_conv(x, ei, w, leaves2[0], leaves2[1], t.bias, heads, True, SLOPE, ea[gr.raw] if de else None, w_edge,
                                    att_e2, t.w_msg)[:n]
            out, _, _ = layer_ref(gr, x, w, leaves[0], leaves[1], heads, c, t.bias, 0, ea, v, t.w_msg)
            assert gk._err(out, conv) <= 1e-12, (window, d, heads, de, msg)
            for a, b in zip(torch.autograd.grad((out * wo).sum(), leaves), torch.autograd.grad((conv * wo).sum(), leaves2)):
                assert gk._err(a, b) <= 1e-12, (window, d, heads, de, msg)


def ce_of(gr):
    return gr.col.numel()


def _assert_exact(pre, case):
    q = pre * 512
    assert torch.equal(q, q.round()) and float(q.abs().max()) < 2 ** 24, case


def test_inputs_graph_and_coverage():
    rows, where = base_rows()
    packed, win = rows_graph(False), rows_graph(True)
    # the graph
    assert N_ROWS % 32 == 3 and N_LIVE == N_ROWS - 5 and N_NODES == N_ROWS + 1 and CAP > N_NODES
    assert all(i % 3 != 1 and i < N_LIVE for i in where.values()) and len(set(where.values())) == len(where)
    for gr in (packed, win):
        assert [int(gr.m[where["deg%d" % m]]) for m in DEGREES] == DEGREES and int(gr.m[where["hub"]]) == HUB
        assert [int(gr.cnt[where["deg%d" % m]]) for m in DEGREES] == DEGREES
        for s in ("", "_hi"):
            assert int(gr.m[where["self_only" + s]]) == 1 and int(gr.cnt[where["self_only" + s]]) == 0
            assert int(gr.m[where["self_among" + s]]) == 6 and int(gr.cnt[where["self_among" + s]]) == 4
        assert int(gr.col.max()) <= NAN_NODE and int(gr.src.max()) < N_READ
    assert where["self_only"] < N_LOCAL and where["self_among"] < N_LOCAL < where["self_only_hi"] < where["self_among_hi"]
    assert 40 < N_LOCAL < N_LIVE - 40 and any(where["deg%d" % m] < N_LOCAL for m in DEGREES) and where["hub"] > N_LOCAL
    dup = rows[where["dup"]]
    assert dup.numel() - dup.unique().numel() == 1 and where["dup"] not in dup.tolist()
    short = win.rp[1:] - win.rowend
    assert int((short > 0).sum()) == N_ROWS // 3 and set(short[short > 0].tolist()) == {1, 2}
    assert int((win.col == NAN_NODE).sum()) == int(short.sum()) and not bool((packed.col == NAN_NODE).any())
    for window in (False, True):
        gr, eid = rows_graph(window), edge_ids("rows", window)
        ce = gr.col.numel()
        assert bool((eid[gr.unused] == ce).all()) and int((eid[gr.pos] == -1).sum()) == (gr.pos.numel() + 4) // 5
        assert int((eid == ce).sum()) == int(gr.unused.sum()) and int(eid.max()) == ce
    t = layer_inputs("rows", 256, 2, 3, True)
    gcol = global_col(t, win, N_LOCAL)
    row_of = torch.repeat_interleave(torch.arange(N_ROWS), win.rp[1:] - win.rp[:-1])
    far = row_of >= N_LOCAL
    assert torch.equal(gcol[~far], win.col[~far]) and torch.equal(gcol[far], t.perm[win.col[far]])
    assert bool((gcol[far] == t.perm[row_of[far]]).any())  # a stored self loop named by its global id
    assert bool(torch.isnan(t.table[t.perm[NAN_NODE]]).all())

    # the inputs: exact logits, the self loop's margin, large logits, the zero rows
    for case in AGG + LARGE:
        dt, d, heads, de, msg, scale, window = case
        t, gr, want, e32 = agg_case("rows", d, heads, de, msg, scale, window)
        assert torch.equal(t.table.half().double()[t.perm[:NAN_NODE]], t.x[:NAN_NODE]), case
        _assert_exact(want["pre"][:gr.pos.numel()], case)
        if de:
            assert float(want["pre"][gr.pos.numel():].abs().min()) >= 1e-3, case
        if scale > 1:
            on_hub = gr.dst == where["hub"]
            pre = want["pre"][:gr.pos.numel()]
            hi, lo = pre[on_hub].max(0).values, pre[on_hub].min(0).values  # per head: the hub row's largest logit, its range
            assert float(hi.max()) >= 20 and float((hi - lo).max()) >= 40, case
        assert not bool(t.dz[:, :N_LIVE][:, t.zero_rows].any()) and int(t.zero_rows.sum()) >= 25
    for n, case in LONG_FWD + LONG_BWD:
        dt, d, heads, de, msg, scale, window = case
        t, gr, want, _ = agg_case(n, d, heads, de, msg, scale, window)
        _assert_exact(want["pre"][:gr.pos.numel()], case)
        assert not de or float(want["pre"][gr.pos.numel():].abs().min()) >= 1e-3, case
    for dt, d, heads, de, msg, act, window in FUSED:
        t, gr, _, _, pre, _ = layer_case("rows", d, heads, de, msg, act, window)
        assert float((t.us * 64).abs().max()) <= 8 and torch.equal(t.us * 64, (t.us * 64).round())
        _assert_exact(pre[:gr.pos.numel()], (d, heads, de))
        assert not de or float(pre[gr.pos.numel():].abs().min()) >= 1e-3
    for dt, d, heads in TWOPASS:
        for window in (False, True):
            _assert_exact(layer_case("rows", d, heads, 0, False, int(d % 8 == 0), window)[4], (d, heads))
    for c, de, msg, scale in INDEXED:
        t, gr = indexed_inputs("rows", c, de, msg, scale)
        assert float(gk.self_logits(t, gr).abs().min()) >= 1e-3
        h64 = torch.nan_to_num(t.h)
        pre = gk._alphas(h64, t.att_src, 1, c)[gr.src] + gk._alphas(h64, t.att_dst, 1, c)[gr.dst] + (t.ea @ t.v.T)[gr.pos]
        _assert_exact(pre, (c, de))
        ok = (t.eid >= 0) & ~gr.unused
        assert torch.equal(t.tab[t.eid[ok]], t.ea[ok]) and not bool(t.ea[gr.pos[::5]].any()) and bool((t.eid[gr.pos[::5]] == -1).all())

    for heads, c, concat, de, msg in INDEXED_FWD:
        t, gr = indexed_inputs("rows", c, de, msg, 1, heads)
        assert float(gk.self_logits(t, gr).abs().min()) >= 1e-3
        h64 = torch.nan_to_num(t.h)
        pre = gk._alphas(h64, t.att_src, heads, c)[gr.src] + gk._alphas(h64, t.att_dst, heads, c)[gr.dst] + (t.ea @ t.v.T)[gr.pos]
        _assert_exact(pre, (heads, c, de))
        ok = (t.eid >= 0) & ~gr.unused
        assert torch.equal(t.tab[t.eid[ok]], t.ea[ok]) and not bool(t.ea[gr.pos[::5]].any()) and bool((t.eid[gr.pos[::5]] == -1).all())
        assert int((t.eid[gr.pos] == -1).sum()) >= 100 and bool((t.eid[gr.unused] == ce_of(gr)).all())

    # coverage, from the case tables and the restated dispatch
    fwd = {(dt, chunks_of(d), heads, de > 0) for dt, d, heads, de, msg, scale, window in AGG}
    assert fwd == {(dt, v, h, e) for dt in (F32, F16) for v in (1, 2, 3, 4) for h in (1, 2, 4) for e in (False, True)}
    bwd = {k for k in fwd if not (k[3] and k[2] == 4 and k[1] == 4)}
    assert {(dt, chunks_of(d), heads, de > 0) for dt, d, heads, de, *_ in AGG if backward_ok(d, heads, de > 0)} == bwd
    assert any(not backward_ok(d, heads, de > 0) for dt, d, heads, de, *_ in AGG)
    assert {forward_u(dt, chunks_of(d), heads, de > 0) for dt, d, heads, de, *_ in AGG} == {8, 4, 2}
    assert forward_u(F16, 3, 2, True) == 8 and forward_u(F32, 3, 2, False) == 4 and forward_u(F16, 3, 4, True) == 2
    assert {d for _, d, *_ in AGG} == {4, 256, 260, 516, 768, 772, 1000, 1024}
    assert {(dt, d) for dt, d, *_ in AGG} == {(dt, d) for dt in (F32, F16) for d in (4, 256, 260, 516, 768, 772, 1000, 1024)}
    assert [chunks_of(d) for d in (4, 256, 260, 516, 768, 772, 1000, 1024)] == [1, 1, 2, 3, 3, 4, 4, 4]
    assert {de for _, _, _, de, *_ in AGG if de} == set(DES) and max(DES) == MAX_DE
    assert {(de, msg) for _, _, _, de, msg, *_ in AGG if de} == {(de, msg) for de in DES for msg in (False, True)}
    assert {(de > 0, msg, window) for _, _, _, de, msg, _, window in AGG} >= {(True, True, True), (True, True, False),
                                                                               (True, False, True), (True, False, False),
                                                                               (False, False, True), (False, False, False)}
    assert {chunks_of(c[1]) for c in FUSED} == {1, 2, 3, 4} and {c[2] for c in FUSED} == {1, 2, 4} and {c[0] for c in FUSED} == {F32, F16}
    assert {(c[3] > 0, c[4]) for c in FUSED} == {(False, False), (True, False), (True, True)} and {c[5] for c in FUSED} == {0, 1}
    assert N_LIVE > 128  # two row tiles of the tiled operand
    assert {h for _, _, h in TWOPASS} == {1, 2, 4} and {chunks_of(d) for _, d, _ in TWOPASS} == {1, 2, 3, 4, 5}
    assert {n % 16 for n, *_ in SCORE_LONG} == {1, 7, 9, 15} and all(n > SCORE_SOURCES for n, *_ in SCORE_LONG)
    assert all(gk.long_graph(n).n_live > max(WAVE_CAPS["edge_weight"], WAVE_CAPS["gather_items"]) for n, *_ in SCORE_LONG)
    assert all(gk.long_graph(n).n_live > WAVE_CAPS["online"] for n, _ in LONG_FWD)
    assert all(gk.long_graph(n).n_live > WAVE_CAPS["onepass"] for n, _ in LONG_BWD)
    assert gk.long_graph(INDEXED_LONG[0]).n_live > WAVE_CAPS["indexed"]
    assert {1 if c <= 256 else 2 for c, *_ in INDEXED} == {1, 2} and {c for c, *_ in INDEXED} == {4, 252, 256, 260, 512}
    assert {de for _, de, *_ in INDEXED} == set(DES) and {m for _, _, m, _ in INDEXED} == {False, True}
    assert {gk.forward_path(h, c, cc, de, m) for h, c, cc, de, m in INDEXED_FWD} == {"fast", "generic"}
    assert {cap for cap, *_ in MSG} >= {63, 64, 65, 130} and MSG_ROWS == 64
    assert any(cap * h * c > 4096 * 256 and cap * h * de > 4096 * 256 for cap, _, h, c, de in MSG)
