"""TEST INFRASTRUCTURE ONLY: the graphs, inputs, float64 references, case lists, bounds and dispatch restatements of
tests/test_gpu_hetero_kernels.py (csrc/hetero.hip) and tests/test_gpu_conv_kernels.py (csrc/gatv2.hip).

Every reference is an edge-list formula whose dtype follows its inputs (float64: the reference; float32: the same formula's
own error, which the bounds are measured against) and whose leaves are the kernel's own inputs, so torch.autograd.grad
returns exactly what the backward kernel returns.  Nothing here is derived from a kernel's output.

Run as a program (`python tests/attn_cases.py hgt <in.pt> <out.pt>`) it is the CHILD of the packed-versus-unpacked test:
GIGL_HGT_NO_PACK is read once per process, so the parent sets it in the child's environment; the child runs
gigl_hgt_aggregate_act on every case of <in.pt> and saves the outputs to <out.pt>."""
import ctypes as C
import functools
import math
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SLOPE = 0.2
SENTINEL = 7.0
E_UNSUPPORTED = -4
INF = float("inf")
NAN = float("nan")

# ---- the "rows" graph -----------------------------------------------------------------------------------------------
# 131 rows in the CSR (3 mod 8), 127 live (*n_rows_dev / n_dst: 7 mod 8, 3 mod 4, 1 mod 2 — a short last wave of the packed
# kernel at every G); sources are < N_READ, so the nodes 128 and 129 are read by nobody; node 130 is a row of NaN that only
# the entries a window skips name; the buffers hold CAP rows.
N_ROWS, N_LIVE, N_READ, NAN_NODE, N_NODES, CAP = 131, 127, 128, 130, 131, 136
DEGREES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65]
HUB = 300
N_ETYPES = 3


def _others(g, i, n, hi):
    """n sources in [0, hi) that are not i"""
    r = torch.randint(0, hi - 1, (n,), generator=g)
    return r + (r >= i)


@functools.lru_cache(None)
def base_rows():
    """-> (rows, index of every special row by name).  The special rows sit at i % 3 != 1, which no window shortens; the
    degree-0 row, the degree-1 row and the hub are the rows 0, 2 and 3: one wave of the packed kernel at G = 8"""
    g = torch.Generator().manual_seed(43)
    specs = [("deg0", 0), ("deg1", 1), ("hub", HUB)] + [("deg%d" % d, d) for d in DEGREES[2:]] + \
            [("self_only", 0), ("self_twice", 0), ("dup", 0)]
    free = [i for i in range(N_LIVE) if i % 3 != 1]
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
        else:
            rows[i] = _others(g, i, m, N_READ)
    for i in range(N_ROWS):
        if rows[i] is None:  # the rest: degree 0..6 (the rows a window shortens: 1..6)
            rows[i] = _others(g, i, max(int(torch.randint(0, 7, (1,), generator=g)), int(i % 3 == 1)), N_READ)
    return rows, where


def _graph_of(rows, window, n_live, nan_node, cap):
    """with `window` every row i % 3 == 1 ends 1 or 2 entries early and the skipped entries name the NaN node.
    raw / raw_dst: the col positions of the live rows inside their windows and their rows (self loops included);
    pos / src / dst: those of them that are no self loop (GATv2 drops the listed ones); cnt: their number per live row"""
    deg = torch.tensor([r.numel() for r in rows])
    rp = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(deg, 0)])
    col, rowend = torch.cat(rows).clone(), rp[1:].clone()
    p = torch.arange(col.numel())
    row_of = torch.repeat_interleave(torch.arange(len(rows)), deg)
    if window:
        short = torch.arange(len(rows)) % 3 == 1
        rowend = rowend - torch.minimum(deg, 1 + (torch.arange(len(rows)) // 3) % 2) * short
        col[p >= rowend[row_of]] = nan_node
    used = (p < rowend[row_of]) & (row_of < n_live)
    keep = used & (col != row_of)
    cnt = torch.zeros(n_live, dtype=torch.int64).index_add_(0, row_of[keep], torch.ones_like(p[keep]))
    return types.SimpleNamespace(rp=rp, rowend=rowend, col=col, window=window, m=rowend - rp[:-1], pos=p[keep],
                                 src=col[keep], dst=row_of[keep], cnt=cnt, raw=p[used], raw_src=col[used],
                                 raw_dst=row_of[used], used=used, keep=keep, n_rows=len(rows), n_live=n_live,
                                 nan_node=nan_node, cap=cap, kind="rows" if len(rows) == N_ROWS else len(rows))


@functools.lru_cache(None)
def rows_graph(window=False):
    return _graph_of(base_rows()[0], window, N_LIVE, NAN_NODE, CAP)


LONG_N = 16400


@functools.lru_cache(None)
def long_graph():
    """16 400 rows of degree 0..3 over as many sources (self loops as they fall), 5 fewer live, node n a row of NaN: more
    rows than the capped grids have waves (16 384; GATv2 backward 4 096)"""
    n = LONG_N
    g = torch.Generator().manual_seed(n)
    deg = torch.randint(0, 4, (n,), generator=g)
    col = torch.randint(0, n, (int(deg.sum()),), generator=g)
    return _graph_of(list(torch.split(col, deg.tolist())), False, n - 5, n, n + 8)


def graph(kind, window=False):
    return rows_graph(window) if kind == "rows" else long_graph()


# ---- the dispatch, restated from hetero.hip and gatv2.hip (the CPU tests assert that every path is run) --------------
def instantiation(n):
    """dispatch_int<1, 2, 4>: the first listed value equal to n, else the last"""
    return n if n in (1, 2) else 4


def lanes_per_head(dim):
    return dim // 4


def hgt_supported(heads, dim):
    """check_shape"""
    lph = dim // 4
    return heads >= 1 and dim >= 4 and dim % 4 == 0 and lph & (lph - 1) == 0 and lph <= 64 and heads * dim <= 1024


def hgt_passes(heads, dim):
    return (heads * dim + 255) // 256


def hgt_partial(heads, dim):
    """a partially filled last pass"""
    return heads * dim % 256 != 0


def hgt_forward_path(heads, dim, no_pack=False):
    """gigl_hgt_aggregate_act: ("packed", G) or ("unpacked", PASSES of the instantiation)"""
    g = heads * dim // 4
    if not no_pack and g in (8, 16, 32) and dim // 4 <= 16:
        return "packed", g
    return "unpacked", instantiation(hgt_passes(heads, dim))


def conv_shape(heads, c):
    """gatv2_shape: (V, the instantiation it lands on, lanes per head), or None when refused"""
    gl, chunks = c // 4, heads * c // 4
    v = (chunks + 63) // 64
    ok = c % 4 == 0 and 1 <= gl <= 64 and gl & (gl - 1) == 0 and 1 <= v <= 4
    return (v, instantiation(v), gl) if ok else None


FWD_WAVES, GATV2_BWD_WAVES = 4096 * 4, 1024 * 4  # the capped grids, in waves (= rows per sweep of the strided loop)

# ---- shapes ----------------------------------------------------------------------------------------------------------
HGT_PACKED = {8: [(8, 4), (2, 16), (1, 32)], 16: [(8, 8), (4, 16), (1, 64)], 32: [(8, 16), (2, 64)]}
HGT_UNPACKED = {1: [(1, 4), (3, 16), (5, 32), (1, 128), (1, 256)], 2: [(3, 128), (2, 256)], 3: [(3, 256), (6, 128)],
                4: [(4, 256), (16, 64), (64, 16)]}  # by pass count
HGT_SHAPES = [s for g in (8, 16, 32) for s in HGT_PACKED[g]] + [s for p in (1, 2, 3, 4) for s in HGT_UNPACKED[p]]
# the weighted aggregate and both backwards: every pass count and every lanes-per-head value (no packed path)
WIDE_SHAPES = [(1, 4), (8, 8), (3, 16), (5, 32), (1, 64), (3, 128), (2, 256), (3, 256), (6, 128), (16, 64), (64, 16)]
HGT_LARGE = [(4, 16), (3, 128)]  # q times 30: logits beyond +-50 (packed; two passes)
RELS = ["typed", "one_type", "plain"]  # etype and p_rel; p_rel alone (every edge of type 0); neither
CONV_SHAPES = {1: [(1, 4), (2, 16), (1, 128), (1, 256), (4, 64)], 2: [(3, 128), (2, 256), (8, 64)],
               3: [(3, 256), (6, 128)], 4: [(4, 256), (16, 64)]}  # by V
CONV_ALL = [s for v in (1, 2, 3, 4) for s in CONV_SHAPES[v]]
CONV_LARGE = (2, 256)
REFUSED = [(2, 5), (2, 12), (1, 512), (257, 4)]  # dim 5, dim 12, dim 512, heads * dim = 1028
GINE_D = [1, 3, 63, 64, 65, 130, 256]
GINE_EPS = [0.0, 0.37]
LONG_SHAPE = (1, 4)
LONG_D = 3


# ---- helpers of the references ---------------------------------------------------------------------------------------
def grid(g, den, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double() / den


def free(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32).double()


def make_dout(g, rows, width):
    """random fp32 values; every 7th row is all zero"""
    d = free(g, rows, width)
    d[torch.arange(rows) % 7 == 3] = 0.0
    return d


def seg_softmax(z, index, n, eps):
    """softmax of z [E, H] within the groups of index [E]: max-shifted, denominator + eps"""
    mx = torch.full((n, z.shape[1]), -INF, dtype=z.dtype).scatter_reduce(0, index[:, None].expand_as(z), z.detach(),
                                                                         reduce="amax")
    ex = torch.exp(z - mx[index])
    den = torch.zeros((n, z.shape[1]), dtype=z.dtype).index_add(0, index, ex)
    return ex / (den[index] + eps)


def err(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max()) if a.numel() else 0.0


def bound(want, e32, grad):
    """the project's tolerances (forward rtol = atol = 1e-5; gradients rtol = 1e-4, atol = 1e-4 * max|want|), or 4 x the
    float32 reference's own maximum error where that is larger (0 on the long graph: the project tolerance only)"""
    want = want.detach().double()
    rtol = 1e-4 if grad else 1e-5
    atol = 1e-4 * float(want.abs().max()) if grad and want.numel() else 1e-5
    return torch.clamp(atol + rtol * want.abs(), min=4.0 * e32)


def beyond(got, want, e32, grad):
    """how many elements of got miss the bound"""
    got, want = got.detach().double().cpu(), want.detach().double()
    return int(((got - want).abs() > bound(want, e32, grad)).sum())


def check(label, name, got, want, e32, grad=False):
    got, want = got.detach().double().cpu(), want.detach().double()
    assert got.shape == want.shape, (label, name, got.shape, want.shape)
    e = (got - want).abs()
    print(f"{label} {name}: err={float(e.max()) if e.numel() else 0.0:.3e} fp32={e32:.3e}")
    assert bool(torch.isfinite(got).all()), f"{label} {name}: non-finite values"
    bad = beyond(got, want, e32, grad)
    assert bad == 0, (f"{label} {name}: {bad} of {got.numel()} beyond the bound, max err {float(e.max()):.3e} "
                      f"(float32 reference {e32:.3e})")


def _leaf(x, dt):
    """(a NaN row is read by nobody; as a leaf it would have a NaN gradient)"""
    return torch.nan_to_num(x.to(dt)).requires_grad_(True)


def _grads(out, dout, leaves):
    g = torch.autograd.grad((out * dout).sum(), list(leaves.values()), allow_unused=True)
    return {"d" + k: (torch.zeros_like(x) if gx is None else gx) for (k, x), gx in zip(leaves.items(), g)}


def _both(fn, kind):
    """-> (float64 results, the float32 formula's maximum error per tensor)"""
    want = fn(torch.float64)
    if kind != "rows":
        return want, {k: 0.0 for k in want}
    lo = fn(torch.float32)
    return want, {k: err(lo[k], want[k]) for k in want}


# ---- HGT and the weighted aggregate ----------------------------------------------------------------------------------
def hgt_ref(gr, heads, dim, q, k, v, etype, p_rel, gelu=False, wrong=None):
    """logit_e = <q_i, k_j> p_rel[t_e, h] / sqrt(D), softmax over the in-edges of i, out_i = sum_e alpha_e v_j (an empty
    row gives 0), optional exact-erf GELU: [n_live, H*D].  wrong: a deliberately wrong variant (the bounds must notice)"""
    n, src, dst = gr.n_live, gr.raw_src, gr.raw_dst
    d = (q[dst].view(-1, heads, dim) * k[src].view(-1, heads, dim)).sum(-1)
    if wrong == "head_pair":  # the head sum taken over two heads
        d = d.view(-1, heads // 2, 2).sum(-1, keepdim=True).expand(-1, -1, 2).reshape(-1, heads)
    z = d if wrong == "no_scale" else d / math.sqrt(dim)
    if p_rel is not None and wrong != "no_p_rel":
        z = z * p_rel[etype[gr.raw] if etype is not None else torch.zeros_like(src)]
    a = seg_softmax(z, dst, n, 0.0)
    out = torch.zeros(n, heads, dim, dtype=q.dtype).index_add(0, dst, a[:, :, None] * v[src].view(-1, heads, dim))
    out = out.reshape(n, heads * dim)
    if gelu:
        out = torch.nn.functional.gelu(out)
    if wrong == "second_pass":  # the second 256-float pass zeroed
        out = torch.cat([out[:, :256], torch.zeros_like(out[:, 256:512]), out[:, 512:]], 1)
    return out


def hgt_logits(t, gr):
    """float64 logits of the live edges, [E, H]"""
    d = (t.q[gr.raw_dst].view(-1, t.heads, t.dim) * t.k[gr.raw_src].view(-1, t.heads, t.dim)).sum(-1) / math.sqrt(t.dim)
    return d * t.p_rel[t.etype[gr.raw]]


@functools.lru_cache(None)
def hgt_inputs(heads, dim, scale=1):
    """float64 values of fp32 numbers: q / dout [N_ROWS, H*D] (q is NaN past the live rows), k / v [N_NODES, H*D] (the
    last row NaN), etype per col entry, p_rel [3, H], alpha [entries, H] (arbitrary, not normalised)"""
    gr = rows_graph()
    g = torch.Generator().manual_seed(100 * heads + dim + 7 * scale)
    hd = heads * dim
    t = types.SimpleNamespace(heads=heads, dim=dim, scale=scale)
    t.q, t.k, t.v = scale * free(g, N_ROWS, hd), free(g, N_NODES, hd), free(g, N_NODES, hd)
    t.q[N_LIVE:], t.k[NAN_NODE:], t.v[NAN_NODE:] = NAN, NAN, NAN
    t.etype = torch.randint(0, N_ETYPES, (gr.col.numel(),), generator=g)
    t.p_rel = (0.5 + torch.rand(N_ETYPES, heads, generator=g, dtype=torch.float32).double()) * \
        (1 - 2 * torch.randint(0, 2, (N_ETYPES, heads), generator=g).double())
    t.alpha = free(g, gr.col.numel(), heads)
    t.dout = make_dout(g, N_ROWS, hd)
    t.zero_rows = torch.arange(N_LIVE) % 7 == 3
    return t


def hgt_rel(t, rel):
    """-> (etype, p_rel) of the variant"""
    return (t.etype if rel == "typed" else None), (None if rel == "plain" else t.p_rel)


def _hgt_eval(t, gr, rel, gelu, dt):
    etype, p_rel = hgt_rel(t, rel)
    leaves = {"q": _leaf(t.q, dt), "k": _leaf(t.k, dt), "v": _leaf(t.v, dt)}
    if p_rel is not None:
        leaves["p_rel"] = _leaf(p_rel, dt)
    out = hgt_ref(gr, t.heads, t.dim, leaves["q"], leaves["k"], leaves["v"], etype, leaves.get("p_rel"), gelu)
    r = {"out": out.detach()}
    if not gelu:  # (the backward kernel is that of the reduce alone)
        r.update(_grads(out, t.dout[:gr.n_live].to(dt), leaves))
    return r


@functools.lru_cache(None)
def hgt_case(heads, dim, rel="typed", gelu=False, scale=1):
    t, gr = hgt_inputs(heads, dim, scale), rows_graph()
    return (t, gr) + _both(lambda dt: _hgt_eval(t, gr, rel, gelu, dt), "rows")


def weighted_ref(gr, heads, dim, alpha, v):
    """out_i = sum_e alpha[e, h] v_j; alpha [entries, H] is indexed at the live entries only"""
    a = alpha[gr.raw]
    out = torch.zeros(gr.n_live, heads, dim, dtype=v.dtype).index_add(0, gr.raw_dst,
                                                                      a[:, :, None] * v[gr.raw_src].view(-1, heads, dim))
    return out.reshape(gr.n_live, heads * dim)


@functools.lru_cache(None)
def weighted_case(heads, dim):
    t, gr = hgt_inputs(heads, dim), rows_graph()

    def run(dt):
        leaves = {"alpha": _leaf(t.alpha, dt), "v": _leaf(t.v, dt)}
        out = weighted_ref(gr, heads, dim, leaves["alpha"], leaves["v"])
        return dict({"out": out.detach()}, **_grads(out, t.dout[:gr.n_live].to(dt), leaves))
    return (t, gr) + _both(run, "rows")


# ---- SimpleHGN alpha -------------------------------------------------------------------------------------------------
SHGN_NODES, SHGN_LONE, SHGN_NEG, SHGN_HUB, SHGN_FIRST_SINK = 40, 0, 1, 2, 30  # sources 30..39 have no out-edge


@functools.lru_cache(None)
def shgn_graph(kind):
    """"small": 257 edges; "hub": the same and 1 000 more out of node 2.  Node 0 has one out-edge, node 1 twelve (its
    logits are all negative by its hl), the nodes 30..39 none; node 40 is a row of NaN"""
    g = torch.Generator().manual_seed(7)
    src = torch.cat([torch.tensor([SHGN_LONE]), torch.full((12,), SHGN_NEG),
                     torch.randint(2, SHGN_FIRST_SINK, (244,), generator=g)])
    if kind == "hub":
        src = torch.cat([src, torch.full((1000,), SHGN_HUB)])
    src = src[torch.randperm(src.numel(), generator=g)]
    dst = torch.randint(0, SHGN_NODES, (src.numel(),), generator=g)
    et = torch.randint(0, N_ETYPES, (src.numel(),), generator=g)
    return types.SimpleNamespace(src=src, dst=dst, etype=et, n=SHGN_NODES, kind=kind)


def shgn_ref(gr, hl, hr, het, hef, slope, wrong=None):
    """leaky_relu(hl[src] + hr[dst] + het[etype] [+ hef]), softmax over the edges sharing the SOURCE, denominator + 1e-16"""
    x = hl[gr.src] + hr[gr.dst] + het[gr.etype]
    if hef is not None:
        x = x + hef
    x = torch.nn.functional.leaky_relu(x, slope)
    return seg_softmax(x, gr.dst if wrong == "by_dst" else gr.src, gr.n, 1e-16)


# (heads, graph, hef, slope, scale of hr): 257 edges at 3 heads end 3 threads into a fourth block
SHGN_CASES = [(h, "small", ef, SLOPE, 1) for h in (1, 2, 3, 8) for ef in (False, True)] + \
             [(3, "hub", True, SLOPE, 1), (8, "hub", False, SLOPE, 1), (1, "hub", True, SLOPE, 1),
              (3, "small", True, 0.0, 1), (2, "hub", False, 0.0, 1),
              (3, "small", True, SLOPE, 512), (2, "hub", False, SLOPE, 512)]


@functools.lru_cache(None)
def shgn_inputs(heads, kind, ef, scale):
    """hl, hr, het, hef on multiples of 1/8 (hr times `scale`): the leaky_relu input is exact in fp32"""
    gr = shgn_graph(kind)
    g = torch.Generator().manual_seed(10 * heads + ef + scale)
    t = types.SimpleNamespace(heads=heads, scale=scale)
    t.hl, t.hr = grid(g, 8, -8, 8, gr.n + 1, heads), scale * grid(g, 8, -8, 8, gr.n + 1, heads)
    t.hl[SHGN_NEG] = -(scale + 3.0)  # hr + het + hef <= scale + 2: every logit of this source is negative
    t.hl[gr.n:], t.hr[gr.n:] = NAN, NAN
    t.het = grid(g, 8, -8, 8, N_ETYPES, heads)
    t.hef = grid(g, 8, -8, 8, gr.src.numel(), heads) if ef else None
    return t


def shgn_pre(t, gr):
    """the pre-activations, float64 [E, H]"""
    x = t.hl[gr.src] + t.hr[gr.dst] + t.het[gr.etype]
    return x + t.hef if t.hef is not None else x


@functools.lru_cache(None)
def shgn_case(heads, kind, ef, slope, scale):
    t, gr = shgn_inputs(heads, kind, ef, scale), shgn_graph(kind)
    run = lambda dt: {"alpha": shgn_ref(gr, t.hl.to(dt), t.hr.to(dt), t.het.to(dt), None if t.hef is None else t.hef.to(dt),
                                        slope)}
    return (t, gr) + _both(run, "rows")


# ---- GATv2 -----------------------------------------------------------------------------------------------------------
def gatv2_ref(gr, heads, c, xl, xr, att, xe=None, slope=SLOPE, wrong=None):
    """self loops among the edges dropped, one added per live row (with edge rows: carrying the mean of the row's kept
    edge rows, 0 when none are kept); z = <att_h, leaky_relu(xl_j + xr_i [+ xe])>; softmax over the in-edges of i,
    denominator + 1e-16; out_i = sum alpha xl_j.  -> (out [n_live, H*C] before bias and activation, s of the self loops)
    xe [entries, H*C] is indexed at the kept entries only"""
    n, dt = gr.n_live, xl.dtype
    loops = torch.arange(n)
    pos, esrc, edst = (gr.raw, gr.raw_src, gr.raw_dst) if wrong == "keep_self" else (gr.pos, gr.src, gr.dst)
    src, dst = torch.cat([esrc, loops]), torch.cat([edst, loops])
    s = xl[src] + xr[dst]
    if xe is not None:
        e = xe[pos]
        mean = torch.zeros(n, e.shape[1], dtype=dt).index_add(0, edst, e)
        if wrong == "self_zero":
            mean = mean * 0
        elif wrong != "self_sum":
            cnt = torch.zeros(n, dtype=dt).index_add(0, edst, torch.ones(edst.numel(), dtype=dt))
            mean = mean / cnt.clamp(min=1)[:, None]
        s = s + torch.cat([e, mean])
    z = (torch.nn.functional.leaky_relu(s, slope).view(-1, heads, c) * att.view(1, heads, c)).sum(-1)
    a = seg_softmax(z, dst, n, 1e-16)
    out = torch.zeros(n, heads, c, dtype=dt).index_add(0, dst, xl[src].view(-1, heads, c) * a[:, :, None])
    return out.reshape(n, heads * c), s[-n:]


def _self_s(t, gr):
    """float64 s of the live rows' self loops, [n_live, H*C]"""
    xl = torch.nan_to_num(t.xl)
    return gatv2_ref(gr, t.heads, t.c, xl, torch.nan_to_num(t.xr), t.att, t.xe)[1]


@functools.lru_cache(None)
def gatv2_inputs(kind, heads, c, edge, scale=1):
    """xl, xr [cap, H*C] and xe [entries, H*C] on multiples of 1/8 in [-1, 1] (zeros included), shared by the packed and the
    windowed graph: xl_j + xr_i + xe_e is exact in fp32, so the kernel's and the reference's `> 0` masks agree by
    construction.  The one inexact sum is the self loop's, through its mean edge row: where the float64 |s_self| is below
    1e-3 the channel of xr[i] is drawn again.  att (times `scale`), bias and dout are free"""
    graphs = [rows_graph(False), rows_graph(True)] if kind == "rows" else [long_graph()]
    gr = graphs[0]
    g = torch.Generator().manual_seed(1000 * heads + 7 * c + edge + 100 * scale + (kind != "rows"))
    hc = heads * c
    t = types.SimpleNamespace(heads=heads, c=c, edge=edge, scale=scale, redrawn=0)
    t.xl, t.xr = grid(g, 8, -8, 8, gr.cap, hc), grid(g, 8, -8, 8, gr.cap, hc)
    t.att = scale * grid(g, 8, -8, 8, hc)
    t.xe = grid(g, 8, -8, 8, gr.col.numel(), hc) if edge else None
    for _ in range(100 if edge else 0):
        bad = torch.zeros(gr.cap, hc, dtype=torch.bool)
        for x in graphs:
            bad[:x.n_live] |= _self_s(t, x).abs() < 1e-3
        if not bool(bad.any()):
            break
        t.xr[bad] = grid(g, 8, -8, 8, int(bad.sum()))
        t.redrawn += int(bad.sum())
    t.xl[gr.nan_node:] = NAN
    t.xr[gr.n_live:] = NAN  # (row i reads xr[i]: only live rows do)
    t.bias = free(g, hc)
    t.dout = make_dout(g, gr.cap, hc)
    t.zero_rows = torch.arange(gr.n_live) % 7 == 3
    return t


def _gatv2_eval(t, gr, dt):
    leaves = {"xl": _leaf(t.xl, dt), "xr": _leaf(t.xr, dt), "att": _leaf(t.att, dt)}
    if t.edge:
        leaves["xe"] = _leaf(t.xe, dt)
    out, _ = gatv2_ref(gr, t.heads, t.c, leaves["xl"], leaves["xr"], leaves["att"], leaves.get("xe"))
    return dict({"out": out.detach()}, **_grads(out, t.dout[:gr.n_live].to(dt), leaves))


@functools.lru_cache(None)
def gatv2_case(kind, heads, c, edge, window=False, scale=1):
    t, gr = gatv2_inputs(kind, heads, c, edge, scale), graph(kind, window)
    return (t, gr) + _both(lambda dt: _gatv2_eval(t, gr, dt), kind)


def finish(out, bias, mode, dt=torch.float64):
    """mode 0: no bias; 1: bias; 2: bias and ReLU (the forward only; the backward takes the pre-bias output)"""
    if mode:
        out = out + bias.to(dt)
    return torch.relu(out) if mode == 2 else out


# ---- GINE ------------------------------------------------------------------------------------------------------------
def gine_ref(gr, x, ee, eps):
    """(1 + eps) x_i + sum relu(x_j + ee_e) over the row's window (self loops are ordinary edges): [n_live, d]"""
    n = gr.n_live
    msg = torch.relu(x[gr.raw_src] + ee[gr.raw])
    return (1.0 + eps) * x[:n] + torch.zeros(n, x.shape[1], dtype=x.dtype).index_add(0, gr.raw_dst, msg)


@functools.lru_cache(None)
def gine_inputs(kind, d):
    """x [cap, d] and ee [entries, d] on multiples of 1/8 in [-1, 1]: x_j + ee_e is exact, messages of exactly 0 included"""
    gr = graph(kind)
    g = torch.Generator().manual_seed(31 * d + (kind != "rows"))
    t = types.SimpleNamespace(d=d)
    t.x, t.ee = grid(g, 8, -8, 8, gr.cap, d), grid(g, 8, -8, 8, gr.col.numel(), d)
    t.x[gr.nan_node:] = NAN
    t.dout = make_dout(g, gr.cap, d)
    t.zero_rows = torch.arange(gr.n_live) % 7 == 3
    return t


@functools.lru_cache(None)
def gine_case(kind, d, eps, window=False):
    t, gr = gine_inputs(kind, d), graph(kind, window)

    def run(dt):
        e = torch.tensor(float(torch.tensor(eps, dtype=torch.float32)), dtype=dt)  # (the kernel's eps is an fp32 value)
        leaves = {"x": _leaf(t.x, dt), "ee": _leaf(t.ee, dt), "eps": e.requires_grad_(True)}
        out = gine_ref(gr, leaves["x"], leaves["ee"], leaves["eps"])
        return dict({"out": out.detach()}, **_grads(out, t.dout[:gr.n_live].to(dt), leaves))
    return (t, gr) + _both(run, kind)


# ---- edge-Transformer ------------------------------------------------------------------------------------------------
def trans_ref(gr, heads, c, q, k, v, xe=None, wrong=None):
    """softmax of <q_i, k_j + xe_e> / sqrt(C) over the row's window, denominator + 1e-16, out_i = sum alpha_e (v_j + xe_e);
    no self loops are added and an empty row gives 0: [n_live, H*C]"""
    n, src, dst = gr.n_live, gr.raw_src, gr.raw_dst
    kk, vv = k[src], v[src]
    if xe is not None:
        kk = kk + xe[gr.raw]
        vv = vv if wrong == "no_xe_values" else vv + xe[gr.raw]
    z = (q[dst].view(-1, heads, c) * kk.view(-1, heads, c)).sum(-1)
    z = z if wrong == "no_scale" else z / math.sqrt(c)
    a = seg_softmax(z, dst, n, 1e-16)
    out = torch.zeros(n, heads, c, dtype=q.dtype).index_add(0, dst, a[:, :, None] * vv.view(-1, heads, c))
    return out.reshape(n, heads * c)


@functools.lru_cache(None)
def trans_inputs(kind, heads, c, scale=1):
    gr = graph(kind)
    g = torch.Generator().manual_seed(500 * heads + 3 * c + scale + (kind != "rows"))
    hc = heads * c
    t = types.SimpleNamespace(heads=heads, c=c, scale=scale)
    t.q, t.k, t.v = scale * free(g, gr.cap, hc), free(g, gr.cap, hc), free(g, gr.cap, hc)
    t.xe = free(g, gr.col.numel(), hc)
    t.q[gr.n_live:], t.k[gr.nan_node:], t.v[gr.nan_node:] = NAN, NAN, NAN
    t.dout = make_dout(g, gr.cap, hc)
    t.zero_rows = torch.arange(gr.n_live) % 7 == 3
    return t


def trans_logits(t, gr):
    kk = torch.nan_to_num(t.k)[gr.raw_src] + t.xe[gr.raw]
    return (t.q[gr.raw_dst].view(-1, t.heads, t.c) * kk.view(-1, t.heads, t.c)).sum(-1) / math.sqrt(t.c)


@functools.lru_cache(None)
def trans_case(kind, heads, c, window=False, scale=1):
    t, gr = trans_inputs(kind, heads, c, scale), graph(kind, window)

    def run(dt):
        leaves = {"q": _leaf(t.q, dt), "k": _leaf(t.k, dt), "v": _leaf(t.v, dt), "xe": _leaf(t.xe, dt)}
        out = trans_ref(gr, heads, c, *leaves.values())
        return dict({"out": out.detach()}, **_grads(out, t.dout[:gr.n_live].to(dt), leaves))
    return (t, gr) + _both(run, kind)


# ---- device side -----------------------------------------------------------------------------------------------------
def i32(t):
    return None if t is None else t.to(torch.int32).cuda()


def f32(t):
    return None if t is None else t.float().cuda()


def count(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def full(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")


def dev_graph(gr):
    return types.SimpleNamespace(rowptr=i32(gr.rp[:-1]), rowend=i32(gr.rowend), col=i32(gr.col))


def nan_where(x, mask):
    """x as the kernel gets it: NaN at the entries nobody may read"""
    x = x.clone()
    x[mask] = NAN
    return f32(x)


def padded(want, rows, fill=NAN):
    """the reference output rounded to fp32, `fill` in the rows past the live ones"""
    out = torch.full((rows, want.shape[1]), fill, dtype=torch.float64)
    out[:want.shape[0]] = want
    return f32(out)


def raw_call(eng, name, *args):
    """an entry point called on buffers of our own (tensors by their pointers): -> its return code"""
    rc = getattr(eng._lib, name)(eng._ctx, *[C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args])
    torch.cuda.synchronize()
    return rc


def run_hgt(eng, t, gr, rel, gelu):
    etype, p_rel = hgt_rel(t, rel)
    out = full(N_ROWS, t.heads * t.dim)
    eng.hgt_aggregate(f32(t.q), f32(t.k), f32(t.v), t.heads, t.dim, i32(gr.rp), i32(gr.col), i32(etype), f32(p_rel),
                      gr.n_live, out, gelu=gelu)
    return out.cpu()


def _child(argv):
    from gigl_amd.engine import HipEngine
    cases = torch.load(argv[1])
    eng = HipEngine(0)
    outs = []
    for c in cases:
        out = full(*c["shape"])
        eng.hgt_aggregate(f32(c["q"]), f32(c["k"]), f32(c["v"]), c["heads"], c["dim"], c["rowptr"].cuda(), c["col"].cuda(),
                          None if c["etype"] is None else c["etype"].cuda(), f32(c["p_rel"]), c["n_dst"], out, gelu=c["gelu"])
        outs.append(out.cpu())
    torch.cuda.synchronize()
    eng.close()
    torch.save(outs, argv[2])
    return 0


if __name__ == "__main__":
    assert sys.argv[1] == "hgt" and len(sys.argv) == 4, sys.argv
    sys.exit(_child(sys.argv[1:]))
