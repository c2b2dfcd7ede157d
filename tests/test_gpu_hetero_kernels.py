"""The attention reduces of csrc/hetero.hip — hgt_aggregate_kernel<1|2|4>, hgt_aggregate_packed_kernel<8|16|32>,
hgt_aggregate_backward_kernel<1|2|4>, weighted_aggregate_kernel<1|2|4> and its backward, the three kernels of
gigl_simplehgn_alpha with atomic_max_float — called directly through HipEngine.hgt_aggregate / hgt_aggregate_backward /
weighted_aggregate / weighted_aggregate_backward / simplehgn_alpha against float64 references computed on the CPU, at the
shapes where the dispatch code changes path.  The conventions are those of tests/test_gpu_gat_kernels.py; the graphs,
inputs, references, case lists and the restated dispatch live in tests/attn_cases.py.

References: hgt_ref, weighted_ref, shgn_ref — edge-list formulas whose leaves are the kernels' own inputs (q, k, v, p_rel;
alpha, v), so torch autograd gives exactly what the backward kernels return.  The CPU test at the end pins them at 1e-12
against oracle/gnn_ref.py's hgt_conv (identity projections and relation transforms: outputs and the gradients of q, k, v)
and simplehgn_conv (outputs and the gradient of the node features).  `out` handed to the backward is the float64
reference output rounded to fp32.

Inputs: HGT and the weighted aggregate have no masks: q, k, v, alpha (arbitrary, not normalised), p_rel (|p| in
[0.5, 1.5], both signs) and dout are random fp32 values, every 7th dout row is all zero; q times 30 in the large-logit
cases (logits beyond +-50 on the hub row).  SimpleHGN's hl, hr, het, hef sit on multiples of 1/8 (hr times 512 in the
large cases), so the leaky_relu input is exact.  NaN: the source row past the last referenced one, q and dout past
n_dst, alpha at the entries of the rows past n_dst, the node past the last one of hl / hr.  Outputs are pre-filled with a
sentinel.

Graph "rows" (attn_cases.rows_graph): 131 rows, n_dst = 127 (7 mod 8, 3 mod 4, 1 mod 2: a short last wave of the packed
kernel at every G), in-degrees 0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65 and a hub of 300; the
degree-0 row, the degree-1 row and the hub are rows 0, 2, 3 (one wave of the packed kernel at G = 8); a duplicated edge, a
row listing itself twice, a row whose only edge is itself; 3 edge types; etype and p_rel both present, p_rel alone,
neither.  SimpleHGN: 257 edges over 40 nodes (at 3 heads the work ends 3 threads into a fourth block), and the same with
a hub source of 1 000 more; a source with one out-edge (alpha is exactly 1), sources without out-edges, a source whose
logits are all negative, logits of exactly 0, slope 0 (-0.0 enters the maximum), logits beyond +-60 in one group.

Packed versus unpacked: every packed shape is also run with GIGL_HGT_NO_PACK=1 in ONE fresh child process (the switch is
read once per process); the two outputs must be torch.equal, and each meets the float64 reference on its own.

Tolerances: forward rtol = atol = 1e-5; gradients rtol = 1e-4, atol = 1e-4 * max|want| per tensor (the project's own), or
4 x the maximum error of the SAME formula evaluated in float32 on the CPU where that is larger.  Exact: sentinels past
n_dst, empty rows (0), the gradient rows of the sources nobody reads, dq and dalpha of the rows whose dout is zero, dalpha
past the live rows, buffers after a refused call.  Every case prints `label tensor: err=<kernel> fp32=<float32 reference>`.

Measured on an MI355X (maximum |kernel - float64| next to the float32 reference's own error; worst case of the class):

    kernels, cases                          tensor        kernel    float32 reference
    HGT forward, packed 8 / 16 / 32         out           8.6e-07   1.0e-06
    HGT forward, wave per row <1|2|4>       out           1.0e-06   8.5e-07
    HGT forward, GIGL_HGT_NO_PACK child     out           8.6e-07   1.0e-06   (torch.equal to the packed output)
    HGT forward + GELU, packed              out           4.3e-07   7.2e-07
    HGT forward + GELU, wave per row        out           7.1e-07   1.0e-06
    HGT backward <1|2|4>                    dq            2.0e-06   1.5e-06
                                            dk / dv       1.3e-06   1.7e-06
                                            dp_rel        4.0e-05   2.0e-05   (max|dp_rel| 0.3 .. 49 over the cases)
    HGT, logits beyond +-50                 out           5.3e-06   1.5e-05
                                            dq            5.8e-06   7.4e-06
                                            dk / dv       1.8e-04   9.2e-05   (max|dk| ~ 80)
                                            dp_rel        1.5e-03   3.2e-04   (max|dp_rel| ~ 200 .. 330)
    weighted aggregate <1|2|4>              out           3.4e-05   3.4e-05   (max|out| ~ 75: alpha is not normalised)
                                            dalpha        5.0e-06   6.5e-06
                                            dv            1.7e-06   2.3e-06
    SimpleHGN alpha                         alpha         7.3e-08   8.8e-08
    SimpleHGN alpha, slope 0                alpha         8.2e-08   8.2e-08
    SimpleHGN alpha, logits beyond +-60     alpha         1.5e-07   1.5e-07

Defect found by this file: the packed kernel did NOT give the wave-per-row kernel's bits (8x4: 35 of 4064 elements
differed in the last place).  Contraction was left to the compiler, which fused acc * r + w * v in three of the packed
kernel's four unrolled edges and not in the fourth; hgt_dot / hgt_fold in hetero.hip now pin the operations for both.
"""
import os
import subprocess
import sys

import pytest
import torch

import attn_cases as ac
from attn_cases import check, f32, i32
from oracle import gnn_ref

gpu = pytest.mark.gpu
N = ac.N_LIVE
GELU_SHAPES = [(8, 4), (4, 16), (2, 64), (1, 4), (5, 32), (3, 128), (6, 128), (16, 64)]


def _id(s):
    return "%dx%d" % s if isinstance(s, tuple) and len(s) == 2 else str(s)


def _label(kind, heads, dim):
    return f"{kind} {heads}x{dim} {ac.hgt_forward_path(heads, dim)} passes={ac.hgt_passes(heads, dim)} " \
           f"lph={ac.lanes_per_head(dim)}"


@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def check_rows_forward(label, got, want, e32, gr):
    check(label, "out", got[:N], want, e32)
    assert bool((got[N:] == ac.SENTINEL).all()), f"{label}: rows past n_dst were written"
    assert not bool(got[:N][gr.m[:N] == 0].any()), f"{label}: an empty row is not exactly 0"


# ---- 1. HGT forward --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rel", ac.RELS)
@pytest.mark.parametrize("shape", ac.HGT_SHAPES, ids=_id)
def test_hgt_forward(eng, shape, rel):
    t, gr, want, e32 = ac.hgt_case(*shape, rel)
    label = _label("hgt", *shape) + f" {rel}"
    check_rows_forward(label, ac.run_hgt(eng, t, gr, rel, False), want["out"], e32["out"], gr)


@gpu
@pytest.mark.parametrize("shape", GELU_SHAPES, ids=_id)
def test_hgt_forward_gelu_epilogue(eng, shape):
    t, gr, want, e32 = ac.hgt_case(*shape, "typed", True)
    check_rows_forward(_label("hgt+gelu", *shape), ac.run_hgt(eng, t, gr, "typed", True), want["out"], e32["out"], gr)


@gpu
@pytest.mark.parametrize("shape", ac.HGT_LARGE, ids=_id)
def test_hgt_large_logits(eng, shape):
    """q times 30: the online softmax rescales across logits beyond +-50, forward and backward"""
    t, gr, want, e32 = ac.hgt_case(*shape, "typed", False, 30)
    label = _label("hgt x30", *shape)
    check_rows_forward(label, ac.run_hgt(eng, t, gr, "typed", False), want["out"], e32["out"], gr)
    check_hgt_backward(label, run_hgt_backward(eng, t, gr, "typed", want), t, gr, want, e32)


@gpu
def test_hgt_packed_equals_unpacked(eng, tmp_path):
    """the source states that the packed kernel gives the wave-per-row kernel's bits: GIGL_HGT_NO_PACK=1 in one child"""
    gr = ac.rows_graph()
    shapes = [(s, gelu) for g in (8, 16, 32) for s in ac.HGT_PACKED[g] for gelu in (False, True)]
    cases = []
    for (heads, dim), gelu in shapes:
        assert ac.hgt_forward_path(heads, dim)[0] == "packed" and ac.hgt_forward_path(heads, dim, True) == ("unpacked", 1)
        t = ac.hgt_inputs(heads, dim)
        cases.append(dict(heads=heads, dim=dim, gelu=gelu, q=t.q, k=t.k, v=t.v, rowptr=gr.rp.to(torch.int32),
                          col=gr.col.to(torch.int32), etype=t.etype.to(torch.int32), p_rel=t.p_rel, n_dst=N,
                          shape=(ac.N_ROWS, heads * dim)))
    torch.save(cases, tmp_path / "in.pt")
    env = dict(os.environ, GIGL_HGT_NO_PACK="1")
    child = subprocess.run([sys.executable, os.path.abspath(ac.__file__), "hgt", str(tmp_path / "in.pt"),
                            str(tmp_path / "out.pt")], env=env, capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    unpacked = torch.load(tmp_path / "out.pt")
    for ((heads, dim), gelu), other in zip(shapes, unpacked):
        t, gr, want, e32 = ac.hgt_case(heads, dim, "typed", gelu)
        label = _label("hgt", heads, dim) + f" gelu={gelu}"
        mine = ac.run_hgt(eng, t, gr, "typed", gelu)
        check_rows_forward(label + " packed", mine, want["out"], e32["out"], gr)
        check_rows_forward(label + " GIGL_HGT_NO_PACK", other, want["out"], e32["out"], gr)
        assert torch.equal(mine, other), f"{label}: packed and unpacked differ in {int((mine != other).sum())} elements"


# ---- 2. HGT backward -------------------------------------------------------------------------------------------------
def run_hgt_backward(eng, t, gr, rel, want):
    etype, p_rel = ac.hgt_rel(t, rel)
    dout = t.dout.clone()
    dout[N:] = ac.NAN
    return eng.hgt_aggregate_backward(f32(t.q), f32(t.k), f32(t.v), t.heads, t.dim, i32(gr.rp), i32(gr.col), i32(etype),
                                      f32(p_rel), N, ac.padded(want["out"], ac.N_ROWS), f32(dout))


def check_unread_sources(label, name, x, gr):
    read = torch.zeros(x.shape[0], dtype=torch.bool)
    read[gr.raw_src] = True
    assert not bool(read[ac.N_READ:].any()) and not bool(x[~read].any()), f"{label} {name}: a source nobody reads has a gradient"


def check_hgt_backward(label, got, t, gr, want, e32):
    dq, dk, dv, dp = (None if x is None else x.cpu() for x in got)
    for name, x in (("dq", dq), ("dk", dk), ("dv", dv)):
        check(label, name, x, want[name], e32[name], grad=True)
    assert not bool(dq[N:].any()) and not bool(dq[:N][t.zero_rows].any()), f"{label}: dq of a row without dout"
    check_unread_sources(label, "dk", dk, gr)
    check_unread_sources(label, "dv", dv, gr)
    assert (dp is None) == ("dp_rel" not in want)
    if dp is not None:
        check(label, "dp_rel", dp, want["dp_rel"], e32["dp_rel"], grad=True)


@gpu
@pytest.mark.parametrize("rel", ac.RELS)
@pytest.mark.parametrize("shape", ac.WIDE_SHAPES, ids=_id)
def test_hgt_backward(eng, shape, rel):
    t, gr, want, e32 = ac.hgt_case(*shape, rel)
    label = _label("hgt bwd", *shape) + f" {rel}"
    check_hgt_backward(label, run_hgt_backward(eng, t, gr, rel, want), t, gr, want, e32)


# ---- 3. the weighted aggregate ---------------------------------------------------------------------------------------
def _alpha_dev(t, gr):
    return ac.nan_where(t.alpha, ~gr.used)


@gpu
@pytest.mark.parametrize("shape", ac.WIDE_SHAPES, ids=_id)
def test_weighted_aggregate(eng, shape):
    heads, dim = shape
    t, gr, want, e32 = ac.weighted_case(heads, dim)
    label = _label("weighted", heads, dim)
    out = ac.full(ac.N_ROWS, heads * dim)
    eng.weighted_aggregate(_alpha_dev(t, gr), f32(t.v), heads, dim, i32(gr.rp), i32(gr.col), N, out)
    check_rows_forward(label, out.cpu(), want["out"], e32["out"], gr)
    dout = t.dout.clone()
    dout[N:] = ac.NAN
    dalpha, dv = (x.cpu() for x in eng.weighted_aggregate_backward(_alpha_dev(t, gr), f32(t.v), heads, dim, i32(gr.rp),
                                                                   i32(gr.col), N, f32(dout)))
    check(label, "dalpha", dalpha, want["dalpha"], e32["dalpha"], grad=True)
    check(label, "dv", dv, want["dv"], e32["dv"], grad=True)
    assert not bool(dalpha[~gr.used].any()), f"{label}: dalpha past the live rows"
    assert not bool(dalpha[gr.raw[t.zero_rows[gr.raw_dst]]].any()), f"{label}: dalpha of a row whose dout is zero"
    check_unread_sources(label, "dv", dv, gr)


# ---- 4. SimpleHGN alpha ----------------------------------------------------------------------------------------------
def _shgn_id(case):
    heads, kind, ef, slope, scale = case
    return f"{heads}-{kind}" + ("-hef" if ef else "") + ("-slope0" if slope == 0 else "") + (f"-x{scale}" if scale > 1 else "")


@gpu
@pytest.mark.parametrize("case", ac.SHGN_CASES, ids=_shgn_id)
def test_simplehgn_alpha(eng, case):
    heads, kind, ef, slope, scale = case
    t, gr, want, e32 = ac.shgn_case(*case)
    got = eng.simplehgn_alpha(f32(t.hl), f32(t.hr), f32(t.het), f32(t.hef), i32(gr.src), i32(gr.dst), i32(gr.etype), gr.n,
                              heads, slope).cpu()
    check(f"shgn {_shgn_id(case)} edges*heads={gr.src.numel() * heads}", "alpha", got, want["alpha"], e32["alpha"])
    assert bool((got[gr.src == ac.SHGN_LONE] == 1.0).all()), "the alpha of a source's only out-edge is 1"
    sums = torch.zeros(gr.n, heads, dtype=torch.float64).index_add_(0, gr.src, got.double())
    has = torch.zeros(gr.n, dtype=torch.bool)
    has[gr.src] = True
    assert float((sums[has] - 1).abs().max()) <= 1e-5 and not bool(has[ac.SHGN_FIRST_SINK:].any())


# ---- 5. refused shapes -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", ac.REFUSED, ids=_id)
def test_refused_shapes_write_nothing(eng, shape):
    from gigl_amd._lib import GiglError
    heads, dim = shape
    assert not ac.hgt_supported(heads, dim)
    gr = ac.rows_graph()
    hd, ce = heads * dim, gr.col.numel()
    g = torch.Generator().manual_seed(hd)
    q, k, v, dout = (f32(ac.free(g, ac.N_ROWS, hd)) for _ in range(4))
    alpha = f32(ac.free(g, ce, heads))
    rp, col, et, p_rel = i32(gr.rp), i32(gr.col), i32(torch.zeros(ce)), f32(torch.ones(ac.N_ETYPES, heads))
    out = ac.full(ac.N_ROWS, hd)
    calls = [lambda: eng.hgt_aggregate(q, k, v, heads, dim, rp, col, et, p_rel, N, out),
             lambda: eng.hgt_aggregate(q, k, v, heads, dim, rp, col, et, p_rel, N, out, gelu=True),
             lambda: eng.weighted_aggregate(alpha, v, heads, dim, rp, col, N, out),
             lambda: eng.hgt_aggregate_backward(q, k, v, heads, dim, rp, col, et, p_rel, N, q, dout),
             lambda: eng.weighted_aggregate_backward(alpha, v, heads, dim, rp, col, N, dout)]
    for call in calls:
        with pytest.raises(GiglError) as info:
            call()
        assert info.value.code == ac.E_UNSUPPORTED
    s = [ac.full(ac.N_ROWS, hd) for _ in range(4)] + [ac.full(ac.N_ETYPES, heads), ac.full(ce, heads)]
    rcs = [ac.raw_call(eng, "gigl_hgt_aggregate_backward", q, k, v, heads, dim, rp, col, et, p_rel, N, q, dout, s[0], s[1],
                       s[2], s[4]),
           ac.raw_call(eng, "gigl_weighted_aggregate_backward", alpha, v, heads, dim, rp, col, N, dout, s[5], s[3])]
    assert rcs == [ac.E_UNSUPPORTED] * 2
    assert all(bool((x == ac.SENTINEL).all()) for x in s + [out]), "a refused call wrote its outputs"


# ---- CPU: the formulas against oracle/gnn_ref.py, the graph, the inputs' conditions, the coverage, the bounds --------
def _pin_hgt(heads, dim):
    t, gr = ac.hgt_inputs(heads, dim), ac.rows_graph()
    f, n_s, dd = heads * dim, ac.N_NODES, torch.float64
    k0, v0, q0 = torch.nan_to_num(t.k), torch.nan_to_num(t.v), t.q[:N]
    xs = torch.cat([k0, torch.zeros(n_s, f, dtype=dd), v0], 1).requires_grad_(True)
    xd = torch.cat([torch.zeros(N, f, dtype=dd), q0, torch.zeros(N, f, dtype=dd)], 1).requires_grad_(True)
    ets = [("s", "r%d" % i, "d") for i in range(ac.N_ETYPES)]
    lin3, lin1 = (torch.eye(3 * f, dtype=dd), torch.zeros(3 * f, dtype=dd)), (torch.eye(f, dtype=dd), torch.zeros(f, dtype=dd))
    rel = torch.eye(dim, dtype=dd).repeat(heads * ac.N_ETYPES, 1, 1)
    p = {"kqv": {"s": lin3, "d": lin3}, "out": {"s": lin1, "d": lin1}, "k_rel": rel, "v_rel": rel, "edge_types": ets,
         "p_rel": {et: t.p_rel[i] for i, et in enumerate(ets)}, "skip": {}}
    ty = t.etype[gr.raw]
    eid = {et: torch.stack([gr.raw_src[ty == i], gr.raw_dst[ty == i]]) for i, et in enumerate(ets)}
    conv = gnn_ref.hgt_conv({"s": xs, "d": xd}, eid, p, heads)["d"]
    w = ac.free(torch.Generator().manual_seed(1), N, f)
    gs, gd = torch.autograd.grad((conv * w).sum(), [xs, xd])
    q, k, v = (x.clone().requires_grad_(True) for x in (torch.nan_to_num(t.q), k0, v0))
    out = ac.hgt_ref(gr, heads, dim, q, k, v, t.etype, t.p_rel, gelu=True)
    dq, dk, dv = torch.autograd.grad((out * w).sum(), [q, k, v])
    assert ac.err(out, conv) <= 1e-12, (heads, dim)
    assert ac.err(dq[:N], gd[:, f:2 * f]) <= 1e-12 and ac.err(dk, gs[:, :f]) <= 1e-12 and ac.err(dv, gs[:, 2 * f:]) <= 1e-12


def _pin_shgn(heads, kind, ef):
    t, gr = ac.shgn_inputs(heads, kind, ef, 1), ac.shgn_graph(kind)
    n, dd = gr.n, torch.float64
    sel = lambda a, b: torch.tensor([a, b], dtype=dd).expand(1, heads, 2)
    p = {"W_nfeat": torch.eye(2 * heads, dtype=dd), "a_l": sel(1, 0), "a_r": sel(0, 1),
         "a_etype": torch.ones(1, heads, 1, dtype=dd), "edge_type_emb": torch.ones(ac.N_ETYPES, 1, dtype=dd),
         "W_etype": (t.het.view(ac.N_ETYPES, 1, heads), torch.zeros(ac.N_ETYPES, heads, dtype=dd)), "residual": None}
    if ef:
        p["W_efeat"] = torch.zeros(heads, heads * heads, dtype=dd)
        p["W_efeat"][torch.arange(heads), torch.arange(heads) * heads] = 1.0
        p["a_efeat"] = torch.ones(1, heads, heads, dtype=dd)
    nf = torch.stack([t.hl[:n], t.hr[:n]], -1).reshape(n, 2 * heads)
    x1, x2 = nf.clone().requires_grad_(True), nf.clone().requires_grad_(True)
    conv = gnn_ref.simplehgn_conv(torch.stack([gr.src, gr.dst]), x1, gr.etype, p, heads, 2, ac.SLOPE, t.hef)
    emb = x2.view(n, heads, 2)
    a = ac.shgn_ref(gr, emb[..., 0], emb[..., 1], t.het, t.hef, ac.SLOPE)
    mine = torch.zeros(n, heads, 2, dtype=dd).index_add(0, gr.dst, emb[gr.src] * a[:, :, None]).reshape(n, 2 * heads)
    w = ac.free(torch.Generator().manual_seed(2), n, 2 * heads)
    assert ac.err(mine, conv) <= 1e-12, (heads, kind, ef)
    assert ac.err(torch.autograd.grad((mine * w).sum(), x2)[0], torch.autograd.grad((conv * w).sum(), x1)[0]) <= 1e-12


def test_references_inputs_and_coverage():
    rows, where = ac.base_rows()
    gr = ac.rows_graph()
    # the graph delivers what the cases rely on
    assert ac.N_ROWS % 8 == 3 and 125 <= ac.N_ROWS <= 135 and (N % 8, N % 4, N % 2) == (7, 3, 1) and N < ac.N_ROWS
    assert [int(gr.m[where["deg%d" % d]]) for d in ac.DEGREES] == ac.DEGREES and int(gr.m[where["hub"]]) == ac.HUB
    assert {where["deg0"], where["deg1"], where["hub"]} == {0, 2, 3}  # one wave of the packed kernel at G = 8
    assert all(i % 3 != 1 and i < N for i in where.values()) and len(set(where.values())) == len(where)
    assert rows[where["self_only"]].tolist() == [where["self_only"]]
    assert int((rows[where["self_twice"]] == where["self_twice"]).sum()) == 2 and rows[where["self_twice"]].numel() == 6
    dup = rows[where["dup"]]
    assert dup.numel() - dup.unique().numel() == 1 and where["dup"] not in dup.tolist()
    assert int(gr.col.max()) < ac.N_READ < ac.NAN_NODE == ac.N_NODES - 1 and int((gr.m[:N] == 0).sum()) >= 2
    assert bool((gr.rp[1:] == gr.rowend).all()) and gr.raw.numel() == int(gr.m[:N].sum())

    # the formulas against gnn_ref (float64): outputs and input gradients
    for heads, dim in ((2, 4), (3, 8), (1, 16)):
        _pin_hgt(heads, dim)
    for heads, kind, ef in ((1, "small", False), (3, "small", True), (2, "hub", True)):
        _pin_shgn(heads, kind, ef)
    # the weighted aggregate is the HGT reduce with the softmax's alpha handed in
    t = ac.hgt_inputs(3, 8)
    z = ac.hgt_logits(t, gr)
    a = torch.zeros(gr.col.numel(), 3, dtype=torch.float64)
    a[gr.raw] = ac.seg_softmax(z, gr.raw_dst, N, 0.0)
    k0, v0 = torch.nan_to_num(t.k), torch.nan_to_num(t.v)
    assert ac.err(ac.weighted_ref(gr, 3, 8, a, v0), ac.hgt_ref(gr, 3, 8, t.q, k0, v0, t.etype, t.p_rel)) <= 1e-12

    # the inputs' conditions
    for shape in ac.HGT_LARGE:
        t = ac.hgt_inputs(*shape, 30)
        z = ac.hgt_logits(t, gr)[gr.raw_dst == where["hub"]]
        assert float(z.max()) >= 50 and float(z.min()) <= -50, (shape, float(z.max()), float(z.min()))
    t = ac.hgt_inputs(2, 16)
    assert int(t.zero_rows.sum()) >= 15 and not bool(t.dout[:N][t.zero_rows].any())
    assert set(t.etype.tolist()) == {0, 1, 2} and bool((t.p_rel < 0).any()) and bool((t.p_rel > 0).any())
    seen = set()
    for case in ac.SHGN_CASES:
        heads, kind, ef, slope, scale = case
        t, sg = ac.shgn_inputs(heads, kind, ef, scale), ac.shgn_graph(kind)
        pre = ac.shgn_pre(t, sg)
        assert torch.equal((t.hl.float()[sg.src] + t.hr.float()[sg.dst] + t.het.float()[sg.etype] +
                            (t.hef.float() if ef else 0)).double(), pre), case  # exact in fp32
        assert int((sg.src == ac.SHGN_LONE).sum()) == 1 and int((sg.src == ac.SHGN_NEG).sum()) == 12
        assert float(pre[sg.src == ac.SHGN_NEG].max()) < 0 and int(sg.src.max()) < ac.SHGN_FIRST_SINK
        mixed = [s for s in range(2, ac.SHGN_FIRST_SINK) if float(pre[sg.src == s].max()) > 0 > float(pre[sg.src == s].min())]
        assert len(mixed) >= 10 and (scale > 1 or bool((pre == 0).any())), case
        assert (kind == "hub") == (int((sg.src == ac.SHGN_HUB).sum()) > 1000)
        if scale > 1:
            act = torch.nn.functional.leaky_relu(pre, slope)
            spread = max(float(act[sg.src == s].max() - act[sg.src == s].min()) for s in mixed)
            assert float(act.max()) >= 60 and float(act.min()) <= -60 and spread >= 120, case
        if slope == 0:  # x * 0 of a negative x is -0.0: the whole group of SHGN_NEG, and members of mixed groups
            assert bool((pre < 0).any())
        seen.add((heads, ef))
        if kind == "small":
            assert sg.src.numel() == 257
    assert {h for h, _ in seen} == {1, 2, 3, 8} and {e for _, e in seen} == {False, True}
    assert 257 * 3 % 256 == 3 and {c[3] for c in ac.SHGN_CASES} == {ac.SLOPE, 0.0} and {c[4] for c in ac.SHGN_CASES} == {1, 512}

    # coverage, from the case lists and the restated dispatch
    assert all(ac.hgt_supported(*s) for s in ac.HGT_SHAPES + ac.WIDE_SHAPES + ac.HGT_LARGE + GELU_SHAPES)
    for g in (8, 16, 32):
        assert all(ac.hgt_forward_path(*s) == ("packed", g) for s in ac.HGT_PACKED[g]) and len(ac.HGT_PACKED[g]) >= 2
    for p in (1, 2, 3, 4):
        assert all(ac.hgt_forward_path(*s) == ("unpacked", ac.instantiation(p)) and ac.hgt_passes(*s) == p
                   for s in ac.HGT_UNPACKED[p])
    assert ac.instantiation(3) == 4 and ac.hgt_forward_path(3, 256) == ("unpacked", 4) and ac.hgt_passes(6, 128) == 3
    assert ac.hgt_forward_path(1, 128) == ("unpacked", 1)  # 32 lanes of one head: dim / 4 > 16 keeps it off the packed kernel
    paths = {ac.hgt_forward_path(*s) for s in ac.HGT_SHAPES}
    assert paths == {("packed", 8), ("packed", 16), ("packed", 32), ("unpacked", 1), ("unpacked", 2), ("unpacked", 4)}
    assert {ac.hgt_forward_path(*s) for s in GELU_SHAPES} == paths
    assert {ac.lanes_per_head(d) for _, d in ac.HGT_SHAPES} == {1, 2, 4, 8, 16, 32, 64}
    assert {ac.lanes_per_head(d) for s in ac.HGT_PACKED.values() for _, d in s} == {1, 2, 4, 8, 16}
    for shapes in (ac.HGT_SHAPES, ac.WIDE_SHAPES):
        assert {ac.hgt_passes(*s) for s in shapes} == {1, 2, 3, 4}
        assert {ac.instantiation(ac.hgt_passes(*s)) for s in shapes} == {1, 2, 4}
        assert {ac.lanes_per_head(d) for _, d in shapes} == {1, 2, 4, 8, 16, 32, 64}
        # a partial last pass under every lanes-per-head branch that can have one, the v_readlane one included
        assert {ac.lanes_per_head(s[1]) for s in shapes if ac.hgt_partial(*s)} >= {1, 2, 4, 8, 16, 32}
        assert any(ac.hgt_partial(*s) and ac.hgt_passes(*s) == 2 for s in shapes)
    assert ac.hgt_partial(3, 128) and ac.hgt_passes(3, 128) == 2 and ac.lanes_per_head(128) == 32
    assert {ac.hgt_forward_path(*s)[0] for s in ac.HGT_LARGE} == {"packed", "unpacked"}
    assert all(not ac.hgt_supported(*s) for s in ac.REFUSED) and [h * d for h, d in ac.REFUSED][3] == 1028
    assert [d for _, d in ac.REFUSED[:3]] == [5, 12, 512]

    # the bounds can fail: a deliberately wrong float64 variant against the right one, through the tests' own bound
    def caught(shape, wrong, **kw):
        t, gr, want, e32 = ac.hgt_case(*shape, "typed")
        bad = ac.hgt_ref(gr, *shape, t.q, torch.nan_to_num(t.k), torch.nan_to_num(t.v), t.etype, t.p_rel, wrong=wrong)
        assert ac.beyond(want["out"], want["out"], e32["out"], False) == 0
        return ac.beyond(bad, want["out"], e32["out"], False) > 0
    assert caught((4, 16), "no_p_rel") and caught((3, 128), "no_p_rel")
    assert caught((4, 16), "no_scale") and caught((1, 4), "no_scale")
    assert ac.lanes_per_head(128) == 32 and caught((6, 128), "head_pair")  # a head sum that crosses heads at 32 lanes
    assert caught((2, 256), "second_pass") and caught((3, 128), "second_pass")
    for case in ((3, "small", True, ac.SLOPE, 1), (2, "hub", False, ac.SLOPE, 1)):
        t, sg, want, e32 = ac.shgn_case(*case)
        bad = ac.shgn_ref(sg, t.hl, t.hr, t.het, t.hef, ac.SLOPE, wrong="by_dst")
        assert ac.beyond(bad, want["alpha"], e32["alpha"], False) > 0
