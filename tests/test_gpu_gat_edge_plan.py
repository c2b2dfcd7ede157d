"""The one-call plan with edge features (gigl_gat_plan_set_edge_features): GATConv(edge_dim) and EdgeAttrGATConv layers
over the resident edge table read in place — plan rows == the staged forward over the staged sample / union == the fp32
restatement in oracle/gnn_ref.py chained over the oracle's union (1e-5, the bar of test_gpu_attn / test_gpu_edge_features),
exact work counts, hipGraph replay, weight updates, and the GRAPH / LAYERS parts."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from helpers import rmat_edges
from oracle import gnn_ref

pytestmark = pytest.mark.gpu
B = 96


def _graph():
    s, d = rmat_edges(11, 30000, seed=5)
    n = 1 << 11
    s = np.concatenate([s, np.arange(0, 100, dtype=np.uint32)])  # some self loops
    d = np.concatenate([d, np.arange(0, 100, dtype=np.uint32)])
    rowptr, col = oracle.build_csc(n, s, d, is_directed=True)
    return n, rowptr, col


def _engine(n, rowptr, col, d, dtype, de):
    from gigl_amd.engine import HipEngine
    x = (np.random.default_rng(d).standard_normal((n, d)) / 4).astype(dtype)
    efeat = (np.random.default_rng(1).standard_normal((len(col), de)) / 2).astype(np.float32)  # row p = edge at col[p]
    eng = HipEngine(0)
    eng.load_csc(rowptr, col)
    eng.load_features(torch.from_numpy(x) if dtype == np.float16 else x)
    dst_of = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rowptr))
    perm = np.random.default_rng(2).permutation(len(col))  # shuffled COO order: the engine restores `col` order
    eng.load_edge_features(col[perm], dst_of[perm], efeat[perm], is_directed=True)
    return eng, x, efeat


def _roots(n, groups):
    roots = np.random.default_rng(3).integers(0, n, size=B * groups).astype(np.uint32)
    roots[5] = roots[6]  # a duplicated root inside a batch
    roots[:5] = np.arange(5)  # nodes with a self loop in the graph
    return roots


def _model(eng, d, hid, out, L, heads, de, conv, share, seed):
    from gigl_amd.models_attn import GAT
    torch.manual_seed(seed)
    model = GAT(d, hid, out, num_layers=L, heads=heads, edge_dim=de, conv=conv,
                share_edge_att_message_weight=share).to(eng.device)
    with torch.no_grad():
        for c in model.conv_layers:
            c.bias.normal_(0, 0.1)
    return model


def _csc_positions(rowptr, col, src, dst):
    out = np.full(len(src), -1, dtype=np.int64)
    for i, (s, d) in enumerate(zip(src, dst)):
        row = col[rowptr[d]:rowptr[d + 1]]
        k = np.searchsorted(row, s)
        if k < len(row) and row[k] == s:
            out[i] = rowptr[d] + k
    return out


def _oracle_rows(model, conv, share, heads, rowptr, col, x, efeat, part, fan):
    """gnn_ref.gat_conv chained over the oracle's union of `part`, rows of the roots; also: the union's self edges"""
    L = len(fan)
    nbr_o, _ = oracle.sample_khop(rowptr, col, part, fan, canonical=True)
    o = oracle.union_build(part, fan, nbr_o)
    ei = gnn_ref.union_edge_index(o["rowptr"], o["col"])
    nodes = np.asarray(o["nodes"])
    pos = _csc_positions(rowptr, col, nodes[ei[0].numpy()], nodes[ei[1].numpy()])
    assert (pos >= 0).all()
    ea = torch.from_numpy(efeat[pos])
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    h = torch.from_numpy(x[nodes].astype(np.float32))
    for l in range(L):
        p = f"conv_layers.{l}."
        w_msg = None
        if conv == "edge_attr_gat":
            w_msg = sd[p + "lin_edge.weight"] if share else sd[p + "lin_edge_message.weight"]
        h = gnn_ref.gat_conv(h, ei, sd[p + "lin.weight"], sd[p + "att_src"], sd[p + "att_dst"], sd[p + "bias"],
                             heads if l < L - 1 else 1, edge_attr=ea, w_edge=sd[p + "lin_edge.weight"],
                             att_edge=sd[p + "att_edge"], w_edge_msg=w_msg)
        if l < L - 1:
            h = torch.relu(h)
    return h[o["root_local"]].numpy(), int((ei[0] == ei[1]).sum())


def _staged_rows(eng, model, part, fan):
    from gigl_amd.models import HipBatch
    tree = eng.sample_khop(part, fan)
    u = eng.union_build(tree)
    return model(HipBatch(eng, tree, u))[u.root_local[:B].long()].cpu().numpy(), tree, u


def _no_overflow(eng, plan):
    acc = torch.zeros(1, dtype=torch.int32, device=eng.device)
    plan.overflow_add(acc)
    return int(acc.item()) == 0


@pytest.mark.parametrize("conv,share,heads,d,dtype,hid,out,de,fan,groups", [
    ("edge_attr_gat", True, 2, 768, np.float16, 128, 24, 16, [9, 6], 1),
    ("gat", True, 4, 320, np.float32, 32, 24, 6, [7, 5], 3),
    ("edge_attr_gat", False, 1, 260, np.float32, 16, 24, 3, [4, 3, 2], 1),
    ("edge_attr_gat", False, 4, 320, np.float32, 64, 32, 64, [6, 4], 3),
    ("gat", True, 2, 768, np.float16, 128, 24, 3, [6, 4], 1),
    ("edge_attr_gat", True, 1, 260, np.float32, 16, 20, 6, [7, 5], 1),
    ("gat", True, 1, 320, np.float32, 16, 24, 64, [9, 6], 1),
    ("edge_attr_gat", False, 2, 768, np.float16, 128, 32, 6, [4, 3, 2], 3)])
def test_edge_plan_matches_the_staged_forward_and_the_oracle(conv, share, heads, d, dtype, hid, out, de, fan, groups):
    """GAT(edge_dim).make_plan rows == forward(HipBatch) over the staged sample / union == gnn_ref.gat_conv over the
    oracle's union, per group of roots; the plan's exact work counts == the staged counts; no call overflowed"""
    from gigl_amd._lib import GIGL_META_LEVEL0, STATS_AGGREGATED, STATS_LEN, STATS_SAMPLED
    n, rowptr, col = _graph()
    eng, x, efeat = _engine(n, rowptr, col, d, dtype, de)
    try:
        L = len(fan)
        model = _model(eng, d, hid, out, L, heads, de, conv, share, seed=d + de)
        roots = _roots(n, groups)
        plan = model.make_plan(eng, B, fan, groups=groups)
        r_dev = torch.from_numpy(roots.view(np.int32)).to(eng.device)
        got = plan.run(r_dev).cpu().numpy()
        assert _no_overflow(eng, plan)  # (a comparison that only saw NaN rows would show nothing)
        assert np.isfinite(got).all()
        acc = torch.zeros(STATS_LEN, dtype=torch.int64, device=eng.device)
        plan.stats(r_dev, acc)
        sampled = aggregated = 0
        for gi in range(groups):
            part = roots[gi * B:(gi + 1) * B]
            want, tree, u = _staged_rows(eng, model, part, fan)
            ref, self_edges = _oracle_rows(model, conv, share, heads, rowptr, col, x, efeat, part, fan)
            assert self_edges >= 1  # the self-loop removal / mean-fill path is exercised
            err_s, err_o = np.abs(got[gi * B:(gi + 1) * B] - want).max(), np.abs(got[gi * B:(gi + 1) * B] - ref).max()
            print(f"group {gi}: max |plan - staged| = {err_s:.3e}, max |plan - oracle| = {err_o:.3e}, "
                  f"self edges {self_edges}")
            np.testing.assert_allclose(got[gi * B:(gi + 1) * B], want, rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(got[gi * B:(gi + 1) * B], ref, rtol=1e-5, atol=1e-5)
            sampled += int(sum(int(c.sum()) for c in tree.cnt))
            rowlen = (u.rowend - u.rowptr).cpu().numpy().astype(np.int64)
            meta = u.meta.cpu().numpy()
            aggregated += int(sum(rowlen[: meta[GIGL_META_LEVEL0 + (L - 1 - l)]].sum() for l in range(L)))
        a = acc.cpu().numpy()
        assert a[STATS_SAMPLED] == sampled and a[STATS_AGGREGATED] == aggregated
    finally:
        eng.close()


@pytest.mark.parametrize("conv,share,heads,d,dtype,hid,de,fan,groups", [
    ("edge_attr_gat", False, 2, 768, np.float16, 128, 16, [9, 6], 1),
    ("gat", True, 4, 320, np.float32, 32, 6, [4, 3, 2], 3)])
def test_edge_plan_replays_and_follows_the_weights(conv, share, heads, d, dtype, hid, de, fan, groups):
    """eager run == captured run == replay, bit for bit (the same kernels in the same order); after att_edge / lin_edge /
    lin_edge_message change in place and set_weights(*plan_params()), the replayed rows follow the staged forward again"""
    n, rowptr, col = _graph()
    eng, x, efeat = _engine(n, rowptr, col, d, dtype, de)
    try:
        model = _model(eng, d, hid, 24, len(fan), heads, de, conv, share, seed=11)
        roots = _roots(n, groups)
        plan = model.make_plan(eng, B, fan, groups=groups)
        r_dev = torch.from_numpy(roots.view(np.int32)).to(eng.device)
        got = plan.run(r_dev).cpu().numpy()
        assert _no_overflow(eng, plan)
        st = torch.cuda.Stream(device=eng.device)  # (the legacy default stream cannot be captured)
        torch.cuda.synchronize()
        eng.bind_stream(st)
        torch.cuda.set_stream(st)
        try:
            plan.use_graph(True)
            again = plan.run(r_dev).cpu().numpy()   # captures
            replay = plan.run(r_dev).cpu().numpy()  # replays
            np.testing.assert_array_equal(again, got)
            np.testing.assert_array_equal(replay, got)
            with torch.no_grad():
                for c in model.conv_layers:
                    c.att_edge.mul_(-1.5)
                    c.lin_edge.weight.add_(0.25)
                    if getattr(c, "lin_edge_message", None) is not None:
                        c.lin_edge_message.weight.mul_(2.0)
            plan.set_weights(*model.plan_params())
            changed = plan.run(r_dev).cpu().numpy()   # captures again: the graphs were dropped
            changed2 = plan.run(r_dev).cpu().numpy()  # replays
            np.testing.assert_array_equal(changed, changed2)
            assert np.abs(changed - got).max() > 1e-4
        finally:
            torch.cuda.synchronize()
            torch.cuda.set_stream(torch.cuda.default_stream(eng.device))
            eng.bind_stream(None)
        for gi in range(groups):
            want, _, _ = _staged_rows(eng, model, roots[gi * B:(gi + 1) * B], fan)
            np.testing.assert_allclose(changed[gi * B:(gi + 1) * B], want, rtol=1e-5, atol=1e-5)
    finally:
        eng.close()


def test_edge_plan_in_two_parts_equals_the_one_call():
    """GIGL_PLAN_PART_GRAPH (sample + union + the edge ids) then GIGL_PLAN_PART_LAYERS on the plan's stream == run"""
    from gigl_amd import _lib
    n, rowptr, col = _graph()
    eng, x, efeat = _engine(n, rowptr, col, 320, np.float32, 6)
    try:
        fan = [7, 5]
        model = _model(eng, 320, 32, 24, 2, 2, 6, "edge_attr_gat", False, seed=5)
        plan = model.make_plan(eng, B, fan)
        rng = np.random.default_rng(5)
        for _ in range(2):
            roots = torch.from_numpy(rng.integers(0, n, size=B).astype(np.uint32).view(np.int32)).to(eng.device)
            want = plan.run(roots).clone()
            assert _no_overflow(eng, plan) and bool(torch.isfinite(want).all())
            got = torch.full_like(want, float("nan"))
            for part in (1, 2):
                _lib.check(eng._lib.gigl_sage_plan_run_part(plan._plan, C.c_void_p(roots.data_ptr()), 42,
                                                            _lib.MODE_SPARK_HASH, C.c_void_p(got.data_ptr()), part),
                           eng._ctx)
            eng.synchronize()
            assert torch.equal(want, got)
    finally:
        eng.close()


def test_edge_plan_needs_the_edge_table_and_a_built_width():
    """without resident edge features make_plan says so; an edge table wider than the plan is built for is
    GIGL_E_UNSUPPORTED (what ResidentGraph turns into the staged forward)"""
    from gigl_amd._lib import GiglError
    from gigl_amd.engine import HipEngine
    from gigl_amd.models_attn import GAT
    n, rowptr, col = _graph()
    eng = HipEngine(0)
    try:
        eng.load_csc(rowptr, col)
        eng.load_features(np.zeros((n, 64), np.float32))
        model = GAT(64, 8, 8, num_layers=2, heads=2, edge_dim=6).to(eng.device)
        with pytest.raises(RuntimeError, match="edge features"):
            model.make_plan(eng, 16, [3, 2])
        eng._set_edge_table(torch.zeros((len(col), 80), dtype=torch.float32, device=eng.device))
        wide = GAT(64, 8, 8, num_layers=2, heads=2, edge_dim=80).to(eng.device)
        with pytest.raises(GiglError) as e:
            wide.make_plan(eng, 16, [3, 2])
        assert e.value.code == -4
    finally:
        eng.close()
