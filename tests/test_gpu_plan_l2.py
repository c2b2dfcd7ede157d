"""L2-normalised output inside the one-call plans (gigl_sage_plan_set_l2_normalize): GraphSAGE on both output paths (the
fused two-layer projection's gigl_sage_fused_out, and gigl_take_rows) and GAT with and without edge features —
rows == F.normalize of the same plan with the flag off (1e-6) == the normalised fp32 CPU forward (1e-5); a zero row stays
zero and finite."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from helpers import rmat_edges
from oracle import gnn_ref

pytestmark = pytest.mark.gpu
B = 96


@pytest.fixture(scope="module")
def graph():
    s, d = rmat_edges(11, 30000, seed=5)
    n = 1 << 11
    s = np.concatenate([s, np.arange(0, 100, dtype=np.uint32)])
    d = np.concatenate([d, np.arange(0, 100, dtype=np.uint32)])
    rowptr, col = oracle.build_csc(n, s, d, is_directed=True)
    lonely = int(np.flatnonzero(np.diff(rowptr) == 0)[0])  # a node without in-edges
    roots = np.random.default_rng(3).integers(0, n, size=B).astype(np.uint32)
    roots[5] = roots[6]
    roots[:5] = np.arange(5)
    roots[7] = lonely
    return n, rowptr, col, roots, lonely


def _engine(graph, d, de=None):
    from gigl_amd.engine import HipEngine
    n, rowptr, col, roots, lonely = graph
    x = (np.random.default_rng(d).standard_normal((n, d)) / 4).astype(np.float32)
    x[lonely] = 0.0  # zero features, no in-edges, no bias: a zero output row
    eng = HipEngine(0)
    eng.load_csc(rowptr, col)
    eng.load_features(x)
    efeat = None
    if de is not None:
        efeat = (np.random.default_rng(1).standard_normal((len(col), de)) / 2).astype(np.float32)
        dst_of = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rowptr))
        eng.load_edge_features(col, dst_of, efeat, is_directed=True)
    return eng, x, efeat


def _check(eng, graph, on, off, fan, want):
    n, rowptr, col, roots, lonely = graph
    r_dev = torch.from_numpy(roots.view(np.int32)).to(eng.device)
    plan_on, plan_off = on.make_plan(eng, B, fan), off.make_plan(eng, B, fan)
    acc = torch.zeros(1, dtype=torch.int32, device=eng.device)
    got = plan_on.run(r_dev)
    plan_on.overflow_add(acc)
    plain = plan_off.run(r_dev)
    plan_off.overflow_add(acc)
    assert int(acc.item()) == 0
    got, plain = got.cpu(), plain.cpu()
    assert bool(torch.isfinite(got).all())
    np.testing.assert_allclose(got.numpy(), F.normalize(plain, p=2, dim=1).numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got.numpy(), F.normalize(want, p=2, dim=1).numpy(), rtol=1e-5, atol=1e-5)
    norms = got.norm(dim=1)
    assert bool((got[7] == 0).all()) and bool((plain[7] == 0).all())  # the root without in-edges
    keep = torch.ones(B, dtype=torch.bool)
    keep[7] = False
    np.testing.assert_allclose(norms[keep].numpy(), 1.0, rtol=1e-5)
    return plan_on, plan_off


def _oracle_union(graph, fan):
    n, rowptr, col, roots, lonely = graph
    nbr_o, _ = oracle.sample_khop(rowptr, col, roots, fan, canonical=True)
    o = oracle.union_build(roots, fan, nbr_o)
    return o, gnn_ref.union_edge_index(o["rowptr"], o["col"])


@pytest.mark.parametrize("hid,fused", [(256, True), (64, False)])
def test_sage_plan_l2_normalises_on_both_output_paths(graph, hid, fused):
    from gigl_amd.models import GraphSAGE
    eng, x, _ = _engine(graph, 100)
    try:
        fan = [9, 6]
        torch.manual_seed(hid)
        kw = dict(num_layers=2, conv_kwargs={"bias": False})
        on = GraphSAGE(100, hid, 47, should_l2_normalize_embedding_layer_output=True, **kw).to(eng.device)
        off = GraphSAGE(100, hid, 47, **kw).to(eng.device)
        off.load_state_dict(on.state_dict())
        o, ei = _oracle_union(graph, fan)
        sd = {k: v.detach().cpu() for k, v in on.state_dict().items()}
        want = gnn_ref.graphsage_forward(torch.from_numpy(x[o["nodes"]]), ei, sd, 2)[o["root_local"]]
        plan_on, plan_off = _check(eng, graph, on, off, fan, want)
        assert plan_on.fused_layers() == fused and plan_off.fused_layers() == fused
    finally:
        eng.close()


@pytest.mark.parametrize("de", [None, 6])
def test_gat_plan_l2_normalises(graph, de):
    from gigl_amd.models_attn import GAT
    n, rowptr, col, roots, lonely = graph
    eng, x, efeat = _engine(graph, 320, de)
    try:
        fan, heads = [7, 5], 2
        torch.manual_seed(3)
        kw = dict(num_layers=2, heads=heads, bias=False)
        if de is not None:
            kw.update(edge_dim=de, conv="edge_attr_gat", share_edge_att_message_weight=False)
        on = GAT(320, 32, 24, should_l2_normalize_embedding_layer_output=True, **kw).to(eng.device)
        off = GAT(320, 32, 24, **kw).to(eng.device)
        off.load_state_dict(on.state_dict())
        o, ei = _oracle_union(graph, fan)
        sd = {k: v.detach().cpu() for k, v in on.state_dict().items()}
        ea = None
        if de is not None:
            nodes = np.asarray(o["nodes"])
            pos = np.empty(ei.shape[1], dtype=np.int64)
            for i, (s, t) in enumerate(zip(nodes[ei[0].numpy()], nodes[ei[1].numpy()])):
                row = col[rowptr[t]:rowptr[t + 1]]
                k = np.searchsorted(row, s)
                assert k < len(row) and row[k] == s
                pos[i] = rowptr[t] + k
            ea = torch.from_numpy(efeat[pos])
        h = torch.from_numpy(x[o["nodes"]])
        for l in range(2):
            p = f"conv_layers.{l}."
            ekw = {} if de is None else dict(edge_attr=ea, w_edge=sd[p + "lin_edge.weight"], att_edge=sd[p + "att_edge"],
                                             w_edge_msg=sd[p + "lin_edge_message.weight"])
            h = gnn_ref.gat_conv(h, ei, sd[p + "lin.weight"], sd[p + "att_src"], sd[p + "att_dst"], None,
                                 heads if l == 0 else 1, **ekw)
            if l == 0:
                h = torch.relu(h)
        _check(eng, graph, on, off, fan, h[o["root_local"]])
    finally:
        eng.close()
