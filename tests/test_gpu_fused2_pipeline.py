"""linear_fused2x_kernel's operand pipeline at its edges: one, two and three 32-k chunks, a ragged last chunk, row counts
that leave a partial last 128-row tile, and tiles that straddle the roots / non-roots boundary (the W_r block skip) or
end exactly on it.  The fused plan's rows against the layers run apart (GIGL_PLAN_NO_FUSE2) at 4e-6 of the largest row
entry, and against the fp32 CPU forward of the reference's execution order at 1e-5 (tests/test_gpu_plan.py's bounds)."""
import os

import numpy as np
import pytest
import torch

import oracle
from helpers import rmat_edges

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def graph():
    s, d = rmat_edges(13, 150000, seed=8)
    n = 1 << 13
    rowptr, col = oracle.build_csc(n, s, d, is_directed=False)
    return rowptr, col, n


def _oracle_rows(rowptr, col, x, roots, fan, model):
    from oracle import gnn_ref
    nbr_o, _ = oracle.sample_khop(rowptr, col, roots, fan, canonical=True)
    o = oracle.union_build(roots, fan, nbr_o)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ei = gnn_ref.union_edge_index(o["rowptr"], o["col"])
    return gnn_ref.graphsage_forward(torch.from_numpy(x[o["nodes"]].astype(np.float32)), ei, sd, 2)[o["root_local"]].numpy()


# (input width d_in -> K = 2 d_in, roots per batch, batches per call, fanouts)
CASES = [
    (16, 200, 1, [6, 4]),   # K = 32: one chunk (no prefetch at all); 200 roots: tile 1 straddles the roots
    (32, 130, 2, [5, 3]),   # K = 64: two chunks; 130 roots: the second tile holds 2 roots
    (48, 5, 1, [4, 2]),     # K = 96: three chunks; a single partial tile, roots and non-roots in it
    (40, 77, 2, [7, 5]),    # K = 80: last chunk of 16 k (its second MFMA step skipped)
    (44, 256, 1, [3, 3]),   # K = 88: last chunk of 24 k (zero-padded step); 256 roots: boundary on a tile edge
    (100, 128, 3, [9, 4]),  # K = 200 (the products shape): seven chunks, the last of 8 k; 128 roots per batch
]


@pytest.mark.parametrize("d_in,b,G,fan", CASES)
def test_fused2_pipeline_edges_against_the_separate_layers_and_the_oracle(graph, d_in, b, G, fan):
    from gigl_amd.engine import HipEngine
    from gigl_amd.models import GraphSAGE
    rowptr, col, n = graph
    rng = np.random.default_rng(300 + d_in)
    x = (rng.standard_normal((n, d_in)) / 4).astype(np.float32)
    eng = HipEngine(0)
    try:
        eng.load_csc(rowptr, col)
        eng.load_features(x)
        torch.manual_seed(d_in + b)
        model = GraphSAGE(d_in, 256, 47, num_layers=2).to(eng.device)
        plan = model.make_plan(eng, b, fan, groups=G)
        assert plan.fused_layers()
        os.environ["GIGL_PLAN_NO_FUSE2"] = "1"
        try:
            apart = model.make_plan(eng, b, fan, groups=G)
        finally:
            del os.environ["GIGL_PLAN_NO_FUSE2"]
        assert not apart.fused_layers()
        roots = rng.integers(0, n, size=G * b).astype(np.uint32)
        r_dev = torch.from_numpy(roots.view(np.int32)).to(eng.device)
        out = plan.run(r_dev).cpu().numpy()
        ref = apart.run(r_dev).cpu().numpy()
        assert np.isfinite(out).all() and out.shape == (G * b, 47)
        assert np.abs(out - ref).max() <= 4e-6 * np.abs(ref).max()
        for gi in range(G):
            want = _oracle_rows(rowptr, col, x, roots[gi * b:(gi + 1) * b], fan, model)
            assert np.abs(out[gi * b:(gi + 1) * b] - want).max() <= 1e-5 * max(np.abs(want).max(), 1e-30)
        again = plan.run(r_dev).cpu().numpy()
        assert np.array_equal(again, out)
        plan.close()
        apart.close()
    finally:
        eng.close()
