"""TEST INFRASTRUCTURE ONLY: the cases and float64 / float32 CPU restatements of tests/test_gpu_gcn_plan.py and
tests/test_gpu_gcn_plan_entry.py — the GCN INFERENCE plan (gigl_gcn_plan_*, csrc/pipeline.hip: sample -> generic union ->
dinv -> layer 1, aggregate-first or over the projected table -> layer 2, fused into the roots' rows or gather + projection +
copy) through engine.GcnPlan.  Graph, feature tables and root sets are tests/gcn_plan_cases.py's, by import.

Reference.  oracle.sample_khop(canonical=True) -> oracle.union_build -> gnn_ref.gcn_conv twice over the WHOLE union graph
(conv1 -> relu -> conv2, no dropout: the eval-time model) -> the roots' rows [-> L2 normalise], in FLOAT64 with the fp32
weights and fp32 / fp16 feature rows widened exactly.  The same restatement in float32 is the yardstick: the bound of a case
is the larger of 1e-5 and 4 x the float32 restatement's largest error against float64 (gcn_plan_cases.py's rule), absolute,
over every element of every row.  Nothing here reads a device result.  The rectifier is continuous, so a pre-activation
next to zero moves a row by no more than its own error: no guard is needed where no gradient is taken.
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch

import gcn_plan_cases as gc
from oracle import gnn_ref

ROW_TOL, FP32_FACTOR = 1e-5, 4.0


@dataclass(frozen=True)
class Case(gc.Case):
    l2: bool = False  # TwoLayerGCN(should_l2_normalize_output=True)


_CASES = [
    Case("base"),
    Case("scalar_paths", dims=(23, 30, 9), seed=2),   # no width a multiple of 4: element paths; fused root off by shape
    Case("wide_input", dims=(260, 16, 47)),           # projected route at 16 rows per wave
    Case("cora_width", dims=(1433, 16, 7)),           # d > 1024 aggregate-first (the element gather), and projected
    Case("fp16_table", dims=(24, 32, 47), half=True),
    Case("no_bias", bias=False),
    Case("long_rows", fan=(70, 3), roots="hubs", seed=2),   # rows beyond 64 edges
    Case("isolated_roots", roots="isolated"),
    Case("one_root_everywhere", roots="all"),         # the same root, with a stored self loop, in all 64 slots
    Case("l2_normalised", l2=True),
    Case("wide_hidden", dims=(24, 260, 7)),           # hidden width beyond the packed path (65 float4s per row)
    Case("overflow", b=16, roots="cluster"),
]
CASES = {c.name: c for c in _CASES}
PLAIN_CASES = [c.name for c in _CASES if c.roots != "cluster"]


def fused_root_by_shape(case: Case) -> bool:
    """include/gigl_hip.h: hid % 4 == 0, hid <= 1024, hid * out * 4 <= 64 KB"""
    hid, out = case.dims[1], case.dims[2]
    return hid % 4 == 0 and hid <= 1024 and hid * out * 4 <= 65536


def state_of(case: Case, seed_shift: int = 0):
    """the model's fp32 state dict; biases start off PyG's zero.  seed_shift: another draw of the same shapes"""
    from gigl_amd.models_attn import TwoLayerGCN
    torch.manual_seed(case.seed + 1000 * seed_shift)
    model = TwoLayerGCN(case.dims[0], case.dims[2], hid_dim=case.dims[1], is_training=False, bias=case.bias,
                        should_l2_normalize_output=case.l2)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if case.bias:
        g = torch.Generator().manual_seed(500 + case.seed + 1000 * seed_shift)
        for n in ("conv1.bias", "conv2.bias"):
            state[n] = (torch.rand(state[n].shape, generator=g) - 0.5) * 0.2
    return state


@functools.lru_cache(maxsize=None)
def batch(name: str):
    """-> (roots uint32 [b], the oracle's tree (nbr, cnt), the oracle's union graph)"""
    case = CASES[name]
    roots = gc._roots(case)[0]
    rowptr, col = gc.graph()[:2]
    nbr, cnt = gc.oracle.sample_khop(rowptr, col, roots, list(case.fan), canonical=True)
    u = gc.oracle.union_build(roots, list(case.fan), nbr)
    assert gc.fits(case, u) == (case.roots != "cluster"), name
    return roots, (nbr, cnt), u


def forward(case: Case, state, u, dtype) -> torch.Tensor:
    """the roots' rows [b, out] of the eval-time model over the whole union graph, in `dtype`"""
    p = {k: v.detach().to(dtype) for k, v in state.items()}
    ei = gnn_ref.union_edge_index(u["rowptr"], u["col"])
    h = torch.relu(gnn_ref.gcn_conv(gc._x(case, u, dtype), ei, p["conv1.lin.weight"], p.get("conv1.bias")))
    out = gnn_ref.gcn_conv(h, ei, p["conv2.lin.weight"], p.get("conv2.bias"))
    out = out[torch.from_numpy(u["root_local"].astype(np.int64))]
    return torch.nn.functional.normalize(out, p=2, dim=1) if case.l2 else out


@functools.lru_cache(maxsize=None)
def reference(name: str, seed_shift: int = 0):
    """-> (float64 rows, the case's bound)"""
    case = CASES[name]
    state, u = state_of(case, seed_shift), batch(name)[2]
    r64, r32 = forward(case, state, u, torch.float64), forward(case, state, u, torch.float32)
    fp32 = float((r32.double() - r64).abs().max())
    if case.l2:  # (a row next to the origin would turn its error into its direction's)
        raw = forward(Case(**{**case.__dict__, "l2": False}), state, u, torch.float64)
        assert float(raw.norm(dim=1).min()) > 1e-3, (name, float(raw.norm(dim=1).min()))
    return r64, max(ROW_TOL, FP32_FACTOR * fp32), fp32
