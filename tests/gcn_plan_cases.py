"""TEST INFRASTRUCTURE ONLY: the cases, batches and float64 / float32 CPU restatements of tests/test_gpu_gcn_train_plan.py —
the GCN training step (gigl_gcn_train_plan_*, csrc/pipeline.hip: sample -> generic union -> dinv, transposed lists ->
gcn gather -> projection + relu [-> dropout] -> gcn gather -> projection -> cross-entropy on the roots -> backward -> Adam)
through engine.GcnTrainPlan.  Modelled on tests/train_step_cases.py.

Reference.  oracle.sample_khop(canonical=True) -> oracle.union_build -> the module's forward restated with
gnn_ref.gcn_conv over the WHOLE union graph (conv1 -> relu [-> the plan's dropout mask, dropout_ref.keep_mask by local id]
-> conv2) -> F.cross_entropy(out[root_local], labels) -> autograd -> torch.optim.Adam(foreach=False), in FLOAT64 with the
fp32 weights and fp32 / fp16 feature rows widened exactly.  The same restatement in float32 is the yardstick: a bound is the
larger of the project's bar for the quantity and 4 x the float32 restatement's own error against float64.  Nothing here
reads a device result.

Rectifier guard, exactly as train_step_cases.py: the smallest |pre-activation| of conv1 in the float64 run — over the rows
the plan computes (the nodes of level <= 1) and over all steps — must exceed 16 x the float32 run's largest pre-activation
error; the seeds in the table were chosen on the CPU so that it does (`python tests/gcn_plan_cases.py seeds N [case ...]`).
`reference` asserts it; no element is left out of any comparison.

Graph: R-MAT over 2^11 nodes, 8 isolated nodes behind them, and explicit self-loop edges on N_LOOPS low-degree nodes (a
stored self loop is what PyG's add_remaining_self_loops replaces; the sampler hands it on like any neighbour).  Every
ordinary batch starts with LOOP_ROOTS roots that carry one and LOOP_PARENTS roots whose sampled children carry one.
"""
import functools
import os
import sys
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

for _p in (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:  # (run as a program: the repository and tests/ are not on the path yet)
        sys.path.insert(0, _p)

import oracle  # noqa: E402
from dropout_ref import keep_mask, scale as dropout_scale  # noqa: E402
from helpers import rmat_edges, torch_adam_moments  # noqa: E402
from oracle import gnn_ref  # noqa: E402

BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
N_RMAT, N_ISOLATED, N_LOOPS = 1 << 11, 8, 64
N_NODES = N_RMAT + N_ISOLATED
META_N_NODES, META_LEVEL0 = 0, 2  # include/gigl_hip.h: meta[0] = nodes, meta[2 + l] = nodes of level <= l
LOOP_ROOTS, LOOP_PARENTS = 4, 4
BAD_ROW = 7
DROP_P, DROP_SEED = 0.5, 0x1234_5678_9ABC_DEF0
NAMES = ("conv1.lin.weight", "conv1.bias", "conv2.lin.weight", "conv2.bias")


@functools.lru_cache(maxsize=None)
def graph():
    """-> (rowptr, col, the nodes that got an explicit self-loop edge, LOOP_PARENTS (parent, child) pairs).  The loops sit
    on nodes of 1..3 neighbours, so that a fan-out of 3 or more takes the loop with all the others; the children of the
    pairs come first: nodes of at most 2 neighbours next to a node of at most 5 (R-MAT has a handful of such edges)"""
    s, d = rmat_edges(11, 40000, seed=21)
    rowptr, col = oracle.build_csc(N_NODES, s, d, is_directed=False)
    deg = np.diff(rowptr)
    pairs = [(p, int(v)) for p in range(N_RMAT) if 1 <= deg[p] <= 5 for v in col[rowptr[p]:rowptr[p + 1]]
             if v != p and 1 <= deg[v] <= 2][:LOOP_PARENTS]
    assert len(pairs) == LOOP_PARENTS and len({v for _, v in pairs} | {p for p, _ in pairs}) == 2 * LOOP_PARENTS
    low = np.nonzero((deg[:N_RMAT] >= 1) & (deg[:N_RMAT] <= 3))[0]
    rest = [int(v) for v in np.random.default_rng(77).permutation(low) if all(int(v) not in pr for pr in pairs)]
    loops = np.array([v for _, v in pairs] + rest[:N_LOOPS - LOOP_PARENTS], dtype=np.uint32)
    rowptr, col = oracle.build_csc(N_NODES, np.concatenate([s, loops]), np.concatenate([d, loops]), is_directed=False)
    assert int(np.diff(rowptr)[N_RMAT:].max()) == 0
    assert all(int(v) in col[rowptr[v]:rowptr[v + 1]] for v in loops) and loops.size >= 32
    return rowptr, col, loops, pairs


@functools.lru_cache(maxsize=None)
def features(d: int, half: bool = False) -> np.ndarray:
    x = (np.random.default_rng(100 + d).standard_normal((N_NODES, d)) / 4).astype(np.float32)
    return x.astype(np.float16) if half else x


@dataclass(frozen=True)
class Case:
    name: str
    dims: Tuple[int, int, int] = (24, 32, 7)  # in, hidden, out (= class width)
    fan: Tuple[int, int] = (5, 3)
    b: int = 64
    steps: int = 1
    n_valid: Optional[int] = None
    lr: float = 0.01
    wd: float = 0.0
    bias: bool = True
    half: bool = False
    seed: int = 0
    roots: str = "perm"      # perm | all | isolated | hubs | cluster
    dropout: bool = False    # TwoLayerGCN(is_training=True): p = 0.5 from the plan's stream
    bad: Optional[Tuple[int, int]] = None  # (step, label value): that batch's row BAD_ROW carries a label outside the width

    @property
    def width(self) -> int:
        return self.dims[2]

    @property
    def k(self) -> int:
        return self.b if self.n_valid is None else self.n_valid


# (the seeds: see "Rectifier guard" above)
_CASES = [
    Case("base"),
    Case("scalar_paths", dims=(23, 30, 9), seed=2),       # no width is a multiple of 4: both kernels' element paths
    Case("wide_input", dims=(260, 16, 47)),               # 64 lanes x 2 float4s over the table, 47 classes
    Case("fp16_table", dims=(24, 32, 47), half=True),
    Case("no_bias", bias=False),
    Case("long_rows", fan=(70, 3), roots="hubs", seed=2),       # root rows beyond 64 edges inside the plan
    Case("isolated_roots", roots="isolated"),
    Case("one_root_everywhere", roots="all"),
    Case("n_valid_1", n_valid=1),
    Case("n_valid_63", n_valid=63),
    Case("three_steps_decay", steps=3, wd=5e-4),
    Case("failed_then_resumed", steps=2, bad=(0, 7)),     # label == width
    Case("overflow_redone", b=16, roots="cluster"),       # roots that are each other's neighbours: the plan grows
    Case("dropout", steps=3, wd=5e-4, dropout=True),
]
CASES = {c.name: c for c in _CASES}
PLAIN_CASES = [c.name for c in _CASES if c.steps == 1 and c.roots != "cluster"]


def level_rows_cap(b: int, fan, level_max: int) -> int:
    """csrc/common.h gigl_level_rows of a regular (not wide) plan"""
    rows, width = 0, b
    for i in range(level_max + 1):
        rows += width
        if i < len(fan):
            width *= fan[i]
    return rows


def _union(case: Case, roots: np.ndarray):
    rowptr, col = graph()[:2]
    nbr, _ = oracle.sample_khop(rowptr, col, roots, list(case.fan), canonical=True)
    return oracle.union_build(roots, list(case.fan), nbr)


def fits(case: Case, u) -> bool:
    return all(int(u["meta"][META_LEVEL0 + l]) <= level_rows_cap(case.b, case.fan, l) for l in range(2))


def stored_self_loops(u):
    """local ids of the union graph's rows that store their own node"""
    rp, col = u["rowptr"], u["col"]
    return [i for i in range(rp.size - 1) if i in col[rp[i]:rp[i + 1]]]


def _loop_seeds():
    """(roots that carry a self loop, roots with a child that carries one): low-degree nodes, so that the sampler takes all
    their neighbours"""
    rowptr, col, loops, pairs = graph()
    deg = np.diff(rowptr)
    own = [int(v) for v in loops[LOOP_PARENTS:] if deg[v] <= 4][:LOOP_ROOTS]
    assert len(own) == LOOP_ROOTS
    return own, [p for p, _ in pairs]


def _roots(case: Case) -> list:
    rowptr, col = graph()[:2]
    deg = np.diff(rowptr)
    rng = np.random.default_rng(1000 + case.seed)
    k = case.k
    perm = rng.permutation(N_RMAT).astype(np.uint32)
    if case.roots == "cluster":
        # a node, the children the sampler gives it, and nodes with a full fan-out: the first root's children are roots
        # themselves, THEIR children move up a level, and the rows of level <= 1 outgrow b (1 + f0)
        for start in perm[deg[perm] >= case.fan[0]]:
            nbr, _ = oracle.sample_khop(rowptr, col, np.array([start], dtype=np.uint32), list(case.fan), canonical=True)
            r = [int(start)] + [int(v) for v in nbr[0] if v != 0xFFFFFFFF and v != start]
            r += [int(v) for v in perm if deg[v] >= case.fan[0] and int(v) not in r][:k - len(r)]
            r = np.array(r[:k], dtype=np.uint32)
            if not fits(case, _union(case, r)):
                return [r]
        raise AssertionError("no cluster of roots overflows the regular workspace")
    own, parents = _loop_seeds()
    head = np.array(own + parents, dtype=np.uint32)
    perm = perm[~np.isin(perm, head)]
    assert case.steps * k <= perm.size
    out = [perm[i * k:(i + 1) * k].copy() for i in range(case.steps)]
    for r in out:
        if k >= 16 and case.roots in ("perm", "isolated"):
            r[:head.size] = head
    r = out[0]
    if case.roots == "all":
        r[:] = own[0]  # (a root with a stored self loop, in every slot)
    elif case.roots == "isolated":
        r[9::8] = np.arange(N_RMAT, N_RMAT + r[9::8].size, dtype=np.uint32)
        assert (deg[r] == 0).sum() >= 6 and (deg[r] > 0).sum() >= k // 2
    elif case.roots == "hubs":
        hubs = perm[deg[perm] >= case.fan[0]]
        assert hubs.size >= k
        r[:] = hubs[:k]
    else:
        assert case.roots == "perm"
    return out


def _labels(case: Case, roots: list) -> list:
    rng = np.random.default_rng(2000 + case.seed)
    out = [rng.integers(0, case.width, r.size).astype(np.int64) for r in roots]
    if out[0].size >= 4 and not case.bad:
        out[0][0], out[0][1] = 0, case.width - 1
    if case.bad:
        out[case.bad[0]][BAD_ROW] = case.bad[1]
    return out


def _x(case: Case, u, dtype):
    return torch.from_numpy(features(case.dims[0], case.half)[u["nodes"].astype(np.int64)].astype(np.float32)).to(dtype)


def _forward(case: Case, params, u, dtype, step: int):
    """-> (the roots' logits, conv1's pre-activations over the rows the plan computes)"""
    ei = gnn_ref.union_edge_index(u["rowptr"], u["col"])
    z = gnn_ref.gcn_conv(_x(case, u, dtype), ei, params["conv1.lin.weight"], params.get("conv1.bias"))
    h = torch.relu(z)
    n1 = int(u["meta"][META_LEVEL0 + 1])
    if case.dropout:
        # rows by LOCAL id, as oracle.union_build numbers them (= gigl_union_build's: the plan's generic union); rows beyond
        # level 1 feed no root
        keep = torch.ones(h.shape, dtype=dtype)
        keep[:n1] = torch.from_numpy(keep_mask(DROP_SEED, step, 0, 0, n1, case.dims[1], DROP_P).astype(np.float64)).to(dtype)
        h = h * keep * float(dropout_scale(DROP_P))
    out = gnn_ref.gcn_conv(h, ei, params["conv2.lin.weight"], params.get("conv2.bias"))
    return out[torch.from_numpy(u["root_local"].astype(np.int64))], z[:n1].reshape(-1)


@functools.lru_cache(maxsize=None)
def setup(name: str):
    """-> (initial state dict (fp32), [(roots uint32 [k], labels int64 [k], oracle union graph) per batch])"""
    from gigl_amd.models_attn import TwoLayerGCN
    case = CASES[name]
    torch.manual_seed(case.seed)
    model = TwoLayerGCN(case.dims[0], case.dims[2], hid_dim=case.dims[1], is_training=case.dropout, bias=case.bias)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert sorted(state) == sorted(n for n in NAMES if case.bias or not n.endswith("bias"))
    if case.bias:  # (PyG starts the biases at zero: start them off it, so that their Adam state is exercised from a real value)
        g = torch.Generator().manual_seed(500 + case.seed)
        for n in ("conv1.bias", "conv2.bias"):
            state[n] = (torch.rand(state[n].shape, generator=g) - 0.5) * 0.2
    roots = _roots(case)
    unions = [_union(case, r) for r in roots]
    assert all(fits(case, u) for u in unions) == (case.roots != "cluster"), name
    return state, list(zip(roots, _labels(case, roots), unions))


@dataclass
class Run:
    losses: list   # of the batches that train (a failed one is skipped)
    grads0: dict   # the first trained step's gradients, before the decay
    params: dict
    moments: dict
    pre: list      # per trained step: conv1's pre-activations


def restate(name: str, dtype) -> Run:
    case = CASES[name]
    state, batches = setup(name)
    params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    opt = torch.optim.Adam(list(params.values()), lr=case.lr, weight_decay=case.wd, betas=(BETA1, BETA2), eps=ADAM_EPS,
                           foreach=False)
    losses, pre, grads0, step = [], [], None, 0
    for i, (roots, labels, u) in enumerate(batches):
        if case.bad and i == case.bad[0]:
            continue
        out, z = _forward(case, params, u, dtype, step)  # (step: Adam's count of APPLIED steps — a failed batch moves nothing)
        pre.append(z.detach())
        loss = torch.nn.functional.cross_entropy(out, torch.from_numpy(labels))
        opt.zero_grad()
        loss.backward()
        if grads0 is None:
            grads0 = {k: p.grad.detach().clone() for k, p in params.items()}
        opt.step()
        step += 1
        losses.append(float(loss.detach()))
    return Run(losses, grads0, {k: p.detach() for k, p in params.items()}, torch_adam_moments(opt, params), pre)


def guard_margin(r64: Run, r32: Run) -> float:
    smallest = min(float(p.abs().min()) for p in r64.pre)
    err = max(float((a.double() - b).abs().max()) for a, b in zip(r32.pre, r64.pre))
    return smallest / max(err, 1e-300)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """-> (float64 run, float32 run) of the case, the rectifier guard asserted"""
    r64, r32 = restate(name, torch.float64), restate(name, torch.float32)
    margin = guard_margin(r64, r32)
    assert margin > 16.0, f"{name}: a pre-activation lies within 16 x the fp32 restatement's error of zero ({margin:.1f} x)"
    return r64, r32


if __name__ == "__main__":  # `seeds N [case ...]`: the guard's margin of the cases for seeds 0..N-1 (how the table's were chosen)
    import dataclasses
    n = int(sys.argv[2])
    for nm in sys.argv[3:] or list(CASES):
        for s in range(n):
            CASES[nm] = dataclasses.replace(CASES[nm], seed=s)
            setup.cache_clear()
            try:
                print(nm, "seed", s, "margin %.1f" % guard_margin(restate(nm, torch.float64), restate(nm, torch.float32)), flush=True)
            except AssertionError as e:
                print(nm, "seed", s, "unusable:", e, flush=True)
