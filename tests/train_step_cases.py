"""TEST INFRASTRUCTURE ONLY: the cases, batches and float64 / float32 CPU restatements of
tests/test_gpu_train_step_edges.py — the node-classification training step (gigl_sage_train_plan_*, csrc/pipeline.hip:
sample -> union -> GraphSAGE forward -> cross-entropy on the roots -> backward -> Adam) at the shapes where the kernels
that exist only inside that step (ce_roots_kernel, loss_sum_kernel, train_stage_kernel, relu_mask_kernel, adam_kernel<false>
with chunk_sum) take another path.

Reference.  The CPU restatement of test_gpu_train_plan.py::test_library_training_step_against_the_cpu_restatement
(oracle.sample_khop(canonical=True) -> oracle.union_build -> gnn_ref.graphsage_forward over the whole union graph ->
F.cross_entropy(out[root_local], labels) -> autograd -> torch.optim.Adam(foreach=False)) in FLOAT64, the fp32 weights and
the fp32 / fp16 feature rows widened exactly.  The same restatement in float32 is the yardstick: a bound is the larger of
the project's bar for the quantity and 4 x the float32 restatement's own error against float64 (summation order, atomics,
__expf / __logf).  Nothing here reads a device result.

Rectifier guard.  A pre-activation within fp32 rounding of zero lets two correct implementations disagree about a
rectifier's mask, which moves a whole row of a weight gradient.  For every case with a rectifier the smallest
|pre-activation| of the float64 run — over the rows the plan computes (layer l: the nodes of level <= L-1-l) and over all
steps — must exceed 16 x the float32 run's largest pre-activation error; the seeds in the table were chosen, on the CPU,
so that it does.  `reference` asserts it; no element is left out of any comparison.
"""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import os
import sys

import numpy as np
import torch

for _p in (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:  # (run as a program: the repository and tests/ are not on the path yet)
        sys.path.insert(0, _p)

import oracle  # noqa: E402
from helpers import rmat_edges, torch_adam_moments  # noqa: E402
from oracle import gnn_ref  # noqa: E402

BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
ADAM_GRID = 208 * 256  # lanes of one pass of adam_kernel: launch_adam(st, 208, ...) x 256 (csrc/pipeline.hip train_enqueue_layers)
CE_LANES = 64          # ce_root_row strides a row's columns by one wave
N_RMAT, N_ISOLATED = 1 << 11, 8
N_NODES = N_RMAT + N_ISOLATED  # the last N_ISOLATED nodes have no edge at all: their mean half is zero
META_LEVEL0 = 2  # include/gigl_hip.h GIGL_META_LEVEL0: meta[2 + l] = nodes of level <= l
BAD_ROW = 7      # the row of a failed batch that carries the label outside [0, width)


@functools.lru_cache(maxsize=None)
def graph():
    s, d = rmat_edges(11, 40000, seed=21)
    rowptr, col = oracle.build_csc(N_NODES, s, d, is_directed=False)
    assert int(np.diff(rowptr)[N_RMAT:].max()) == 0
    return rowptr, col


@functools.lru_cache(maxsize=None)
def features(d: int, half: bool = False) -> np.ndarray:
    x = (np.random.default_rng(100 + d).standard_normal((N_NODES, d)) / 4).astype(np.float32)
    return x.astype(np.float16) if half else x


@dataclass(frozen=True)
class Case:
    name: str
    dims: Tuple[int, int, int]  # in, hidden, out (= class width)
    fan: Tuple[int, ...] = (5, 3)
    b: int = 64
    steps: int = 1              # batches handed to the plan (a failed one included)
    n_valid: Optional[int] = None  # real roots per batch (None: b)
    lr: float = 0.01
    wd: float = 0.0
    bias: bool = True
    act_last: bool = False
    half: bool = False          # fp16 feature table
    seed: int = 0               # of the weights, the roots and the labels
    roots: str = "perm"         # perm | twice | thrice | all | isolated
    labels: str = "cover"       # cover | extreme
    logits: float = 0.0         # > 0: the last layer is scaled so that the float64 max |logit| of step 0 is this
    peak: Optional[Tuple[int, float, float]] = None  # (column, its bias, the others' bias) of the last layer, after the scaling
    hidden_bias: float = 0.0    # > 0: the hidden layers' biases start at +- this (even units +, odd units -)
    bad: Optional[Tuple[int, int]] = None  # (step, label value): that batch's row BAD_ROW carries a label outside the width

    @property
    def L(self) -> int:
        return len(self.fan)

    @property
    def width(self) -> int:
        return self.dims[2]

    @property
    def k(self) -> int:
        return self.b if self.n_valid is None else self.n_valid

    @property
    def layer_dims(self):
        """dims[l] -> dims[l + 1] of layer l, as SageTrainPlan.dims"""
        return [self.dims[0]] + [self.dims[1]] * (self.L - 1) + [self.dims[2]]

    @property
    def n_t(self) -> int:
        """TrainPrep.n_t: the W_l^T that train_stage_kernel lays out (layers >= 1)"""
        return self.L - 1


WIDTHS = (1, 2, 63, 64, 65, 128, 129, 200)
BAD_LABELS = {"m1": -1, "width": 7, "2p40": 2 ** 40}
# (the seeds: see "Rectifier guard" above — `python tests/train_step_cases.py seeds N [case ...]` prints the margin of the
# cases for seeds 0..N-1)
_CASES = [
    # A.1 class widths on either side of one, two and three trips of the 64-lane stride
    *[Case(f"width_{w}", (24, 32, w)) for w in WIDTHS],
    Case("fp16_table", (24, 32, 47), half=True),
    # A.2 one node in several root slots, every copy with its own label
    Case("repeat_2", (24, 32, 7), roots="twice"),
    Case("repeat_3", (24, 32, 7), roots="thrice"),
    Case("repeat_64", (24, 32, 64), roots="all"),
    # A.3 real roots below the capacity
    Case("n_valid_1", (24, 32, 7), n_valid=1),
    Case("n_valid_63", (24, 32, 7), n_valid=63),
    Case("n_valid_64", (24, 32, 7), n_valid=64),
    # A.4 roots without in-edges beside ordinary ones
    Case("isolated_roots", (24, 32, 7), roots="isolated"),
    # A.5 logits of +-75: labels on the largest logit (loss ~ 0) and on the smallest (its probability underflows)
    Case("large_logits_47", (24, 32, 47), labels="extreme", logits=75.0),
    Case("large_logits_130", (24, 32, 130), labels="extreme", logits=75.0),
    # ... and one column of the second trip ~ 86 over all the others at ~ -8: a row maximum that misses it leaves
    # exp(logit - max) = exp(> 89) = inf in fp32 (any smaller shift gives the same log-sum-exp, mathematically)
    Case("peak_column_100", (24, 32, 130), labels="extreme", logits=2.0, peak=(100, 86.0, -8.0)),
    # B.1-3 a failed batch, then a good one: the reference trains the good one alone (Adam at t = 1)
    *[Case(f"failed_{k}", (24, 32, 7), steps=2, bad=(0, v)) for k, v in BAD_LABELS.items()],
    # B.4 five batches, the third fails
    Case("failed_in_queue", (24, 32, 7), steps=5, wd=5e-4, bad=(2, 7)),
    # C layer counts and optional tensors (layers_4: b = 48 — at b = 64 none of the seeds 0..23 met the rectifier guard over
    # its three rectified layers)
    Case("layers_1", (22, 30, 9), fan=(6,), steps=3, wd=5e-4),
    Case("layers_3", (22, 30, 9), fan=(4, 3, 2), steps=3, wd=5e-4),
    Case("layers_4", (22, 30, 9), fan=(3, 2, 2, 2), b=48, steps=3, wd=5e-4, seed=16),
    Case("layers_3_no_bias", (22, 30, 9), fan=(4, 3, 2), steps=3, wd=5e-4, bias=False, seed=13),
    Case("layers_3_act_last", (22, 30, 9), fan=(4, 3, 2), steps=3, wd=5e-4, act_last=True, seed=5),
    # D.1 W_0 (300 x 200) larger than one pass of the Adam grid, 30 steps.  Over thirty steps the float32 restatement's
    # pre-activations drift 1e-5 .. 1e-3 from float64's (an element whose gradient is rounding noise moves by up to lr per
    # step whatever the precision) and no seed leaves 2e6 pre-activations 16 x that far from zero: the hidden biases start at
    # +-1.5, so that every hidden unit stays on one side of its rectifier (smallest |pre-activation| 0.28) — half the units
    # are dead, their rows of W_0 move by the decay alone; the rectifier's mask per element is the other cases' business
    Case("adam_two_passes", (100, 300, 7), steps=30, wd=5e-4, hidden_bias=1.5),
    # D.2 chunks of partial sums that hold real rows: see CHUNK_TARGETS
    Case("chunks_15", (24, 32, 7), b=192),
    Case("chunks_16", (24, 32, 7), b=192),
    Case("chunks_17", (24, 32, 7), b=192),
    Case("chunks_33", (24, 32, 7), b=1000, fan=(1, 1)),
]
# the first layer's chunk count of the chunk cases (chunks_33: at least): the number of real roots — the shortest prefix of
# the permutation that gives it, from the oracle's level sizes — decides the rows.  The plan's capacity b only has to keep
# the rule at 32 rows per chunk (b (1 + f0) < 2048); with roots of one permutation the first layer of this graph stays
# below 29 chunks at fan-outs above 1, so the 33-chunk case takes 1000 roots at fan-outs (1, 1)
CHUNK_TARGETS = {"chunks_15": 15, "chunks_16": 16, "chunks_17": 17, "chunks_33": 33}
CASES = {c.name: c for c in _CASES}
LOSS_CASES = [c.name for c in _CASES if c.steps == 1]
LAYER_CASES = [c.name for c in _CASES if c.name.startswith("layers_")]


# ---- the chunk rule ---------------------------------------------------------------------------------------------------
def wgrad_rows_per_chunk(m_cap: int, n: int, k: int) -> int:
    """csrc/agg.hip wgrad_rows_per_chunk (what gigl_linear_weight_grad_chunks hands the plan as part_rc; no binding):
    256 rows, halved down to 32 while the capacity gives fewer than 32 chunks, doubled while chunks x tiles > 4096"""
    rcw = 256
    while rcw > 32 and m_cap // rcw < 32:
        rcw >>= 1
    tiles = ((n + 63) // 64) * ((k + 63) // 64)
    while rcw < 8192 and ((m_cap + rcw - 1) // rcw) * tiles > 4096:
        rcw <<= 1
    return rcw


def level_rows_cap(b: int, fan, level_max: int) -> int:
    """csrc/common.h gigl_level_rows of a regular (not wide) plan: b (1 + f0 + f0 f1 + ...) over level_max fan-outs"""
    rows, width = 0, b
    for i in range(level_max + 1):
        rows += width
        if i < len(fan):
            width *= fan[i]
    return rows


def chunk_counts(case: Case, u) -> list:
    """per layer: the chunks of the weight gradient's partial sums that hold real rows of the batch — what adam_kernel
    hands chunk_sum (ceil(level rows / part_rc))"""
    L, d = case.L, case.layer_dims
    out = []
    for l in range(L):
        rc = wgrad_rows_per_chunk(level_rows_cap(case.b, case.fan, L - 1 - l), d[l + 1], 2 * d[l])
        out.append(-(-int(u["meta"][META_LEVEL0 + L - 1 - l]) // rc))
    return out


# ---- batches ----------------------------------------------------------------------------------------------------------
def _union(case: Case, roots: np.ndarray):
    rowptr, col = graph()
    nbr, _ = oracle.sample_khop(rowptr, col, roots, list(case.fan), canonical=True)
    return oracle.union_build(roots, list(case.fan), nbr)


def fits(case: Case, u) -> bool:
    """the batch fits the regular workspace (no root's children moved up a level past a buffer): the plan need not grow"""
    return all(int(u["meta"][META_LEVEL0 + l]) <= level_rows_cap(case.b, case.fan, l) for l in range(case.L))


def _roots(case: Case) -> list:
    rowptr, _ = graph()
    deg = np.diff(rowptr)
    rng = np.random.default_rng(1000 + case.seed)
    k = case.k
    if case.name in CHUNK_TARGETS:
        # the number of real roots decides the rows of the first layer: the first prefix of the permutation that gives the
        # wanted number of chunks
        perm = rng.permutation(N_RMAT).astype(np.uint32)
        want = CHUNK_TARGETS[case.name]
        lo, hi = 1, case.b  # (a longer prefix never has fewer rows: bisect for the shortest one that reaches the count)
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if chunk_counts(case, _union(case, perm[:mid]))[0] >= want else (mid + 1, hi)
        n = chunk_counts(case, _union(case, perm[:lo]))[0]
        if n == want or (n > 33 and case.name == "chunks_33"):
            return [perm[:lo]]
        raise AssertionError(f"{case.name}: no prefix gives {CHUNK_TARGETS[case.name]} chunks")
    perm = rng.permutation(N_RMAT).astype(np.uint32)
    assert case.steps * k <= N_RMAT
    out = [perm[i * k:(i + 1) * k].copy() for i in range(case.steps)]
    r = out[0]
    if case.roots == "twice":
        r[5] = r[4]
    elif case.roots == "thrice":
        r[20] = r[41] = r[3]
    elif case.roots == "all":
        r[:] = perm[np.nonzero(deg[perm] >= 8)[0][0]]
    elif case.roots == "isolated":
        r[1::8] = np.arange(N_RMAT, N_NODES, dtype=np.uint32)
        assert (deg[r] == 0).sum() >= N_ISOLATED and (deg[r] > 0).sum() >= k // 2
    else:
        assert case.roots == "perm"
    return out


REPEATS = {"twice": (4, 5), "thrice": (3, 20, 41), "all": tuple(range(64))}


def _labels(case: Case, roots: list, logits0) -> list:
    rng = np.random.default_rng(2000 + case.seed)
    w = case.width
    out = [rng.integers(0, w, r.size).astype(np.int64) for r in roots]
    y = out[0]
    if case.labels == "extreme":
        # a third on the row's largest logit, a third on its smallest, the rest anywhere
        t = y.size // 3
        y[:t] = logits0[:t].argmax(1)
        y[t:2 * t] = logits0[t:2 * t].argmin(1)
    elif case.roots in REPEATS:
        slots = REPEATS[case.roots]
        y[list(slots)] = rng.permutation(w)[: len(slots)]  # every copy its own label
    elif y.size >= 4 and not case.bad:
        y[0], y[1] = 0, w - 1
        if w > CE_LANES:
            y[2], y[3] = CE_LANES, w - 1
    if case.bad:
        out[case.bad[0]][BAD_ROW] = case.bad[1]
    return out


def _forward(case: Case, params, u, dtype):
    x = torch.from_numpy(features(case.dims[0], case.half)[u["nodes"].astype(np.int64)].astype(np.float32)).to(dtype)
    ei = gnn_ref.union_edge_index(u["rowptr"], u["col"])
    out = gnn_ref.graphsage_forward(x, ei, params, case.L, case.act_last)
    return out[torch.from_numpy(u["root_local"].astype(np.int64))]


def _pre_activations(case: Case, params, u, dtype):
    """the inputs of every rectifier, over the rows the plan computes (layer l: level <= L-1-l; the union graph is numbered
    level by level) — one flat tensor"""
    pre = []
    with torch.no_grad():
        h = torch.from_numpy(features(case.dims[0], case.half)[u["nodes"].astype(np.int64)].astype(np.float32)).to(dtype)
        ei = gnn_ref.union_edge_index(u["rowptr"], u["col"])
        for l in range(case.L):
            if not (l < case.L - 1 or case.act_last):
                break
            p = f"conv_layers.{l}."
            z = gnn_ref.sage_conv(h, ei, params[p + "lin_l.weight"], params.get(p + "lin_l.bias"), params[p + "lin_r.weight"])
            pre.append(z[: int(u["meta"][META_LEVEL0 + case.L - 1 - l])].reshape(-1))
            h = torch.relu(z)
    return torch.cat(pre) if pre else torch.zeros(0, dtype=dtype)


@functools.lru_cache(maxsize=None)
def setup(name: str):
    """-> (initial state dict (fp32), [(roots uint32 [k], labels int64 [k], oracle union graph) per batch])"""
    from gigl_amd.models import GraphSAGE
    case = CASES[name]
    torch.manual_seed(case.seed)
    model = GraphSAGE(case.dims[0], case.dims[1], case.dims[2], num_layers=case.L,
                      activation_after_last_conv=case.act_last, bias=case.bias)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert (f"conv_layers.0.lin_l.bias" in state) == case.bias
    if case.hidden_bias > 0:
        for l in range(case.L - 1):
            sign = 1.0 - 2.0 * (torch.arange(case.dims[1]) % 2).float()
            state[f"conv_layers.{l}.lin_l.bias"] = sign * case.hidden_bias
    roots = _roots(case)
    unions = [_union(case, r) for r in roots]
    assert all(fits(case, u) for u in unions), name
    logits0 = None
    if case.logits > 0:
        last = f"conv_layers.{case.L - 1}."
        wide = {k: v.double() for k, v in state.items()}
        with torch.no_grad():
            s = np.float32(case.logits / float(_forward(case, wide, unions[0], torch.float64).abs().max()))
            for k in ("lin_l.weight", "lin_r.weight", "lin_l.bias"):
                state[last + k] = state[last + k] * s  # (fp32: the tensors the plan is created over)
            if case.peak:
                state[last + "lin_l.bias"] = torch.full((case.width,), case.peak[2])
                state[last + "lin_l.bias"][case.peak[0]] = case.peak[1]
            logits0 = _forward(case, {k: v.double() for k, v in state.items()}, unions[0], torch.float64).numpy()
    labels = _labels(case, roots, logits0)
    return state, list(zip(roots, labels, unions))


# ---- the restatement ---------------------------------------------------------------------------------------------------
@dataclass
class Run:
    losses: list     # of the batches that train (a failed one is skipped)
    logits0: torch.Tensor
    grads0: dict     # the first trained step's gradients, before the decay
    params: dict
    moments: dict
    pre: list        # per trained step: the rectifiers' inputs


def restate(name: str, dtype) -> Run:
    case = CASES[name]
    state, batches = setup(name)
    params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    opt = torch.optim.Adam(list(params.values()), lr=case.lr, weight_decay=case.wd, betas=(BETA1, BETA2), eps=ADAM_EPS,
                           foreach=False)
    losses, pre, grads0, logits0 = [], [], None, None
    for i, (roots, labels, u) in enumerate(batches):
        if case.bad and i == case.bad[0]:
            continue
        pre.append(_pre_activations(case, params, u, dtype))
        out = _forward(case, params, u, dtype)
        loss = torch.nn.functional.cross_entropy(out, torch.from_numpy(labels))
        opt.zero_grad()
        loss.backward()
        if grads0 is None:
            grads0, logits0 = {k: p.grad.detach().clone() for k, p in params.items()}, out.detach().clone()
        opt.step()
        losses.append(float(loss.detach()))
    return Run(losses, logits0, grads0, {k: p.detach() for k, p in params.items()}, torch_adam_moments(opt, params), pre)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """-> (float64 run, float32 run) of the case, the rectifier guard asserted"""
    r64, r32 = restate(name, torch.float64), restate(name, torch.float32)
    margin = guard_margin(r64, r32)
    assert margin > 16.0, f"{name}: a pre-activation lies within 16 x the fp32 restatement's error of zero ({margin:.1f} x)"
    return r64, r32


def guard_margin(r64: Run, r32: Run) -> float:
    """smallest |pre-activation| of the float64 run / the float32 run's largest pre-activation error (inf: no rectifier)"""
    if not sum(p.numel() for p in r64.pre):
        return float("inf")
    smallest = min(float(p.abs().min()) for p in r64.pre if p.numel())
    err = max(float((a.double() - b).abs().max()) for a, b in zip(r32.pre, r64.pre) if b.numel())
    return smallest / max(err, 1e-300)


def fused(d: dict, l: int) -> torch.Tensor:
    """[W_l | W_r] of layer l, as the plan trains it, from tensors keyed like the model's state dict"""
    return torch.cat([d[f"conv_layers.{l}.lin_l.weight"], d[f"conv_layers.{l}.lin_r.weight"]], dim=1)


if __name__ == "__main__":  # `seeds N [case ...]`: the guard's margin of the cases for seeds 0..N-1 (how the table's were chosen)
    import dataclasses
    import sys
    n = int(sys.argv[2])
    for nm in sys.argv[3:] or list(CASES):
        for s in range(n):
            CASES[nm] = dataclasses.replace(CASES[nm], seed=s)
            setup.cache_clear()
            try:
                print(nm, "seed", s, "margin %.1f" % guard_margin(restate(nm, torch.float64), restate(nm, torch.float32)), flush=True)
            except AssertionError as e:  # (a batch that does not fit the regular workspace)
                print(nm, "seed", s, "unusable:", e, flush=True)
