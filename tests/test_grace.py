"""GRACE: the fused two-view contrastive loss (csrc/contrast.hip), the augmentations and the task against an fp64 restatement
of the reference (python/gigl/src/common/models/layers/loss.py:362-416 in log space, task.py:212-279).  Row tile of the MFMA
kernels: 64, K chunk 32, backward column chunk 128.  Bars: loss within 1e-5 max(1, |want|) (relative: at small T the loss is
in the hundreds and one fp32 ulp exceeds 1e-5), gradient within 1e-4 of max|grad64|.

Measured on an MI355X: the largest loss error is 3.5e-7 (relative); gradient errors stay below 5e-7 of max|grad64| over the
shape grid, 2.4e-6 on the near-identical views, 2.0e-5 at T = 0.001 (the largest).  At d = 1 the true gradient is zero: the
kernels return exact zeros and the fp64 reference 1e-17 of rounding noise, which is why `check` floors the gradient bar at
the reference's own rounding error."""
import copy
from types import SimpleNamespace

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"


def views(n, d, seed, kind="plain"):
    """two views' rows, randn * 3 (not normalised), on the device"""
    g = torch.Generator().manual_seed(seed)
    h1, h2 = 3 * torch.randn(n, d, generator=g), 3 * torch.randn(n, d, generator=g)
    if kind == "near":
        h2 = h1 + 1e-3 * torch.randn(n, d, generator=g)
    elif kind == "dup":
        h1, h2 = (h[:(n + 1) // 2].repeat_interleave(2, dim=0)[:n] for h in (h1, h2))
    elif kind == "zero":
        h1[n // 3] = 0
    if kind == "view":  # rows of a wider matrix: ld > d
        return tuple(torch.cat((h, torch.randn(n, 7, generator=g)), dim=1).to(DEV)[:, :d] for h in (h1, h2))
    return h1.to(DEV), h2.to(DEV)


def grace64(h1, h2, t):
    a, b = (h / h.norm(dim=1, keepdim=True).clamp_min(1e-8) for h in (h1, h2))
    eye = torch.eye(a.shape[0], dtype=torch.bool)
    z11, z12, z22 = a @ a.T / t, a @ b.T / t, b @ b.T / t
    l1 = torch.logsumexp(torch.cat((z11.masked_fill(eye, float("-inf")), z12), dim=1), dim=1)
    l2 = torch.logsumexp(torch.cat((z22.masked_fill(eye, float("-inf")), z12.T), dim=1), dim=1)
    return ((l1 + l2) / 2 - z12.diag()).mean()


def close(got, want, got_grads, want_grads, floor=0.0):
    errs = [abs(float(got) - float(want)) / max(1.0, abs(float(want)))]
    for mine, ref in zip(got_grads, want_grads):
        errs.append(float((mine.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300))
    print("max errors (loss rel, grad rel to max): %.3g %.3g" % (errs[0], max(errs[1:])))
    assert errs[0] <= 1e-5, (float(got), float(want))
    for mine, ref in zip(got_grads, want_grads):
        assert float((mine.double().cpu() - ref).abs().max()) <= max(1e-4 * float(ref.abs().max()), floor), errs


def check(h1, h2, t):
    """GRACELoss(t) on the device against grace64 in fp64, value and both gradients"""
    from gigl_amd.link_prediction import GRACELoss
    h1, h2 = h1.detach().requires_grad_(True), h2.detach().requires_grad_(True)
    got, count = GRACELoss(temperature=t)(h1, h2, device=torch.device(DEV))
    assert count == 1
    got.backward()
    r1, r2 = (h.detach().double().cpu().requires_grad_(True) for h in (h1, h2))
    want = grace64(r1, r2, t)
    want.backward()
    assert torch.isfinite(got) and torch.isfinite(h1.grad).all() and torch.isfinite(h2.grad).all()
    # the reference's own rounding: its gradient is a difference of terms up to 4 / (n T |h_i|), each good to 2^-52 of
    # itself.  Where the true gradient vanishes (d = 1: a row's direction cannot change), 1e-4 of max|grad64| is 1e-4 of
    # that noise (1e-17), which only the same noise could meet; the kernels return exact zeros there
    floor = 2.0 ** -50 / (h1.shape[0] * t * max(float(min(r1.norm(dim=1).min(), r2.norm(dim=1).min())), 1e-8))
    close(got, want, (h1.grad, h2.grad), (r1.grad, r2.grad), floor)


SHAPES = [(n, d) for n in (1, 2, 3, 63, 64, 65, 129, 257) for d in (16, 30)] + \
         [(n, d) for n in (65, 129) for d in (1, 4, 36, 260)] + \
         [(65, 100), (65, 97), (65, 512)]  # a partly filled 64-column group and 32-column block of the backward; the widest rows


@gpu
@pytest.mark.parametrize("t", [0.5, 0.05])
@pytest.mark.parametrize("n,d", SHAPES)
def test_grace_against_fp64(n, d, t):
    check(*views(n, d, 1), t)


@gpu
@pytest.mark.parametrize("kind", ["view", "near", "dup", "zero"])
def test_grace_hard_inputs(kind):
    check(*views(129, 16, 3, kind), 0.5)


@gpu
def test_grace_at_the_reference_default_temperature():
    """T = 0.001, where the literal exp(sim / T) overflows and the reference's loss is NaN"""
    check(*views(129, 16, 4), 0.001)


@gpu
def test_reproducible():
    from gigl_amd.link_prediction import GRACELoss
    out = []
    for _ in range(2):
        h1, h2 = (h.requires_grad_(True) for h in views(257, 36, 5))
        loss, _ = GRACELoss(temperature=0.5)(h1, h2)
        loss.backward()
        out.append((loss.detach().cpu(), h1.grad.cpu(), h2.grad.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*out))


@gpu
def test_errors():
    from gigl_amd.link_prediction import GRACELoss
    with pytest.raises(RuntimeError, match="d=513"):
        GRACELoss(temperature=0.5)(*views(4, 513, 6))
    with pytest.raises(RuntimeError, match="CPU"):
        GRACELoss(temperature=0.5)(torch.randn(4, 8), torch.randn(4, 8))
    with pytest.raises(ValueError):
        GRACELoss(temperature=None)


class StubEncoder(torch.nn.Module):
    hid_dim, out_dim = 12, 8

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(6, self.out_dim)

    def forward(self, graph):
        return self.lin(graph.x)


@gpu
def test_grace_task():
    from gigl_amd.nablp_spec import GRACE, NodeAnchorBasedLinkPredictionTaskInputs
    from gigl_amd.nn import GraphData
    torch.manual_seed(7)
    enc = StubEncoder().to(DEV)
    task = GRACE(encoder=enc, temperature=0.5, feat_drop_1=0, edge_drop_1=0, feat_drop_2=0, edge_drop_2=0).to(DEV)
    assert all(k.startswith("head.") for k in task.state_dict())  # (the encoder is not the task's)
    graph = GraphData(x=3 * torch.randn(70, 6), edge_index=torch.randint(0, 70, (2, 200)))
    roots = torch.arange(0, 70, 2)
    ti = NodeAnchorBasedLinkPredictionTaskInputs(main_batch=SimpleNamespace(graph=graph, root_node_indices=roots),
                                                 random_neg_batch=None, batch_embeddings=None)
    got, count = task(ti, None, False, torch.device(DEV))
    assert count == 1
    got.backward()
    enc64, head64 = copy.deepcopy(enc).double().cpu(), copy.deepcopy(task.head).double().cpu()
    h = head64(enc64.lin(graph.x.double())[roots])
    want = grace64(h, h, 0.5)  # (no drop: both views are the graph itself)
    want.backward()
    mine, ref = list(task.head.parameters()) + list(enc.parameters()), list(head64.parameters()) + list(enc64.parameters())
    close(got, want, [p.grad for p in mine], [p.grad for p in ref])


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_augmented_graph():
    from gigl_amd.augmentations import get_augmented_graph
    from gigl_amd.nn import GraphData
    n = 50
    ei = torch.randint(0, n, (2, 400), generator=torch.Generator().manual_seed(8))
    graph = GraphData(x=torch.rand(n, 32) + 1, edge_index=ei)
    before = {(int(s), int(d)) for s, d in ei.t() if s != d}
    out = [get_augmented_graph(graph, 0.4, 0.4, generator=torch.Generator().manual_seed(s)) for s in (0, 0, 1)]
    for g in out:
        src, dst = g.edge_index
        kept = [(int(s), int(d)) for s, d in zip(src[src != dst], dst[src != dst])]
        assert set(kept) <= before and 0 < len(kept) < (ei[0] != ei[1]).sum()
        assert sorted(src[src == dst].tolist()) == list(range(n))  # exactly one self loop per node
        zeroed = (g.x == 0).all(dim=0)
        assert 0 < int(zeroed.sum()) < 32 and torch.equal(g.x[:, ~zeroed], graph.x[:, ~zeroed])  # whole columns only
    assert torch.equal(out[0].edge_index, out[1].edge_index) and torch.equal(out[0].x, out[1].x)
    assert not torch.equal(out[0].x, out[2].x) and out[0].edge_index.shape != out[2].edge_index.shape
    same = get_augmented_graph(graph, 0.0, 0.0)
    assert torch.equal(same.x, graph.x) and same.num_edges == len([1 for s, d in ei.t() if s != d]) + n
    for bad in ((-0.1, 0.3), (0.3, 1.1)):
        with pytest.raises(ValueError):
            get_augmented_graph(graph, *bad)


def test_spec_wiring():
    from gigl_amd.nablp_spec import GRACE, HipNodeAnchorLinkPredictionSpec
    spec = HipNodeAnchorLinkPredictionSpec(task_path="gigl_amd.nablp_spec.GRACE", softmax_temp="0.07", grace_temperature="0.5",
                                           feat_drop_1="0.1", edge_drop_1="0.2", feat_drop_2="0.4", edge_drop_2="0.0")
    (task,) = spec.tasks._task_to_fn_map.values()
    assert type(task) is GRACE and task.loss.temperature == 0.5
    assert (task.feat_drop_1, task.edge_drop_1, task.feat_drop_2, task.edge_drop_2) == (0.1, 0.2, 0.4, 0.0)
    assert spec.tasks.result_types == {"input_batch"} and spec._train_plan_task_kwargs() is None
    # init_model binds the encoder; the head is the model's `task_heads.GRACE`, and a checkpoint without it still loads
    cfg = SimpleNamespace(is_heterogeneous=False, preprocessed_metadata=SimpleNamespace(nodes=[SimpleNamespace(feature_dim=6)]))
    model = spec.init_model(cfg)
    state = model.state_dict()
    assert task._encoder_ref[0] is model.encoder and "task_heads.GRACE.2.bias" in state
    assert {id(p) for p in task.parameters()} <= {id(p) for p in model.parameters()}
    spec.init_model(cfg, state_dict={k: v for k, v in state.items() if not k.startswith("task_heads.")})
    default = HipNodeAnchorLinkPredictionSpec(task_path="gigl_amd.nablp_spec.GRACE", softmax_temp="0.07")
    assert default.tasks._task_to_fn_map["GRACE"].loss.temperature == 0.001  # (never the softmax temperature)
