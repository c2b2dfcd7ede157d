"""GBT and WhiteningDecorrelation: the fused d x d correlation losses (csrc/correlate.hip) and their tasks against an fp64
restatement of the reference (python/gigl/src/common/models/layers/loss.py:444-534, task.py:351-480) through torch autograd.
Output tile 64 x 64, K step 32 rows, split-K chunks of at least CORRELATE_MIN_CHUNK_ROWS rows, statistics chunks of 256 rows,
backward column chunk 128.  Bars: loss within 1e-5 max(1, |want|), gradient within 1e-4 of max|grad64|; on the hard inputs the
larger of that and twice the error of the same formulas in torch fp32 on the CPU; floored at the fp64 reference's own rounding.

Measured on an MI355X: loss within 4.7e-7; gradients within 3.7e-6 of max|grad64| over the shape grid and the multi-chunk shapes,
1.9e-6 on the hard inputs and the constant column.  At n = 2 the true gradient is identically zero (a standardised column of
two rows is +-1 / sqrt 2): the kernels return exact zeros and the fp64 reference 1e-15 of rounding noise, under the floor."""
import math
from types import SimpleNamespace

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"
LOSSES = ["gbt", "wd"]


def views(n, d, seed, kind="plain"):
    """two views' rows on the device: randn * 3, the second the first plus randn noise"""
    g = torch.Generator().manual_seed(seed)
    h1 = 3 * torch.randn(n, d, generator=g)
    h2 = h1 + (1e-3 if kind == "near" else 1.0) * torch.randn(n, d, generator=g)
    if kind == "dup":
        h1, h2 = (h[:(n + 1) // 2].repeat_interleave(2, dim=0)[:n] for h in (h1, h2))
    elif kind == "offset":  # 30 standard deviations
        h1[:, 1] += 90
        h2[:, 1] += 90
    elif kind == "const":
        h1[:, 2] = 5.0
    if kind == "view":  # rows of a wider matrix: ld > d
        return tuple(torch.cat((h, torch.randn(n, 7, generator=g)), dim=1).to(DEV)[:, :d] for h in (h1, h2))
    return h1.to(DEV), h2.to(DEV)


def formula(loss, h1, h2, lambd):
    """the reference's literal formulas in the dtype of h1"""
    n, d = h1.shape
    eye = torch.eye(d, dtype=h1.dtype)
    if loss == "gbt":
        za, zb = ((h - h.mean(0)) / (h.std(0) + 1e-15) for h in (h1, h2))
        c = za.T @ zb / n
        return (1 - c.diagonal()).pow(2).sum() + c[~eye.bool()].pow(2).sum() / d
    z1, z2 = ((h - h.mean(0)) / h.std(0) for h in (h1, h2))
    norm = torch.linalg.matrix_norm
    return norm((z1 - z2) / n) + lambd * (norm(eye - z1.T @ z1 / n) + norm(eye - z2.T @ z2 / n))


def run(loss, h1, h2, lambd):
    from gigl_amd.link_prediction import GBTLoss, WhiteningDecorrelationLoss
    h1, h2 = h1.detach().requires_grad_(True), h2.detach().requires_grad_(True)
    if loss == "gbt":
        got, count = GBTLoss()(h1, h2, torch.device(DEV))
    else:
        got, count = WhiteningDecorrelationLoss(lambd=lambd)(h1, h2, h1.shape[0], torch.device(DEV))
    assert count == 1
    got.backward()
    return got.detach().cpu(), h1.grad.cpu(), h2.grad.cpu()


def reference(loss, h1, h2, lambd, dtype=torch.float64):
    r1, r2 = (h.detach().to(dtype).cpu().requires_grad_(True) for h in (h1, h2))
    want = formula(loss, r1, r2, lambd)
    want.backward()
    return want.detach(), r1.grad, r2.grad


def check(loss, h1, h2, lambd=1e-3, hard=False, skip_col=None):
    got, want = run(loss, h1, h2, lambd), reference(loss, h1, h2, lambd)
    n, d = h1.shape
    # the reference's own rounding: a gradient element is a sum of about d terms, each at most 4 |z| / (n s) with |z| <=
    # sqrt(n), good to 2^-52 of itself
    floor = 2.0 ** -50 * d * 4 * math.sqrt(n) / (n * max(float(h1.double().std(0).min()), 1e-8))
    fp32 = reference(loss, h1, h2, lambd, torch.float32) if hard else want
    errs = [abs(float(got[0]) - float(want[0])) / max(1.0, abs(float(want[0])))]
    bars = [max(1e-5, 2 * abs(float(fp32[0]) - float(want[0])) / max(1.0, abs(float(want[0]))))]
    for mine, ref, ref32 in zip(got[1:], want[1:], fp32[1:]):
        assert torch.isfinite(mine).all()
        if skip_col is not None:  # (a constant column: the reference's own gradient is NaN there)
            keep = [c for c in range(d) if c != skip_col]
            mine, ref, ref32 = mine[:, keep], ref[:, keep], ref32[:, keep]
        top = float(ref.abs().max())
        errs.append(float((mine.double() - ref).abs().max()) / max(top, 1e-300))
        bars.append(max(1e-4, 2 * float((ref32.double() - ref).abs().max()) / max(top, 1e-300), floor / max(top, 1e-300)))
    print("errors (loss rel, grads rel to max): %.3g %.3g %.3g; bars %.3g %.3g %.3g" % (*errs, *bars))
    assert torch.isfinite(got[0]) and all(e <= b for e, b in zip(errs, bars)), (errs, bars)
    return got


def multi_chunk_rows():
    """two n whose split has >= 2 chunks and a ragged last one, from the kernel's shortest chunk"""
    from gigl_amd.engine import CORRELATE_MIN_CHUNK_ROWS as rows
    return [2 * rows + 37, 4 * rows + 45]


SHAPES = [(n, d) for n in (2, 3, 63, 64, 65, 129) for d in (16, 30)] + \
         [(n, d) for n in (65, 129) for d in (1, 4, 36, 65, 100, 260)] + [(65, 512)] + \
         [(n, d) for n in multi_chunk_rows() for d in (30, 100)]


@gpu
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_against_fp64(loss, n, d):
    check(loss, *views(n, d, 1))


@gpu
@pytest.mark.parametrize("n", multi_chunk_rows())
def test_split_is_ragged(n):
    from gigl_amd.engine import default_engine
    for d, products in ((30, 1), (30, 2), (100, 1), (100, 2)):
        rows = default_engine(torch.device(DEV)).correlate_chunk_rows(n, d, products)
        assert rows % 32 == 0 and rows >= 64 and -(-n // rows) >= 2 and n % rows != 0


@gpu
@pytest.mark.parametrize("loss,kind,lambd", [(loss, kind, 1e-3) for loss in LOSSES for kind in ("view", "near", "dup", "offset")] +
                         [("wd", "plain", 1.0)])
def test_hard_inputs(loss, kind, lambd):
    check(loss, *views(129, 16, 3, kind), lambd=lambd, hard=True)


@gpu
def test_gbt_constant_column():
    """z = 0 as in the reference's forward; its autograd gradient is NaN in that column, ours exactly zero"""
    h1, h2 = views(129, 16, 4, "const")
    _, g1, g2 = check("gbt", h1, h2, skip_col=2)
    assert not g1[:, 2].any() and torch.isfinite(g2).all()


@gpu
@pytest.mark.parametrize("loss", LOSSES)
def test_reproducible(loss):
    n = multi_chunk_rows()[1]
    out = [run(loss, *views(n, 36, 5), 1e-3) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*out))


@gpu
def test_errors():
    from gigl_amd.link_prediction import GBTLoss, WhiteningDecorrelationLoss
    for mod, extra in ((GBTLoss(), ()), (WhiteningDecorrelationLoss(), (4,))):
        with pytest.raises(RuntimeError, match="d=513"):
            mod(*views(4, 513, 6), *extra)
        with pytest.raises(RuntimeError, match="CPU"):
            mod(torch.randn(4, 8), torch.randn(4, 8), *extra)
    with pytest.raises(RuntimeError, match="n=1"):
        GBTLoss()(*views(1, 8, 6))
    with pytest.raises(RuntimeError, match="n=1"):
        WhiteningDecorrelationLoss()(*views(1, 8, 6), 1)
    with pytest.raises(ValueError, match="N=5"):
        WhiteningDecorrelationLoss()(*views(4, 8, 6), 5)


class StubEncoder(torch.nn.Module):
    hid_dim, out_dim = 12, 8

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(6, self.out_dim)

    def forward(self, graph):
        return self.lin(graph.x)


@gpu
@pytest.mark.parametrize("name", ["GBT", "WhiteningDecorrelation"])
def test_task(name):
    import gigl_amd.nablp_spec as spec
    from gigl_amd.nn import GraphData
    torch.manual_seed(7)
    enc = StubEncoder().to(DEV)
    graph = GraphData(x=3 * torch.randn(70, 6), edge_index=torch.randint(0, 70, (2, 200)))
    ti = spec.NodeAnchorBasedLinkPredictionTaskInputs(
        main_batch=SimpleNamespace(graph=graph, root_node_indices=torch.arange(0, 70, 2)), random_neg_batch=None,
        batch_embeddings=None)
    losses = []
    for _ in range(2):
        torch.manual_seed(8)  # (the same head)
        task = getattr(spec, name)(encoder=enc, seed=11).to(DEV)
        assert (task.head is None) == (name == "GBT") and all(k.startswith("head.") for k in task.state_dict())
        enc.zero_grad()
        got, count = task(ti, None, False, torch.device(DEV))
        got.backward()
        assert count == 1 and torch.isfinite(got)
        for p in list(enc.parameters()) + list(task.parameters()):
            assert p.grad is not None and torch.isfinite(p.grad).all()
        # (the biases' gradients vanish: the standardisation removes a column's mean)
        assert enc.lin.weight.grad.abs().max() > 0 and (task.head is None or task.head[0].weight.grad.abs().max() > 0)
        losses.append(float(got))
    assert losses[0] == losses[1]


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_spec_wiring():
    from gigl_amd.nablp_spec import GBT, HipNodeAnchorLinkPredictionSpec, WhiteningDecorrelation
    cfg = SimpleNamespace(is_heterogeneous=False, preprocessed_metadata=SimpleNamespace(nodes=[SimpleNamespace(feature_dim=6)]))
    for cls, key in ((GBT, None), (WhiteningDecorrelation, "task_heads.WhiteningDecorrelation.2.bias")):
        spec = HipNodeAnchorLinkPredictionSpec(task_path=f"gigl_amd.nablp_spec.{cls.__name__}", wd_lambd="0.5", feat_drop_1="0.1",
                                               edge_drop_2="0.0", augment_seed="3")
        (task,) = spec.tasks._task_to_fn_map.values()
        assert type(task) is cls and getattr(task.loss, "lambd", 0.5) == 0.5
        assert (task.feat_drop_1, task.edge_drop_1, task.feat_drop_2, task.edge_drop_2) == (0.1, 0.2, 0.2, 0.0)
        assert task._generator.initial_seed() == 3 and spec.tasks.result_types == {"input_batch"}
        state = spec.init_model(cfg).state_dict()
        assert task._encoder_ref[0] is spec.model.encoder
        assert [k for k in state if k.startswith("task_heads.")] == [] if key is None else key in state
        with pytest.raises(NotImplementedError, match="homogeneous"):
            spec.init_model(SimpleNamespace(is_heterogeneous=True))
    assert HipNodeAnchorLinkPredictionSpec(task_path="gigl_amd.nablp_spec.WhiteningDecorrelation").tasks._task_to_fn_map[
        "WhiteningDecorrelation"].loss.lambd == 1e-3
