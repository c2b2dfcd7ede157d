"""BGRL and TBGRL: the fused predictor head and cosine loss (csrc/bootstrap.hip), the moving average of the offline encoder and
the tasks against the reference's literal formulas (python/gigl/src/common/models/layers/loss.py:537-588 after a torch Linear ->
ReLU -> Linear) in fp64 on the CPU through torch autograd.  Row tile 64, 64-column blocks, K chunks of 32; widths that are no
multiple of 4 take the scalar loader; hid = out = 512 is the LDS ceiling.  Bars: loss within 1e-5 max(1, |want|), each gradient
within 1e-4 of that tensor's max|grad64|; on the hard inputs the larger of that and twice the error of the same formulas in torch
fp32 on the CPU; floored at the fp64 reference's own rounding (at out = 1 a cosine is a sign: the true gradient is zero, the kernels
return exact zeros and the reference 1e-17 of noise).

Measured on an MI355X: loss within 5.5e-8; gradients within 5.3e-7 of max|grad64| over the shape grid, 2.9e-7 on the hard inputs
(every fp32 bar there stayed below 1e-4).  At out = 1 the relative figure is 1 — zeros against noise — under a floor of 6 to 47."""
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["bgrl", "tbgrl"]
LAMBDA = 0.12


def inputs(n, out, hid, seed, kind="plain"):
    """[e1, e2, y1, y2, yneg, W1, b1, W2, b2] on the CPU, fp32"""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randn(n, out, generator=g) for _ in range(5)]
    head = [torch.randn(hid, out, generator=g) / math.sqrt(out), 0.1 * torch.randn(hid, generator=g),
            torch.randn(out, hid, generator=g) / math.sqrt(hid), 0.1 * torch.randn(out, generator=g)]
    if kind == "clamp":  # a target row of zeros; a row whose pre-activations are all negative with b2 = 0: q = 0
        rows[3][3] = 0
        rows[0][5] = 0
        head[1], head[3] = -head[1].abs() - 0.01, torch.zeros(out)
    elif kind == "scaled":
        rows[0][::2] *= 1e4
        rows[2][1::3] *= 1e4
    elif kind == "parallel":  # the first half of view 1's q within 1e-3 of its target's direction: cos near 1
        q1 = F.linear(F.relu(F.linear(rows[0].double(), head[0].double(), head[1].double())), head[2].double(), head[3].double())
        rows[3][:n // 2] = (2 * q1 * (1 + 1e-3 * torch.randn(n, out, generator=g)))[:n // 2].float()
    return rows + head


def formula(mode, e1, e2, y1, y2, yneg, w1, b1, w2, b2, first_term=False):
    """the reference's literal formulas in the dtype of the inputs; first_term: with |q| held constant — the first of the two
    terms of a cosine's gradient, which cancel where q is parallel to its target"""
    q1, q2 = (F.linear(F.relu(F.linear(e, w1, b1)), w2, b2) for e in (e1, e2))
    cos = F.cosine_similarity
    if first_term:
        cos = lambda q, y, dim=-1: (q * F.normalize(y, dim=-1)).sum(-1) / q.detach().norm(dim=-1).clamp_min(1e-8)
    if mode == "bgrl":
        return 2 - cos(q1, y2.detach(), dim=-1).mean() - cos(q2, y1.detach(), dim=-1).mean()
    return LAMBDA * (cos(q1, yneg.detach()).mean() + cos(q2, yneg.detach()).mean()) - (1 - LAMBDA) * (
        cos(q1, y2.detach()).mean() + cos(q2, y1.detach()).mean())


def reference(mode, ts, dtype=torch.float64, first_term=False):
    ts = [t.detach().to(dtype).cpu().requires_grad_(k not in (2, 3, 4)) for k, t in enumerate(ts)]
    want = formula(mode, *ts, first_term=first_term)
    want.backward()
    return [want.detach()] + [t.grad for k, t in enumerate(ts) if k not in (2, 3, 4)]


def run(mode, ts, wide=False):
    """-> [loss, de1, de2, dW1, db1, dW2, db2] on the CPU; wide: the rows are views of wider matrices (ld > d)"""
    from gigl_amd.engine import default_engine
    from gigl_amd.link_prediction import _FusedBootstrapHead
    ts = [t.to(DEV) for t in ts]
    if wide:
        ts[:5] = [torch.cat((t, torch.ones(t.shape[0], 4 + k, device=DEV)), dim=1)[:, :t.shape[1]] for k, t in enumerate(ts[:5])]
    ts = [t.detach().requires_grad_(k not in (2, 3, 4)) for k, t in enumerate(ts)]
    rows = ts[:4] + [ts[4] if mode == "tbgrl" else None]
    got = _FusedBootstrapHead.apply(*rows, *ts[5:], default_engine(torch.device(DEV)), LAMBDA)
    got.backward()
    return [got.detach().cpu()] + [t.grad.cpu() for k, t in enumerate(ts) if k not in (2, 3, 4)]


def check(mode, ts, hard=False, wide=False):
    got, want = run(mode, ts, wide), reference(mode, ts)
    fp32 = reference(mode, ts, torch.float32) if hard else want
    # the reference's own rounding: 2^-50 of the terms it subtracts (at out = 1 they cancel exactly: the true gradient is zero)
    floors = [2.0 ** -50 * float(t.abs().max()) for t in reference(mode, ts, first_term=True)]
    errs = [abs(float(got[0]) - float(want[0])) / max(1.0, abs(float(want[0])))]
    bars = [max(1e-5, 2 * abs(float(fp32[0]) - float(want[0])) / max(1.0, abs(float(want[0]))))]
    for mine, ref, ref32, floor in zip(got[1:], want[1:], fp32[1:], floors[1:]):
        assert mine.shape == ref.shape and torch.isfinite(mine).all()
        top = max(float(ref.abs().max()), 1e-300)
        errs.append(float((mine.double() - ref).abs().max()) / top)
        bars.append(max(1e-4, 2 * float((ref32.double() - ref).abs().max()) / top, floor / top))
    print("errors (loss rel; e1 e2 W1 b1 W2 b2 rel to max): " + " ".join("%.3g" % e for e in errs) + "; bars " +
          " ".join("%.3g" % b for b in bars))
    assert torch.isfinite(got[0]) and all(e <= b for e, b in zip(errs, bars)), (errs, bars)


SHAPES = [(n, o, h) for n in (1, 2, 63, 64, 65, 129) for o, h in ((16, 16), (30, 12))] + \
         [(n, o, h) for n in (65, 129) for o, h in ((1, 4), (36, 65), (65, 36), (100, 260))] + [(65, 512, 512), (64 * 3 + 37, 30, 100)]


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,out,hid", SHAPES)
def test_against_fp64(mode, n, out, hid):
    check(mode, inputs(n, out, hid, 1))


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["view", "clamp", "scaled", "parallel"])
def test_hard_inputs(mode, kind):
    check(mode, inputs(129, 16, 12, 3, kind), hard=True, wide=kind == "view")


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_reproducible(mode):
    out = [run(mode, inputs(64 * 3 + 37, 36, 65, 5)) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*out))


@gpu
@pytest.mark.parametrize("mm", [0.0, 0.99, 1.0])
def test_ema(mm):
    from gigl_amd.engine import default_engine
    g = torch.Generator().manual_seed(6)
    dst, src = ([torch.randn(k, generator=g).to(DEV) for k in (1, 3, 64, 1000, 4097)] for _ in range(2))
    before = [t.clone() for t in dst]
    default_engine(torch.device(DEV)).ema_update(dst, src, mm)
    for d, b, s in zip(dst, before, src):
        want = mm * b.double() + (1 - mm) * s.double()
        # mm and 1 - mm are rounded to fp32 (2^-24 each), as are the two products and the sum: within 4 x 2^-24 of |b| + |s|
        assert torch.equal(d, b) if mm == 1.0 else ((d.double() - want).abs() <= 2.0 ** -22 * (b.abs() + s.abs()).double()).all()


@gpu
def test_errors():
    from gigl_amd.link_prediction import BGRLLoss, TBGRLLoss
    rows = lambda n, d, k: [torch.randn(n, d, device=DEV) for _ in range(k)]
    for mod, k in ((BGRLLoss(), 4), (TBGRLLoss(), 5)):
        with pytest.raises(RuntimeError, match="out=513"):
            mod(*rows(4, 513, k))
        with pytest.raises(RuntimeError, match="CPU"):
            mod(*[t.cpu() for t in rows(4, 8, k)])
        with pytest.raises(ValueError, match="different shapes"):
            mod(torch.randn(4, 8, device=DEV), *rows(5, 8, k - 1))
    # (the modules on already-projected rows: the kernels' path without the head)
    ts = [t.cpu() for t in rows(70, 9, 5)]
    q1, q2 = (t.to(DEV).requires_grad_(True) for t in ts[:2])
    got, count = TBGRLLoss(LAMBDA)(q1, q2, *(t.to(DEV) for t in ts[2:]))
    got.backward()
    r1, r2 = (t.double().requires_grad_(True) for t in ts[:2])
    cos = lambda a, b: F.cosine_similarity(a, b.double()).mean()
    want = LAMBDA * (cos(r1, ts[4]) + cos(r2, ts[4])) - (1 - LAMBDA) * (cos(r1, ts[3]) + cos(r2, ts[2]))
    want.backward()
    assert count == 1 and abs(float(got.detach()) - float(want.detach())) <= 1e-5
    for mine, ref in ((q1.grad, r1.grad), (q2.grad, r2.grad)):
        assert (mine.cpu().double() - ref).abs().max() <= 1e-4 * ref.abs().max()


class StubEncoder(torch.nn.Module):
    hid_dim, out_dim = 12, 8

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(6, self.out_dim)

    def forward(self, graph):
        return self.lin(graph.x)


@gpu
@pytest.mark.parametrize("name", ["BGRL", "TBGRL"])
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
        offline = [p.detach().clone() for p in task.offline_encoder.parameters()]
        enc.zero_grad()
        got, count = task(ti, None, False, torch.device(DEV))
        got.backward()
        assert count == 1 and torch.isfinite(got)
        for p in list(enc.parameters()) + list(task.head.parameters()):
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
        for p, before in zip(task.offline_encoder.parameters(), offline):
            assert p.grad is None and not p.requires_grad and torch.equal(p, before)
        losses.append(float(got.detach()))
    assert losses[0] == losses[1]
    with torch.no_grad():
        for p in enc.parameters():
            p.add_(1.0)
    task.update_offline_encoder(0.5)
    for p, before, online in zip(task.offline_encoder.parameters(), offline, enc.parameters()):
        want = 0.5 * before.double() + 0.5 * online.detach().double()
        assert (p.double() - want).abs().max() <= 2.0 ** -22 * (before.abs() + online.abs()).max()


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_spec_wiring():
    from gigl_amd.nablp_spec import BGRL, TBGRL, HipNodeAnchorLinkPredictionSpec
    cfg = SimpleNamespace(is_heterogeneous=False, preprocessed_metadata=SimpleNamespace(nodes=[SimpleNamespace(feature_dim=6)]))
    for cls in (BGRL, TBGRL):
        spec = HipNodeAnchorLinkPredictionSpec(task_path=f"gigl_amd.nablp_spec.{cls.__name__}", neg_lambda="0.3", feat_drop_2="0.2",
                                               edge_drop_neg="0.9", offline_momentum="0.9", augment_seed="3")
        (task,) = spec.tasks._task_to_fn_map.values()
        assert type(task) is cls and task.neg_lambda == (0.3 if cls is TBGRL else 0.0) and spec.offline_momentum == 0.9
        assert (task.feat_drop_1, task.edge_drop_1, task.feat_drop_2, task.edge_drop_2) == (0.8, 0.8, 0.2, 0.8)
        assert task._neg_drops == ((0.9, 0.95) if cls is TBGRL else None)
        assert task._generator.initial_seed() == 3 and spec.tasks.result_types == {"input_batch"}
        state = spec.init_model(cfg).state_dict()
        prefix = f"task_heads.{cls.__name__}."
        assert task._encoder_ref[0] is spec.model.encoder and not any(p.requires_grad for p in task.offline_encoder.parameters())
        online = [k for k in state if k.startswith("_encoder.")]  # (the model's name for its encoder)
        assert online and sorted(k for k in state if k not in online) == sorted(
            [prefix + "offline" + k for k in online] + [prefix + f"head.{l}.{w}" for l in (0, 2) for w in ("weight", "bias")])
        with pytest.raises(NotImplementedError, match="homogeneous"):
            spec.init_model(SimpleNamespace(is_heterogeneous=True))
    assert HipNodeAnchorLinkPredictionSpec(task_path="gigl_amd.nablp_spec.TBGRL").offline_momentum == 0.99


def test_graph_perm():
    from gigl_amd.augmentations import get_augmented_graph
    from gigl_amd.nn import GraphData
    n = 50
    graph = GraphData(x=torch.arange(3.0 * n).view(n, 3), edge_index=torch.randint(0, n, (2, 400)))
    views = [get_augmented_graph(graph, edge_drop_ratio=0.5, feat_drop_ratio=0.0, graph_perm=True,
                                 generator=torch.Generator().manual_seed(2)) for _ in range(2)]
    x, ei = views[0].x, views[0].edge_index
    assert torch.equal(x, views[1].x) and torch.equal(ei, views[1].edge_index)
    assert not torch.equal(x, graph.x) and torch.equal(x[x[:, 0].argsort()], graph.x)
    loops = ei[0] == ei[1]
    assert int(ei.min()) >= 0 and int(ei.max()) < n and torch.equal(ei[0, loops].sort().values, torch.arange(n))
    assert 100 < int((~loops).sum()) < 300  # (400 redrawn edges, half of them dropped)
