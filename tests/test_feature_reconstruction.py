"""FeatureReconstruction: the fused root-row decoder and scaled-cosine-error loss (csrc/reconstruct.hip) and the task against the
reference's LITERAL formulation (python/gigl/src/common/models/layers/task.py:282-348, loss.py:419-441) in fp64 on the CPU through
torch autograd: a Linear over all N rows, the roots' rows zeroed, GraphConv (index_add over the edge list, lin_rel + lin_root) over
all N rows, the roots selected, both sides normalised, (1 - <x, y>)^alpha averaged — not the collapsed form the kernels compute.
Row tile 64, 64-column blocks, K chunks of 32; widths that are no multiple of 4 take the scalar loader; out = 512 is the LDS
ceiling.  Bars (tests/test_bootstrap.py's, the same three-plane products): loss within 1e-5 max(1, |want|), each gradient within
1e-4 of that tensor's max|grad64|; on the hard inputs the larger of that and twice the error of the same formulas in torch fp32
on the CPU.

Measured on an MI355X: loss within 2.3e-7; gradients within 5.9e-7 of max|grad64| over the shape grid, 4.1e-7 on the hard inputs
(every fp32 bar there stayed below 1e-4)."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["E", "X", "W_ed", "W_rel", "b_rel", "W_root"]
GRADS = ["E", "W_ed", "W_rel", "b_rel", "W_root"]


def formula(t, alpha):
    """the literal reference over a dict of tensors (E, X, W_ed, W_rel, b_rel, W_root, ei, roots) in their dtype"""
    ei, roots = t["ei"], t["roots"]
    h = (t["E"] @ t["W_ed"].T).index_fill(0, roots, 0.0)
    agg = torch.zeros_like(h).index_add(0, ei[1], h[ei[0]])
    y = (agg @ t["W_rel"].T + t["b_rel"] + h @ t["W_root"].T)[roots]
    return (1 - (F.normalize(t["X"][roots], dim=-1) * F.normalize(y, dim=-1)).sum(-1)).pow(alpha).mean()


def inputs(b, out, d_in, seed, kind="plain"):
    """E [N, out], X [N, in], the decoder, ei [2, edges] (about 4 in-edges a node and a self loop each), roots [b] unsorted"""
    g = torch.Generator().manual_seed(seed)
    n = 3 * b + 5
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    t = dict(E=rnd(n, out), X=rnd(n, d_in), W_ed=rnd(out, out) / out ** 0.5, W_rel=rnd(d_in, out) / out ** 0.5,
             b_rel=0.1 * rnd(d_in), W_root=rnd(d_in, out) / out ** 0.5)
    ei = torch.cat((torch.randint(0, n, (2, 4 * n), generator=g), torch.arange(n).expand(2, n)), dim=1)
    roots = torch.randperm(n, generator=g)[:b]
    if kind == "dup":
        roots[1] = roots[0]
    elif kind in ("isolated", "zero_pred"):  # roots[0]: only its self loop; roots[1]: every neighbour a root
        ei = ei[:, (ei[1] != roots[0]) | (ei[0] == roots[0])]
        to_r1 = (ei[1] == roots[1]) & (ei[0] != roots[1])
        ei[0, to_r1] = roots[2 + torch.arange(int(to_r1.sum())) % (b - 2)]
        if kind == "zero_pred":
            t["b_rel"] = torch.zeros(d_in)
    elif kind == "zero_target":
        t["X"][roots[3]] = 0
    elif kind == "scaled":
        t["E"][::3] *= 1e4
    t.update(ei=ei, roots=roots)
    if kind == "parallel":  # half the rows' predictions within 1e-3 of their target's direction (p does not depend on X)
        d = {k: v.double() if v.is_floating_point() else v for k, v in t.items()}
        h = (d["E"] @ d["W_ed"].T).index_fill(0, roots, 0.0)
        p = (torch.zeros_like(h).index_add(0, ei[1], h[ei[0]]) @ d["W_rel"].T + d["b_rel"])[roots]
        t["X"][roots[:b // 2]] = (2 * p * (1 + 1e-3 * rnd(b, d_in)))[:b // 2].float()
    return t


def reference(t, alpha, dtype=torch.float64):
    t = {k: v.to(dtype).requires_grad_(k in GRADS) if k in NAMES else v for k, v in t.items()}
    want = formula(t, alpha)
    want.backward()
    return [want.detach()] + [t[k].grad for k in GRADS]


def run(t, alpha, wide=False):
    """-> [loss, dE, dW_ed, dW_rel, db_rel] on the CPU; wide: E and X are column slices of wider matrices (ld > d)"""
    from gigl_amd.link_prediction import feature_reconstruction_loss
    from gigl_amd.nn import GraphData
    d = {k: v.to(DEV) for k, v in t.items()}
    if wide:
        for k, pad in (("E", 4), ("X", 5)):
            d[k] = torch.cat((d[k], torch.ones(d[k].shape[0], pad, device=DEV)), dim=1)[:, :d[k].shape[1]]
    d = {k: v.detach().requires_grad_(k in GRADS[:4]) if k in NAMES else v for k, v in d.items()}
    graph = GraphData(x=d["X"], edge_index=d["ei"])
    graph._build_csr()
    got = feature_reconstruction_loss(d["E"], d["X"], graph, d["roots"], d["W_ed"], d["W_rel"], d["b_rel"], alpha)
    got.backward()
    return [got.detach().cpu()] + [d[k].grad.cpu() for k in GRADS[:4]]


def check(t, alpha=3.0, hard=False, wide=False):
    got, want = run(t, alpha, wide), reference(t, alpha)
    fp32 = reference(t, alpha, torch.float32) if hard else want
    scale = max(1.0, abs(float(want[0])))
    errs, bars = [abs(float(got[0]) - float(want[0])) / scale], [max(1e-5, 2 * abs(float(fp32[0]) - float(want[0])) / scale)]
    for mine, ref, ref32 in zip(got[1:], want[1:5], fp32[1:5]):
        assert mine.shape == ref.shape and torch.isfinite(mine).all()
        top = max(float(ref.abs().max()), 1e-300)
        errs.append(float((mine.double() - ref).abs().max()) / top)
        bars.append(max(1e-4, 2 * float((ref32.double() - ref).abs().max()) / top))
    print("errors (loss rel; E W_ed W_rel b_rel rel to max): " + " ".join("%.3g" % e for e in errs) + "; bars " +
          " ".join("%.3g" % b for b in bars))
    assert torch.isfinite(got[0]) and all(e <= b for e, b in zip(errs, bars)), (errs, bars)
    # the collapse to root rows: lin_root gets nothing, dE only reaches non-roots that some root lists
    ei, roots = t["ei"], t["roots"]
    listed = torch.zeros(t["E"].shape[0], dtype=torch.bool)
    listed[ei[0][torch.isin(ei[1], roots)]] = True
    listed[roots] = False
    assert not want[5].any() and not got[1][roots].any() and not got[1][~listed].any()
    return got


SHAPES = [(b, o, i, 3.0) for b in (1, 2, 63, 64, 65, 129) for o, i in ((16, 16), (30, 12))] + \
         [(b, o, i, 3.0) for b in (65, 129) for o, i in ((36, 65), (65, 36), (100, 260), (12, 1433))] + \
         [(65, 512, 512, 3.0), (65, 16, 16, 1.5), (129, 30, 12, 1.5)]


@gpu
@pytest.mark.parametrize("b,out,d_in,alpha", SHAPES)
def test_against_fp64(b, out, d_in, alpha):
    check(inputs(b, out, d_in, 1), alpha)


@gpu
@pytest.mark.parametrize("kind", ["dup", "isolated", "zero_pred", "zero_target", "parallel", "scaled", "view"])
def test_hard_inputs(kind):
    check(inputs(129, 16, 12, 3, kind), hard=True, wide=kind == "view")


@gpu
def test_in_dim_one():
    t = inputs(65, 16, 1, 4)
    got, want = run(t, 3.0), reference(t, 3.0)
    assert abs(float(got[0]) - float(want[0])) <= 1e-5 * max(1.0, abs(float(want[0])))
    assert all(not g.any() for g in got[1:])  # (a cosine of one column is a sign: the true gradient is zero)


@gpu
def test_loss_module():
    """FeatureReconstructionLoss on already-decoded rows: the kernels' path without the gather and the products"""
    from gigl_amd.link_prediction import FeatureReconstructionLoss
    torch.manual_seed(2)
    x, y = torch.randn(70, 9), torch.randn(70, 9)
    mine = y.to(DEV).requires_grad_(True)
    got, count = FeatureReconstructionLoss(alpha=2.5)(x_target=x.to(DEV), x_pred=mine)
    got.backward()
    ref = y.double().requires_grad_(True)
    want = (1 - (F.normalize(x.double(), dim=-1) * F.normalize(ref, dim=-1)).sum(-1)).pow(2.5).mean()
    want.backward()
    assert count == 1 and abs(float(got.detach()) - float(want.detach())) <= 1e-5 * max(1.0, abs(float(want.detach())))
    assert (mine.grad.cpu().double() - ref.grad).abs().max() <= 1e-4 * ref.grad.abs().max()


@gpu
def test_reproducible():
    t = inputs(64 * 3 + 37, 36, 65, 5)
    assert all(torch.equal(a, b) for a, b in zip(run(t, 3.0), run(t, 3.0)))


@gpu
def test_task():
    import gigl_amd.nablp_spec as spec
    from gigl_amd.augmentations import get_augmented_graph
    from gigl_amd.engine import default_engine
    from gigl_amd.models import GraphSAGE
    from gigl_amd.nn import GraphData
    torch.manual_seed(7)
    n, b, d_in, seed = 40, 7, 12, 11
    enc = GraphSAGE(in_dim=d_in, hid_dim=16, out_dim=16, num_layers=2).to(DEV)
    enc.engine = default_engine(torch.device(DEV))
    graph = GraphData(x=torch.randn(n, d_in), edge_index=torch.randint(0, n, (2, 150)))
    roots = torch.randperm(n)[:b]
    task = spec.FeatureReconstruction(encoder=enc, edge_drop=0.3, seed=seed).to(DEV)
    with torch.no_grad():
        task.reconstruction_mask.copy_(0.3 * torch.randn(1, d_in))
    ti = spec.NodeAnchorBasedLinkPredictionTaskInputs(main_batch=SimpleNamespace(graph=graph, root_node_indices=roots),
                                                      random_neg_batch=None, batch_embeddings=None)
    got, count = task(ti, None, False, torch.device(DEV))
    got.backward()
    # the same augmented graph and masked input through the task's own encoder as fp64 torch ops
    ei = get_augmented_graph(graph.to(DEV), edge_drop_ratio=0.3, feat_drop_ratio=0.0,
                             generator=torch.Generator().manual_seed(seed)).edge_index.cpu()
    dec = task.reconstruction_decoder
    params = [task.reconstruction_mask, task.reconstruction_enc_dec.weight, dec.lin_rel.weight, dec.lin_rel.bias]
    mask, w_ed, w_rel, b_rel = leaves = [p.detach().double().cpu().requires_grad_(True) for p in params]
    h = graph.x.double().index_copy(0, roots, mask.expand(b, -1))
    for l, conv in enumerate(enc.conv_layers):
        mean = torch.zeros_like(h).index_add(0, ei[1], h[ei[0]]) / torch.bincount(ei[1], minlength=n)[:, None]
        w_l, b_l, w_r = (p.detach().double().cpu() for p in (conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight))
        h = mean @ w_l.T + b_l + h @ w_r.T
        h = torch.relu(h) if l == 0 else h
    want = formula(dict(E=h, X=graph.x.double(), W_ed=w_ed, W_rel=w_rel, b_rel=b_rel, W_root=dec.lin_root.weight.detach().double().cpu(),
                        ei=ei, roots=roots), 3.0)
    want.backward()
    assert count == 1 and abs(float(got.detach()) - float(want.detach())) <= 1e-5 * max(1.0, abs(float(want.detach())))
    for p, ref in zip(params, leaves):
        assert (p.grad.cpu().double() - ref.grad).abs().max() <= 1e-4 * ref.grad.abs().max()
    assert dec.lin_root.weight.grad is None
    # the spec: the task whole under task_heads, the reference's five keys; heterogeneous configs refused
    s = spec.HipNodeAnchorLinkPredictionSpec(task_path="gigl_amd.nablp_spec.FeatureReconstruction", fr_alpha="2.0", edge_drop="0.1",
                                             augment_seed="3")
    (built,) = s.tasks._task_to_fn_map.values()
    assert (built.alpha, built.edge_drop, built._generator.initial_seed()) == (2.0, 0.1, 3)
    cfg = SimpleNamespace(is_heterogeneous=False, preprocessed_metadata=SimpleNamespace(nodes=[SimpleNamespace(feature_dim=d_in)]))
    keys = [k for k in s.init_model(cfg).state_dict() if k.startswith("task_heads.")]
    assert sorted(keys) == sorted("task_heads.FeatureReconstruction." + k for k in (
        "reconstruction_mask", "reconstruction_enc_dec.weight", "reconstruction_decoder.lin_rel.weight",
        "reconstruction_decoder.lin_rel.bias", "reconstruction_decoder.lin_root.weight"))
    with pytest.raises(NotImplementedError):
        s.init_model(SimpleNamespace(is_heterogeneous=True))
    with pytest.raises(NotImplementedError):
        task(ti, SimpleNamespace(is_heterogeneous=True), False, torch.device(DEV))
