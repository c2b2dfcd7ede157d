"""The Margin and Softmax tasks inside the link-prediction training plans (gigl_nablp_train_plan_set_task; csrc/pipeline.hip
calls csrc/loss.hip's launchers over the head's score matrix): training steps against the autograd step at equal weights,
evaluation, Retrieval at weight 1 bit for bit against the plan as it was, grow(), the setter's refusals, a batch that
overflows the workspace.

Graph and batches: tests/lp_task_cases.py (the 390-node graph of test_gpu_lp_hard_negatives.py, 100 features, fan-out
[10, 5]; batches built on the host so that the CPU restatement runs over the same ones).

Margin's kink.  The plan's kernel counts a pair with m - pos + neg == 0 as active (clamp_min, as the reference's
margin_ranking_loss differentiates), torch.relu in the autograd step here does not, and two fp32 score computations differ
in the last bits: a pair within 1e-4 of the kink could land on either side.  The tests assert, from the reference side's
scores of every step, that there is NO such pair.  Seeds chosen with the CPU restatement (lp_task_cases.cpu_margin_kink,
three steps): GraphSAGE dims (100, 32, 16), b = 6: batch seed 5, model seed 4 -> 226 pairs, closest 3.2e-2;
dims (100, 32, 70), b = 48: batch seed 5, model seed 4 -> 4755 pairs, closest 2.0e-2; GAT (4 heads of 8 -> 16), b = 24:
batch seed 9, model seed 6 -> 1225 pairs, closest 2.6e-1."""
import numpy as np
import pytest
import torch

from helpers import assert_adam_state, torch_adam_moments
from lp_task_cases import FAN, MARGIN, N, SOFTMAX_T, graph_and_features, host_batches, task_loss_torch

pytestmark = pytest.mark.gpu

PARAM = {"Margin": MARGIN, "Softmax": SOFTMAX_T}
WEIGHT = 0.75


def _engine():
    from gigl_amd.engine import HipEngine
    rowptr, col, x = graph_and_features()
    eng = HipEngine(0)
    eng.load_csc(rowptr, col)
    eng.load_features(x)
    dst = np.repeat(np.arange(N, dtype=np.uint32), np.diff(rowptr).astype(np.int64))
    eng.build_from_coo(N, dst, col.astype(np.uint32), is_directed=True, out_graph=True)
    return eng, rowptr, col


@pytest.fixture(scope="module")
def setup():
    eng, rowptr, col = _engine()
    yield eng, rowptr, col
    eng.close()


def _dev(batches, dev):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else a).to(dev)
    return [(up(r), up(c), up(rn)) for r, c, rn in batches]


def _plan_steps(eng, plan, batches, prefetch=False, grads_after_first=None):
    """the batches through plan.step on a stream of its own -> [loss], [rows]; grads_after_first: called once after step 0"""
    st = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    first = None
    try:
        got = []
        with torch.cuda.stream(st):
            for i, (roots, cnt, rn) in enumerate(batches):
                nxt = (batches[i + 1][0], batches[i + 1][2]) if prefetch and i + 1 < len(batches) else None
                got.append(plan.step(roots, cnt, rn, next_roots=nxt).clone())
                if i == 0 and grads_after_first is not None:
                    first = grads_after_first()
        eng.synchronize()
    finally:
        eng.bind_stream(torch.cuda.current_stream(eng.device))
    return [float(v[0]) for v in got], [float(v[1]) for v in got], first


def _assert_no_pair_at_the_kink(hs):
    h = torch.cat(hs)
    close = int((h.abs() < 1e-4).sum())
    print(f"Margin: {h.numel()} pairs over the steps, closest to the kink {float(h.abs().min()):.2e}, within 1e-4: {close}")
    assert close == 0


@pytest.mark.parametrize("kind", ["Margin", "Softmax"])
@pytest.mark.parametrize("dims,b,P,H,n_rn,prefetch", [((100, 32, 16), 6, 2, 3, 5, False), ((100, 32, 70), 48, 1, 2, 32, True)])
def test_graphsage_step_equals_the_autograd_step(setup, kind, dims, b, P, H, n_rn, prefetch):
    """three steps at weight 0.75: the loss history at rtol 2e-5 / atol 2e-6 and Adam's state at 1e-4 (the bounds of
    test_step_with_hard_negatives_equals_the_autograd_step, the same encoder against the same kind of reference), the first
    step's gradients (gigl_nablp_train_plan_grads) within 1e-4 of the largest element, rows = the positives that took part"""
    from gigl_amd.engine import NablpTrainPlan
    from gigl_amd.models import GraphSAGE, HipBatch
    eng, rowptr, col = setup
    batches = _dev(host_batches(rowptr, col, b, P, H, n_rn, 3, seed=5), eng.device)
    torch.manual_seed(4)
    kw = dict(num_layers=2, should_l2_normalize_embedding_layer_output=True)
    ref = GraphSAGE(*dims, **kw).to(eng.device)
    lib = GraphSAGE(*dims, **kw).to(eng.device)
    lib.load_state_dict(ref.state_dict())
    ref.train()
    opt = torch.optim.Adam(ref.parameters(), lr=5e-3, weight_decay=1e-6, foreach=False)
    want, hs, want_grads = [], [], None
    for roots, cnt, rn in batches:
        embs = []
        for r in (roots, rn):
            tree = eng.sample_khop(r, FAN)
            u = eng.union_build(tree)
            embs.append(ref(HipBatch(eng, tree, u, train=True))[u.root_local[: r.numel()].long()])
        loss, h = task_loss_torch(embs[0], embs[1], cnt, b, P, H, kind, PARAM[kind], WEIGHT)
        if h is not None:
            hs.append(h)
        opt.zero_grad()
        loss.backward()
        if want_grads is None:
            want_grads = [torch.cat([cv.lin_l.weight.grad, cv.lin_r.weight.grad], dim=1).clone() for cv in ref.conv_layers]
        opt.step()
        want.append(float(loss.detach()))
    if kind == "Margin":
        _assert_no_pair_at_the_kink(hs)
    plan = NablpTrainPlan(eng, lib, b, P, n_rn, FAN, lr=5e-3, weight_decay=1e-6, num_hard_negatives=H, task=kind,
                          margin=MARGIN, softmax_temperature=SOFTMAX_T, task_weight=WEIGHT)
    got, rows, got_grads = _plan_steps(eng, plan, batches, prefetch, lambda: [plan.grads(l)[0] for l in range(2)])
    plan.store(lib)
    moments = plan.moments()
    plan.close()
    print(f"{kind}: plan losses {got} autograd losses {want}")
    assert rows == [float(int(c[:b].clamp(max=P).sum())) for _, c, _ in batches]
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)
    for l in range(2):
        err = float((got_grads[l] - want_grads[l]).abs().max()) / float(want_grads[l].abs().max())
        print(f"{kind}: layer {l} gradient error {err:.2e} of the largest element")
        assert err <= 1e-4, (kind, l, err)
    assert_adam_state(f"{kind} plan vs autograd", lib.state_dict(), moments, ref.state_dict(),
                      torch_adam_moments(opt, dict(ref.named_parameters())), tol_m=1e-4, tol_v=1e-4, tol_p=1e-4)


@pytest.mark.parametrize("kind", ["Margin", "Softmax"])
def test_gat_step_equals_the_autograd_step(kind):
    """the GAT kind shares the head: the shape and the bounds of test_gat_step_with_hard_negatives_equals_the_autograd_step
    (four heads of 8, 16 out, not normalised; losses rtol 1e-3 / atol 1e-5, Adam's state 1e-3 / 1e-3 / 1e-4), three steps"""
    from gigl_amd.engine import GatNablpTrainPlan
    from gigl_amd.hbm import ResidentGraph
    from gigl_amd.models_attn import GAT
    eng, rowptr, col = _engine()  # (an engine of its own: ResidentGraph.from_engine borrows it)
    try:
        b, P, H, n_rn = 24, 1, 2, 16
        batches = _dev(host_batches(rowptr, col, b, P, H, n_rn, 3, seed=9), eng.device)
        torch.manual_seed(6)
        kw = dict(num_layers=2, heads=4, should_l2_normalize_embedding_layer_output=False)
        ref = GAT(100, 8, 16, **kw).to(eng.device)
        lib = GAT(100, 8, 16, **kw).to(eng.device)
        lib.load_state_dict(ref.state_dict())
        ref.train()
        ref.engine = eng
        res = ResidentGraph.from_engine(eng, np.arange(N, dtype=np.int64), FAN)
        res.train_as_graph_data, res.defer_x = True, True
        opt = torch.optim.Adam(ref.parameters(), lr=5e-3, weight_decay=1e-6, foreach=False)
        want, hs, want_grads = [], [], None
        for roots, cnt, rn in batches:
            embs = []
            for r in (roots, rn):
                g, ri = res.train_graph(r)
                embs.append(ref(g)[ri])
            loss, h = task_loss_torch(embs[0], embs[1], cnt, b, P, H, kind, PARAM[kind], WEIGHT)
            if h is not None:
                hs.append(h)
            opt.zero_grad()
            loss.backward()
            if want_grads is None:
                want_grads = [c.lin.weight.grad.clone() for c in ref.conv_layers]
            opt.step()
            want.append(float(loss.detach()))
        if kind == "Margin":
            _assert_no_pair_at_the_kink(hs)
        plan = GatNablpTrainPlan(eng, lib, b, P, n_rn, FAN, lr=5e-3, weight_decay=1e-6, num_hard_negatives=H, task=kind,
                                 margin=MARGIN, softmax_temperature=SOFTMAX_T, task_weight=WEIGHT)
        got, rows, got_grads = _plan_steps(eng, plan, batches, True, lambda: [plan.grads(l)[0] for l in range(2)])
        plan.store(lib)
        moments = plan.moments()
        plan.close()
        print(f"GAT {kind}: plan losses {got} autograd losses {want}")
        assert rows == [float(int(c[:b].clamp(max=P).sum())) for _, c, _ in batches]
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-5)
        for l in range(2):
            err = float((got_grads[l] - want_grads[l]).abs().max()) / float(want_grads[l].abs().max())
            print(f"GAT {kind}: layer {l} weight gradient error {err:.2e} of the largest element")
            assert err <= 1e-3, (kind, l, err)
        flat = lambda sd: {k: v.reshape(-1) for k, v in sd.items()}
        assert_adam_state(f"GAT {kind} plan vs autograd", flat(lib.state_dict()), moments, flat(ref.state_dict()),
                          {k: (m.reshape(-1), v.reshape(-1)) for k, (m, v) in
                           torch_adam_moments(opt, dict(ref.named_parameters())).items()},
                          tol_m=1e-3, tol_v=1e-3, tol_p=1e-4)
    finally:
        eng.close()


@pytest.mark.parametrize("kind", ["Margin", "Softmax"])
def test_evaluate_gives_the_tasks_loss_and_the_same_rank_metrics(setup, kind):
    """evaluate() of a Margin / Softmax plan: the loss is the mean over the batches of the task's weighted loss (the torch
    restatement over the same parameters; 2e-5 as the step's), MRR and hits EQUAL a Retrieval plan's over the same parameters —
    the same forward kernels write the same scores, and the rank metrics do not look at the task.  Evaluation moves no
    optimiser state."""
    from gigl_amd.engine import NablpTrainPlan
    from gigl_amd.models import GraphSAGE, HipBatch
    eng, rowptr, col = setup
    b, P, H, n_rn = 48, 1, 2, 32
    batches = _dev(host_batches(rowptr, col, b, P, H, n_rn, 3, seed=5), eng.device)
    torch.manual_seed(4)
    model = GraphSAGE(100, 32, 70, num_layers=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)
    model.eval()
    want = []
    with torch.no_grad():
        for roots, cnt, rn in batches:
            embs = []
            for r in (roots, rn):
                tree = eng.sample_khop(r, FAN)
                u = eng.union_build(tree)
                embs.append(model(HipBatch(eng, tree, u))[u.root_local[: r.numel()].long()])
            want.append(float(task_loss_torch(embs[0], embs[1], cnt, b, P, H, kind, PARAM[kind], WEIGHT)[0]))
    ks = (1, 5, 10)
    plan = NablpTrainPlan(eng, model, b, P, n_rn, FAN, num_hard_negatives=H, task=kind, margin=MARGIN,
                          softmax_temperature=SOFTMAX_T, task_weight=WEIGHT)
    base = NablpTrainPlan(eng, model, b, P, n_rn, FAN, num_hard_negatives=H)
    try:
        got, ret = plan.evaluate(batches, ks), base.evaluate(batches, ks)
        assert plan.adam_steps() == 0
    finally:
        plan.close()
        base.close()
    print(f"{kind}: evaluate {got} want loss {np.mean(want)!r}; Retrieval plan {ret}")
    assert got["batches"] == 3 and got["rank_nodes"] == ret["rank_nodes"] > 0
    np.testing.assert_allclose(got["loss"], np.mean(want), rtol=2e-5, atol=2e-6)
    assert got["mrr"] == ret["mrr"] and got["hits"] == ret["hits"]
    assert abs(got["loss"] - ret["loss"]) > 0.1  # (the Retrieval plan's loss is another loss)


def _matching_graph_runs(variants):
    """the perfect-matching graph and batches of test_gpu_lp_hard_negatives._matching_runs (every float sum of a step whose
    order is open has two terms at the most there: two runs of one plan give the same bits — the reason is given at that
    function), one run of 4 steps per variant from the same weights: variant -> (losses, first step's gradients, parameters)"""
    import oracle
    from gigl_amd.engine import HipEngine, NablpTrainPlan
    from gigl_amd.models import GraphSAGE
    from test_gpu_lp_hard_negatives import TEMP, _plain_batches
    n, b, P, n_rn = 384, 48, 1, 32
    rng = np.random.default_rng(8)
    pairs = rng.permutation(n).astype(np.uint32).reshape(-1, 2)
    rowptr, col = oracle.build_csc(n, pairs[:, 0], pairs[:, 1], is_directed=False)
    assert np.diff(rowptr).tolist() == [1] * n
    eng = HipEngine(0)
    try:
        eng.load_csc(rowptr, col)
        eng.load_features((rng.standard_normal((n, 100)) / 4).astype(np.float32))
        eng.build_from_coo(n, np.arange(n, dtype=np.uint32), col.astype(np.uint32), is_directed=True, out_graph=True)
        batches = _plain_batches(eng, n, b, P, n_rn, 4, seed=13)
        torch.manual_seed(4)
        init = GraphSAGE(100, 32, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True).state_dict()
        out = {}
        for name, (kwargs, setter) in variants.items():
            lib = GraphSAGE(100, 32, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)
            lib.load_state_dict(init)
            plan = NablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, lr=5e-3, weight_decay=1e-6, **kwargs)
            if setter is not None:
                plan.set_task(**setter)
            losses, _, grads = _plan_steps(eng, plan, batches, False, lambda: [plan.grads(l)[0].clone() for l in range(2)])
            plan.store(lib)
            plan.close()
            out[name] = (losses, grads, {k: v.clone() for k, v in lib.state_dict().items()})
        return out
    finally:
        eng.close()


def test_retrieval_at_weight_one_is_the_plan_as_it_was_and_a_weight_scales_it():
    """a plan created without the task arguments, one created with task="Retrieval", task_weight=1 and one on which
    gigl_nablp_train_plan_set_task(RETRIEVAL, weight 1) was CALLED give bit-equal losses, gradients and parameters over 4
    steps (the plain plan is run twice and must repeat itself, or the comparison would say nothing).  Retrieval at weight 0.5:
    the first step's loss and gradients are EXACTLY half — the weight multiplies the loss word and dscores once, and every
    later rounding acts on exactly halved operands."""
    runs = _matching_graph_runs({
        "plain": ({}, None), "plain#again": ({}, None),
        "argument": (dict(task="Retrieval", task_weight=1.0), None),
        "setter": ({}, dict(task="Retrieval", task_weight=1.0)),
        "half": (dict(task="Retrieval", task_weight=0.5), None)})
    base = runs["plain"]
    assert np.isfinite(base[0]).all()
    for name in ("plain#again", "argument", "setter"):
        other = runs[name]
        assert other[0] == base[0], name
        for l in range(2):
            assert torch.equal(other[1][l], base[1][l]), (name, l)
        for k in base[2]:
            assert torch.equal(other[2][k], base[2][k]), (name, k)
    half = runs["half"]
    assert half[0][0] * 2 == base[0][0]
    for l in range(2):
        assert torch.equal(half[1][l] * 2, base[1][l]), l


def test_the_task_survives_grow_and_the_setter_is_refused_after_a_step(setup):
    """grow() re-creates the plan through create(): the wide plan trains the Margin loss too (its first step's loss is the
    Margin loss of the batch, not the Retrieval plan's ~ log C / T); after a step set_task is refused (GIGL_E_INVALID_ARG:
    the step is captured), as are arguments the library cannot take before one"""
    from gigl_amd._lib import GiglError
    from gigl_amd.engine import NablpTrainPlan
    from gigl_amd.models import GraphSAGE, HipBatch
    eng, rowptr, col = setup
    b, P, H, n_rn = 6, 2, 3, 5
    roots, cnt, rn = _dev(host_batches(rowptr, col, b, P, H, n_rn, 2, seed=5), eng.device)[0]
    torch.manual_seed(4)
    model = GraphSAGE(100, 32, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)
    with torch.no_grad():
        embs = []
        for r in (roots, rn):
            tree = eng.sample_khop(r, FAN)
            u = eng.union_build(tree)
            embs.append(model(HipBatch(eng, tree, u, train=True))[u.root_local[: r.numel()].long()])
        want = float(task_loss_torch(embs[0], embs[1], cnt, b, P, H, "Margin", MARGIN, WEIGHT)[0])
    plan = NablpTrainPlan(eng, model, b, P, n_rn, FAN, num_hard_negatives=H, task="Margin", margin=MARGIN, task_weight=WEIGHT)
    try:
        for bad in (dict(task="Softmax", softmax_temperature=0.0), dict(task="Margin", margin=float("nan")),
                    dict(task="Margin", task_weight=0.0), dict(task="Retrieval", task_weight=float("inf"))):
            with pytest.raises(GiglError):
                plan.set_task(**bad)
        plan.grow()
        assert plan.wide
        got, _, _ = _plan_steps(eng, plan, [(roots, cnt, rn)])
        print(f"the grown plan's Margin loss {got[0]!r}, want {want!r}")
        np.testing.assert_allclose(got[0], want, rtol=2e-5, atol=2e-6)
        with pytest.raises(GiglError):
            plan.set_task("Softmax")
        with pytest.raises(GiglError):
            plan.set_task("Margin", margin=MARGIN, task_weight=WEIGHT)
    finally:
        plan.close()
    with pytest.raises(ValueError):
        NablpTrainPlan(eng, model, b, P, n_rn, FAN, num_hard_negatives=H, task="Hinge")


def test_an_overflowed_batch_gives_nan_and_leaves_adams_counter():
    """the shared rule on a Margin plan, over the graph and batches of test_gpu_overflow.py (measured: none of the four
    batches fits a regular plan's workspace there): a batch that does not fit gives a NaN loss and leaves Adam's step counter
    where it was; step_checked then grows the plan — the task with it — and the batch trains: a finite Margin loss (well
    below 1, where the Retrieval loss of these batches is near log C) and the counter moved by one.  A batch that does fit
    a regular plan is held to the same two statements, should the sampler ever produce one here."""
    import oracle
    from gigl_amd.engine import HipEngine, NablpTrainPlan
    from gigl_amd.models import GraphSAGE
    from test_gpu_overflow import FAN as fan, N as n, _graph, _lp_batches
    d, b, P, n_rn = 64, 48, 1, 32
    rowptr, col, x = _graph(d)
    eng = HipEngine(0)
    try:
        eng.load_csc(rowptr, col)
        eng.load_features(x)
        dst = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rowptr).astype(np.int64))
        eng.build_from_coo(n, dst, col.astype(np.uint32), is_directed=True, out_graph=True)
        batches = _lp_batches(eng, n, b, P, n_rn, 4, seed=11)
        over = [int(oracle.union_build(r.cpu().numpy().view(np.uint32), list(fan), oracle.sample_khop(
            rowptr, col, r.cpu().numpy().view(np.uint32), list(fan), canonical=True)[0])["meta"][3]) > r.numel() * (1 + fan[0])
            for r, _, _ in batches]
        assert any(over), over
        torch.manual_seed(6)
        model = GraphSAGE(d, 32, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)
        plan = NablpTrainPlan(eng, model, b, P, n_rn, list(fan), task="Margin", margin=MARGIN, task_weight=WEIGHT)
        st = torch.cuda.Stream(device=eng.device)
        torch.cuda.synchronize()
        eng.bind_stream(st)
        try:
            seen_nan, counter = [], 0
            with torch.cuda.stream(st):
                for i, bt in enumerate(batches):
                    out = plan.step(*bt).clone()
                    eng.synchronize()
                    loss, steps = float(out[0]), plan.adam_steps()
                    seen_nan.append(loss != loss)
                    if loss != loss:
                        assert steps == counter, (i, steps, counter)
                    else:
                        assert 0.0 < loss < 1.0 and steps == counter + 1, (i, loss, steps, counter)
                    counter = steps
                bad = seen_nan.index(True)
                redone = plan.step_checked(*batches[bad])
                eng.synchronize()
            print(f"overflowed batches {seen_nan} (the main batch alone outgrows: {over}); redone after grow(): {redone!r}")
            assert all(s for s, o in zip(seen_nan, over) if o)
            assert plan.wide and 0.0 < redone < 1.0 and plan.adam_steps() == counter + 1
        finally:
            eng.bind_stream(torch.cuda.current_stream(eng.device))
            plan.close()
    finally:
        eng.close()
