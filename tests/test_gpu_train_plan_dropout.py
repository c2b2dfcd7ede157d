"""Dropout in the library training plans (gigl_sage_train_plan_set_dropout / gigl_nablp_train_plan_set_dropout,
csrc/pipeline.hip) on the GPU: the mask entry point against the restatement in Python integers (tests/dropout_ref.py), the
link-prediction and the node-classification plan at p = 0.5 against the autograd step whose dropout module multiplies by
the SAME mask (HipEngine.dropout_mask for the step, encode and layer at hand) — the comparisons, graphs and tolerances of
tests/test_gpu_train_plan.py —, evaluation without dropout, the setter's edge cases, a grown plan, and a trainer job with
trainerArgs dropout end to end."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import dropout_ref
from conftest import seed_trainer
from helpers import assert_adam_state, torch_adam_moments
from test_gpu_lp_hard_negatives import FAN as HN_FAN
from test_gpu_lp_hard_negatives import _designed_batches
from test_gpu_lp_hard_negatives import _lp_loss_torch as _lp_loss_torch_hard
from test_gpu_lp_hard_negatives import setup as hn_setup  # noqa: F401  (its 390-node graph with designed hard negatives)
from test_gpu_nablp import CFG, workdir  # noqa: F401  (the module-scoped fixture: the sampled toy job)
from test_gpu_train_plan import _lp_batches, _lp_loss_torch, setup  # noqa: F401  (its 8192-node graph)

pytestmark = pytest.mark.gpu

SEED, P_DROP, TEMP, KS = 0x5EED0123456789AB, 0.5, 0.07, (1, 5, 10)


# ---- 1. the mask entry point

@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.9])
def test_mask_entry_point_equals_the_restatement(setup, p):
    """gigl_dropout_mask bit for bit, at one row / a few / more than a workgroup's lanes, widths of one column, one whole
    block, a block and a half, a tail after eight blocks, whole blocks only"""
    eng = setup[0]
    for rows in (1, 3, 257):
        for cols in (1, 4, 6, 33, 256):
            step, encode, layer = rows % 5, cols & 1, cols % 3
            got = eng.dropout_mask(SEED, step, encode, layer, rows, cols, p)
            eng.synchronize()
            want = dropout_ref.keep_mask(SEED, step, encode, layer, rows, cols, p)
            assert np.array_equal(got.cpu().numpy(), want), (rows, cols, p)


# ---- the reference side: the model's dropout module multiplies by the plan's mask

class _PlanDropout(torch.nn.Module):
    """stands in for the reference model's nn.Dropout: multiplies by the mask the plan applies at (step, encode, layer) —
    GraphSAGE._post calls it once per activated layer, in layer order.  mask(...) -> uint8 [rows, cols] on the device.
    The mask's row is the node's local id in the PLAN's batch graph: `rows_in_plan` (int64 [rows of the reference's graph])
    maps the reference's local ids to them (None: the same numbering)"""

    def __init__(self, p, mask):
        super().__init__()
        self.p, self.mask, self.step, self.encode, self.layer, self.rows_in_plan = p, mask, 0, 0, 0, None

    def at(self, step, encode, rows_in_plan=None):
        self.step, self.encode, self.layer, self.rows_in_plan = step, encode, 0, rows_in_plan

    def forward(self, h):
        if self.rows_in_plan is None:
            keep = self.mask(self.step, self.encode, self.layer, h.shape[0], h.shape[1])
        else:
            rows = self.rows_in_plan[: h.shape[0]]
            keep = self.mask(self.step, self.encode, self.layer, int(rows.max()) + 1, h.shape[1])[rows]
        self.layer += 1
        return h * (keep.to(h.dtype) * float(dropout_ref.scale(self.p)))


class _PlanOrder:
    """the node order of a regular (not wide) two-hop training plan's batch graphs.  Its graph part is the one-call plan's
    (sample + the leaf-global union build), whose nodes of level 1 are numbered in another order than engine.union_build's
    (tests/test_gpu_plan.py compares them sorted): a one-call plan of the same batch shape, run over the same padded roots,
    shows the numbering (SagePlan.last_batch_to_host)"""

    def __init__(self, eng, in_dim, b, fan, pad):
        from gigl_amd.models import GraphSAGE
        self.eng, self.b, self.pad = eng, b, pad
        self.plan = GraphSAGE(in_dim, 8, 8, num_layers=len(fan)).to(eng.device).make_plan(eng, b, fan)

    def rows_in_plan(self, roots, u):
        """int64 [nodes of u]: the plan's local id of u's node i (0 for the leaves, which no layer computes)"""
        from gigl_amd._lib import GIGL_META_LEVEL0
        k = int(roots.numel())
        if k < self.b:
            roots = torch.cat([roots, roots[:1].expand(self.b - k) if self.pad == "first" else
                               torch.full((self.b - k,), -1, dtype=torch.int32, device=roots.device)])
        self.plan.run(roots.contiguous())
        hb = self.plan.last_batch_to_host()
        assert hb["meta"][8] == 0  # (no overflow)
        inner = int(hb["meta"][GIGL_META_LEVEL0 + 1])  # nodes of level <= 1
        where = {int(v): i for i, v in enumerate(hb["nodes"][:inner])}
        mine = u.nodes.cpu().numpy().view(np.uint32)
        n_mine = int(u.meta.cpu()[GIGL_META_LEVEL0 + 1])
        assert n_mine == inner and set(where) == {int(v) for v in mine[:n_mine]}  # (the same inner nodes, numbered differently)
        return torch.tensor([where.get(int(v), 0) for v in mine], dtype=torch.int64, device=self.eng.device)

    def close(self):
        self.plan.close()


def _engine_mask(eng, p=P_DROP, seed=SEED):
    return lambda step, encode, layer, rows, cols: eng.dropout_mask(seed, step, encode, layer, rows, cols, p)


def _restated_mask(eng, p=P_DROP, seed=SEED):
    return lambda step, encode, layer, rows, cols: torch.from_numpy(
        dropout_ref.keep_mask(seed, step, encode, layer, rows, cols, p)).to(eng.device)


def _lp_reference(eng, ref, fan, batches, loss_of, mask, b_main, n_rn, wide_from=None):
    """the autograd steps of test_library_link_prediction_step_equals_the_autograd_step with the plan's masks (b_main, n_rn:
    the plan's root capacities; wide_from: the step from which the plan is a wide one — numbered as engine.union_build)"""
    from gigl_amd.models import HipBatch
    orders = [_PlanOrder(eng, ref.in_dim, nb, fan, "absent") for nb in (b_main, n_rn)]
    ref.dropout = _PlanDropout(ref.dropout.p, mask)
    ref.train()
    opt = torch.optim.Adam(ref.parameters(), lr=5e-3, weight_decay=1e-6, foreach=False)
    want = []
    for i, (roots, cnt, rn) in enumerate(batches):
        embs = []
        for encode, r in enumerate((roots, rn)):
            tree = eng.sample_khop(r, fan)
            u = eng.union_build(tree)
            rows_in_plan = None if wide_from is not None and i >= wide_from else orders[encode].rows_in_plan(r, u)
            ref.dropout.at(i, encode, rows_in_plan)  # (no batch fails: Adam's count of applied steps is the batch's index)
            embs.append(ref(HipBatch(eng, tree, u, train=True))[u.root_local[: r.numel()].long()])
        loss = loss_of(embs[0], embs[1], roots, cnt, rn)
        opt.zero_grad()
        loss.backward()
        opt.step()
        want.append(float(loss.detach()))
    for o in orders:
        o.close()
    return want, torch_adam_moments(opt, dict(ref.named_parameters()))


def _plan_steps(eng, plan, batches, prefetch=True, before_step=None):
    st = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    try:
        got = []
        with torch.cuda.stream(st):
            for i, (roots, cnt, rn) in enumerate(batches):  # (eager once, captured on the second step, replayed from then on)
                if before_step is not None:
                    before_step(i)
                nxt = (batches[i + 1][0], batches[i + 1][2]) if prefetch and i + 1 < len(batches) and i % 3 != 2 else None
                got.append(plan.step(roots, cnt, rn, next_roots=nxt).clone())
        eng.synchronize()
    finally:
        eng.bind_stream(torch.cuda.current_stream(eng.device))
    return [float(v[0]) for v in got]


def _models(eng, dims, **kw):
    from gigl_amd.models import GraphSAGE
    torch.manual_seed(4)
    kw = dict(num_layers=2, dropout=P_DROP, **kw)
    ref = GraphSAGE(*dims, **kw).to(eng.device)
    lib = GraphSAGE(*dims, **kw).to(eng.device)
    lib.load_state_dict(ref.state_dict())
    return ref, lib


def _out_graph(eng, rowptr, col, n):
    if getattr(eng, "_graph_out", None) is None:
        dst = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rowptr).astype(np.int64))
        eng.build_from_coo(n, dst, col.astype(np.uint32), is_directed=True, out_graph=True)  # (out-edges = reversed in-edges)


# ---- 2. the link-prediction plan against the autograd step

@pytest.mark.parametrize("hid,act_last,fork", [(32, False, True), (32, False, False), (30, False, False), (32, True, True)])
def test_link_prediction_plan_with_dropout_equals_the_autograd_step(setup, monkeypatch, hid, act_last, fork):
    """100 -> hid -> 16, fan-outs [10, 5], 48 anchors, one positive, 32 random negatives, 8 steps (eager, captured, replayed;
    most announce the next batch), the last batch short (30 anchors, 20 negatives).  fork: the random negatives' encode and
    the main batch's weight gradients on streams of their own (the default) or the whole step in one captured chain
    (GIGL_LP_FORK=0: the path whose backward used the masked read).  hid = 30: a hidden width that is no multiple of 4 — the
    plan accepts it (the input gradients then take the scatter backward), the dropout kernels take their column-by-column
    path.  act_last: dropout after the last layer too, ahead of the normalisation.  Tolerances: those of
    test_library_link_prediction_step_equals_the_autograd_step for the normalised encoder."""
    from gigl_amd.engine import NablpTrainPlan
    eng, rowptr, col, x, n = setup
    _out_graph(eng, rowptr, col, n)
    if not fork:
        monkeypatch.setenv("GIGL_LP_FORK", "0")
    b, P, n_rn, fan, steps = 48, 1, 32, [10, 5], 8
    batches = _lp_batches(eng, n, b, P, n_rn, steps, seed=5)
    na = 30
    batches[-1] = (batches[-1][0][: (1 + P) * na].contiguous(), batches[-1][1][:na].contiguous(), batches[-1][2][:20].contiguous())
    ref, lib = _models(eng, (100, hid, 16), should_l2_normalize_embedding_layer_output=True, activation_after_last_conv=act_last)
    want, ref_moments = _lp_reference(
        eng, ref, fan, batches, lambda em, er, roots, cnt, rn: _lp_loss_torch(em, er, roots, cnt, rn, cnt.numel(), P, TEMP),
        _engine_mask(eng), b * (1 + P), n_rn)
    plan = NablpTrainPlan(eng, lib, b, P, n_rn, fan, temperature=TEMP, remove_accidental_hits=True, lr=5e-3, weight_decay=1e-6,
                          dropout_seed=SEED)  # (dropout: the model's own 0.5)
    got = _plan_steps(eng, plan, batches)
    plan.store(lib)
    moments = plan.moments()
    plan.close()
    print(f"hid={hid} act_last={act_last} fork={fork}: plan losses {got} autograd losses {want}")
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)
    assert_adam_state("link-prediction plan with dropout vs autograd", lib.state_dict(), moments, ref.state_dict(), ref_moments,
                      tol_m=1e-4, tol_v=1e-4, tol_p=1e-4)


def test_link_prediction_plan_with_dropout_and_hard_negatives(hn_setup):
    """the same with num_hard_negatives = 2: the designed batches of tests/test_gpu_lp_hard_negatives.py (48 anchors, one
    positive, two hard-negative slots, 32 random negatives, 8 steps) on its graph"""
    from gigl_amd.engine import NablpTrainPlan
    eng, rowptr, col, x, n = hn_setup
    b, P, H, n_rn, steps = 48, 1, 2, 32, 8
    batches = _designed_batches(eng, n, b, P, H, n_rn, steps, seed=5, list_name="neg_dropout")
    ref, lib = _models(eng, (100, 32, 16), should_l2_normalize_embedding_layer_output=True)
    want, ref_moments = _lp_reference(
        eng, ref, HN_FAN, batches, lambda em, er, roots, cnt, rn: _lp_loss_torch_hard(em, er, roots, cnt, rn, b, P, H, TEMP),
        _engine_mask(eng), b * (1 + P + H), n_rn)
    plan = NablpTrainPlan(eng, lib, b, P, n_rn, HN_FAN, temperature=TEMP, remove_accidental_hits=True, lr=5e-3,
                          weight_decay=1e-6, num_hard_negatives=H, dropout_seed=SEED)
    got = _plan_steps(eng, plan, batches)
    plan.store(lib)
    moments = plan.moments()
    plan.close()
    print(f"H={H}: plan losses {got} autograd losses {want}")
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)
    assert_adam_state("hard-negative plan with dropout vs autograd", lib.state_dict(), moments, ref.state_dict(), ref_moments,
                      tol_m=1e-4, tol_v=1e-4, tol_p=1e-4)


# ---- 3. the node-classification plan against the autograd step

def test_node_classification_plan_with_dropout_equals_the_autograd_step(setup):
    """100 -> 64 -> 7, fan-outs [10, 5], 256 roots: 6 steps issued through run_steps with no host read between them (each
    step's mask is keyed by the DEVICE step counter), against the autograd step of
    test_library_training_step_equals_the_autograd_step with the plan's masks — that case's tolerances"""
    import torch.nn.functional as F
    from gigl_amd.engine import SageTrainPlan
    from gigl_amd.models import HipBatch
    eng, rowptr, col, x, n = setup
    dims, fan, b, steps = (100, 64, 7), [10, 5], 256, 6
    rng = np.random.default_rng(3)
    roots_all = torch.from_numpy(rng.permutation(n)[: steps * b].astype(np.uint32).view(np.int32)).to(eng.device)
    labels_all = torch.from_numpy(rng.integers(0, dims[2], steps * b)).to(eng.device)
    ref, lib = _models(eng, dims)
    ref.dropout = _PlanDropout(P_DROP, _engine_mask(eng))
    ref.train()
    opt = torch.optim.Adam(ref.parameters(), lr=0.01, weight_decay=5e-4, foreach=False)
    order = _PlanOrder(eng, dims[0], b, fan, "first")
    want = []
    for i in range(steps):
        roots = roots_all[i * b:(i + 1) * b]
        tree = eng.sample_khop(roots, fan)
        u = eng.union_build(tree)
        ref.dropout.at(i, 0, order.rows_in_plan(roots, u))
        out = ref(HipBatch(eng, tree, u, train=True))
        loss = F.cross_entropy(out[u.root_local[: roots.numel()].long()], labels_all[i * b:(i + 1) * b])
        opt.zero_grad()
        loss.backward()
        opt.step()
        want.append(float(loss.detach()))
    order.close()
    st = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    try:
        plan = SageTrainPlan(eng, lib, b, fan, lr=0.01, weight_decay=5e-4, dropout_seed=SEED)
        with torch.cuda.stream(st):
            got = plan.run_steps(steps, lambda i: dict(roots=roots_all[i * b:(i + 1) * b], labels=labels_all[i * b:(i + 1) * b],
                                                       next_roots=roots_all[(i + 1) * b:(i + 2) * b])).clone()
        eng.synchronize()
        got = [float(v) for v in got]
        assert not plan.wide  # (no batch was redone: step i ran at counter i)
        plan.store(lib)
        moments = plan.moments()
        plan.close()
    finally:
        eng.bind_stream(torch.cuda.current_stream(eng.device))
    print(f"node classification: plan losses {got} autograd losses {want}")
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-6)
    assert_adam_state("node-classification plan with dropout vs autograd", lib.state_dict(), moments, ref.state_dict(),
                      torch_adam_moments(opt, dict(ref.named_parameters())), tol_m=2e-5, tol_v=2e-5, tol_p=2e-5)


# ---- 4. evaluation runs without dropout

def test_evaluation_runs_without_dropout(setup):
    """a dropout plan and a plain plan over the same weights: evaluate() gives the same loss, MRR and hits@k — the bound
    tests/test_gpu_lp_eval_plan.py holds two plans' passes over the same inputs to — while their training steps differ"""
    from gigl_amd.engine import NablpTrainPlan
    eng, rowptr, col, x, n = setup
    _out_graph(eng, rowptr, col, n)
    b, P, n_rn, fan = 48, 1, 32, [10, 5]
    batches = _lp_batches(eng, n, b, P, n_rn, 3, seed=21)
    _, lib = _models(eng, (100, 32, 16), should_l2_normalize_embedding_layer_output=True)
    st = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    try:
        passes, first = {}, {}
        with torch.cuda.stream(st):
            for name, p in (("dropout", None), ("plain", 0.0)):
                plan = NablpTrainPlan(eng, lib, b, P, n_rn, fan, temperature=TEMP, lr=0.0, weight_decay=0.0, dropout=p,
                                      dropout_seed=SEED)
                passes[name] = plan.evaluate(batches[:2], KS)
                first[name] = plan.step(*batches[2]).clone()  # (lr 0: the shared weights stay what they are)
                plan.close()
        eng.synchronize()
    finally:
        eng.bind_stream(torch.cuda.current_stream(eng.device))
    got, want = passes["dropout"], passes["plain"]
    print("evaluation of a dropout plan:", got, "of a plain plan:", want, "first training losses:", first)
    assert got["batches"] == want["batches"] == 2 and got["rank_nodes"] == want["rank_nodes"] > 0
    np.testing.assert_allclose([got["loss"], got["mrr"], *got["hits"]], [want["loss"], want["mrr"], *want["hits"]], rtol=1e-6, atol=0)
    assert abs(float(first["dropout"][0]) - float(first["plain"][0])) > 1e-3  # (the training step does drop)


# ---- 5. the setters' edge cases

def test_setter_edge_cases(setup):
    """p = 0 through the setter is OK and changes nothing: the losses stay within the bound two runs of the same plan are
    held to (rtol 2e-5 / atol 2e-6: tests/test_gpu_lp_eval_plan.py) of a plan that never saw the call; p outside [0, 1) is
    refused; after the first step both plans' setters are refused"""
    from gigl_amd._lib import GiglError, check
    from gigl_amd.engine import NablpTrainPlan, SageTrainPlan
    from gigl_amd.models import GraphSAGE
    eng, rowptr, col, x, n = setup
    _out_graph(eng, rowptr, col, n)
    b, P, n_rn, fan = 48, 1, 32, [10, 5]
    batches = _lp_batches(eng, n, b, P, n_rn, 4, seed=5)
    lib_ = eng._lib
    losses = {}
    for name in ("never", "p = 0"):
        torch.manual_seed(4)
        model = GraphSAGE(100, 32, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)
        plan = NablpTrainPlan(eng, model, b, P, n_rn, fan, temperature=TEMP, lr=5e-3, weight_decay=1e-6)
        if name == "p = 0":
            check(lib_.gigl_nablp_train_plan_set_dropout(plan._plan, 0.0, SEED), eng._ctx)
            for bad in (1.0, -0.25, 1.5, float("nan")):
                with pytest.raises(GiglError):
                    check(lib_.gigl_nablp_train_plan_set_dropout(plan._plan, bad, SEED), eng._ctx)
        losses[name] = _plan_steps(eng, plan, batches)
        for p in (0.0, 0.5):
            with pytest.raises(GiglError):  # (the step is captured)
                check(lib_.gigl_nablp_train_plan_set_dropout(plan._plan, p, SEED), eng._ctx)
        plan.close()
    print("losses of a plan that never saw the setter / saw it with p = 0:", losses)
    np.testing.assert_allclose(losses["p = 0"], losses["never"], rtol=2e-5, atol=2e-6)
    # the node-classification plan's setter
    torch.manual_seed(1)
    model = GraphSAGE(100, 32, 7, num_layers=2).to(eng.device)
    plan = SageTrainPlan(eng, model, 64, fan)
    check(lib_.gigl_sage_train_plan_set_dropout(plan._plan, 0.0, SEED), eng._ctx)
    with pytest.raises(GiglError):
        check(lib_.gigl_sage_train_plan_set_dropout(plan._plan, 1.0, SEED), eng._ctx)
    roots = torch.arange(64, dtype=torch.int32, device=eng.device)
    labels = torch.zeros(64, dtype=torch.int64, device=eng.device)
    torch.cuda.synchronize()
    loss = plan.step(roots, labels)
    eng.synchronize()
    assert np.isfinite(float(loss[0]))
    with pytest.raises(GiglError):
        check(lib_.gigl_sage_train_plan_set_dropout(plan._plan, 0.5, SEED), eng._ctx)
    plan.close()


# ---- 6. a grown plan drops the same elements

def test_a_grown_plan_carries_p_and_seed(setup):
    """one step, plan.grow() (the wide plan is created anew and adopts the optimiser state), one more step: both match the
    autograd steps under the RESTATED masks of steps 0 and 1 — the wide plan was handed p and seed"""
    from gigl_amd.engine import NablpTrainPlan
    eng, rowptr, col, x, n = setup
    _out_graph(eng, rowptr, col, n)
    b, P, n_rn, fan = 48, 1, 32, [10, 5]
    batches = _lp_batches(eng, n, b, P, n_rn, 2, seed=9)
    ref, lib = _models(eng, (100, 32, 16), should_l2_normalize_embedding_layer_output=True)
    want, ref_moments = _lp_reference(
        eng, ref, fan, batches, lambda em, er, roots, cnt, rn: _lp_loss_torch(em, er, roots, cnt, rn, b, P, TEMP),
        _restated_mask(eng), b * (1 + P), n_rn, wide_from=1)
    plan = NablpTrainPlan(eng, lib, b, P, n_rn, fan, temperature=TEMP, remove_accidental_hits=True, lr=5e-3, weight_decay=1e-6,
                          dropout_seed=SEED)

    def grow_before_the_second(i):
        if i == 1:
            eng.synchronize()
            plan.grow()
    got = _plan_steps(eng, plan, batches, prefetch=False, before_step=grow_before_the_second)
    assert plan.wide and plan.adam_steps() == 2
    plan.store(lib)
    moments = plan.moments()
    plan.close()
    print(f"grown plan: losses {got} autograd losses under the restated masks {want}")
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)
    assert_adam_state("grown dropout plan vs autograd", lib.state_dict(), moments, ref.state_dict(), ref_moments,
                      tol_m=1e-4, tol_v=1e-4, tol_p=1e-4)


# ---- 7. the trainer end to end

def test_trainer_runs_a_dropout_job_through_the_library_plan(workdir, tmp_path, monkeypatch):  # noqa: F811
    """the homogeneous link-prediction fixture of tests/test_gpu_nablp.py with trainerArgs dropout 0.5: the job gets a
    library plan, trains to finite losses, and the inferencer over the trained model (eval mode: dropout is the identity)
    takes the one-call plan, whose embeddings equal the staged forward's"""
    import yaml
    from gigl_amd import hbm
    from gigl_amd.inferencer import Inferencer
    from gigl_amd.nablp_spec import HipNodeAnchorLinkPredictionSpec
    from gigl_amd.trainer import Trainer
    base = str(tmp_path / "job")
    shutil.copytree(workdir, base)
    shutil.rmtree(os.path.join(base, "out", "nablp", "split"), ignore_errors=True)
    doc = yaml.safe_load(open(os.path.join(base, CFG)))
    doc["trainerConfig"]["trainerArgs"].update(dropout="0.5", dropout_seed="7")
    doc["inferencerConfig"]["inferencerArgs"].update(doc["trainerConfig"]["trainerArgs"])
    yaml.safe_dump(doc, open(os.path.join(base, CFG), "w"))
    monkeypatch.setenv("GIGL_AMD_ROUTE", "hbm")
    picked = []
    pick = HipNodeAnchorLinkPredictionSpec._library_train_plan

    def recording_pick(self, cfg):
        plan = pick(self, cfg)
        picked.append((type(plan).__name__, getattr(plan, "_dropout", None)))
        return plan
    monkeypatch.setattr(HipNodeAnchorLinkPredictionSpec, "_library_train_plan", recording_pick)
    seed_trainer()
    tr = Trainer()
    tr.run("job", CFG, None, uri_base=base)
    spec = tr.training_process.trainer
    assert tr.training_process.route == "hbm"
    assert picked == [("NablpTrainPlan", (0.5, 7))], picked
    losses = [h["loss"] for h in spec.history]
    print("dropout job: plan losses", losses)
    assert int(getattr(spec, "train_plan_steps", 0)) == len(losses) >= 4 and np.isfinite(losses).all()
    enc = (spec.model.module if hasattr(spec.model, "module") else spec.model).encoder
    assert enc.dropout.p == 0.5
    # the inferencer: the one-call plan, then the same job with the plan withheld (the staged forward)
    seen = []
    close = hbm.ResidentGraph.close

    def recording_close(self):
        seen.append(list(self._plans.values()))
        close(self)
    monkeypatch.setattr(hbm.ResidentGraph, "close", recording_close)
    inf = Inferencer()
    out = inf.run("job", CFG, None, uri_base=base, route="hbm")
    assert inf.route == "hbm" and inf.rows_written == 27
    assert seen and seen[-1] and any(p is not None for p in seen[-1])  # a one-call plan, not the staged forward
    rows = {r["node_id"]: r["emb"] for r in (json.loads(l) for l in open(out["embeddings"]))}
    monkeypatch.setattr(hbm.ResidentGraph, "_plan_for", lambda self, *a, **k: None)
    staged = Inferencer()
    out_s = staged.run("job", CFG, None, uri_base=base, route="hbm")
    assert staged.route == "hbm" and staged.rows_written == 27 and not any(p is not None for p in seen[-1])
    rows_s = {r["node_id"]: r["emb"] for r in (json.loads(l) for l in open(out_s["embeddings"]))}
    assert rows.keys() == rows_s.keys() and len(rows) == 27
    ids = sorted(rows)
    np.testing.assert_allclose(np.array([rows[i] for i in ids], np.float32), np.array([rows_s[i] for i in ids], np.float32),
                               rtol=1e-5, atol=1e-5)
