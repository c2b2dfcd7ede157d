"""The GCN training step (gigl_gcn_train_plan_*, csrc/pipeline.hip) through engine.GcnTrainPlan against a FLOAT64
restatement: TwoLayerGCN over the oracle's union graph, cross-entropy on the roots, autograd, torch.optim.Adam — cases,
batches and references in tests/gcn_plan_cases.py.  Scalar and vector paths of both gather kernels, an fp16 table, no
biases, root rows beyond 64 edges, roots without in-edges, one root in every slot, short batches, three steps with weight
decay, a failed batch and resume(), a batch that overflows the regular workspace (redone after grow()), and dropout from the
plan's own stream — which also pins the numbering: the restatement masks h1's rows by oracle.union_build's local ids.

With weight_decay = 0 the first step leaves exp_avg = (1 - beta1) g: plan.moments() hands out the step's raw gradient of
every tensor to one fp32 rounding.

Bounds, each or 4 x the float32 restatement's error against float64, whichever is larger: loss rtol 1e-4 / atol 1e-5;
first-step gradients 1e-4 of the tensor's largest; Adam's moments and the determined parameters 1e-4 through
helpers.assert_adam_state.  NaN losses and unchanged state of failed or halted steps are exact.

Measured on an MI355X (worst over the cases of a class; err = plan against float64, fp32 = the float32 restatement against
float64; losses absolute, gradients and moments relative to the tensor's largest, parameters absolute on the determined
set):

    class of case                      quantity           err       fp32
    shapes, fp16 table, no bias        loss           2.4e-07    2.3e-07
    shapes, fp16 table, no bias        grad           5.6e-07    9.2e-07
    shapes, fp16 table, no bias        exp_avg_sq     1.3e-05    1.7e-06
    shapes, fp16 table, no bias        param          1.6e-08    1.7e-08
    roots and short batches            loss           1.7e-07    3.1e-07
    roots and short batches            grad           4.5e-07    8.3e-07
    roots and short batches            exp_avg_sq     1.4e-05    1.8e-06
    roots and short batches            param          1.6e-08    1.6e-08
    three steps, weight decay          loss           1.8e-07    1.8e-07
    three steps, weight decay          exp_avg        4.1e-07    4.2e-07
    three steps, weight decay          exp_avg_sq     1.3e-05    5.0e-07
    three steps, weight decay          param          4.0e-08    4.4e-08
    failed, resumed                    loss           7.0e-08    7.0e-08
    failed, resumed                    grad           3.2e-07    7.5e-07
    failed, resumed                    exp_avg_sq     1.3e-05    1.2e-06
    failed, resumed                    param          1.6e-08    1.6e-08
    overflow, redone                   loss           1.1e-07    7.4e-09
    overflow, redone                   grad           2.6e-07    3.9e-07
    overflow, redone                   exp_avg_sq     1.3e-05    5.0e-07
    overflow, redone                   param          1.5e-08    1.6e-08
    dropout, three steps               loss           9.3e-08    1.5e-07
    dropout, three steps               exp_avg        4.4e-07    3.6e-07
    dropout, three steps               exp_avg_sq     1.3e-05    4.2e-07
    dropout, three steps               param          4.1e-08    3.6e-08

exp_avg_sq sits at 1.3e-5 everywhere, as in test_gpu_train_step_edges.py: adam_kernel takes beta2 as the fp32 0.999.
"""
import contextlib

import numpy as np
import pytest
import torch

import gcn_plan_cases as gc
from helpers import adam_state_errors, assert_adam_state

LOSS_RTOL, LOSS_ATOL, GRAD_TOL, STATE_TOL, FP32_FACTOR = 1e-4, 1e-5, 1e-4, 1e-4, 4.0


# ---- the device side ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    rowptr, col = gc.graph()[:2]
    e = HipEngine(0)
    e.load_csc(rowptr, col)
    e._gcn_case_table = None
    yield e
    e.close()


def _model(case, state):
    from gigl_amd.models_attn import TwoLayerGCN
    model = TwoLayerGCN(case.dims[0], case.dims[2], hid_dim=case.dims[1], is_training=case.dropout, bias=case.bias)
    model.load_state_dict(state)
    return model


@contextlib.contextmanager
def _plan_of(eng, case, state):
    """the case's plan on a stream of its own, over the case's feature table (the engine keeps the last one loaded)"""
    from gigl_amd.engine import GcnTrainPlan
    key = (case.dims[0], case.half)
    if eng._gcn_case_table != key:
        eng.load_features(gc.features(*key))
        eng._gcn_case_table = key
    model = _model(case, state).to(eng.device)
    st = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    plan = GcnTrainPlan(eng, model, case.b, list(case.fan), lr=case.lr, weight_decay=case.wd, betas=(gc.BETA1, gc.BETA2),
                        eps=gc.ADAM_EPS, dropout_seed=gc.DROP_SEED)
    try:
        with torch.cuda.stream(st):
            yield plan, model
        eng.synchronize()
    finally:
        plan.close()
        eng.bind_stream(torch.cuda.current_stream(eng.device))


def _dev(eng, batches):
    return [(torch.from_numpy(r.view(np.int32)).to(eng.device), torch.from_numpy(y).to(eng.device)) for r, y, _ in batches]


def _snapshot(eng, plan, model):
    """(parameters, moments) on the host, keyed like the model's state dict"""
    eng.synchronize()
    plan.store(model)
    params = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    moments = {k: (m.cpu().clone(), v.cpu().clone()) for k, (m, v) in plan.moments().items()}
    eng.synchronize()
    return params, moments


def _assert_same_state(a, b, what):
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), (what, "parameter", k)
    for k in a[1]:
        assert torch.equal(a[1][k][0], b[1][k][0]) and torch.equal(a[1][k][1], b[1][k][1]), (what, "moments", k)


# ---- the comparisons ----------------------------------------------------------------------------------------------------
def _check_losses(label, got, r64, r32):
    assert len(got) == len(r64.losses)
    for i, (g, w, w32) in enumerate(zip(got, r64.losses, r32.losses)):
        err, fp32 = abs(g - w), abs(w32 - w)
        print(f"{label} loss[{i}]: err={err:.3e} fp32={fp32:.3e} (loss {w:.6g})")
        assert err <= max(LOSS_ATOL + LOSS_RTOL * abs(w), FP32_FACTOR * fp32), (label, i, g, w, err, fp32)


def _check_first_step(label, moments, r64, r32):
    """exp_avg / (1 - beta1) against the float64 gradient of every tensor, exp_avg_sq against (1 - beta2) g^2"""
    assert set(moments) == set(r64.grads0)
    for k, want in r64.grads0.items():
        m, v = (t.double() for t in moments[k])
        big = float(want.abs().max())
        d = (m / (1.0 - gc.BETA1) - want).abs()
        e32 = float((r32.grads0[k].double() - want).abs().max())
        print(f"{label} grad {k}: err={float(d.max()) / max(big, 1e-300):.3e} fp32={e32 / max(big, 1e-300):.3e}")
        assert float(d.max()) <= max(GRAD_TOL * big, FP32_FACTOR * e32), (label, k, float(d.max()), big, e32)
        v64, v32 = r64.moments[k][1], r32.moments[k][1].double()
        vbig = float(v64.max())
        ev, ev32 = float((v - v64).abs().max()) / max(vbig, 1e-300), float((v32 - v64).abs().max()) / max(vbig, 1e-300)
        print(f"{label} exp_avg_sq {k}: err={ev:.3e} fp32={ev32:.3e}")
        assert ev <= max(STATE_TOL, FP32_FACTOR * ev32), (label, k, ev, ev32)


def _check_state(label, params, moments, r64, r32):
    """Adam's moments and the determined parameters of every tensor, through helpers.assert_adam_state"""
    assert set(moments) == set(r64.moments) and set(params) == set(r64.params)
    e32 = adam_state_errors(r32.params, r32.moments, r64.params, r64.moments)
    got = adam_state_errors(params, moments, r64.params, r64.moments)
    for k in r64.moments:
        for what, i in (("exp_avg", 0), ("exp_avg_sq", 1), ("param", 2)):
            print(f"{label} {what} {k}: err={got[k][i]:.3e} fp32={e32[k][i]:.3e}")
        tol = [max(STATE_TOL, FP32_FACTOR * e32[k][i]) for i in range(3)]
        assert_adam_state(f"{label} {k}", {k: params[k]}, {k: moments[k]}, {k: r64.params[k]}, {k: r64.moments[k]}, *tol)


# ---- one step, weight_decay = 0: loss, raw gradients, state -------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", gc.PLAIN_CASES)
def test_first_step_against_float64(eng, name):
    case = gc.CASES[name]
    assert case.wd == 0.0 and case.steps == 1
    state, batches = gc.setup(name)
    r64, r32 = gc.reference(name)
    with _plan_of(eng, case, state) as (plan, model):
        (roots, labels), = _dev(eng, batches)
        loss = float(plan.step(roots, labels).clone())
        after = _snapshot(eng, plan, model)
        assert not plan.wide
    assert sorted(after[0]) == sorted(n for n in gc.NAMES if case.bias or not n.endswith("bias"))
    _check_losses(name, [loss], r64, r32)
    _check_first_step(name, after[1], r64, r32)
    _check_state(name, after[0], after[1], r64, r32)


# ---- three steps with weight decay, every step announcing the next batches ----------------------------------------------
@pytest.mark.gpu
def test_three_steps_with_weight_decay_against_float64(eng):
    name = "three_steps_decay"
    case = gc.CASES[name]
    state, batches = gc.setup(name)
    r64, r32 = gc.reference(name)
    with _plan_of(eng, case, state) as (plan, model):
        dev = _dev(eng, batches)
        got = plan.run_steps(case.steps, lambda i: dict(roots=dev[i][0], labels=dev[i][1],
                                                        next_roots=dev[i + 1][0] if i + 1 < case.steps else None,
                                                        next_roots2=dev[i + 2][0] if i + 2 < case.steps else None))
        got = [float(v) for v in got.cpu()]
        after = _snapshot(eng, plan, model)
        assert not plan.wide
    _check_losses(name, got, r64, r32)
    _check_state(name, after[0], after[1], r64, r32)


# ---- a label outside [0, width) -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_failed_batch_trains_nothing_and_halts_until_resume(eng):
    """label == width -> NaN, nothing moves; a good batch behind it, no resume() -> NaN, nothing moves (the sticky halt);
    resume(), the same good batch -> the float64 trajectory that never saw the failed one: Adam at t = 1"""
    name = "failed_then_resumed"
    case = gc.CASES[name]
    state, batches = gc.setup(name)
    assert int(batches[0][1][gc.BAD_ROW]) == case.width
    r64, r32 = gc.reference(name)
    with _plan_of(eng, case, state) as (plan, model):
        start = _snapshot(eng, plan, model)
        bad, good = _dev(eng, batches)
        loss_bad = float(plan.step(*bad).clone())
        after_bad = _snapshot(eng, plan, model)
        loss_halted = float(plan.step(*good).clone())
        after_halted = _snapshot(eng, plan, model)
        plan.resume()
        loss_good = float(plan.step(*good).clone())
        after = _snapshot(eng, plan, model)
    assert loss_bad != loss_bad and loss_halted != loss_halted
    _assert_same_state(start, after_bad, "failed step")
    _assert_same_state(start, after_halted, "halted step")
    assert all(float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0 for m, v in after_halted[1].values())
    _check_losses(name, [loss_good], r64, r32)
    _check_first_step(name, after[1], r64, r32)
    _check_state(name, after[0], after[1], r64, r32)


# ---- a batch beyond the regular workspace -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_overflowing_batch_is_redone_after_growing(eng):
    """roots that are each other's sampled neighbours: step() reports NaN and moves nothing, step_checked() grows the plan
    (wide workspaces, Adam state adopted), clears nothing it should not, and redoes the batch: the float64 step"""
    name = "overflow_redone"
    case = gc.CASES[name]
    state, batches = gc.setup(name)
    assert not gc.fits(case, batches[0][2])
    r64, r32 = gc.reference(name)
    with _plan_of(eng, case, state) as (plan, model):
        start = _snapshot(eng, plan, model)
        (roots, labels), = _dev(eng, batches)
        first = float(plan.step(roots, labels).clone())
        assert first != first and not plan.wide
        _assert_same_state(start, _snapshot(eng, plan, model), "overflowed step")
        plan.resume()
        loss = plan.step_checked(roots, labels)
        after = _snapshot(eng, plan, model)
        assert plan.wide and plan.overflow_redone == 1
    _check_losses(name, [loss], r64, r32)
    _check_first_step(name, after[1], r64, r32)
    _check_state(name, after[0], after[1], r64, r32)


# ---- dropout from the plan's stream -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dropout_steps_against_the_restated_mask(eng):
    """TwoLayerGCN(is_training=True): p = 0.5 on h1.  The restatement drops dropout_ref.keep_mask(seed, step, 0, 0, n1, hid,
    0.5) by the oracle's local ids — it only agrees if the plan numbers its nodes as gigl_union_build does.  A step that
    fails (label == width) does not move the step counter: the batch after resume() sees the mask of the failed attempt's
    step, which the restatement's count of applied steps reproduces"""
    name = "dropout"
    case = gc.CASES[name]
    state, batches = gc.setup(name)
    r64, r32 = gc.reference(name)
    with _plan_of(eng, case, state) as (plan, model):
        assert plan._dropout == (gc.DROP_P, gc.DROP_SEED)
        dev = _dev(eng, batches)
        got = [float(plan.step(*dev[0]).clone())]
        # a failed attempt at the second batch, then its redo: the same step number, the same mask
        bad_labels = dev[1][1].clone()
        bad_labels[gc.BAD_ROW] = case.width
        failed = float(plan.step(dev[1][0], bad_labels).clone())
        assert failed != failed
        plan.resume()
        got += [float(plan.step(*dev[i]).clone()) for i in (1, 2)]
        after = _snapshot(eng, plan, model)
    _check_losses(name, got, r64, r32)
    _check_state(name, after[0], after[1], r64, r32)


@pytest.mark.gpu
def test_plan_refuses_what_it_does_not_compute(eng):
    from gigl_amd.engine import GcnTrainPlan
    from gigl_amd.models_attn import TwoLayerGCN
    eng.load_features(gc.features(24))
    eng._gcn_case_table = (24, False)
    with pytest.raises(NotImplementedError):
        GcnTrainPlan(eng, TwoLayerGCN(24, 7, should_l2_normalize_output=True).to(eng.device), 8, [5, 3])
    with pytest.raises(NotImplementedError):
        GcnTrainPlan(eng, TwoLayerGCN(20, 7).to(eng.device), 8, [5, 3])
    with pytest.raises(NotImplementedError):
        GcnTrainPlan(eng, TwoLayerGCN(24, 7).to(eng.device), 8, [5, 3, 2])


# ---- the CPU self-check -------------------------------------------------------------------------------------------------
def test_case_table_covers_what_it_claims():
    """from the parameters and the oracle's batches alone"""
    rowptr, col, loops, pairs = gc.graph()
    deg = np.diff(rowptr)
    assert loops.size >= 32 and int(deg[gc.N_RMAT:].max()) == 0 and gc.N_NODES - gc.N_RMAT == 8
    # some roots and some level-1 nodes of the ordinary batches store a self loop
    for name in ("base", "scalar_paths", "three_steps_decay", "dropout"):
        for _, _, u in gc.setup(name)[1]:
            n0, n1 = int(u["meta"][gc.META_LEVEL0]), int(u["meta"][gc.META_LEVEL0 + 1])
            sl = gc.stored_self_loops(u)
            assert sum(i < n0 for i in sl) >= gc.LOOP_ROOTS and sum(n0 <= i < n1 for i in sl) >= 2, (name, sl, n0, n1)
    # widths on both kernels' element paths and on the 2-float4 instantiation; an fp16 table; no bias tensors
    assert all(d % 4 for d in gc.CASES["scalar_paths"].dims) and gc.CASES["wide_input"].dims == (260, 16, 47)
    assert gc.CASES["fp16_table"].half and gc.features(24, True).dtype == np.float16
    assert sorted(gc.setup("no_bias")[0]) == ["conv1.lin.weight", "conv2.lin.weight"]
    # root rows beyond 64 edges
    u = gc.setup("long_rows")[1][0][2]
    n0 = int(u["meta"][gc.META_LEVEL0])
    assert int(np.diff(u["rowptr"])[:n0].max()) > 64 and int(np.diff(u["rowptr"])[:n0].min()) >= 65
    # roots without in-edges beside ordinary ones; one root in every slot; short batches
    r = gc.setup("isolated_roots")[1][0][0]
    assert (deg[r] == 0).sum() >= 6 and (deg[r] > 0).sum() >= 32
    r = gc.setup("one_root_everywhere")[1][0][0]
    assert r.size == 64 and len(set(r.tolist())) == 1
    assert [gc.setup(f"n_valid_{k}")[1][0][0].size for k in (1, 63)] == [1, 63] and gc.CASES["n_valid_1"].b == 64
    # the failed batch, the overflowing one, the dropout mask's rows
    assert gc.CASES["failed_then_resumed"].bad == (0, 7) and len(gc.reference("failed_then_resumed")[0].losses) == 1
    u = gc.setup("overflow_redone")[1][0][2]
    c = gc.CASES["overflow_redone"]
    assert int(u["meta"][gc.META_LEVEL0 + 1]) > gc.level_rows_cap(c.b, c.fan, 1)
    assert gc.CASES["dropout"].dropout and gc.CASES["dropout"].steps == 3
    keep = gc.keep_mask(gc.DROP_SEED, 0, 0, 0, 16, 32, gc.DROP_P)
    assert 0.3 < keep.mean() < 0.7 and not np.array_equal(keep, gc.keep_mask(gc.DROP_SEED, 1, 0, 0, 16, 32, gc.DROP_P))
    # the restatement against an independent formula: dense A_hat of the base batch
    state, ((roots, labels, u),) = gc.setup("base")
    nn = int(u["meta"][gc.META_N_NODES])
    a = np.zeros((nn, nn))
    rp, cl = u["rowptr"], u["col"]
    dg = np.array([1 + sum(int(j) != i for j in cl[rp[i]:rp[i + 1]]) for i in range(nn)], dtype=np.float64)
    for i in range(nn):
        a[i, i] += 1.0 / dg[i]
        for j in cl[rp[i]:rp[i + 1]]:
            if int(j) != i:
                a[i, j] += 1.0 / np.sqrt(dg[i] * dg[j])
    x = gc.features(24)[u["nodes"].astype(np.int64)].astype(np.float64)
    p = {k: v.double().numpy() for k, v in state.items()}
    h = np.maximum(a @ (x @ p["conv1.lin.weight"].T) + p["conv1.bias"], 0)
    z = (a @ (h @ p["conv2.lin.weight"].T) + p["conv2.bias"])[u["root_local"].astype(np.int64)]
    lse = np.log(np.exp(z - z.max(1, keepdims=True)).sum(1)) + z.max(1)
    loss = float((lse - z[np.arange(z.shape[0]), labels]).mean())
    assert abs(loss - gc.reference("base")[0].losses[0]) <= 1e-12
