"""The node-classification training step (gigl_sage_train_plan_*, csrc/pipeline.hip) against a FLOAT64 restatement at the
shapes where the kernels that exist only inside it take another path: ce_roots_kernel / ce_root_row (class widths on either
side of one, two and three trips of the 64-lane stride, repeated real roots that share a dout row, short batches, roots
without in-edges, logits of +-75), loss_sum_kernel and the halt / resume bookkeeping (labels outside the width),
train_stage_kernel (one, three and four layers: zero, two and three W_l^T of their own shapes), relu_mask_kernel on the
loss's own dout, adam_kernel<false> past one pass of its grid and without bias entries, chunk_sum at 1, 15, 16, 17 and 33
chunks.  Everything goes through engine.SageTrainPlan; cases, batches and references: tests/train_step_cases.py.

With weight_decay = 0 the first step leaves exp_avg = (1 - beta1) g: plan.moments() hands out the step's raw gradient of
every tensor to one fp32 rounding — the pin on ce_roots_kernel's dout and, through it, on the backward chain.

Bounds.  Per tensor and case the larger of the project's bar against the CPU restatement (loss: rtol 1e-4 / atol 1e-5;
first-step gradients: rtol 1e-4 with atol 1e-4 max|want|; moments and determined parameters: 1e-4 through
helpers.assert_adam_state) and 4 x the error of the float32 CPU restatement of the same case against float64.  Unchanged
state after a failed or halted step, the width-1 case and the NaN-ness of failed losses are exact.

Measured on an MI355X (worst per class of case; err = plan against float64, fp32 = the float32 restatement against
float64; losses absolute, parameters absolute on the determined set, everything else relative to the tensor's largest).
exp_avg_sq sits at 1.3e-5 everywhere: adam_kernel takes beta2 as the fp32 0.999 (1 - beta2 is 1.29e-5 short of 0.001) in the
moment and, consistently, in the bias correction — the parameters agree to 1e-8 after one step.

    class of case                      quantity           err       fp32
    A.1 widths, fp16 table             loss           3.0e-07    3.9e-07
    A.1 widths, fp16 table             grad           4.6e-07    8.8e-07
    A.1 widths, fp16 table             exp_avg_sq     1.3e-05    1.6e-06
    A.2 repeated roots                 loss           3.3e-07    3.3e-07
    A.2 repeated roots                 grad           3.6e-06    1.8e-06
    A.2 repeated roots                 exp_avg_sq     1.3e-05    2.2e-06
    A.3 short batches                  loss           1.8e-07    5.9e-08
    A.3 short batches                  grad           4.4e-07    6.0e-07
    A.3 short batches                  exp_avg_sq     1.3e-05    1.2e-06
    A.4 roots without in-edges         loss           5.8e-08    5.8e-08
    A.4 roots without in-edges         grad           3.4e-07    5.5e-07
    A.4 roots without in-edges         exp_avg_sq     1.3e-05    9.1e-07
    A.5 logits of +-75                 loss           2.3e-06    5.3e-06
    A.5 logits of +-75                 grad           1.3e-06    6.1e-07
    A.5 logits of +-75                 exp_avg_sq     1.4e-05    1.2e-06
    D.2 chunk counts                   loss           1.6e-07    2.2e-07
    D.2 chunk counts                   grad           1.1e-06    7.2e-07
    D.2 chunk counts                   exp_avg_sq     1.4e-05    9.9e-07
    B.1-3 failed, resumed              loss           1.5e-07    9.2e-08
    B.1-3 failed, resumed              grad           2.9e-07    3.4e-07
    B.1-3 failed, resumed              exp_avg_sq     1.3e-05    6.5e-07
    B.1-3 failed, resumed              exp_avg        2.9e-07    3.3e-07
    B.1-3 failed, resumed              param          8.1e-09    8.9e-09
    B.4 failed in a queue              loss           9.0e-08    1.7e-07
    B.4 failed in a queue              exp_avg        6.8e-07    3.9e-07
    B.4 failed in a queue              exp_avg_sq     1.3e-05    5.8e-07
    B.4 failed in a queue              param          1.7e-07    6.3e-08
    C 1 / 3 / 4 layers                 loss           2.2e-07    2.2e-07
    C 1 / 3 / 4 layers                 exp_avg        2.4e-06    9.1e-07
    C 1 / 3 / 4 layers                 exp_avg_sq     1.4e-05    1.1e-06
    C 1 / 3 / 4 layers                 param          8.1e-06    5.4e-07
    D.1 30 steps                       loss           1.3e-06    1.1e-06
    D.1 30 steps                       exp_avg        2.7e-06    1.8e-06
    D.1 30 steps                       exp_avg_sq     1.3e-05    1.2e-06
    D.1 30 steps                       param          6.0e-07    1.5e-06
    D.1 30 steps, tail group           exp_avg        4.5e-07    6.7e-07
    D.1 30 steps, tail group           exp_avg_sq     1.3e-05    6.3e-07
    D.1 30 steps, tail group           param          2.1e-07    2.3e-07

Which case names a slip (reasoned from the code):
  * `c += 64` -> `c += 128` in a loop of ce_root_row: in the sum or the gradient loop width_65 .. width_200 and the
    130-wide cases (columns 64..127 drop out; labels sit on column 64 and width-1); in the max loop peak_column_100 alone
    (a smaller shift gives the same log-sum-exp until exp overflows: there the loss is inf); widths <= 64 cannot see it
  * the atomicAdd of ce_root_row -> a plain store: repeat_2, repeat_3, repeat_64 (the copies' gradients must add up)
  * `*step += 1` above the overflow check of loss_sum_kernel: failed_m1 / failed_width / failed_2p40 (the batch after
    resume() would run at t = 2: its displacement is 0.74 lr, not lr) and failed_in_queue
  * rows and cols of `pa` entry 1 swapped: layers_3* (entry 1 is the last layer's 9 x 60) and layers_4 (its 30 x 60): the
    W^T of that layer is scrambled and with it the gradient of everything below
  * the tail loop of chunk_sum dropped: every case whose chunk count is no multiple of 16 — chunks_15, chunks_17, chunks_33
    and the 1..12-chunk layers of all the others (chunks_16 alone would pass)
  * the grid-stride loop of adam_kernel capped at one pass: adam_two_passes, its "W_0 from flat index 53248" group
"""
import contextlib

import numpy as np
import pytest
import torch

import train_step_cases as tc
from helpers import adam_state_errors, assert_adam_state

LOSS_RTOL, LOSS_ATOL, GRAD_TOL, STATE_TOL, FP32_FACTOR = 1e-4, 1e-5, 1e-4, 1e-4, 4.0


# ---- the device side ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    rowptr, col = tc.graph()
    e = HipEngine(0)
    e.load_csc(rowptr, col)
    e._train_step_table = None
    yield e
    e.close()


@contextlib.contextmanager
def _plan_of(eng, case, state):
    """the case's plan on a stream of its own, over the case's feature table (the engine keeps the last one loaded)"""
    from gigl_amd.engine import SageTrainPlan
    from gigl_amd.models import GraphSAGE
    key = (case.dims[0], case.half)
    if eng._train_step_table != key:
        eng.load_features(tc.features(*key))
        eng._train_step_table = key
    model = GraphSAGE(case.dims[0], case.dims[1], case.dims[2], num_layers=case.L, activation_after_last_conv=case.act_last,
                      bias=case.bias)
    model.load_state_dict(state)
    model = model.to(eng.device)
    st = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    plan = SageTrainPlan(eng, model, case.b, list(case.fan), lr=case.lr, weight_decay=case.wd, betas=(tc.BETA1, tc.BETA2),
                         eps=tc.ADAM_EPS)
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
    for k, want in r64.grads0.items():
        m, v = (t.double() for t in moments[k])
        big = float(want.abs().max())
        d = (m / (1.0 - tc.BETA1) - want).abs()
        e32 = float((r32.grads0[k].double() - want).abs().max())
        print(f"{label} grad {k}: err={float(d.max()) / max(big, 1e-300):.3e} fp32={e32 / max(big, 1e-300):.3e}")
        bound = torch.clamp(GRAD_TOL * want.abs() + GRAD_TOL * big, min=FP32_FACTOR * e32)
        assert bool((d <= bound).all()), (label, k, float(d.max()), big, e32)
        v64, v32 = r64.moments[k][1], r32.moments[k][1].double()
        vbig = float(v64.max())
        ev, ev32 = float((v - v64).abs().max()) / max(vbig, 1e-300), float((v32 - v64).abs().max()) / max(vbig, 1e-300)
        print(f"{label} exp_avg_sq {k}: err={ev:.3e} fp32={ev32:.3e}")
        assert ev <= max(STATE_TOL, FP32_FACTOR * ev32), (label, k, ev, ev32)


def _check_state(label, params, moments, r64, r32):
    """Adam's moments and the determined parameters of every tensor, through helpers.assert_adam_state"""
    e32 = adam_state_errors(r32.params, r32.moments, r64.params, r64.moments)
    got = adam_state_errors(params, moments, r64.params, r64.moments)
    for k in r64.moments:
        for what, i in (("exp_avg", 0), ("exp_avg_sq", 1), ("param", 2)):
            print(f"{label} {what} {k}: err={got[k][i]:.3e} fp32={e32[k][i]:.3e}")
        tol = [max(STATE_TOL, FP32_FACTOR * e32[k][i]) for i in range(3)]
        assert_adam_state(f"{label} {k}", {k: params[k]}, {k: moments[k]}, {k: r64.params[k]}, {k: r64.moments[k]}, *tol)


# ---- A (and D.2): the loss kernel, first step, weight_decay = 0 ---------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", tc.LOSS_CASES)
def test_first_step_loss_and_gradients_against_float64(eng, name):
    case = tc.CASES[name]
    assert case.wd == 0.0 and case.steps == 1
    state, batches = tc.setup(name)
    r64, r32 = tc.reference(name)
    if case.logits > 0:
        assert 60.0 <= float(r64.logits0.abs().max()) <= 90.0
    with _plan_of(eng, case, state) as (plan, model):
        start = _snapshot(eng, plan, model)
        (roots, labels), = _dev(eng, batches)
        loss = float(plan.step(roots, labels).clone())
        after = _snapshot(eng, plan, model)
        assert not plan.wide
    if case.width == 1:  # one class: the loss is exactly 0, the gradient exactly 0, nothing moves
        assert loss == 0.0 and r64.losses == [0.0]
        _assert_same_state(start, after, name)
        return
    _check_losses(name, [loss], r64, r32)
    _check_first_step(name, after[1], r64, r32)


# ---- B: labels outside [0, width) ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(tc.BAD_LABELS))
def test_failed_batch_trains_nothing_and_halts_until_resume(eng, kind):
    """bad batch -> NaN, nothing moves; a good batch behind it, no resume() -> NaN, nothing moves (the sticky halt); resume(),
    the same good batch -> the float64 trajectory that never saw the failed ones: Adam at t = 1"""
    name = f"failed_{kind}"
    case = tc.CASES[name]
    state, batches = tc.setup(name)
    assert int(batches[0][1][tc.BAD_ROW]) == tc.BAD_LABELS[kind] and not 0 <= tc.BAD_LABELS[kind] < case.width
    r64, r32 = tc.reference(name)
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
    # the first step's displacement lr g / (|g| + eps') at t = 1 (a counter moved by a failed batch gives 0.74 lr where
    # the gradient decides the direction), on the determined set of every tensor
    for k, p0 in start[0].items():
        rms = r64.moments[k][1].sqrt()
        det = rms >= 1e-3 * rms.max()
        want = (state[k].double() - r64.params[k])[det] / case.lr
        got = (p0.double() - after[0][k].double())[det] / case.lr
        err = float((got - want).abs().max())
        print(f"{name} displacement/lr {k}: err={err:.3e} (|want| {float(want.abs().min()):.4f} .. {float(want.abs().max()):.4f})")
        # (d [g / (|g| + eps)] / dg <= eps / g^2 = 100 at the determined set's smallest |g| ~ 1e-5, times a gradient error of
        # 1e-4 max|g| ~ 1e-6; one fp32 rounding of a parameter of ~0.2 is 1.5e-6 lr)
        assert err <= 1e-3, (name, k, err)


@pytest.mark.gpu
@pytest.mark.parametrize("wide_first", [True, False])
def test_run_steps_skips_the_failed_batch_of_a_queue(eng, wide_first):
    """five batches issued without a host read, the third with a label == width, every step announcing the next roots: its
    loss is NaN, the other four and the final state are the float64 trajectory without it.  A plan that is not wide yet grows
    first (the failure could have been its workspace's), then skips"""
    name = "failed_in_queue"
    case = tc.CASES[name]
    state, batches = tc.setup(name)
    r64, r32 = tc.reference(name)
    with _plan_of(eng, case, state) as (plan, model):
        if wide_first:
            plan.grow()
        dev = _dev(eng, batches)
        got = plan.run_steps(case.steps, lambda i: dict(roots=dev[i][0], labels=dev[i][1],
                                                        next_roots=dev[i + 1][0] if i + 1 < case.steps else None))
        got = [float(v) for v in got.cpu()]
        after = _snapshot(eng, plan, model)
        assert plan.wide and getattr(plan, "overflow_redone", 0) == (0 if wide_first else 1)
    assert got[case.bad[0]] != got[case.bad[0]]
    label = f"{name}[{'wide' if wide_first else 'grows'}]"
    _check_losses(label, [v for i, v in enumerate(got) if i != case.bad[0]], r64, r32)
    _check_state(label, after[0], after[1], r64, r32)


# ---- C: layer counts and optional tensors -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", tc.LAYER_CASES)
def test_layer_counts_and_optional_tensors_against_float64(eng, name):
    case = tc.CASES[name]
    state, batches = tc.setup(name)
    r64, r32 = tc.reference(name)
    with _plan_of(eng, case, state) as (plan, model):
        got = [float(plan.step(r, y).clone()) for r, y in _dev(eng, batches)]
        after = _snapshot(eng, plan, model)
        assert not plan.wide
    assert set(after[1]) == set(r64.moments) and (any(k.endswith("bias") for k in after[1]) == case.bias)
    _check_losses(name, got, r64, r32)
    _check_state(name, after[0], after[1], r64, r32)


# ---- D.1: the optimiser past one pass of its grid, at length ------------------------------------------------------------
@pytest.mark.gpu
def test_adam_beyond_one_pass_of_its_grid_over_thirty_steps(eng):
    name = "adam_two_passes"
    case = tc.CASES[name]
    state, batches = tc.setup(name)
    r64, r32 = tc.reference(name)
    with _plan_of(eng, case, state) as (plan, model):
        dev = _dev(eng, batches)
        got = []
        for i, (r, y) in enumerate(dev):  # (two steps out of three announce the next batch)
            nxt = dev[i + 1][0] if (i + 1 < len(dev) and i % 3 != 2) else None
            got.append(plan.step(r, y, next_roots=nxt).clone())
        got = [float(v) for v in got]
        after = _snapshot(eng, plan, model)
    _check_losses(name, got, r64, r32)
    _check_state(name, after[0], after[1], r64, r32)
    # the elements of the fused W_0 that only a second pass of the grid reaches, as a group of their own
    tail = lambda d: {"W_0 from flat index 53248": tc.fused(d, 0).reshape(-1)[tc.ADAM_GRID:]}
    tail_m = lambda mo: {"W_0 from flat index 53248": tuple(tc.fused({k: v[j] for k, v in mo.items()}, 0).reshape(-1)[tc.ADAM_GRID:]
                                                            for j in range(2))}
    _check_state(f"{name} tail", tail(after[0]), tail_m(after[1]),
                 tc.Run(None, None, None, tail(r64.params), tail_m(r64.moments), None),
                 tc.Run(None, None, None, tail(r32.params), tail_m(r32.moments), None))


# ---- the CPU self-check -------------------------------------------------------------------------------------------------
def _numpy_loss_and_dlogits(logits, labels):
    """log-sum-exp written out -> (mean loss, (softmax - onehot) / n per root slot)"""
    z = logits.astype(np.float64)
    mx = z.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(z - mx).sum(1))
    n = z.shape[0]
    g = np.exp(z - lse[:, None])
    g[np.arange(n), labels] -= 1.0
    return float((lse - z[np.arange(n), labels]).sum() / n), g / n


def test_reference_and_case_table_self_check():
    """the float64 restatement against an independent formula (A.1, A.2, A.5), and the case table covers what it claims —
    from the parameters and the oracle's batches alone"""
    from oracle import gnn_ref
    for name in [f"width_{w}" for w in tc.WIDTHS] + ["repeat_2", "repeat_3", "repeat_64", "large_logits_47", "large_logits_130",
                                                            "peak_column_100"]:
        case = tc.CASES[name]
        state, ((roots, labels, u),) = tc.setup(name)
        r64, _ = tc.reference(name)
        rl = u["root_local"].astype(np.int64)
        assert int(u["meta"][tc.META_LEVEL0]) == len(set(roots.tolist()))  # (the last layer's rows: the distinct roots)
        loss, g = _numpy_loss_and_dlogits(r64.logits0.numpy(), labels)
        assert abs(loss - r64.losses[0]) <= 1e-12, (name, loss, r64.losses[0])
        # d loss / d out: the slots' gradients ADDED onto their rows (repeated roots share one); the last layer's gradients
        # are its products with the layer's operand [mean(h) | h] and its column sums
        with torch.no_grad():
            p = {k: v.double() for k, v in state.items()}
            x = torch.from_numpy(tc.features(case.dims[0])[u["nodes"].astype(np.int64)]).double()
            ei = gnn_ref.union_edge_index(u["rowptr"], u["col"])
            h = torch.relu(gnn_ref.sage_conv(x, ei, p["conv_layers.0.lin_l.weight"], p["conv_layers.0.lin_l.bias"],
                                             p["conv_layers.0.lin_r.weight"]))
            mean = gnn_ref.scatter_mean(h[ei[0]], ei[1], h.shape[0]).numpy()
        dout = np.zeros((h.shape[0], case.width))
        np.add.at(dout, rl, g)
        for k, want in (("lin_l.weight", dout.T @ mean), ("lin_r.weight", dout.T @ h.numpy()), ("lin_l.bias", dout.sum(0))):
            assert np.abs(r64.grads0["conv_layers.1." + k].numpy() - want).max() <= 1e-12, (name, k)
    # A.1: the widths, and labels in every trip of the 64-lane stride
    assert [tc.CASES[f"width_{w}"].width for w in tc.WIDTHS] == [1, 2, 63, 64, 65, 128, 129, 200]
    for w in tc.WIDTHS:
        y = tc.setup(f"width_{w}")[1][0][1]
        assert 0 in y and w - 1 in y and (w <= 64 or 64 in y) and y.min() >= 0 and y.max() < w
        assert -(-w // tc.CE_LANES) == {1: 1, 2: 1, 63: 1, 64: 1, 65: 2, 128: 2, 129: 3, 200: 4}[w]
    # A.2: repeat counts, every copy its own label, the three-fold one not adjacent
    for name, copies in (("repeat_2", 2), ("repeat_3", 3), ("repeat_64", 64)):
        roots, labels, _ = tc.setup(name)[1][0]
        ids, cnt = np.unique(roots, return_counts=True)
        assert cnt.max() == copies and (cnt > 1).sum() == 1
        slots = np.nonzero(roots == ids[cnt.argmax()])[0]
        assert len(set(labels[slots].tolist())) == copies
        assert copies != 3 or np.diff(slots).min() > 1
    # A.3 / A.4
    assert [tc.setup(f"n_valid_{k}")[1][0][0].size for k in (1, 63, 64)] == [1, 63, 64] and tc.CASES["n_valid_1"].b == 64
    deg = np.diff(tc.graph()[0])
    r = tc.setup("isolated_roots")[1][0][0]
    assert (deg[r] == 0).sum() >= tc.N_ISOLATED and (deg[r] > 0).sum() >= 32
    # A.5: labels on the largest and on the smallest logit of their rows, logits in [60, 90]
    for name in ("large_logits_47", "large_logits_130"):
        z, y = tc.reference(name)[0].logits0.numpy(), tc.setup(name)[1][0][1]
        assert 60.0 <= np.abs(z).max() <= 90.0
        rows = np.arange(y.size)
        assert (z[rows, y] == z.max(1)).sum() >= 16 and (z[rows, y] == z.min(1)).sum() >= 16
        assert (z.max(1) - z[rows, y]).max() >= 100.0  # (exp(-100) underflows fp32's normal range: the label's probability)
    # ... and the column that alone decides every row's maximum, in the second trip, more than log(FLT_MAX) above the rest
    z = tc.reference("peak_column_100")[0].logits0.numpy()
    col = tc.CASES["peak_column_100"].peak[0]
    assert tc.CE_LANES <= col < 2 * tc.CE_LANES and 60.0 <= np.abs(z).max() <= 90.0 and (z.argmax(1) == col).all()
    assert (z[:, col] - np.delete(z, col, axis=1).max(1)).min() > 89.0 > np.log(np.finfo(np.float32).max)
    # B: the labels outside the width
    assert sorted(tc.BAD_LABELS.values()) == [-1, 7, 2 ** 40] and tc.CASES["failed_in_queue"].bad == (2, 7)
    assert len(tc.reference("failed_in_queue")[0].losses) == 4
    # C: W_l^T laid out per step, shapes that are not square and no multiple of 4, a pack without bias entries
    assert sorted({tc.CASES[n].n_t for n in tc.LAYER_CASES}) == [0, 2, 3]
    for n in tc.LAYER_CASES:
        c = tc.CASES[n]
        assert len(set(c.dims)) == 3 and all(d % 4 for d in c.dims) and c.steps == 3 and c.wd == 5e-4
    assert not tc.CASES["layers_3_no_bias"].bias and tc.CASES["layers_3_act_last"].act_last
    # D.1: W_0 does not fit one pass of the Adam grid, every other tensor does
    c = tc.CASES["adam_two_passes"]
    assert tc.ADAM_GRID == 53248 and c.dims[1] * 2 * c.dims[0] == 60000 > tc.ADAM_GRID and c.steps == 30
    assert c.dims[2] * 2 * c.dims[1] <= tc.ADAM_GRID
    # D.2: the chunk counts chunk_sum sees, over the cases of this file
    seen = set()
    for name in tc.LOSS_CASES + tc.LAYER_CASES:
        for _, _, u in tc.setup(name)[1]:
            seen.update(tc.chunk_counts(tc.CASES[name], u))
    assert {1, 15, 16, 17} <= seen and max(seen) >= 33, sorted(seen)
    for name, n in tc.CHUNK_TARGETS.items():
        got = tc.chunk_counts(tc.CASES[name], tc.setup(name)[1][0][2])[0]
        assert got == n or (name == "chunks_33" and got >= 33), (name, got)
