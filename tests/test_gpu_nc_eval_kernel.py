"""gigl_nc_eval_metrics (csrc/loss.hip: nc_eval_rows_kernel + nc_eval_sum_kernel — the prediction, its comparison with the
label and the cross-entropy of every row, summed into a small fp64 accumulator on the device) through
HipEngine.nc_eval_metrics against torch on the same device rows; reference and inputs: tests/nc_eval_cases.py.

Predictions and the CORRECT / EVALUATED / LOSS_ROWS / CALLS / SKIPPED words are compared exactly.  The loss sum is compared
with the float64 logsumexp at the project's bar for a loss, rtol 1e-4 / atol 1e-5.  Measured on gfx950 (MI355X), the
largest |loss sum - float64| / |float64| over the 75 comparisons below: 4.1e-8 (width 260, two NaN rows left out); with the
logits shifted by +-1e4 1.7e-8 — the kernel subtracts the maximum from the label's logit before it adds log(sum), so
nothing of size 1e4 is rounded.  A row holding NaN with a label inside it makes the loss sum NaN on both sides."""
import ctypes as C
import math

import pytest
import torch

import nc_eval_cases as nc
from gigl_amd._lib import (NC_EVAL_CALLS, NC_EVAL_CORRECT, NC_EVAL_EVALUATED, NC_EVAL_LEN, NC_EVAL_LOSS_ROWS, NC_EVAL_LOSS_SUM,
                           NC_EVAL_SKIPPED)

WIDTHS = [1, 2, 3, 4, 5, 7, 47, 63, 64, 65, 128, 255, 256, 257, 1000]
NS = [0, 1, 3, 4, 5, 255, 256, 257, 1025]


@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _acc(eng):
    return torch.zeros(NC_EVAL_LEN, dtype=torch.float64, device=eng.device)


def _call(eng, rows, labels, acc, **kw):
    """rows / labels: device tensors (rows may be a strided or offset view)"""
    torch.cuda.synchronize()  # (the inputs were written on torch's stream, the call runs on the engine's)
    eng.nc_eval_metrics(rows, labels, acc, **kw)
    eng.synchronize()
    return acc.cpu().tolist()


def _check(a, ref, calls=1, what=""):
    """a: the accumulator's words after `calls` calls that each added `ref`"""
    _, correct, evaluated, loss_sum, loss_rows = ref
    got = a[NC_EVAL_LOSS_SUM]
    rel = abs(got - calls * loss_sum) / max(abs(calls * loss_sum), 1e-300) if math.isfinite(loss_sum) else float("nan")
    print(f"{what}: loss sum {got!r} against float64 {calls * loss_sum!r} (relative {rel:.3e}), correct {a[NC_EVAL_CORRECT]} "
          f"of {a[NC_EVAL_EVALUATED]}, loss rows {a[NC_EVAL_LOSS_ROWS]}")
    assert a[NC_EVAL_CORRECT] == calls * correct and a[NC_EVAL_EVALUATED] == calls * evaluated
    assert a[NC_EVAL_LOSS_ROWS] == calls * loss_rows and a[NC_EVAL_CALLS] == calls and a[NC_EVAL_SKIPPED] == 0
    assert a[6] == 0 and a[7] == 0
    if math.isnan(loss_sum):
        assert math.isnan(got)
    else:
        assert abs(got - calls * loss_sum) <= nc.LOSS_ATOL + nc.LOSS_RTOL * abs(calls * loss_sum)


def _run_and_check(eng, rows, labels, what, **kw):
    """one call over device rows / labels, predictions included"""
    n = labels.numel()
    pred = torch.full((n + 1,), -7, dtype=torch.int64, device=eng.device)
    a = _call(eng, rows, labels, _acc(eng), pred_out=pred, **kw)
    sel = rows if kw.get("row_index") is None else rows[kw["row_index"].long()]
    ref = nc.reference(sel[:n], labels)
    assert torch.equal(pred[:n].cpu(), ref[0]) and int(pred[n]) == -7, what
    _check(a, ref, what=what)
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_every_width_against_torch(eng, width):
    rows, labels = nc.random_rows(37, width, seed=width)
    _run_and_check(eng, rows.to(eng.device), labels.to(eng.device), f"width {width}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("width", [7, 64])
def test_every_row_count_against_torch(eng, n, width):
    rows, labels = nc.random_rows(max(n, 1), width, seed=1000 + n)
    a = _run_and_check(eng, rows.to(eng.device), labels[:n].to(eng.device), f"n {n} width {width}")
    assert a[NC_EVAL_EVALUATED] == n and a[NC_EVAL_CALLS] == 1  # (n == 0: a call, nothing else)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [7, 8, 47, 64])
def test_row_index_stride_and_offset_base(eng, width):
    dev = eng.device
    rows, labels = nc.random_rows(40, width, seed=5)
    # row_index: a permutation with one row repeated
    g = torch.Generator().manual_seed(9)
    idx = torch.randperm(40, generator=g).to(torch.int32)
    idx[7] = idx[3]
    _run_and_check(eng, rows.to(dev), labels.to(dev), f"row_index width {width}", row_index=idx.to(dev))
    # rows `width + 4` (16-byte path kept) and `width + 3` floats apart
    for pad in (4, 3):
        wide = torch.full((40, width + pad), 1e9, dtype=torch.float32)  # (what lies between the rows must never be read)
        wide[:, :width] = rows
        _run_and_check(eng, wide.to(dev)[:, :width], labels.to(dev), f"stride width + {pad}, width {width}")
    # the base one float into a buffer: no row starts on a 16-byte boundary -> the element path
    flat = torch.full((40 * width + 1,), 1e9, dtype=torch.float32)
    flat[1:] = rows.reshape(-1)
    view = flat.to(dev)[1:].view(40, width)
    assert view.data_ptr() % 16 == 4
    _run_and_check(eng, view, labels.to(dev), f"offset base width {width}")


@pytest.mark.gpu
@pytest.mark.parametrize("width", [2, 5, 8, 64, 65, 132, 257, 1000])
def test_ties_take_the_first_index(eng, width):
    rows, first = nc.tie_rows(width)
    for offset in (False, True):  # (the 16-byte path where the width allows it, and the element path)
        dev_rows = rows.to(eng.device)
        if offset:
            flat = torch.zeros(rows.numel() + 1, dtype=torch.float32, device=eng.device)
            flat[1:] = dev_rows.reshape(-1)
            dev_rows = flat[1:].view(rows.shape)
        pred = torch.empty(rows.shape[0], dtype=torch.int64, device=eng.device)
        a = _call(eng, dev_rows, first.to(eng.device), _acc(eng), pred_out=pred)
        assert torch.equal(pred.cpu(), first), (width, offset)
        assert torch.equal(pred.cpu(), torch.argmax(dev_rows, dim=1).cpu())
        assert a[NC_EVAL_CORRECT] == rows.shape[0] == a[NC_EVAL_EVALUATED]


@pytest.mark.gpu
@pytest.mark.parametrize("width", [3, 7, 64, 260])
def test_infinities_shifts_nan_and_labels_outside(eng, width):
    dev = eng.device
    rows, labels = nc.random_rows(12, width, seed=21)
    # rows of -inf except one entry: the loss of its own label is 0, of another label +inf is not produced here
    for i in range(4):
        keep = (5 * i + 2) % width
        v = rows[i, keep].clone()
        rows[i] = float("-inf")
        rows[i, keep] = v
        labels[i] = keep
    a = _run_and_check(eng, rows.to(dev), labels.to(dev), f"-inf rows width {width}")
    assert math.isfinite(a[NC_EVAL_LOSS_SUM])
    # logits far from zero: logsumexp stays finite and exact
    base, lab = nc.random_rows(12, width, seed=22)
    for shift in (1e4, -1e4):
        a = _run_and_check(eng, (base + shift).to(dev), lab.to(dev), f"shift {shift:+.0e} width {width}")
        assert math.isfinite(a[NC_EVAL_LOSS_SUM])
    # labels -1 and width: evaluated, not correct, no loss
    out = lab.clone()
    out[1], out[4], out[7] = -1, width, -1
    a = _run_and_check(eng, base.to(dev), out.to(dev), f"labels outside width {width}")
    assert a[NC_EVAL_EVALUATED] == 12 and a[NC_EVAL_LOSS_ROWS] == 9
    # a NaN in the middle of a row: the row predicts its first NaN; its loss is NaN unless its label lies outside
    nan = base.clone()
    nan[3, width // 2] = float("nan")
    nan[6, width // 2] = float("nan")
    nan[6, width - 1] = float("nan")
    pred = torch.empty(12, dtype=torch.int64, device=dev)
    lab_nan = lab.clone()
    lab_nan[3], lab_nan[6] = width, width // 2
    a = _call(eng, nan.to(dev), lab_nan.to(dev), _acc(eng), pred_out=pred)
    ref = nc.reference(nan.to(dev), lab_nan.to(dev))
    assert int(pred[3]) == width // 2 == int(pred[6]) and torch.equal(pred.cpu(), ref[0])
    _check(a, ref, what=f"nan width {width}")
    assert math.isnan(a[NC_EVAL_LOSS_SUM]) and a[NC_EVAL_LOSS_ROWS] == 11
    lab_nan[6] = -1  # both NaN rows outside: the sum is finite again
    _check(_call(eng, nan.to(dev), lab_nan.to(dev), _acc(eng)), nc.reference(nan.to(dev), lab_nan.to(dev)), what="nan rows outside")


@pytest.mark.gpu
def test_calls_add_up_repeat_bit_for_bit_and_skip(eng):
    dev = eng.device
    r1, l1 = nc.random_rows(300, 47, seed=31)
    r2, l2 = nc.random_rows(1025, 47, seed=32)
    r1, l1, r2, l2 = r1.to(dev), l1.to(dev), r2.to(dev), l2.to(dev)
    ref1, ref2 = nc.reference(r1, l1), nc.reference(r2, l2)
    acc = _acc(eng)
    a1 = _call(eng, r1, l1, acc)
    _check(a1, ref1, what="first call")
    a12 = _call(eng, r2, l2, acc)
    b2 = _call(eng, r2, l2, _acc(eng))
    _check(b2, ref2, what="second call alone")
    assert a12[NC_EVAL_CORRECT] == ref1[1] + ref2[1] and a12[NC_EVAL_EVALUATED] == 1325 and a12[NC_EVAL_CALLS] == 2
    assert a12[NC_EVAL_LOSS_ROWS] == 1325 and a12[NC_EVAL_LOSS_SUM] == a1[NC_EVAL_LOSS_SUM] + b2[NC_EVAL_LOSS_SUM]
    # the same inputs again: the same bits
    again = _acc(eng)
    _call(eng, r1, l1, again)
    assert _call(eng, r2, l2, again) == a12
    # skip_flag: NULL and 0 run the call, non-zero counts a skipped call and touches nothing else
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    seven = torch.full((1,), 7, dtype=torch.int32, device=dev)
    assert _call(eng, r2, l2, _acc(eng), skip_flag=zero) == b2
    pred = torch.full((1025,), -7, dtype=torch.int64, device=dev)
    acc = _acc(eng)
    acc[NC_EVAL_CORRECT] = 3.0
    s = _call(eng, r2, l2, acc, skip_flag=seven, pred_out=pred)
    assert s[NC_EVAL_SKIPPED] == 1 and s[NC_EVAL_CORRECT] == 3 and sum(s) == 4 and bool((pred == -7).all())
    s = _call(eng, r2[:1], l2[:0], acc, skip_flag=seven)  # (an empty call is skipped the same way)
    assert s[NC_EVAL_SKIPPED] == 2 and s[NC_EVAL_CALLS] == 0
    s = _call(eng, r1, l1, acc, skip_flag=zero)
    assert s[NC_EVAL_SKIPPED] == 2 and s[NC_EVAL_CALLS] == 1 and s[NC_EVAL_CORRECT] == 3 + ref1[1]


@pytest.mark.gpu
def test_invalid_arguments_launch_nothing(eng):
    dev = eng.device
    rows, labels = nc.random_rows(8, 5, seed=41)
    rows, labels, acc = rows.to(dev), labels.to(dev), _acc(eng)
    p = lambda t: C.c_void_p(t.data_ptr())
    f = eng._lib.gigl_nc_eval_metrics
    torch.cuda.synchronize()
    bad = [
        (p(rows), 0, 5, None, p(labels), 8, None, p(acc), None),    # width < 1
        (p(rows), -3, 5, None, p(labels), 8, None, p(acc), None),
        (p(rows), 5, 5, None, p(labels), -1, None, p(acc), None),   # a negative n
        (None, 5, 5, None, p(labels), 8, None, p(acc), None),       # null rows / labels / acc
        (p(rows), 5, 5, None, None, 8, None, p(acc), None),
        (p(rows), 5, 5, None, p(labels), 8, None, None, None),
    ]
    for args in bad:
        assert f(eng._ctx, *args) == -1  # GIGL_E_INVALID_ARG
        assert eng._lib.gigl_last_error(eng._ctx)
    assert f(None, p(rows), 5, 5, None, p(labels), 8, None, p(acc), None) == -1
    eng.synchronize()
    assert acc.cpu().tolist() == [0.0] * NC_EVAL_LEN  # nothing ran
    assert f(eng._ctx, p(rows), 5, 5, None, p(labels), 8, None, p(acc), None) == 0
    eng.synchronize()
    assert acc.cpu().tolist()[NC_EVAL_CALLS] == 1
