"""The host side of the in-plan evaluation, without a GPU: the eval_plan trainer argument, and NablpTrainPlan.eval_batch /
evaluate over a fake library — what they pad, what they pass, how the accumulators become metrics, and the redo of a pass
that overflowed a regular plan's workspace."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from gigl_amd._lib import (LP_EVAL_BATCHES, LP_EVAL_HITS0, LP_EVAL_LEN, LP_EVAL_LOSS_SUM, LP_EVAL_MRR_SUM,
                           LP_EVAL_RANK_NODES, MODE_SPARK_HASH)


def test_eval_plan_argument_parses():
    from gigl_amd.nablp_spec import HipNodeAnchorLinkPredictionSpec
    assert HipNodeAnchorLinkPredictionSpec()._eval_in_plan()
    assert HipNodeAnchorLinkPredictionSpec(eval_plan="auto")._eval_in_plan()
    assert HipNodeAnchorLinkPredictionSpec(eval_plan="on")._eval_in_plan()
    assert not HipNodeAnchorLinkPredictionSpec(eval_plan="off")._eval_in_plan()
    assert not HipNodeAnchorLinkPredictionSpec(eval_plan="OFF")._eval_in_plan()
    with pytest.raises(ValueError):
        HipNodeAnchorLinkPredictionSpec(eval_plan="sometimes")._eval_in_plan()


class _FakeLib:
    """gigl_nablp_train_plan_eval as the library documents it, on host memory: records its arguments, adds fixed amounts"""

    def __init__(self, b, P, n_rn, overflow_on=()):
        self.b, self.P, self.n_rn, self.overflow_on = b, P, n_rn, set(overflow_on)
        self.calls = []

    def gigl_nablp_train_plan_eval(self, plan, main, cnt, rn, seed, mode, ks, n_ks, acc, overflow):
        rd = lambda p, n: list((C.c_int32 * n).from_address(p.value))
        i = len(self.calls)
        self.calls.append(dict(plan=plan, main=rd(main, self.b * (1 + self.P)), cnt=rd(cnt, self.b), rn=rd(rn, self.n_rn),
                               seed=seed, mode=mode, ks=list(ks)[:n_ks]))
        if i in self.overflow_on:
            (C.c_int32 * 1).from_address(overflow.value)[0] += 1
            return 0
        a = (C.c_double * LP_EVAL_LEN).from_address(acc.value)
        ranked = sum(1 for c in self.calls[-1]["cnt"] if c > 0)
        a[LP_EVAL_LOSS_SUM] += 0.5 * (len(self.calls[-1]["rn"]) - self.calls[-1]["rn"].count(-1))
        a[LP_EVAL_BATCHES] += 1
        a[LP_EVAL_MRR_SUM] += 0.25 * ranked
        a[LP_EVAL_RANK_NODES] += ranked
        for k in range(n_ks):
            a[LP_EVAL_HITS0 + k] += ranked * (k + 1) / 8.0
        return 0


def _plan(lib, b, P, n_rn):
    from gigl_amd.engine import NablpTrainPlan
    plan = object.__new__(NablpTrainPlan)
    plan.eng = SimpleNamespace(device=torch.device("cpu"), _ctx=None)
    plan._lib, plan._plan, plan.b, plan.P, plan.n_rn, plan.wide = lib, 7, b, P, n_rn, False
    return plan


def _batches():
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    # b = 4 anchors x (1 + 2) roots, 5 negatives: a full batch, and a short one (3 anchors, 2 negatives)
    full = (i32([10, 11, 12, 20, 21, 20, 30, 30, 30, 40, 41, 42]), i32([2, 1, 0, 2]), i32([1, 2, 3, 4, 5]))
    short = (i32([50, 51, 50, 60, 60, 60, 70, 71, 72]), i32([1, 0, 2]), i32([6, 7]))
    return [full, short]


def test_evaluate_pads_as_step_does_and_divides_in_double():
    lib = _FakeLib(4, 2, 5)
    plan = _plan(lib, 4, 2, 5)
    got = plan.evaluate(_batches(), ks=[1, 5, 10], sampling_seed=9, mode=MODE_SPARK_HASH)
    assert len(lib.calls) == 2 and all(c["plan"] == 7 and c["seed"] == 9 and c["mode"] == MODE_SPARK_HASH and
                                       c["ks"] == [1, 5, 10] for c in lib.calls)
    assert lib.calls[0]["main"] == [10, 11, 12, 20, 21, 20, 30, 30, 30, 40, 41, 42] and lib.calls[0]["cnt"] == [2, 1, 0, 2]
    assert lib.calls[0]["rn"] == [1, 2, 3, 4, 5]
    # the short batch: absent anchors and negatives are 0xFFFFFFFF (-1 as int32) with no positives
    assert lib.calls[1]["main"] == [50, 51, 50, 60, 60, 60, 70, 71, 72, -1, -1, -1] and lib.calls[1]["cnt"] == [1, 0, 2, 0]
    assert lib.calls[1]["rn"] == [6, 7, -1, -1, -1]
    # accumulators -> metrics: loss sum (2.5 + 1.0) / 2 batches; 3 + 2 ranked anchors
    assert got["batches"] == 2 and got["rank_nodes"] == 5 and plan.eval_overflowed == 0 and not plan.wide
    assert got["loss"] == (2.5 + 1.0) / 2
    assert got["mrr"] == 0.25 and got["hits"] == [1 / 8.0, 2 / 8.0, 3 / 8.0]
    assert all(isinstance(v, float) for v in (got["loss"], got["mrr"], *got["hits"]))


def test_evaluate_of_nothing_and_of_anchors_without_positives_is_zero():
    lib = _FakeLib(4, 2, 5)
    plan = _plan(lib, 4, 2, 5)
    assert plan.evaluate([], ks=[1]) == {"loss": 0.0, "mrr": 0.0, "hits": [0.0], "batches": 0, "rank_nodes": 0}
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    got = plan.evaluate([(i32([1, 1, 1]), i32([0]), i32([2]))], ks=[1, 5])
    assert got == {"loss": 0.5, "mrr": 0.0, "hits": [0.0, 0.0], "batches": 1, "rank_nodes": 0}


def test_evaluate_grows_the_plan_and_redoes_the_pass():
    lib = _FakeLib(4, 2, 5, overflow_on={1})  # the second call of the first pass overflows
    plan = _plan(lib, 4, 2, 5)
    grown = []

    def grow():
        grown.append(len(lib.calls))
        plan.wide = True
    plan.grow = grow
    got = plan.evaluate(_batches(), ks=[1, 5, 10])
    assert grown == [2] and plan.overflow_redone == 1 and len(lib.calls) == 4  # the whole pass again, after growing
    assert got["batches"] == 2 and got["rank_nodes"] == 5 and got["loss"] == (2.5 + 1.0) / 2 and plan.eval_overflowed == 0
    # a wide plan does not grow again: the batch is left out and counted
    lib2 = _FakeLib(4, 2, 5, overflow_on={0})
    wide = _plan(lib2, 4, 2, 5)
    wide.wide = True
    wide.grow = lambda: pytest.fail("a wide plan must not grow")
    got = wide.evaluate(_batches(), ks=[1])
    assert len(lib2.calls) == 2 and wide.eval_overflowed == 1 and got["batches"] == 1 and got["loss"] == 1.0
