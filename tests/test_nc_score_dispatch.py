"""The host side of the node-classification score pass, without a GPU: the eval_plan trainer argument, and where the
validation / test passes go — ResidentGraph.score_roots (one host read per pass) on the in-HBM route of one process over a
replica graph when the model has a one-call plan, score() over _split_batches everywhere else (WORLD_SIZE > 1, a sharded
graph, no plan, the TFRecord route, eval_plan off, an encoder `auto` does not cover)."""
import numpy as np
import pytest
import torch


def _spec(**kw):
    from gigl_amd.task_specs import HipGraphSageNodeClassificationSpec
    return HipGraphSageNodeClassificationSpec(**kw)


def test_eval_plan_argument_is_checked():
    """an unknown value raises, as the link-prediction spec's does"""
    for bad in ("sometimes", "yes", "1", ""):
        with pytest.raises(ValueError, match="eval_plan must be auto, on or off"):
            _spec(eval_plan=bad)
    for ok, want in (("auto", "auto"), ("on", "on"), ("off", "off"), ("OFF", "off"), ("Auto", "auto")):
        assert _spec(eval_plan=ok)._eval_plan == want
    assert _spec()._eval_plan == "auto"


class _FakeResident:
    def __init__(self, world=1, sharded=False, answer=None):
        self.world, self.sharded, self.answer, self.calls = world, sharded, answer, []

    def score_roots(self, model, ids, labels, batch_size):
        self.calls.append((type(model).__name__, ids.tolist(), labels.tolist(), batch_size, model.training))
        return self.answer


SPLITS = {"val": (np.array([4, 9, 2], np.int64), np.array([1, 0, 2], np.int64)),
          "test": (np.array([7], np.int64), np.array([2], np.int64))}
ANSWER = {"correct": 2, "evaluated": 3, "loss": 0.7, "calls": 1, "redone": 0}


def _wired(monkeypatch, model, resident, hbm=True, **kw):
    """a spec whose data side is faked: _hbm_split hands out SPLITS (None: the TFRecord route), score() answers -1"""
    spec = _spec(main_sample_batch_size=2, **kw)
    spec.model = model
    spec._resident = resident
    monkeypatch.setattr(type(spec), "_hbm_split", lambda self, cfg: SPLITS if hbm else None)
    monkeypatch.setattr(type(spec), "_split_batches", lambda self, cfg, split: iter(()))
    old = []
    monkeypatch.setattr(type(spec), "score", lambda self, batches, device: old.append(1) or -1.0)
    return spec, old


def _sage():
    from gigl_amd.models import GraphSAGE
    return GraphSAGE(in_dim=4, hid_dim=4, out_dim=3, num_layers=2)


@pytest.mark.parametrize("mode", ["auto", "on"])
def test_the_pass_goes_to_score_roots(monkeypatch, mode):
    res = _FakeResident(answer=ANSWER)
    model = _sage().train()
    spec, old = _wired(monkeypatch, model, res, eval_plan=mode)
    assert spec._score_split(None, "val", torch.device("cpu")) == 2 / 3
    assert res.calls == [("GraphSAGE", [4, 9, 2], [1, 0, 2], 2, False)] and not old  # (scored in eval mode ...)
    assert model.training and spec.last_score == ANSWER  # (... and the training flag restored)
    assert spec._score_split(None, "test", torch.device("cpu")) == 2 / 3 and len(res.calls) == 2
    # no roots: 0 / max(0, 1)
    res.answer = {"correct": 0, "evaluated": 0, "loss": 0.0, "calls": 0, "redone": 0}
    assert spec._score_split(None, "val", torch.device("cpu")) == 0.0


@pytest.mark.parametrize("why", ["off", "world", "sharded", "no_plan", "tfrecord", "auto_kind"])
def test_the_pass_falls_back_to_score(monkeypatch, why):
    res = _FakeResident(world=2 if why == "world" else 1, sharded=why == "sharded",
                        answer=None if why == "no_plan" else ANSWER)
    model = torch.nn.Linear(2, 2) if why == "auto_kind" else _sage()  # (an encoder class `auto` was not measured for)
    spec, old = _wired(monkeypatch, model, res, hbm=why != "tfrecord", eval_plan="off" if why == "off" else "auto")
    assert spec._score_split(None, "val", torch.device("cpu")) == -1.0 and old == [1]
    assert len(res.calls) == (1 if why == "no_plan" else 0)
    if why == "auto_kind":  # `on` takes every encoder that has a plan
        spec._eval_plan = "on"
        assert spec._score_split(None, "val", torch.device("cpu")) == 2 / 3


def test_score_roots_applies_to_one_process_over_a_replica_with_a_plan():
    from gigl_amd.hbm import ResidentGraph
    ids, labels = np.arange(5, dtype=np.int64), np.zeros(5, np.int64)
    for world, sharded, plan in ((2, False, object()), (2, True, object()), (1, True, object()), (1, False, None)):
        res = object.__new__(ResidentGraph)
        res.world, res.sharded, res.device = world, sharded, torch.device("cpu")
        asked = []
        res._plan_for = lambda model, b, groups, _p=plan: asked.append((b, groups)) or _p
        assert res.score_roots(None, ids, labels, 4) is None
        assert asked == ([(4, 1)] if (world, sharded) == (1, False) else [])  # (groups = 1: today's plan shapes)
    # an empty pass over an applicable graph: zeros, nothing issued
    res = object.__new__(ResidentGraph)
    res.world, res.sharded, res.device = 1, False, torch.device("cpu")
    res._plan_for = lambda model, b, groups: object()
    assert res.score_roots(None, ids[:0], labels[:0], 4) == {"correct": 0, "evaluated": 0, "loss": 0.0, "calls": 0, "redone": 0}
