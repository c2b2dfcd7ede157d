"""Which TASKS of a link-prediction job reach the library's training plans (no GPU: the predicate only).
HipNodeAnchorLinkPredictionSpec._train_plan_task_kwargs hands engine.NablpTrainPlan (and its GAT kinds) the job's ONE task —
Retrieval (its own cross-entropy, no candidate-sampling correction), Margin or Softmax — at any finite positive weight; a
job with several tasks, a Retrieval task the plan's head does not compute, or a weight it cannot take keeps the autograd
loop (None)."""
import inspect

import pytest
import torch


def _spec(**trainer_args):
    from gigl_amd.nablp_spec import HipNodeAnchorLinkPredictionSpec
    return HipNodeAnchorLinkPredictionSpec(**trainer_args)


@pytest.mark.parametrize("trainer_args,want", [
    ({}, dict(task="Retrieval", task_weight=1.0, temperature=0.07, remove_accidental_hits=True)),
    (dict(softmax_temp="0.2", should_remove_accidental_hits="False"),
     dict(task="Retrieval", task_weight=1.0, temperature=0.2, remove_accidental_hits=False)),
    (dict(task_path="gigl_amd.nablp_spec.Margin", margin="0.3"), dict(task="Margin", task_weight=1.0, margin=0.3)),
    (dict(task_path="gigl_amd.nablp_spec.Margin"), dict(task="Margin", task_weight=1.0, margin=0.5)),
    (dict(task_path="gigl_amd.nablp_spec.Softmax", softmax_temp="0.1"),
     dict(task="Softmax", task_weight=1.0, softmax_temperature=0.1)),
])
def test_a_single_task_gives_its_plan_arguments(trainer_args, want):
    assert _spec(**trainer_args)._train_plan_task_kwargs() == want


def test_the_plans_take_what_the_helper_hands_them():
    from gigl_amd.engine import GatEdgeNablpTrainPlan, GatNablpTrainPlan, NablpTrainPlan
    for cls in (NablpTrainPlan, GatNablpTrainPlan, GatEdgeNablpTrainPlan):
        params = inspect.signature(cls.__init__).parameters
        for k, v in dict(task="Retrieval", margin=0.5, softmax_temperature=0.07, task_weight=1.0, temperature=0.07,
                         remove_accidental_hits=True).items():
            assert k in params and params[k].default == v, (cls.__name__, k)


def test_any_finite_positive_weight_is_taken():
    from gigl_amd.nablp_spec import Margin, NodeAnchorBasedLinkPredictionTasks
    spec = _spec()
    for w in (0.25, 1.0, 3.0):
        spec.tasks = NodeAnchorBasedLinkPredictionTasks()
        spec.tasks.add_task(Margin(margin=0.3), weight=w)
        assert spec._train_plan_task_kwargs() == dict(task="Margin", task_weight=w, margin=0.3)


def test_what_keeps_the_autograd_loop():
    from gigl_amd.nablp_spec import Margin, NodeAnchorBasedLinkPredictionTasks, Retrieval, Softmax
    spec = _spec()

    def with_tasks(*pairs):
        spec.tasks = NodeAnchorBasedLinkPredictionTasks()
        for task, w in pairs:
            spec.tasks.add_task(task, weight=w)
        return spec._train_plan_task_kwargs()
    # two tasks
    assert with_tasks((Retrieval(), 1.0), (Margin(), 1.0)) is None
    assert with_tasks((Margin(), 0.5), (Softmax(), 0.5)) is None
    # Retrieval with the sampling correction, with a custom loss
    assert with_tasks((Retrieval(should_enable_candidate_sampling_correction=True), 1.0)) is None
    assert with_tasks((Retrieval(loss=torch.nn.CrossEntropyLoss(reduction="sum")), 1.0)) is None
    # a weight that is not finite and > 0
    for w in (0.0, -1.0, float("inf"), float("nan"), None):
        assert with_tasks((Retrieval(), w)) is None, w
        assert with_tasks((Margin(), w)) is None, w
        assert with_tasks((Softmax(), w)) is None, w
    # parameters the library refuses
    assert with_tasks((Softmax(softmax_temperature=0.0), 1.0)) is None
    assert with_tasks((Margin(margin=float("inf")), 1.0)) is None

    class MyMargin(Margin):  # (a subclass may compute anything)
        pass
    assert with_tasks((MyMargin(), 1.0)) is None
    # no task at all
    assert with_tasks() is None
