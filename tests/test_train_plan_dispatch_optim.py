"""Which OPTIMISER settings of a link-prediction job reach the library's training plans (no GPU: the predicate only).
HipNodeAnchorLinkPredictionSpec._train_plan_optim_kwargs hands engine.NablpTrainPlan (and its GAT kinds) the trainer's
optim_lr / optim_weight_decay, clip_grad_norm and the ConstantLR schedule (factor, total_iters); any other optimiser,
optimiser argument or scheduler class keeps the autograd loop (None)."""
import pytest

DEFAULTS = dict(lr=5e-3, weight_decay=1e-6, clip_grad_norm=0.0, lr_factor=1.0, lr_total_iters=0)


def _spec(**trainer_args):
    from gigl_amd.nablp_spec import HipNodeAnchorLinkPredictionSpec
    return HipNodeAnchorLinkPredictionSpec(**trainer_args)


@pytest.mark.parametrize("trainer_args,want", [
    ({}, DEFAULTS),
    (dict(optim_lr="0.01", optim_weight_decay="0.0005"), dict(DEFAULTS, lr=0.01, weight_decay=5e-4)),
    (dict(clip_grad_norm="0.5"), dict(DEFAULTS, clip_grad_norm=0.5)),
    (dict(factor="0.5", total_iters="4"), dict(DEFAULTS, lr_factor=0.5, lr_total_iters=4)),
    (dict(clip_grad_norm="2.0", factor="0.25", total_iters="3"),
     dict(DEFAULTS, clip_grad_norm=2.0, lr_factor=0.25, lr_total_iters=3)),
    # (factor 1 is no schedule whatever total_iters says: the plan's defaults, so that nothing is set on the plan)
    (dict(factor="1.0", total_iters="7"), DEFAULTS),
    # (the trainer clips only when clip_grad_norm > 0)
    (dict(clip_grad_norm="-1"), DEFAULTS),
])
def test_optimiser_settings_the_plan_takes(trainer_args, want):
    got = _spec(**trainer_args)._train_plan_optim_kwargs()
    assert got == want
    assert {k: type(v) for k, v in got.items()} == {k: type(v) for k, v in want.items()}


def test_the_plans_accept_exactly_these_keyword_arguments():
    import inspect

    from gigl_amd.engine import GatEdgeNablpTrainPlan, GatNablpTrainPlan, NablpTrainPlan
    for cls in (NablpTrainPlan, GatNablpTrainPlan, GatEdgeNablpTrainPlan):
        params = inspect.signature(cls.__init__).parameters
        for k, v in DEFAULTS.items():
            assert k in params, (cls.__name__, k)
            if k not in ("lr", "weight_decay"):  # (the knobs are off by default)
                assert params[k].default == v, (cls.__name__, k)


def test_other_schedulers_and_optimisers_keep_the_autograd_loop():
    assert _spec(lr_scheduler_name="torch.optim.lr_scheduler.StepLR")._train_plan_optim_kwargs() is None
    assert _spec(lr_scheduler_name="torch.optim.lr_scheduler.LinearLR", factor="0.5")._train_plan_optim_kwargs() is None
    assert _spec(optim_class_path="torch.optim.SGD")._train_plan_optim_kwargs() is None
    assert _spec(optim_class_path="torch.optim.AdamW", clip_grad_norm="0.5")._train_plan_optim_kwargs() is None
    spec = _spec(clip_grad_norm="0.5")
    spec._optim_kwargs["amsgrad"] = True  # (an optimiser argument beyond lr / weight_decay)
    assert spec._train_plan_optim_kwargs() is None
    spec = _spec()
    spec._optim_kwargs["betas"] = (0.8, 0.99)
    assert spec._train_plan_optim_kwargs() is None
