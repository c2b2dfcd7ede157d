"""Margin and Softmax jobs through the trainer's entry point: on the in-HBM route HipNodeAnchorLinkPredictionSpec.train
hands a job whose task_path names Margin or Softmax to the library's training plan (trainer.train_plan_steps counts its
steps — 0 before the plan's head computed these losses) and reaches the autograd loop's loss history (`train_plan: off`)."""
import os
import shutil

import numpy as np
import pytest

from conftest import seed_trainer

pytestmark = pytest.mark.gpu

CFG = "configs/nablp_frozen_gbml_config.yaml"


@pytest.fixture(scope="module")
def workdir(golden_dir, tmp_path_factory):
    """the reference fixture job of tests/test_gpu_nablp.py"""
    base = tmp_path_factory.mktemp("gigl_lp_task")
    shutil.copytree(os.path.join(golden_dir, "configs"), base / "configs")
    shutil.copytree(os.path.join(golden_dir, "ref_assets"), base / "ref_assets")
    from gigl_amd.subgraph_sampler import SubgraphSampler
    SubgraphSampler().run("job", CFG, None, uri_base=str(base))
    return str(base)


@pytest.mark.parametrize("task", ["Margin", "Softmax"])
def test_trainer_runs_margin_and_softmax_jobs_through_the_library_plan(workdir, task):
    """`train_plan: auto` against `off` at margin 0.3 / softmax_temp 0.1: every step ran in the plan, at least four of them,
    the histories agree at rtol 2e-3 (test_trainer_runs_the_gat_encoder_through_the_library_plan's bound for a plan's history
    against the autograd loop's), the final metrics — validation in the plan against validate()'s loop — are finite"""
    import yaml
    from gigl_amd.trainer import Trainer
    doc = yaml.safe_load(open(os.path.join(workdir, CFG)))
    args = doc["trainerConfig"]["trainerArgs"]
    args.update(task_path=f"gigl_amd.nablp_spec.{task}", margin="0.3", softmax_temp="0.1")
    runs = {}
    old = os.environ.get("GIGL_AMD_ROUTE")
    os.environ["GIGL_AMD_ROUTE"] = "hbm"
    try:
        for mode in ("auto", "off"):
            args["train_plan"] = mode
            doc["sharedConfig"]["trainedModelMetadata"]["trainedModelUri"] = f"out/lp_task_{task}_{mode}/model.pt"
            doc["sharedConfig"]["trainedModelMetadata"]["evalMetricsUri"] = f"out/lp_task_{task}_{mode}/eval_metrics.json"
            cfg_uri = f"configs/lp_task_{task}_{mode}_gbml_config.yaml"
            yaml.safe_dump(doc, open(os.path.join(workdir, cfg_uri), "w"))
            seed_trainer()
            tr = Trainer()
            metrics = tr.run("job", cfg_uri, None, uri_base=workdir)
            assert tr.training_process.route == "hbm"
            spec = tr.training_process.trainer
            assert type(next(iter(spec.tasks._task_to_fn_map.values()))).__name__ == task
            runs[mode] = ([h["loss"] for h in spec.history], int(getattr(spec, "train_plan_steps", 0)),
                          {k: float(m.value) for k, m in metrics.metrics.items()})
    finally:
        if old is None:
            os.environ.pop("GIGL_AMD_ROUTE", None)
        else:
            os.environ["GIGL_AMD_ROUTE"] = old
    (h_plan, n_plan, m_plan), (h_auto, n_auto, m_auto) = runs["auto"], runs["off"]
    print(f"{task}: plan history {h_plan} autograd history {h_auto}; metrics {m_plan} / {m_auto}")
    assert n_plan == len(h_plan) >= 4 and n_auto == 0
    np.testing.assert_allclose(h_plan, h_auto, rtol=2e-3)
    assert all(np.isfinite(v) for v in m_plan.values()) and all(np.isfinite(v) for v in m_auto.values())
    assert 0.0 < m_plan["mrr"] <= 1.0
