"""The stock node-classification job (gnn_model_class_path = gigl_amd.models_attn.TwoLayerGCN) through Trainer().run on the
in-HBM route: the spec hands the epochs to engine.GcnTrainPlan (gigl_gcn_train_plan_*: one library call per step),
GIGL_AMD_TRAIN_PLAN=0 keeps the autograd loop, and close() closes the plan."""
import os
import shutil

import numpy as np
import pytest
import torch
import yaml

from conftest import seed_trainer
from gigl_amd.config import GbmlConfigPbWrapper

SNC = "configs/snc_frozen_gbml_config.yaml"
EPOCHS = 8


@pytest.fixture(scope="module")
def workdir(golden_dir, tmp_path_factory):
    from gigl_amd.subgraph_sampler import SubgraphSampler
    base = tmp_path_factory.mktemp("gigl_gcn_entry")
    shutil.copytree(os.path.join(golden_dir, "configs"), base / "configs")
    shutil.copytree(os.path.join(golden_dir, "ref_assets"), base / "ref_assets")
    SubgraphSampler().run("job", SNC, None, uri_base=str(base))
    return str(base)


def _config(workdir, name):
    doc = yaml.safe_load(open(os.path.join(workdir, SNC)))
    doc["trainerConfig"]["trainerArgs"].update(gnn_model_class_path="gigl_amd.models_attn.TwoLayerGCN", hid_dim="8", out_dim="3",
                                               num_epochs=str(EPOCHS), data_route="hbm")
    doc["inferencerConfig"]["inferencerArgs"].update(gnn_model_class_path="gigl_amd.models_attn.TwoLayerGCN", hid_dim="8",
                                                     out_dim="3")
    doc["sharedConfig"]["trainedModelMetadata"].update(trainedModelUri=f"out/{name}/model.pt",
                                                        evalMetricsUri=f"out/{name}/eval_metrics.json")
    uri = f"configs/{name}_gbml_config.yaml"
    yaml.safe_dump(doc, open(os.path.join(workdir, uri), "w"))
    return uri


def _watch(monkeypatch):
    """-> (plans created, what the spec held as _train_plan when close() was called)"""
    from gigl_amd.engine import GcnTrainPlan
    from gigl_amd.task_specs import HipGraphSageNodeClassificationSpec as Spec
    made, held = [], []
    init, close = GcnTrainPlan.__init__, Spec.close

    def init_(self, *a, **k):
        init(self, *a, **k)
        made.append(self)

    def close_(self):
        held.append(getattr(self, "_train_plan", None))
        close(self)
    monkeypatch.setattr(GcnTrainPlan, "__init__", init_)
    monkeypatch.setattr(Spec, "close", close_)
    return made, held


@pytest.mark.gpu
def test_stock_gcn_job_trains_through_the_library_plan(workdir, monkeypatch):
    from gigl_amd.engine import GcnTrainPlan
    from gigl_amd.trainer import Trainer
    monkeypatch.delenv("GIGL_AMD_TRAIN_PLAN", raising=False)
    made, held = _watch(monkeypatch)
    uri = _config(workdir, "snc_gcn_plan")
    seed_trainer()
    tr = Trainer()
    metrics = tr.run("job", uri, None, uri_base=workdir)
    spec = tr.training_process.trainer
    assert tr.training_process.route == "hbm"
    assert len(made) == 1 and type(held[0]) is GcnTrainPlan and held[0] is made[0]  # one plan, held over every epoch
    assert made[0]._dropout[0] == 0.5  # (the module's own: TwoLayerGCN(is_training=True))
    hist = spec.history
    assert len(hist) == EPOCHS and all(np.isfinite(h["loss"]) for h in hist)
    assert min(h["loss"] for h in hist[1:]) < hist[0]["loss"], [h["loss"] for h in hist]
    assert 0.0 <= metrics.metrics["acc"].value <= 1.0
    cfg = GbmlConfigPbWrapper.from_uri(uri, uri_base=workdir)
    sd = torch.load(cfg.trained_model_uri, map_location="cpu")
    assert set(sd) == {"conv1.lin.weight", "conv1.bias", "conv2.lin.weight", "conv2.bias"}  # PyG GCNConv's names
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    # after close() the plan is gone
    assert spec._train_plan is None and made[0]._plan is None


@pytest.mark.gpu
def test_switch_keeps_the_autograd_loop(workdir, monkeypatch):
    from gigl_amd.trainer import Trainer
    monkeypatch.setenv("GIGL_AMD_TRAIN_PLAN", "0")
    made, held = _watch(monkeypatch)
    uri = _config(workdir, "snc_gcn_autograd")
    seed_trainer()
    tr = Trainer()
    tr.run("job", uri, None, uri_base=workdir)
    assert tr.training_process.route == "hbm"
    assert made == [] and held == [None]
    hist = tr.training_process.trainer.history
    assert len(hist) == EPOCHS and all(np.isfinite(h["loss"]) for h in hist)
    sd = torch.load(GbmlConfigPbWrapper.from_uri(uri, uri_base=workdir).trained_model_uri, map_location="cpu")
    assert set(sd) == {"conv1.lin.weight", "conv1.bias", "conv2.lin.weight", "conv2.bias"}
