"""The reference's node-classification fixture job through Trainer with trainerArgs eval_plan on and off, for the stock
TwoLayerGCN and for GraphSAGE: every epoch's validation accuracy (history's val_acc) and eval()'s test accuracy are equal.

`off` is the parent's route — score() with a host read per batch, over ResidentGraph.encode for the GCN and over the staged
train_batches forward for GraphSAGE; `on` is ResidentGraph.score_roots, one host read per pass.  The two runs train alike
(same seed, same library plan), so every pass scores the same weights.  GCN: both routes run the same plan over the same
rows, the accuracies are exactly equal.  GraphSAGE: the routes' rows agree within the project's 1e-5 forward bound, so the
test first asserts that in every pass of the `off` run every root's two largest logits lie at least 1e-3 + 2e-5 apart —
2e-5 being what the fp32 rows' own error can take from the float64 gap — no root left out; the seed is chosen for it."""
import os
import shutil

import pytest
import torch
import yaml

SNC = "configs/snc_frozen_gbml_config.yaml"
EPOCHS = 4
SEEDS = {"gigl_amd.models_attn.TwoLayerGCN": 1, "gigl_amd.models.GraphSAGE": 1}
MARGIN = 1e-3 + 2e-5


@pytest.fixture(scope="module")
def workdir(golden_dir, tmp_path_factory):
    from gigl_amd.subgraph_sampler import SubgraphSampler
    base = tmp_path_factory.mktemp("gigl_nc_score_entry")
    shutil.copytree(os.path.join(golden_dir, "configs"), base / "configs")
    shutil.copytree(os.path.join(golden_dir, "ref_assets"), base / "ref_assets")
    SubgraphSampler().run("job", SNC, None, uri_base=str(base))
    return str(base)


def _config(workdir, model, mode):
    name = f"nc_score_{model.rsplit('.', 1)[1]}_{mode}"
    doc = yaml.safe_load(open(os.path.join(workdir, SNC)))
    doc["trainerConfig"]["trainerArgs"].update(gnn_model_class_path=model, hid_dim="8", out_dim="3", num_epochs=str(EPOCHS),
                                               data_route="hbm", eval_plan=mode)
    doc["sharedConfig"]["trainedModelMetadata"].update(trainedModelUri=f"out/{name}/model.pt",
                                                        evalMetricsUri=f"out/{name}/eval_metrics.json")
    uri = f"configs/{name}_gbml_config.yaml"
    yaml.safe_dump(doc, open(os.path.join(workdir, uri), "w"))
    return uri


def _run(workdir, model, mode, monkeypatch):
    """-> (val_acc per epoch, test accuracy, score_roots passes, the smallest top-2 gap of the rows score() saw)"""
    from gigl_amd.hbm import ResidentGraph
    from gigl_amd.task_specs import HipGraphSageNodeClassificationSpec as Spec
    from gigl_amd.trainer import Trainer
    passes, gaps = [], []
    score_roots, infer_batch = ResidentGraph.score_roots, Spec.infer_batch

    def watched_pass(self, *a, **k):
        out = score_roots(self, *a, **k)
        passes.append(out)
        return out

    def watched_batch(self, *a, **k):
        out = infer_batch(self, *a, **k)
        top = torch.topk(out.embeddings.detach().double(), 2, dim=1).values
        gaps.append(float((top[:, 0] - top[:, 1]).min()))
        return out
    with monkeypatch.context() as m:
        m.setattr(ResidentGraph, "score_roots", watched_pass)
        m.setattr(Spec, "infer_batch", watched_batch)
        torch.manual_seed(SEEDS[model])
        tr = Trainer()
        metrics = tr.run("job", _config(workdir, model, mode), None, uri_base=workdir)
    assert tr.training_process.route == "hbm"
    hist = tr.training_process.trainer.history
    assert len(hist) == EPOCHS and set(hist[0]) == {"epoch", "loss", "val_acc"}
    return [h["val_acc"] for h in hist], metrics.metrics["acc"].value, passes, (min(gaps) if gaps else None)


@pytest.mark.gpu
@pytest.mark.parametrize("model", list(SEEDS))
def test_eval_plan_on_and_off_score_alike(workdir, monkeypatch, model):
    val_off, test_off, passes_off, gap = _run(workdir, model, "off", monkeypatch)
    assert not passes_off and gap is not None  # the parent's route: score() batch by batch
    print(f"{model}: off val_acc {val_off} test {test_off}, smallest top-2 gap {gap:.3e}")
    if model.endswith("GraphSAGE"):
        assert gap >= MARGIN
    val_on, test_on, passes_on, gap_on = _run(workdir, model, "on", monkeypatch)
    print(f"{model}: on  val_acc {val_on} test {test_on}, passes {passes_on}")
    assert len(passes_on) == EPOCHS + 1 and all(p is not None for p in passes_on) and gap_on is None
    assert all(p["evaluated"] > 0 and p["calls"] >= 1 for p in passes_on)
    assert val_on == val_off and test_on == test_off
    assert [p["correct"] / p["evaluated"] for p in passes_on] == val_off + [test_off]
