"""The stock node-classification model (models_attn.TwoLayerGCN) reaches the one-call inference plan (engine.GcnPlan,
gigl_gcn_plan_*) through ResidentGraph.encode — one plan per (b, groups), refreshed with the projected table when the
weights move, a batch set that overflows redone through the staged launches — and through the SNC fixture job: Trainer
(validation / test passes) and Inferencer each create a plan, and the predictions equal those of a pass whose batches are
forced through the staged launches.  Bound and references: tests/gcn_infer_cases.py."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
import yaml

import gcn_infer_cases as ic
import gcn_plan_cases as gc
from conftest import seed_trainer

SNC = "configs/snc_frozen_gbml_config.yaml"
EPOCHS = 8


def _watch(monkeypatch):
    from gigl_amd.engine import GcnPlan
    made, init = [], GcnPlan.__init__

    def init_(self, *a, **k):
        init(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(GcnPlan, "__init__", init_)
    return made


def _staged(res, model, ids, b, groups):
    (hb,) = list(res.root_batches(ids, b, groups))
    hb.force_staged = True
    return res.encode(model, hb)


def _planned(res, model, ids, b, groups):
    (hb,) = list(res.root_batches(ids, b, groups))
    return res.encode(model, hb)


@pytest.mark.gpu
def test_encode_runs_the_plan_and_follows_the_weights(monkeypatch):
    from gigl_amd.engine import HipEngine
    from gigl_amd.hbm import ResidentGraph
    from gigl_amd.models_attn import TwoLayerGCN
    name = "wide_input"
    case = ic.CASES[name]
    made = _watch(monkeypatch)
    rowptr, col = gc.graph()[:2]
    eng = HipEngine(0)
    try:
        eng.load_csc(rowptr, col)
        eng.load_features(gc.features(case.dims[0]))
        res = ResidentGraph.from_engine(eng, np.arange(gc.N_NODES), list(case.fan))
        model = TwoLayerGCN(case.dims[0], case.dims[2], hid_dim=case.dims[1], is_training=False)
        model.load_state_dict(ic.state_of(case))
        model = model.to(eng.device)
        assert model.projected_input_pays(eng)
        ids = ic.batch(name)[0].astype(np.int64)
        want, bound, fp32 = ic.reference(name)
        out = _planned(res, model, ids, 64, 1)
        assert len(made) == 1 and made[0]._proj is not None and not made[0].fused_root()  # (off by default)
        staged = _staged(res, model, ids, 64, 1)
        err, diff = float((out.cpu().double() - want).abs().max()), float((out - staged).abs().max())
        print(f"plan against float64 {err:.3e} (fp32 {fp32:.3e}), plan against staged {diff:.3e}, bound {bound:.3e}")
        assert err <= bound and diff <= bound
        # one plan per (b, groups)
        g4 = _planned(res, model, ids, 16, 4)
        assert len(made) == 2 and float((g4 - _staged(res, model, ids, 16, 4)).abs().max()) <= bound
        _planned(res, model, ids, 64, 1), _planned(res, model, ids, 16, 4)
        assert len(made) == 2
        # an optimiser step: the stamp moves, the weights and the projected table follow
        table = made[0]._proj
        opt = torch.optim.SGD(model.parameters(), lr=0.5)
        g = torch.Generator().manual_seed(3)
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=g).to(p.device)
        opt.step()
        moved = _planned(res, model, ids, 64, 1)
        assert len(made) == 2 and float((moved - out).abs().max()) > 1e-2
        assert float((moved - _staged(res, model, ids, 64, 1)).abs().max()) <= bound
        assert made[0]._proj is table  # (refilled in place: one table per model state)
        # roots that are each other's neighbours: the call is redone through the staged launches
        cl = ic.CASES["overflow"]
        before = res.overflow_redone
        rows = _planned(res, model, ic.batch("overflow")[0].astype(np.int64), cl.b, 1)
        assert res.overflow_redone == before + 1 and tuple(rows.shape) == (cl.b, case.dims[2])
        assert bool(torch.isfinite(rows).all())
        res.close()
    finally:
        eng.close()


# ---- the SNC fixture job end to end (the config helper of tests/test_gpu_gcn_train_entry.py)
@pytest.fixture(scope="module")
def workdir(golden_dir, tmp_path_factory):
    from gigl_amd.subgraph_sampler import SubgraphSampler
    base = tmp_path_factory.mktemp("gigl_gcn_infer_entry")
    shutil.copytree(os.path.join(golden_dir, "configs"), base / "configs")
    shutil.copytree(os.path.join(golden_dir, "ref_assets"), base / "ref_assets")
    SubgraphSampler().run("job", SNC, None, uri_base=str(base))
    return str(base)


def _config(workdir, name, out):
    doc = yaml.safe_load(open(os.path.join(workdir, SNC)))
    doc["trainerConfig"]["trainerArgs"].update(gnn_model_class_path="gigl_amd.models_attn.TwoLayerGCN", hid_dim="8", out_dim="3",
                                               num_epochs=str(EPOCHS), data_route="hbm")
    doc["inferencerConfig"]["inferencerArgs"].update(gnn_model_class_path="gigl_amd.models_attn.TwoLayerGCN", hid_dim="8",
                                                     out_dim="3")
    doc["sharedConfig"]["trainedModelMetadata"].update(trainedModelUri=f"out/{name}/model.pt",
                                                        evalMetricsUri=f"out/{name}/eval_metrics.json")
    info = doc["sharedConfig"]["inferenceMetadata"]["nodeTypeToInferencerOutputInfoMap"]["user"]
    info.update(embeddingsPath=f"out/{out}/embeddings.jsonl", predictionsPath=f"out/{out}/predictions.jsonl")
    uri = f"configs/{out}_gbml_config.yaml"
    yaml.safe_dump(doc, open(os.path.join(workdir, uri), "w"))
    return uri


def _rows(path):
    with open(path) as f:
        return {int(r["node_id"]): r for r in map(json.loads, f)}


@pytest.mark.gpu
def test_stock_gcn_job_validates_and_serves_through_the_plan(workdir, monkeypatch):
    from gigl_amd.engine import GcnPlan
    from gigl_amd.hbm import ResidentGraph
    from gigl_amd.inferencer import Inferencer
    from gigl_amd.trainer import Trainer
    made = _watch(monkeypatch)
    uri = _config(workdir, "snc_gcn_infer", "snc_gcn_infer")
    seed_trainer()
    tr = Trainer()
    metrics = tr.run("job", uri, None, uri_base=workdir)
    assert tr.training_process.route == "hbm" and 0.0 <= metrics.metrics["acc"].value <= 1.0
    trained = len(made)
    assert trained >= 1 and all(type(p) is GcnPlan for p in made)  # the validation / test passes
    inf = Inferencer()
    out = inf.run("job", uri, None, uri_base=workdir, route="hbm")
    assert inf.route == "hbm" and inf.rows_written == 16 and len(made) > trained
    # the same model, every batch through the staged launches
    encode = ResidentGraph.encode

    def staged_encode(self, model, batch):
        batch.force_staged = True
        return encode(self, model, batch)
    monkeypatch.setattr(ResidentGraph, "encode", staged_encode)
    n_plans = len(made)
    uri2 = _config(workdir, "snc_gcn_infer", "snc_gcn_infer_staged")
    inf2 = Inferencer()
    out2 = inf2.run("job", uri2, None, uri_base=workdir, route="hbm")
    assert inf2.rows_written == 16 and len(made) == n_plans
    assert out["predictions"] != out2["predictions"]
    a, b = _rows(out["predictions"]), _rows(out2["predictions"])
    assert len(a) == 16 and set(a) == set(b) and all(a[k]["pred"] == b[k]["pred"] for k in a)
    ea, eb = _rows(out["embeddings"]), _rows(out2["embeddings"])
    for k in ea:
        np.testing.assert_allclose(np.array(ea[k]["emb"], np.float32), np.array(eb[k]["emb"], np.float32), rtol=0, atol=1e-5)
