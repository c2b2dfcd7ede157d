"""Through the drop-in entry point: a link-prediction TRAINING job with a GAT(edge_dim) encoder over a graph with edge
features runs its steps through engine.GatEdgeNablpTrainPlan on the in-HBM route (`train_plan: auto`), reaches the loss
history of the autograd loop (`train_plan: off`), and the saved model then infers through the edge one-call plan.  The job
is built as tests/test_gpu_gat_edge_entry.py builds its own, on test_gpu_hbm_route._write_small_job (20,000 nodes, 32-wide
node rows, a 3-wide edge table); 2 heads x 8 hidden channels stay below the node rows (the input-side first layer).  The
conv is GATConv(edge_dim): the autograd loop's EdgeAttrGATConv backward is built for layer widths that are multiples of 256
only, which no first layer narrower than these rows can be (the plan itself has no such bound:
tests/test_gpu_gat_edge_train_plan.py)."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from gigl_amd import wire
from gigl_amd.config import GbmlConfigPbWrapper

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lp_train_job(tmp_path_factory):
    from test_gpu_gat_edge_entry import _edge_feats
    from test_gpu_hbm_route import _write_small_job
    base = str(tmp_path_factory.mktemp("gigl_hbm_edge_lp_train"))
    n, src, dst, x = _write_small_job(base)
    w, v = _edge_feats(src, dst)
    wire.write_tfrecords(os.path.join(base, "tables/edges/data.tfrecord"), [
        wire.encode_tf_example({"src": np.array([s], np.int64), "dst": np.array([t], np.int64),
                                "w": np.array([w[i]], np.float32), "v": v[i]})
        for i, (s, t) in enumerate(zip(src.tolist(), dst.tolist()))])
    pm = yaml.safe_load(open(os.path.join(base, "configs/pm.yaml")))
    pm["condensedEdgeTypeToPreprocessedMetadata"]["0"]["mainEdgeInfo"].update(featureKeys=["w", "v"], featureDim=3)
    yaml.safe_dump(pm, open(os.path.join(base, "configs/pm.yaml"), "w"))
    doc = yaml.safe_load(open(os.path.join(base, "configs/job.yaml")))
    et = {"dstNodeType": "paper", "relation": "cites", "srcNodeType": "paper"}
    doc["taskMetadata"] = {"nodeAnchorBasedLinkPredictionTaskMetadata": {"supervisionEdgeTypes": [et]}}
    doc["datasetConfig"]["subgraphSamplerConfig"]["numPositiveSamples"] = 1
    doc["sharedConfig"]["flattenedGraphMetadata"] = {"nodeAnchorBasedLinkPredictionOutput": {
        "tfrecordUriPrefix": "out/lp/node_anchor_based_link_prediction_samples/",
        "nodeTypeToRandomNegativeTfrecordUriPrefix": {"paper": "out/lp/random_negative_rooted_neighborhood_samples/paper/"}}}
    doc["sharedConfig"]["trainedModelMetadata"] = {"trainedModelUri": "out/lp/model/model.pt",
                                                   "evalMetricsUri": "out/lp/model/eval.json"}
    doc["sharedConfig"]["inferenceMetadata"] = {"nodeTypeToInferencerOutputInfoMap": {"paper": {
        "embeddingsPath": "out/lp/inference/embeddings.jsonl"}}}
    spec = "gigl_amd.nablp_spec.HipNodeAnchorLinkPredictionSpec"
    args = {"hidden_dim": "8", "out_channels": "16", "gnn_model_class_path": "gigl_amd.models_attn.GAT", "edge_dim": "3",
            "conv": "gat", "num_heads": "2"}
    train = dict(args, main_sample_batch_size="2048", random_negative_sample_batch_size="256",
                 random_negative_sample_batch_size_for_evaluation="256", num_val_batches="2", num_test_batches="2",
                 val_every_num_batches="1000")
    doc["trainerConfig"] = {"trainerClsPath": spec, "trainerArgs": train}
    doc["inferencerConfig"] = {"inferencerClsPath": spec, "inferencerArgs": dict(args),
                               "inferenceBatchSize": doc["inferencerConfig"]["inferenceBatchSize"]}
    yaml.safe_dump(doc, open(os.path.join(base, "configs/lp.yaml"), "w"))
    return base, n


def test_trainer_runs_the_edge_featured_gat_through_the_library_plan(lp_train_job, monkeypatch):
    from conftest import seed_trainer
    from gigl_amd import hbm
    from gigl_amd.inferencer import Inferencer
    from gigl_amd.trainer import Trainer
    base, n = lp_train_job
    cfg_uri = "configs/lp.yaml"
    doc = yaml.safe_load(open(os.path.join(base, cfg_uri)))
    runs, picked = {}, []
    monkeypatch.setenv("GIGL_AMD_ROUTE", "hbm")
    from gigl_amd.nablp_spec import HipNodeAnchorLinkPredictionSpec
    pick = HipNodeAnchorLinkPredictionSpec._library_train_plan

    def recording_pick(self, cfg):
        plan = pick(self, cfg)
        # (the resident graph exists once a plan was built, and is closed after the run)
        picked.append((type(plan).__name__, None if plan is None else self._resident.engine.edge_feat_dim))
        return plan
    monkeypatch.setattr(HipNodeAnchorLinkPredictionSpec, "_library_train_plan", recording_pick)
    for mode in ("off", "auto"):  # (the plan's model is the one left on disk for the inferencer)
        doc["trainerConfig"]["trainerArgs"]["train_plan"] = mode
        yaml.safe_dump(doc, open(os.path.join(base, cfg_uri), "w"))
        seed_trainer()
        tr = Trainer()
        tr.run("job", cfg_uri, None, uri_base=base)
        assert tr.training_process.route == "hbm"
        spec = tr.training_process.trainer
        enc = (spec.model.module if hasattr(spec.model, "module") else spec.model).encoder
        assert enc.edge_dim == 3
        runs[mode] = ([h["loss"] for h in spec.history], int(getattr(spec, "train_plan_steps", 0)))
    (h_plan, n_plan), (h_auto, n_auto) = runs["auto"], runs["off"]
    print("edge GAT trainer: plan losses", h_plan, "| autograd losses", h_auto)
    assert picked == [("NoneType", None), ("GatEdgeNablpTrainPlan", 3)], picked  # (the plan over the resident 3-wide edge table)
    assert n_plan == len(h_plan) >= 4 and n_auto == 0
    assert np.isfinite(h_plan).all()
    np.testing.assert_allclose(h_plan, h_auto, rtol=2e-3)
    # the saved model infers through the edge one-call plan
    cfg = GbmlConfigPbWrapper.from_uri(cfg_uri, uri_base=base)
    sd = torch.load(cfg.trained_model_uri, map_location="cpu")
    assert {"_encoder.conv_layers.0.lin_edge.weight", "_encoder.conv_layers.1.att_edge"} <= set(sd)
    seen = []
    close = hbm.ResidentGraph.close

    def recording_close(self):
        seen.append(list(self._plans.values()))
        close(self)
    monkeypatch.setattr(hbm.ResidentGraph, "close", recording_close)
    inf = Inferencer()
    out = inf.run("job", cfg_uri, None, uri_base=base, route="hbm")
    assert inf.route == "hbm" and inf.rows_written == n
    assert seen and seen[-1] and any(p is not None for p in seen[-1])  # a one-call plan, not the staged forward
    rows = [json.loads(l) for l in open(out["embeddings"])]
    emb = np.array([r["emb"] for r in rows], np.float32)
    assert emb.shape == (n, 16) and np.isfinite(emb).all()
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1.0, rtol=1e-5)
