"""Through the drop-in entry point: a link-prediction inference job with an EdgeAttrGAT encoder over a graph with edge
features and the spec's default L2-normalised output takes the one-call plan on the in-HBM route — rows == the TFRecord
route's rows == the fp32 CPU forward over oracle-collated batches (1e-5)."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from gigl_amd import wire
from gigl_amd.config import GbmlConfigPbWrapper

pytestmark = pytest.mark.gpu
FAN = [10, 5]


def _edge_feats(a, b):
    """two feature columns (a scalar `w`, a 2-vector `v`), symmetric in the endpoints: the graph is bidirectionalised"""
    lo, hi = np.minimum(a, b).astype(np.int64), np.maximum(a, b).astype(np.int64)
    w = ((lo * 7 + hi * 3) % 11).astype(np.float32) / 11 - 0.5
    v = np.stack([((hi - lo) % 5).astype(np.float32) / 5 - 0.4, 0.5 * ((hi % 7).astype(np.float32) / 7)], axis=1)
    return w.astype(np.float32), v.astype(np.float32)


@pytest.fixture(scope="module")
def lp_job(tmp_path_factory):
    from test_gpu_hbm_route import _write_small_job
    base = str(tmp_path_factory.mktemp("gigl_hbm_edge_lp"))
    n, src, dst, x = _write_small_job(base)  # 20,000 nodes, fan-out (10, 5), inferenceBatchSize 512
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
    args = {"hidden_dim": "16", "out_channels": "12", "gnn_model_class_path": "gigl_amd.models_attn.GAT", "edge_dim": "3",
            "conv": "edge_attr_gat", "num_heads": "2"}  # (should_l2_normalize_embedding_layer_output: the default, on)
    doc["trainerConfig"] = {"trainerClsPath": spec, "trainerArgs": dict(args)}
    doc["inferencerConfig"] = {"inferencerClsPath": spec, "inferencerArgs": dict(args),
                               "inferenceBatchSize": doc["inferencerConfig"]["inferenceBatchSize"]}
    yaml.safe_dump(doc, open(os.path.join(base, "configs/lp.yaml"), "w"))
    cfg = GbmlConfigPbWrapper.from_uri("configs/lp.yaml", uri_base=base)
    from gigl_amd.nablp_spec import HipNodeAnchorLinkPredictionSpec
    torch.manual_seed(5)
    model = HipNodeAnchorLinkPredictionSpec(**cfg.inferencer_args).init_model(cfg)
    with torch.no_grad():
        for c in model.encoder.conv_layers:
            c.bias.normal_(0, 0.1)
    assert model.encoder.should_l2_normalize_embedding_layer_output and model.encoder.edge_dim == 3
    os.makedirs(os.path.join(base, "out/lp/model"), exist_ok=True)
    torch.save(model.state_dict(), os.path.join(base, "out/lp/model/model.pt"))
    return base, n, src, dst, x


def _rows(path):
    return [json.loads(l) for l in open(path)]


def test_link_prediction_gat_with_edge_features_takes_the_plan(lp_job, monkeypatch):
    import oracle
    from gigl_amd import config, hbm
    from gigl_amd.inferencer import Inferencer
    from gigl_amd.subgraph_sampler import SubgraphSampler
    from oracle import gnn_ref
    from test_gpu_hbm_route import _variant
    base, n, src, dst, x = lp_job
    monkeypatch.setattr(config, "RECORDS_PER_PART_FILE", 3000)
    SubgraphSampler().run("job", "configs/lp.yaml", None, uri_base=base)
    seen = []
    close = hbm.ResidentGraph.close

    def recording_close(self):
        seen.append(list(self._plans.values()))
        close(self)
    monkeypatch.setattr(hbm.ResidentGraph, "close", recording_close)
    a, b = Inferencer(), Inferencer()
    out_t = a.run("job", _variant(base, "configs/lp.yaml", "tf"), None, uri_base=base, route="tfrecord")
    out_h = b.run("job", _variant(base, "configs/lp.yaml", "hbm"), None, uri_base=base, route="hbm")
    assert a.route == "tfrecord" and b.route == "hbm" and a.rows_written == b.rows_written == n
    # the in-HBM route went through a one-call plan (not the staged forward), several batches per call, none redone
    assert b.hbm_groups > 1
    assert seen and seen[-1] and any(p is not None for p in seen[-1])
    assert b.hbm_overflow_redone == 0
    rt, rh = _rows(out_t["embeddings"]), _rows(out_h["embeddings"])
    ids = [r["node_id"] for r in rh]
    assert ids == [r["node_id"] for r in rt] and sorted(ids) == list(range(n))
    eh, et = np.array([r["emb"] for r in rh], np.float32), np.array([r["emb"] for r in rt], np.float32)
    print("max |hbm - tfrecord| =", np.abs(eh - et).max())
    np.testing.assert_allclose(eh, et, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(np.linalg.norm(eh, axis=1), 1.0, rtol=1e-5)  # the spec's default: L2-normalised rows
    # oracle: sample -> collate -> fp32 forward of the first and of the last (partial: 20000 % 512 = 32 roots) batch
    rowptr, col = oracle.build_csc(n, src.astype(np.uint32), dst.astype(np.uint32), is_directed=False)
    cfg = GbmlConfigPbWrapper.from_uri("configs/lp.yaml", uri_base=base)
    sd = torch.load(cfg.trained_model_uri, map_location="cpu")
    for lo, hi in ((0, 512), (n - n % 512, n)):
        roots = np.array(ids[lo:hi], dtype=np.uint32)
        nbr, _ = oracle.sample_khop(rowptr, col, roots, FAN, canonical=True)
        u = oracle.union_build(roots, FAN, nbr)
        ei = gnn_ref.union_edge_index(u["rowptr"], u["col"])
        nodes = u["nodes"].astype(np.int64)
        w, v = _edge_feats(nodes[ei[0].numpy()], nodes[ei[1].numpy()])
        ea = torch.from_numpy(np.concatenate([w[:, None], v], axis=1))
        h = torch.from_numpy(x[nodes])
        for l in range(2):
            p = f"_encoder.conv_layers.{l}."
            h = gnn_ref.gat_conv(h, ei, sd[p + "lin.weight"], sd[p + "att_src"], sd[p + "att_dst"], sd[p + "bias"],
                                 2 if l == 0 else 1, edge_attr=ea, w_edge=sd[p + "lin_edge.weight"],
                                 att_edge=sd[p + "att_edge"], w_edge_msg=sd[p + "lin_edge.weight"])
            if l == 0:
                h = torch.relu(h)
        want = torch.nn.functional.normalize(h, p=2, dim=1)[u["root_local"]].numpy()
        print(f"batch [{lo},{hi}): max |hbm - oracle| =", np.abs(eh[lo:hi] - want).max())
        np.testing.assert_allclose(eh[lo:hi], want, rtol=1e-5, atol=1e-5)
