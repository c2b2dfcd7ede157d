"""A job with user-defined label edges (positiveEdgeInfo / negativeEdgeInfo: the reference's
UserDefinedLabelsNodeAnchorBasedLinkPredictionTask) end to end through the trainer on the reference's own UDL fixture — the
config tests/test_gpu_nablp.py::test_user_defined_labels_on_the_reference_fixture_tables writes.  Such a job used to take the
TFRecord route whatever was asked; now `data_route: hbm` trains it in HBM, through the library plan with two hard-negative
slots per anchor, and the three ways to train it — the plan, the autograd loop over in-HBM batches (`train_plan: off`), the
TFRecord route — see the same anchors in the same order and reach the same losses and the same trained weights."""
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import seed_trainer

from gigl_amd.config import GbmlConfigPbWrapper

pytestmark = pytest.mark.gpu

CFG = "configs/nablp_frozen_gbml_config.yaml"
UDL_CFG = "configs/nablp_udl_gbml_config.yaml"
ASSETS = "ref_assets/subgraph_sampler/node_anchor_based_link_prediction/"


@pytest.fixture(scope="module")
def workdir(golden_dir, tmp_path_factory):
    """the fixture tables, the UDL job's config and its sampled TFRecords (what the TFRecord route trains from)"""
    import yaml
    from gigl_amd.subgraph_sampler import SubgraphSampler
    base = str(tmp_path_factory.mktemp("gigl_lp_udl"))
    shutil.copytree(os.path.join(golden_dir, "configs"), os.path.join(base, "configs"))
    shutil.copytree(os.path.join(golden_dir, "ref_assets"), os.path.join(base, "ref_assets"))
    pm = yaml.safe_load(open(os.path.join(base, "configs/nablp_preprocessed_metadata.yaml")))
    em = pm["condensedEdgeTypeToPreprocessedMetadata"]["0"]
    for key, d in (("positiveEdgeInfo", "user_defined_pos"), ("negativeEdgeInfo", "user_defined_neg")):
        em[key] = {"featureDim": 3, "featureKeys": ["f0", "f1", "f2"], "tfrecordUriPrefix": ASSETS + d}
    yaml.safe_dump(pm, open(os.path.join(base, "configs/nablp_udl_preprocessed_metadata.yaml"), "w"))
    doc = yaml.safe_load(open(os.path.join(base, CFG)))
    doc["sharedConfig"]["preprocessedMetadataUri"] = "configs/nablp_udl_preprocessed_metadata.yaml"
    doc["datasetConfig"]["subgraphSamplerConfig"].update(numUserDefinedPositiveSamples=2, numUserDefinedNegativeSamples=2)
    out = doc["sharedConfig"]["flattenedGraphMetadata"]["nodeAnchorBasedLinkPredictionOutput"]
    out["tfrecordUriPrefix"] = "out/nablp_udl/main/samples/"
    out["nodeTypeToRandomNegativeTfrecordUriPrefix"] = {k: "out/nablp_udl/random_negative/" + k + "/samples/"
                                                        for k in out["nodeTypeToRandomNegativeTfrecordUriPrefix"]}
    yaml.safe_dump(doc, open(os.path.join(base, UDL_CFG), "w"))
    SubgraphSampler().run("job", UDL_CFG, None, uri_base=base)
    return base


def _variant(workdir, name, **trainer_args):
    import yaml
    doc = yaml.safe_load(open(os.path.join(workdir, UDL_CFG)))
    doc["trainerConfig"]["trainerArgs"].update(trainer_args)
    doc["sharedConfig"]["trainedModelMetadata"] = {"trainedModelUri": f"out/nablp_udl/model_{name}/model.pt",
                                                   "evalMetricsUri": f"out/nablp_udl/model_{name}/eval.json"}
    uri = UDL_CFG.replace(".yaml", f"_{name}.yaml")
    yaml.safe_dump(doc, open(os.path.join(workdir, uri), "w"))
    return uri


def test_udl_batches_in_hbm_are_the_collated_records(workdir):
    """the anchors and their order, the positives and the hard negatives of every in-HBM batch are the TFRecord route's"""
    from gigl_amd.nablp_spec import HipNodeAnchorLinkPredictionSpec
    cfg = GbmlConfigPbWrapper.from_uri(UDL_CFG, uri_base=workdir)
    dev = torch.device("cuda", 0)
    specs = {}
    for route in ("tfrecord", "hbm"):
        spec = HipNodeAnchorLinkPredictionSpec(**cfg.trainer_args, data_route=route)
        torch.manual_seed(3)
        spec.init_model(cfg)
        spec.model = spec.model.to(dev)
        spec._ensure_engine(dev)
        specs[route] = spec
    try:
        mains = {r: list(specs[r]._main_batches(cfg, "train", loop=False)) for r in specs}
        assert len(mains["hbm"]) == len(mains["tfrecord"]) >= 2 and specs["hbm"]._resident is not None
        assert specs["tfrecord"]._resident is None
        saw_neg = saw_fewer = False
        for mb_h, mb_t in zip(mains["hbm"], mains["tfrecord"]):
            l2g = mb_t.condensed_node_type_to_subgraph_id_to_global_node_id[0]
            roots_t = mb_t.root_node_indices.tolist()
            assert mb_h.anchor_ids.tolist() == [l2g[i] for i in roots_t] and mb_h.trees_per_anchor == 5
            pos_map = mb_t.pos_supervision_edge_data[0].root_node_to_target_node_id
            neg_map = mb_t.hard_neg_supervision_edge_data[0].root_node_to_target_node_id
            assert mb_h.root_ids.index_select(0, mb_h.pos_rows).tolist() == [l2g[p] for r in roots_t for p in pos_map[r].tolist()]
            assert mb_h.root_ids.index_select(0, mb_h.neg_rows).tolist() == [l2g[p] for r in roots_t for p in neg_map[r].tolist()]
            assert mb_h.n_neg.tolist() == [int(neg_map[r].numel()) for r in roots_t]
            saw_neg |= bool(mb_h.n_neg.sum())
            saw_fewer |= bool((mb_h.n_neg < 2).any())
        assert saw_neg and saw_fewer
    finally:
        for spec in specs.values():
            spec.close()


def test_trainer_trains_the_udl_job_in_hbm_as_the_other_routes_do(workdir):
    from gigl_amd.trainer import Trainer
    runs = {}
    for name, args in (("plan", dict(data_route="hbm")), ("autograd", dict(data_route="hbm", train_plan="off")),
                       ("tfrecord", dict(data_route="tfrecord"))):
        uri = _variant(workdir, name, **args)
        seed_trainer()
        tr = Trainer()
        tr.run("job", uri, None, uri_base=workdir)
        spec = tr.training_process.trainer
        cfg = GbmlConfigPbWrapper.from_uri(uri, uri_base=workdir)
        runs[name] = (tr.training_process.route, int(getattr(spec, "train_plan_steps", 0)), [h["loss"] for h in spec.history],
                      torch.load(cfg.trained_model_uri, map_location="cpu"))
        print(f"UDL job, {name}: route {runs[name][0]}, {runs[name][1]} plan steps, losses {runs[name][2]}")
    assert runs["plan"][0] == "hbm" and runs["plan"][1] > 0 and runs["plan"][1] == len(runs["plan"][2])
    assert runs["autograd"][0] == "hbm" and runs["autograd"][1] == 0
    assert runs["tfrecord"][0] == "tfrecord" and runs["tfrecord"][1] == 0
    assert len(runs["plan"][2]) >= 2
    for name in ("autograd", "tfrecord"):
        np.testing.assert_allclose(runs["plan"][2], runs[name][2], rtol=1e-4, atol=1e-5, err_msg=f"plan vs {name}")
    np.testing.assert_allclose(runs["autograd"][2], runs["tfrecord"][2], rtol=1e-4, atol=1e-5)
    for name in ("autograd", "tfrecord"):
        for k, v in runs["plan"][3].items():
            np.testing.assert_allclose(v.numpy(), runs[name][3][k].numpy(), rtol=1e-3, atol=1e-4, err_msg=f"{k}: plan vs {name}")
