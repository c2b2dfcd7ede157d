"""A clipped, warm-up-scheduled link-prediction job end to end through the trainer: trainerArgs clip_grad_norm / factor /
total_iters (node_anchor_based_link_prediction_modeling_task_spec.py:118-132) no longer send the job back to the autograd
loop — HipNodeAnchorLinkPredictionSpec.train hands it to engine.NablpTrainPlan, whose Adam clips and schedules — and the
plan reaches the autograd loop's loss history.  The recipe of
tests/test_gpu_nablp.py::test_trainer_runs_the_gat_encoder_through_the_library_plan with the default GraphSAGE encoder."""
import os
import shutil

import numpy as np
import pytest

from conftest import seed_trainer
from test_gpu_nablp import CFG, workdir  # noqa: F401  (the module-scoped fixture: the sampled toy job)

pytestmark = pytest.mark.gpu


def test_trainer_runs_a_clipped_warm_up_job_through_the_library_plan(workdir, tmp_path):  # noqa: F811
    import yaml
    from gigl_amd import wire
    from gigl_amd.trainer import Trainer
    base = str(tmp_path / "job")
    shutil.copytree(workdir, base)
    shutil.rmtree(os.path.join(base, "out", "nablp", "split"), ignore_errors=True)
    meta_uri = os.path.join(base, "configs", "nablp_preprocessed_metadata.yaml")
    meta = yaml.safe_load(open(meta_uri))
    node = meta["condensedNodeTypeToPreprocessedMetadata"]["0"]
    src_dir = os.path.join(base, node["tfrecordUriPrefix"])
    ids = sorted(int(wire.decode_tf_example(r)["node_id"][0])
                 for f in sorted(os.listdir(src_dir)) for r in wire.iter_tfrecords(open(os.path.join(src_dir, f), "rb").read()))
    rng = np.random.default_rng(0)
    wide = os.path.join(base, "tables", "nodes_wide")
    os.makedirs(wide)
    wire.write_tfrecords(os.path.join(wide, "data.tfrecord"), [
        wire.encode_tf_example({"node_id": np.array([i], np.int64), "feat": rng.standard_normal(8).astype(np.float32)})
        for i in ids])
    node.update(featureDim=8, featureKeys=["feat"], tfrecordUriPrefix="tables/nodes_wide")
    yaml.safe_dump(meta, open(meta_uri, "w"))
    doc = yaml.safe_load(open(os.path.join(base, CFG)))
    args = doc["trainerConfig"]["trainerArgs"]
    args.update(clip_grad_norm="0.5", factor="0.5", total_iters="2")
    doc["inferencerConfig"]["inferencerArgs"].update(args)
    runs = {}
    old = os.environ.get("GIGL_AMD_ROUTE")
    os.environ["GIGL_AMD_ROUTE"] = "hbm"
    try:
        for mode in ("auto", "off"):
            args["train_plan"] = mode
            yaml.safe_dump(doc, open(os.path.join(base, CFG), "w"))
            seed_trainer()
            tr = Trainer()
            tr.run("job", CFG, None, uri_base=base)
            assert tr.training_process.route == "hbm"
            spec = tr.training_process.trainer
            assert spec.clip_grad_norm == 0.5 and spec._lr_scheduler_kwargs == {"factor": 0.5, "total_iters": 2}
            runs[mode] = ([h["loss"] for h in spec.history], int(getattr(spec, "train_plan_steps", 0)))
    finally:
        if old is None:
            os.environ.pop("GIGL_AMD_ROUTE", None)
        else:
            os.environ["GIGL_AMD_ROUTE"] = old
    (h_plan, n_plan), (h_auto, n_auto) = runs["auto"], runs["off"]
    print("clipped warm-up job: plan losses", h_plan, "autograd losses", h_auto)
    assert n_plan == len(h_plan) >= 4 and n_auto == 0
    np.testing.assert_allclose(h_plan, h_auto, rtol=2e-3)
