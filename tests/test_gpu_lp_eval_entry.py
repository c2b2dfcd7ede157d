"""The link-prediction trainer's validation and test passes inside the library plan (trainerArgs eval_plan, default auto:
NablpTrainPlan.evaluate, one library call per batch) against the per-anchor Python loop they replace (eval_plan = "off"),
on the reference fixture job of tests/test_gpu_nablp.py over the in-HBM route: same history, same metrics, and no
per-anchor metric call left in the auto run."""
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import seed_trainer

from gigl_amd.base import EvalMetricType

pytestmark = pytest.mark.gpu

CFG = "configs/nablp_frozen_gbml_config.yaml"


@pytest.fixture(scope="module")
def workdir(golden_dir, tmp_path_factory):
    base = tmp_path_factory.mktemp("gigl_lp_eval")
    shutil.copytree(os.path.join(golden_dir, "configs"), base / "configs")
    shutil.copytree(os.path.join(golden_dir, "ref_assets"), base / "ref_assets")
    from gigl_amd.subgraph_sampler import SubgraphSampler
    SubgraphSampler().run("job", CFG, None, uri_base=str(base))
    shutil.rmtree(os.path.join(str(base), "out", "nablp", "split"), ignore_errors=True)  # (no split-generator output)
    return str(base)


def test_fixture_job_validates_in_the_plan_as_the_python_loop_does(workdir, tmp_path, monkeypatch):
    import yaml
    import gigl_amd.base as base_mod
    import gigl_amd.nablp_spec as spec_mod
    from gigl_amd.trainer import Trainer
    calls = {"n": 0}
    real = base_mod.hit_rate_at_k

    def counted(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)
    monkeypatch.setattr(base_mod, "hit_rate_at_k", counted)
    monkeypatch.setattr(spec_mod, "hit_rate_at_k", counted)
    monkeypatch.setenv("GIGL_AMD_ROUTE", "hbm")
    runs = {}
    for mode in ("auto", "off"):
        job = str(tmp_path / mode)
        shutil.copytree(workdir, job)
        if mode != "auto":  # (auto is the default: the job's own arguments)
            doc = yaml.safe_load(open(os.path.join(job, CFG)))
            doc["trainerConfig"]["trainerArgs"]["eval_plan"] = mode
            yaml.safe_dump(doc, open(os.path.join(job, CFG), "w"))
        calls["n"] = 0
        seed_trainer()
        tr = Trainer()
        metrics = tr.run("job", CFG, None, uri_base=job)
        trn = tr.training_process.trainer
        assert tr.training_process.route == "hbm" and trn.train_plan_steps > 0  # (the step ran as the library plan)
        runs[mode] = (trn.history, {k: m.value for k, m in metrics.metrics.items()}, calls["n"])
    (h_a, m_a, n_a), (h_o, m_o, n_o) = runs["auto"], runs["off"]
    print("validation in the plan:", [h["val"] for h in h_a if "val" in h], m_a)
    print("validation in Python:  ", [h["val"] for h in h_o if "val" in h], m_o, f"({n_o} hit_rate_at_k calls)")
    assert n_o > 0 and n_a == 0, (n_o, n_a)  # the auto run issued no per-anchor work
    assert len(h_a) == len(h_o) >= 4 and any("val" in h for h in h_a)
    np.testing.assert_allclose([h["loss"] for h in h_a], [h["loss"] for h in h_o], rtol=2e-3)
    for a, b in zip(h_a, h_o):
        assert ("val" in a) == ("val" in b)
        if "val" in a:
            assert set(a["val"]) == set(b["val"]) == {EvalMetricType.mrr, EvalMetricType.loss, EvalMetricType.hits}
            assert isinstance(a["val"][EvalMetricType.mrr], float) and isinstance(a["val"][EvalMetricType.loss], float)
            assert isinstance(a["val"][EvalMetricType.hits], list) and len(a["val"][EvalMetricType.hits]) == 6
            np.testing.assert_allclose(a["val"][EvalMetricType.loss], b["val"][EvalMetricType.loss], rtol=2e-3)
            np.testing.assert_allclose(a["val"][EvalMetricType.mrr], b["val"][EvalMetricType.mrr], rtol=0, atol=8e-3)
            np.testing.assert_allclose(a["val"][EvalMetricType.hits], b["val"][EvalMetricType.hits], rtol=0, atol=8e-3)
    assert m_a.keys() == m_o.keys()
    np.testing.assert_allclose(m_a["loss"], m_o["loss"], rtol=2e-3)
    for k in m_a:
        if k != "loss":
            np.testing.assert_allclose(m_a[k], m_o[k], rtol=0, atol=8e-3)
