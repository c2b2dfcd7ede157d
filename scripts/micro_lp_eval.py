#!/usr/bin/env python3
"""What one validation pass of a default link-prediction job costs through its two routes, at the default shape: 10 batches
(num_val_batches) x 2,048 anchors (main_sample_batch_size) + 1 positive each, 512 random negatives per batch, fan-out
[25, 10], GraphSAGE 100 -> 256 -> 128 L2-normalised over the products-shaped graph bench/train.py builds.
  plan    eval_plan on:  HipNodeAnchorLinkPredictionSpec._validate_with_plan -> engine.NablpTrainPlan.evaluate (one library
          call per batch, one host read per pass)
  python  eval_plan off: HipNodeAnchorLinkPredictionSpec.validate (batch graphs sampled in HBM, the autograd-free forward, then
          hit_rate_at_k / mean_reciprocal_rank once per anchor)
Both in one process over the same anchors and negatives, from the same weights: a warm-up pass of each, then --reps passes
of each, alternating; a host clock around each pass, which ends in a synchronise (the plan's single host read; the Python
loop's .item()).  Both times and both routes' metrics go to --out (profiles/lp_eval.txt) and to stdout as one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gigl_amd.base import EvalMetricType  # noqa: E402
from gigl_amd.engine import HipEngine, NablpTrainPlan  # noqa: E402
from gigl_amd.hbm import ResidentGraph  # noqa: E402
from gigl_amd.link_prediction import LinkPredictionDecoder, LinkPredictionGNN  # noqa: E402
from gigl_amd.models import GraphSAGE  # noqa: E402
from gigl_amd.nablp_spec import HipNodeAnchorLinkPredictionSpec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--batches", type=int, default=10)
ap.add_argument("--anchors", type=int, default=2048)
ap.add_argument("--negatives", type=int, default=512)
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "lp_eval.txt"))
a = ap.parse_args()

eng = HipEngine(0)
dev = eng.device
wl = argparse.Namespace(workload="products")
n, d = bench.build_workload(eng, wl)
eng._graph_out = eng._graph  # (bidirectionalised: a node's out-neighbours are its in-neighbours)
fan, hid, emb, P = [25, 10], wl._workload[2], 128, 1
st = torch.cuda.Stream(device=dev)
torch.cuda.synchronize()
eng.bind_stream(st)
torch.cuda.set_stream(st)
res = ResidentGraph.from_engine(eng, np.arange(n, dtype=np.int64), fan)
torch.manual_seed(0)
model = LinkPredictionGNN(encoder=GraphSAGE(d, hid, emb, num_layers=2, should_l2_normalize_embedding_layer_output=True),
                          decoder=LinkPredictionDecoder()).to(dev)
model.encoder.engine = model.decoder.engine = eng
spec = HipNodeAnchorLinkPredictionSpec(main_sample_batch_size=a.anchors,
                                       random_negative_sample_batch_size_for_evaluation=a.negatives)
spec.model, spec._resident, spec._engine, spec._device = model, res, eng, dev
# the validation split: anchors with at least one positive, and how many each has
ids = np.random.default_rng(42).permutation(n)[: 2 * a.batches * a.anchors].astype(np.int64)
_, cnt = eng.sample_positives(torch.from_numpy(ids.astype(np.uint32).view(np.int32)).to(dev), P, sampling_seed=res.seed)
cnt = cnt.cpu().numpy().astype(np.int64)
ids, n_pos = ids[cnt > 0][: a.batches * a.anchors], cnt[cnt > 0][: a.batches * a.anchors]
assert ids.size == a.batches * a.anchors, "too few anchors with a positive"
task = next(iter(spec.tasks._task_to_fn_map.values()))
plan = NablpTrainPlan(eng, model.encoder, a.anchors, P, a.negatives, fan, temperature=float(task.loss._temperature or 0.0),
                      remove_accidental_hits=bool(task.loss._remove_accidental_hits))


def in_plan():
    return spec._validate_with_plan(plan, res.nablp_root_batches(ids, n_pos, a.anchors, P),
                                    res.random_negative_root_batches(a.negatives), a.batches)


def in_python():
    return spec.validate(res.nablp_batches(ids, n_pos, a.anchors, P), res.random_negative_batches(a.negatives), None, dev,
                         a.batches)


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = f()
    torch.cuda.synchronize()  # (both routes have synchronised already: their results are host values)
    return time.perf_counter() - t0, m


routes = {"plan": in_plan, "python": in_python}
times = {k: [] for k in routes}
metrics = {}
for k, f in routes.items():  # warm-up: first-call allocations, the plan's eager and captured graph parts
    timed(f)
for _ in range(a.reps):
    for k, f in routes.items():
        t, metrics[k] = timed(f)
        times[k].append(t)
plan.close()
flat = lambda m: {"loss": m[EvalMetricType.loss], "mrr": m[EvalMetricType.mrr], "hits": list(m[EvalMetricType.hits])}
out = dict(nodes=n, feature_dim=d, hidden=hid, out=emb, fanouts=fan, batches=a.batches, anchors_per_batch=a.anchors,
           negatives_per_batch=a.negatives, reps=a.reps,
           seconds_per_pass={k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in times.items()},
           python_over_plan=float(np.median(times["python"]) / np.median(times["plan"])),
           metrics={k: flat(m) for k, m in metrics.items()})
line = json.dumps(out)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write("# scripts/micro_lp_eval.py: one validation pass (seconds, host clock around work that ends in a synchronise)\n")
    for k, v in times.items():
        fh.write(f"{k:7s} median {np.median(v):.4f} s  min {min(v):.4f} s  max {max(v):.4f} s  ({a.reps} passes, alternating)\n")
    for k, m in metrics.items():
        fh.write(f"{k:7s} metrics {json.dumps(flat(m))}\n")
    fh.write(line + "\n")
torch.cuda.synchronize()
torch.cuda.set_stream(torch.cuda.default_stream(dev))
eng.bind_stream(None)
eng._graph_out = None  # (an alias of the main graph: freed once)
eng.close()
