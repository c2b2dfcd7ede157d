#!/usr/bin/env python3
"""What scoring on the device (ResidentGraph.score_roots: one call of the one-call plan per batch, gigl_nc_eval_metrics on
its rows, ONE host read per pass) buys a validation pass of a node-classification job over the spec's score() as the
trainer routed it before — a host read per batch; for the stock TwoLayerGCN over ResidentGraph.encode (the one-call plan
with its own blocking overflow read), for GraphSAGE over train_batches and the module's staged forward — at two shapes:
  cora      the Cora-shaped graph of bench (2,708 nodes, d = 1,433, hidden 16, 7 classes), fan-out [10, 10], B = 256;
  products  the products-shaped graph of bench (d = 100, hidden 256, 47 classes), fan-out [25, 10], B = 1,024.
A pass is --batches batches.  One process holds both routes over the same roots and labels and times them ALTERNATELY on
a device-synchronised host clock: --reps timings after a warm-up pass of each, the spread printed beside the medians.
`keeps_auto` applies the default rule: the new route beats the old one by more than the larger of the two spreads.

One JSON line per (shape, model), appended to --out (profiles/nc_score.txt)."""
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
from gigl_amd.engine import HipEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--shapes", type=str, default="cora,products")
ap.add_argument("--models", type=str, default="TwoLayerGCN,GraphSAGE")
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "nc_score.txt"))
a = ap.parse_args()
SHAPES = {"cora": ([10, 10], 256), "products": ([25, 10], 1024)}


def measure(shape, kind):
    from gigl_amd.hbm import ResidentGraph
    from gigl_amd.models import GraphSAGE
    from gigl_amd.models_attn import TwoLayerGCN
    from gigl_amd.task_specs import HipGraphSageNodeClassificationSpec
    fan, B = SHAPES[shape]
    eng = HipEngine(0)
    args = argparse.Namespace(workload=shape)
    n, d = bench.build_workload(eng, args)
    hid, classes = args._workload[2], args._workload[3]
    dev = eng.device
    gp = torch.Generator(device="cpu")
    gp.manual_seed(42)
    k = min(a.batches, n // B)
    ids = torch.randperm(n, generator=gp)[: k * B].numpy()
    labels = torch.randint(0, classes, (ids.size,), generator=gp).numpy()
    torch.manual_seed(0)
    if kind == "TwoLayerGCN":
        model = TwoLayerGCN(d, classes, hid_dim=hid, is_training=False).to(dev)
    else:
        model = GraphSAGE(in_dim=d, hid_dim=hid, out_dim=classes, num_layers=2).to(dev)
    res = ResidentGraph.from_engine(eng, np.arange(n), fan)
    res.train_as_graph_data = kind != "GraphSAGE"
    spec = HipGraphSageNodeClassificationSpec(main_sample_batch_size=B, out_dim=classes, hid_dim=hid)
    spec.model, spec._engine, spec._resident, spec._device = model, eng, res, dev
    model.engine = eng

    def old_pass():  # the parent's _split_batches + score()
        if spec._scores_through_encode():
            batches = res.root_batches(ids, B, 1, labels=labels)
        else:
            batches = res.train_batches(ids, labels, B)
        return spec.score(batches, dev)

    def new_pass():
        model.eval()
        m = res.score_roots(model, ids, labels, B)
        return m["correct"] / max(m["evaluated"], 1), m

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    acc_old = old_pass()          # warm-up of each route (plans are created and captured here)
    acc_new, first = new_pass()
    old_pass(), new_pass()
    times = {"score": [], "score_roots": []}
    redone = 0
    for _ in range(a.reps):
        times["score"].append(timed(old_pass)[0])
        t, (_, m) = timed(new_pass)
        times["score_roots"].append(t)
        redone = max(redone, m["redone"])
    stat = lambda v: {"median": float(np.median(v)), "min": min(v), "max": max(v)}
    spread = {r: max(v) - min(v) for r, v in times.items()}
    gain = float(np.median(times["score"]) - np.median(times["score_roots"]))
    out = dict(model=kind, nodes=n, feature_dim=d, hidden=hid, classes=classes, fanouts=fan, batch=B, batches=k,
               old_route="encode" if spec._scores_through_encode() else "train_batches",
               accuracy={"score": acc_old, "score_roots": acc_new}, calls_redone_staged_per_pass=redone,
               calls_redone_staged_in_the_first_pass=first["redone"],
               ms_per_pass={r: stat(v) for r, v in times.items()}, spread_ms=spread,
               speedup=float(np.median(times["score"]) / np.median(times["score_roots"])),
               keeps_auto=bool(gain > max(spread.values())))
    res.close()
    torch.cuda.synchronize()
    eng.close()
    return out


def main():
    lines = [dict(mode="validation_pass", shape=s, reps=a.reps, **measure(s, m))
             for s in a.shapes.split(",") for m in a.models.split(",")]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            text = json.dumps(line)
            print(text, flush=True)
            f.write(text + "\n")


main()
