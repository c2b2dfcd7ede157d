#!/usr/bin/env python3
"""What the one-call GCN inference plan (engine.GcnPlan, gigl_gcn_plan_*) buys a validation pass of the stock TwoLayerGCN
job over the staged route ResidentGraph.encode took before it (batch.force_staged: hip_batch's sample and union calls +
models_attn.TwoLayerGCN._forward_union per batch), and what each of the plan's two fast paths buys over its fallback, at two
shapes:
  cora      the Cora-shaped graph of bench (2,708 nodes, d = 1,433, hidden 16, 7 classes), fan-out [10, 10], B = 256;
  products  the products-shaped graph of bench (d = 100, hidden 256, 47 classes), fan-out [25, 10], B = 1,024.
A pass is --batches batches through ResidentGraph.encode.  One process holds every route over the same batches and times
them ALTERNATELY on a device-synchronised host clock: --reps timings after a warm-up, the spread printed beside the medians.
Routes: staged; the plan with layer 1 aggregate-first or over the projected table (X W1^T once per model state), each with
layer 2 fused into the roots' rows or as gather + projection + copy.

One JSON line per shape, appended to --out (profiles/gcn_plan.txt)."""
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
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "gcn_plan.txt"))
a = ap.parse_args()
SHAPES = {"cora": ([10, 10], 256), "products": ([25, 10], 1024)}
PLAN_ROUTES = [(proj, fused) for proj in (False, True) for fused in (True, False)]


def routes(shape):
    from gigl_amd.hbm import ResidentGraph
    from gigl_amd.models_attn import TwoLayerGCN
    fan, B = SHAPES[shape]
    eng = HipEngine(0)
    args = argparse.Namespace(workload=shape)
    n, d = bench.build_workload(eng, args)
    hid, classes = args._workload[2], args._workload[3]
    dev = eng.device
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_stream(st)
    gp = torch.Generator(device="cpu")
    gp.manual_seed(42)
    k = min(a.batches, n // B)
    ids = torch.randperm(n, generator=gp)[: k * B].numpy()
    torch.manual_seed(0)
    model = TwoLayerGCN(d, classes, hid_dim=hid, is_training=False).to(dev)
    res = ResidentGraph.from_engine(eng, np.arange(n), fan)
    batches = list(res.root_batches(ids, B, 1))
    staged = list(res.root_batches(ids, B, 1))
    for hb in staged:
        hb.force_staged = True
    rows = [res.encode(model, hb) for hb in batches]  # creates the plan; a batch that overflows is redone staged
    (plan,) = [p for p in res._plans.values() if p is not None]
    redone = int(res.overflow_redone)
    as_configured = (plan._proj is not None, plan.fused_root())  # what ResidentGraph.encode set up: the entry points' route
    table = eng.gcn_project_features(model.conv1.lin.weight)
    eng.synchronize()

    def set_route(proj, fused):
        plan.set_projected_input(table if proj else None)
        plan.set_fused_root(fused)

    def one_pass(which):
        for hb in which:
            res.encode(model, hb)

    def timed(which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one_pass(which)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    name = lambda proj, fused: ("projected" if proj else "aggregate_first") + ("+fused_root" if fused else "+root_fallback")
    times = {"staged": []}
    worst = 0.0
    ref = [res.encode(model, hb) for hb in staged]
    for proj, fused in PLAN_ROUTES:  # warm-up of every route, and the routes against the staged rows
        set_route(proj, fused)
        times[name(proj, fused)] = []
        for hb, want in zip(batches, ref):
            worst = max(worst, float((res.encode(model, hb) - want).abs().max()))
        one_pass(batches)
    one_pass(staged)
    for _ in range(a.reps):
        times["staged"].append(timed(staged))
        for proj, fused in PLAN_ROUTES:
            set_route(proj, fused)
            times[name(proj, fused)].append(timed(batches))
    stat = lambda v: {"median": float(np.median(v)), "min": min(v), "max": max(v)}
    default = name(*as_configured)
    out = dict(nodes=n, feature_dim=d, hidden=hid, classes=classes, fanouts=fan, batch=B, batches=k,
               fused_root_by_shape=bool((set_route(False, True), plan.fused_root())[1]),
               calls_redone_staged_in_the_first_pass=redone, largest_difference_from_the_staged_rows=worst,
               route_the_entry_points_take=default,
               ms_per_pass={r: stat(v) for r, v in times.items()},
               spread_ms={r: max(v) - min(v) for r, v in times.items()},
               speedup_over_staged=float(np.median(times["staged"]) / np.median(times[default])))
    del rows
    res.close()
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    eng.close()
    return out


def main():
    lines = [dict(mode="validation_pass", shape=s, reps=a.reps, **routes(s)) for s in a.shapes.split(",")]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            text = json.dumps(line)
            print(text, flush=True)
            f.write(text + "\n")


main()
