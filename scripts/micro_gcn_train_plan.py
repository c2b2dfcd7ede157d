#!/usr/bin/env python3
"""What the library's GCN training plan (engine.GcnTrainPlan, gigl_gcn_train_plan_*) buys over the autograd route the stock
TwoLayerGCN job took before it (GIGL_AMD_TRAIN_PLAN=0: a GraphData built on the device per batch, models_attn.TwoLayerGCN's
autograd forward / backward, torch.optim.Adam), at two shapes:
  cora      the Cora-shaped graph of bench (2,708 nodes, d = 1,433, hidden 16, 7 classes), fan-out [10, 10], B = 256;
  products  the products-shaped graph of bench (d = 100, hidden 256, 47 classes), fan-out [25, 10], B = 1,024.
One process holds both routes over the same seeded batches and times them ALTERNATELY on a device-synchronised host clock:
--reps timings of --steps steps each after a warm-up, the spread printed beside the medians.

--kernels (meant for a run of its own under `rocprofv3 --kernel-trace --stats`): at the products shape, the first layer's
aggregation over ONE batch graph and the table by the three kernels that can do it — gcn_gather_rows_kernel
(gigl_gcn_gather), gather_mean_kernel (gigl_gather_mean: the yardstick) and the older gcn_gather_kernel (gigl_gcn_aggregate)
— --launches times each, with the bytes each has to move computed from the batch's shapes and, from device events around
the back-to-back launches, the implied share of the HBM peak.

One JSON line per run, appended to --out (profiles/gcn_train_plan.txt)."""
import argparse
import copy
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from bench.common import HBM_PEAK_GBS  # noqa: E402
from gigl_amd._lib import GIGL_META_LEVEL0, check  # noqa: E402
from gigl_amd.engine import GcnTrainPlan, HipEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--shapes", type=str, default="cora,products")
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "gcn_train_plan.txt"))
a = ap.parse_args()
SHAPES = {"cora": ([10, 10], 256), "products": ([25, 10], 1024)}
POOL = 8


def _engine(shape):
    eng = HipEngine(0)
    args = argparse.Namespace(workload=shape)
    n, d = bench.build_workload(eng, args)
    return eng, n, d, args._workload[2], args._workload[3]


def routes(shape):
    from gigl_amd.hbm import ResidentGraph
    from gigl_amd.models_attn import TwoLayerGCN
    fan, B = SHAPES[shape]
    eng, n, d, hid, classes = _engine(shape)
    dev = eng.device
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    torch.cuda.set_stream(st)
    gp = torch.Generator(device="cpu")
    gp.manual_seed(42)
    pool = min(POOL, n // B)
    roots = torch.randperm(n, generator=gp)[: pool * B].view(pool, B).to(torch.int32).to(dev)
    labels = torch.randint(0, classes, (pool, B), generator=gp).to(dev)
    torch.manual_seed(0)
    model = TwoLayerGCN(d, classes, hid_dim=hid).to(dev)  # (is_training: p = 0.5 in both routes, each from its own stream)
    # ---- the plan
    plan = GcnTrainPlan(eng, copy.deepcopy(model), B, fan, lr=0.01, weight_decay=5e-4, dropout_seed=1)

    def plan_steps(k):
        for i in range(k):
            j = i % pool
            plan.step(roots[j], labels[j], next_roots=roots[(j + 1) % pool] if i + 1 < k else None)
    # ---- the autograd route, as HipGraphSageNodeClassificationSpec._train runs it over ResidentGraph.train_batches
    res = ResidentGraph.from_engine(eng, np.arange(n), fan)
    res.train_as_graph_data = True
    auto = copy.deepcopy(model)
    auto.engine = eng
    auto.train()
    opt = torch.optim.Adam(auto.parameters(), lr=0.01, weight_decay=5e-4, capturable=True)

    def auto_steps(k):
        for i in range(k):
            j = i % pool
            opt.zero_grad()
            g, ri = res.graph_data(roots[j])
            loss = torch.nn.functional.cross_entropy(auto(g)[ri], labels[j])
            loss.backward()
            opt.step()
        eng.bind_stream(st)  # (graph_data binds the engine to the current stream: the same one)

    # warm-up: the plan's eager step, its captured step, replays — growing first if a batch outgrows the regular workspace
    losses = plan.run_steps(2 * pool, lambda i: dict(roots=roots[i % pool], labels=labels[i % pool]))
    assert bool(torch.isfinite(losses).all()), "a warm-up batch failed in the wide plan"
    auto_steps(pool)
    torch.cuda.synchronize()

    def timed(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(a.steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    times = {"plan": [], "autograd": []}
    for _ in range(a.reps):
        times["plan"].append(timed(plan_steps))
        times["autograd"].append(timed(auto_steps))
    assert np.isfinite(float(plan.loss.cpu()[0])), "a timed batch failed"
    stat = lambda v: {"median": float(np.median(v)), "min": min(v), "max": max(v)}
    out = dict(nodes=n, feature_dim=d, hidden=hid, classes=classes, fanouts=fan, batch=B, plan_wide=bool(plan.wide),
               ms_per_step={k: stat(v) for k, v in times.items()},
               spread_ms={k: max(v) - min(v) for k, v in times.items()},
               speedup=float(np.median(times["autograd"]) / np.median(times["plan"])))
    plan.close()
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    eng.bind_stream(None)
    eng.close()
    return out


def kernels():
    fan, B = SHAPES["products"]
    eng, n, d, _, _ = _engine("products")
    dev, lib = eng.device, eng._lib
    gp = torch.Generator(device="cpu")
    gp.manual_seed(42)
    roots = torch.randperm(n, generator=gp)[:B].to(torch.int32).to(dev)
    u = eng.union_build(eng.sample_khop(roots, fan))
    meta = u.meta.cpu().tolist()
    n_nodes, n1 = meta[0], meta[GIGL_META_LEVEL0 + 1]
    rows_cap = B * (1 + fan[0])
    assert n1 <= rows_cap
    rp, re, col = u.rowptr.cpu().numpy(), u.rowend.cpu().numpy(), u.col.cpu().numpy()
    lens = (re[:n1] - rp[:n1]).astype(np.int64)
    edges = int(lens.sum())
    # who reads whom among the ROOT rows (the backward's transposed lists): the longest list
    n0 = meta[GIGL_META_LEVEL0]
    root_cols = np.concatenate([col[rp[i]:re[i]] for i in range(n0)]) if n0 else np.zeros(0, np.int32)
    readers = np.bincount(root_cols, minlength=1)
    s = 4 if eng.feat_dtype == 0 else 2
    by = dict(gcn_gather=edges * (4 + 4 + d * s) + n1 * (d * s + 4 + 4 * d + 8),
              gather_mean=edges * (4 + d * s) + n1 * (d * s + 8 * d + 8))
    p_ = lambda t: C.c_void_p(t.data_ptr())
    dinv = torch.empty(int(u.nodes.numel()), dtype=torch.float32, device=dev)
    out = torch.empty((rows_cap, 2 * d), dtype=torch.float32, device=dev)
    n1_dev = u.meta[GIGL_META_LEVEL0 + 1: GIGL_META_LEVEL0 + 2]
    torch.cuda.synchronize()
    check(lib.gigl_gcn_dinv(eng._ctx, p_(u.rowptr), p_(u.rowend), p_(u.col), p_(u.meta), int(u.nodes.numel()), p_(dinv)), eng._ctx)

    def new():
        check(lib.gigl_gcn_gather(eng._ctx, eng._feat_ptr, eng.feat_dtype, d, p_(u.nodes), p_(dinv), p_(u.rowptr), p_(u.rowend),
                                  p_(u.col), p_(n1_dev), rows_cap, p_(out)), eng._ctx)
    agg = torch.empty((int(u.nodes.numel()), d), dtype=torch.float32, device=dev)
    calls = {"gcn_gather_rows_kernel": new,
             "gather_mean_kernel": lambda: eng.gather_mean(None, d, u.nodes, u.rowptr, u.rowend, u.col, n1_dev, rows_cap, out=out),
             "gcn_gather_kernel (+ gcn_dinv_kernel)": lambda: eng.gcn_aggregate(None, d, u.nodes, u, n1_dev, None, 0, out=agg)}
    us = {}
    for name, fn in calls.items():
        for _ in range(10):
            fn()
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.launches):
            fn()
        eng.synchronize()
        us[name] = (time.perf_counter() - t0) * 1e6 / a.launches
    res = dict(mode="kernels", nodes=n, feature_dim=d, fanouts=fan, batch=B, union_nodes=n_nodes, rows=n1, edges=edges,
               row_length={"median": float(np.median(lens)), "max": int(lens.max())},
               reader_list_of_the_root_rows={"median": float(np.median(readers[readers > 0])), "max": int(readers.max())},
               bytes=by, us_per_back_to_back_launch=us,
               hbm_share_from_those={k: by[k] / (us[{"gcn_gather": "gcn_gather_rows_kernel", "gather_mean": "gather_mean_kernel"}[k]]
                                                 * 1e-6) / 1e9 / HBM_PEAK_GBS for k in by},
               note="kernel times proper: the rocprofv3 --kernel-trace --stats table of this run")
    eng.close()
    return res


def main():
    lines = [kernels()] if a.kernels else [dict(mode="routes", shape=s, steps_per_timing=a.steps, reps=a.reps, **routes(s))
                                           for s in a.shapes.split(",")]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            text = json.dumps(line)
            print(text, flush=True)
            f.write(text + "\n")


main()
