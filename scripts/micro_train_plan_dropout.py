#!/usr/bin/env python3
"""What dropout costs in the library training plans (gigl_nablp_train_plan_set_dropout / gigl_sage_train_plan_set_dropout:
after every activated layer one more launch that reads and writes the layer's output in place, and in the backward one mask
+ scale launch in place of the rectifier's mask), at the shapes the benchmark trains on the products-shaped graph:
  lp   bench/train.py's link-prediction leg — GraphSAGE 100 -> 256 -> 128 L2-normalised, 2048 anchors + 1 positive each +
       512 random negatives, fan-out [25, 10];
  snc  its node-classification leg — GraphSAGE 100 -> 256 -> 47, 1024 roots, fan-out [25, 10].
One process holds, per task, the plan WITHOUT the setter (the baseline: the launches the plans always had) and the plan at
p = 0.5 over the same seeded batches from the same weights and times them ALTERNATELY: --steps steps per timing between two
HIP events on the plans' stream (the next batch announced, as the trainers issue them), --reps timings each after a warm-up,
so that the spread is visible next to the difference.  Beside the times: the bytes the forward's extra pass moves per step
— 2 * rows * width * 4 per activated layer and encode, rows read from the first batch's graph — and the HBM rate the
difference would imply if that pass were all of it.  One JSON line, appended to --out (profiles/train_plan_dropout.txt)."""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gigl_amd._lib import GIGL_META_LEVEL0  # noqa: E402
from gigl_amd.engine import HipEngine, NablpTrainPlan, SageTrainPlan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--p", type=float, default=0.5)
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "train_plan_dropout.txt"))
a = ap.parse_args()
POOL, FAN, SEED = 16, [25, 10], 1


def extra_bytes(eng, root_sets, model):
    """2 * rows * width * 4 per activated layer and encode: rows = the nodes layer l computes in the first batch's graph"""
    L, total = model.num_layers, 0
    for roots in root_sets:
        u = eng.union_build(eng.sample_khop(roots, FAN))
        meta = u.meta.cpu()
        for l, conv in enumerate(model.conv_layers):
            if l < L - 1 or model.activation_after_last_conv:
                total += 2 * int(meta[GIGL_META_LEVEL0 + (L - 1 - l)]) * int(conv.out_channels) * 4
    return total


def main():
    from gigl_amd.models import GraphSAGE
    eng = HipEngine(0)
    dev = eng.device
    args = argparse.Namespace(workload="products")
    n, d = bench.build_workload(eng, args)
    eng._graph_out = eng._graph  # (bidirectionalised: a node's out-neighbours are its in-neighbours)
    hid, classes = args._workload[2], args._workload[3]
    gp = torch.Generator(device="cpu")
    gp.manual_seed(42)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    torch.cuda.set_stream(st)
    tasks = {}
    # ---- link prediction
    B, n_neg, emb = 2048, 512, 128
    torch.manual_seed(0)
    lp_model = GraphSAGE(d, hid, emb, num_layers=2, should_l2_normalize_embedding_layer_output=True).to(dev)
    anchors = torch.randperm(n, generator=gp)[: POOL * B].view(POOL, B).to(torch.int32).to(dev)
    negs = torch.randint(0, n, (POOL, n_neg), generator=gp).to(torch.int32).to(dev)
    lp_batches = []
    for i in range(POOL):
        roots, cnt = eng.nablp_main_roots(anchors[i], 1, 0, sampling_seed=42)
        lp_batches.append((roots, cnt[:B].contiguous(), negs[i].contiguous()))
    lp_plans = {p: NablpTrainPlan(eng, copy.deepcopy(lp_model), B, 1, n_neg, FAN, temperature=0.07, remove_accidental_hits=True,
                                  lr=5e-3, weight_decay=1e-6, dropout=p, dropout_seed=SEED) for p in (0.0, a.p)}

    def lp_steps(p, k):
        for i in range(k):
            j, jn = i % POOL, (i + 1) % POOL
            lp_plans[p].step(*lp_batches[j], next_roots=(lp_batches[jn][0], lp_batches[jn][2]) if i + 1 < k else None)
    tasks["lp"] = (lp_steps, lambda p: lp_plans[p].step(*lp_batches[0]).clone()[0],
                   extra_bytes(eng, (lp_batches[0][0], lp_batches[0][2]), lp_model))
    # ---- node classification
    Bn = 1024
    torch.manual_seed(0)
    nc_model = GraphSAGE(d, hid, classes, num_layers=2).to(dev)
    nc_roots = torch.randperm(n, generator=gp)[: POOL * Bn].view(POOL, Bn).to(torch.int32).to(dev)
    nc_labels = torch.randint(0, classes, (POOL, Bn), generator=gp).to(dev)
    nc_plans = {p: SageTrainPlan(eng, copy.deepcopy(nc_model), Bn, FAN, lr=0.01, weight_decay=5e-4, dropout=p, dropout_seed=SEED)
                for p in (0.0, a.p)}

    def nc_steps(p, k):
        for i in range(k):
            j = i % POOL
            nc_plans[p].step(nc_roots[j], nc_labels[j], next_roots=nc_roots[(j + 1) % POOL] if i + 1 < k else None)
    tasks["snc"] = (nc_steps, lambda p: nc_plans[p].step(nc_roots[0], nc_labels[0]).clone()[0],
                    extra_bytes(eng, (nc_roots[0],), nc_model))
    st.synchronize()

    def timed(steps, p, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(st)
        steps(p, k)
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    out = {}
    for name, (steps, first, nbytes) in tasks.items():
        for p in (0.0, a.p):  # warm-up: eager step, captured step, replays
            assert np.isfinite(float(first(p))), f"{name} p={p}: the first batch outgrew the plan's workspace"
            steps(p, 8)
        times = {p: [] for p in (0.0, a.p)}
        for _ in range(a.reps):
            for p in (0.0, a.p):
                times[p].append(timed(steps, p, a.steps))
        stat = lambda v: {"median": float(np.median(v)), "min": min(v), "max": max(v)}
        delta_ms = float(np.median(times[a.p]) - np.median(times[0.0]))
        out[name] = dict(ms_per_step={"no setter": stat(times[0.0]), f"p={a.p}": stat(times[a.p])},
                         spread_us=1e3 * max(max(v) - min(v) for v in times.values()), delta_us=1e3 * delta_ms,
                         forward_extra_bytes_per_step=nbytes,
                         implied_hbm_GBps=(nbytes / (delta_ms * 1e-3) / 1e9) if delta_ms > 0 else None)
    for plans in (lp_plans, nc_plans):
        for p in plans.values():
            p.close()
    line = json.dumps(dict(nodes=n, feature_dim=d, hidden=hid, fanouts=FAN, steps_per_timing=a.steps, reps=a.reps, p=a.p, **out))
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    eng.bind_stream(None)
    eng._graph_out = None  # (an alias of the main graph: freed once)
    eng.close()


main()
