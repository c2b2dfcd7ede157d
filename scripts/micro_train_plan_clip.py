#!/usr/bin/env python3
"""What gradient-norm clipping costs inside the link-prediction training plans (the norm pass re-reads the weight
gradients' partial sums once and adds two launches to the step), at the two shapes the benchmark trains:
  sage  bench/train.py's link-prediction leg: the products-shaped graph, GraphSAGE 100 -> 256 -> 128 L2-normalised,
        2048 anchors + 1 positive each + 512 random negatives, fan-out [25, 10]            (engine.NablpTrainPlan)
  gat   bench/gat_lp.py's training leg's step: 768-wide fp16 rows, GAT 2 heads x 128 -> 128, 1024 anchors + 1 positive each
        + 512 random negatives, fan-out [25, 10], over an RMAT graph of --gat-scale            (engine.GatNablpTrainPlan)
Per leg one process holds three plans over the same seeded batches from the same weights — clipping off, clipping on
(max_norm = half of the first step's norm: it bites), clipping on with the ConstantLR warm-up as well — and times them
ALTERNATELY: --steps steps per timing between two HIP events on the plans' stream (next batch prefetched, as the trainer
issues them), --reps timings each, so that the spread is visible next to the difference.  One JSON line per leg."""
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
from gigl_amd.engine import GatNablpTrainPlan, HipEngine, NablpTrainPlan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--legs", type=str, default="sage,gat")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--gat-scale", type=int, default=22)
ap.add_argument("--gat-edges", type=int, default=48_000_000)
a = ap.parse_args()
HYPER = dict(temperature=0.07, remove_accidental_hits=True, lr=5e-3, weight_decay=1e-6)
POOL = 16


def lp_batches(eng, anchors, negs):
    out = []
    for i in range(anchors.shape[0]):
        pos, cnt = eng.sample_positives(anchors[i], 1, sampling_seed=42)
        a2 = anchors[i].view(-1, 1)
        roots = torch.cat([a2, torch.where(cnt.view(-1, 1) > 0, pos.view(-1, 1), a2)], dim=1).reshape(-1)
        out.append((roots.contiguous(), cnt.to(torch.int32).contiguous(), negs[i].contiguous()))
    return out


def measure(tag, eng, make_plan, batches, shape):
    """three plans, warmed up (eager step, captured step, replays), timed alternately between HIP events"""
    st = torch.cuda.current_stream(eng.device)

    def steps(p, k):
        for i in range(k):
            j, jn = i % POOL, (i + 1) % POOL
            p.step(*batches[j], next_roots=(batches[jn][0], batches[jn][2]) if i + 1 < k else None)

    def timed(p, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(st)
        steps(p, k)
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    probe = make_plan(clip_grad_norm=1e30)  # (never bites: measures the first step's norm)
    first = float(probe.step(*batches[0]).clone()[0])
    assert np.isfinite(first), "the first batch outgrew the plan's workspace"
    norm0, _ = probe.grad_norm()
    probe.close()
    plans = {"clip_off": make_plan(), "clip_on": make_plan(clip_grad_norm=0.5 * norm0),
             "clip_on_warm_up": make_plan(clip_grad_norm=0.5 * norm0, lr_factor=0.25, lr_total_iters=100)}
    for p in plans.values():
        steps(p, 8)
    coef = plans["clip_on"].grad_norm()[1]
    times = {k: [] for k in plans}
    for _ in range(a.reps):
        for k, p in plans.items():
            times[k].append(timed(p, a.steps))
    for p in plans.values():
        p.close()
    stat = lambda v: {"median": float(np.median(v)), "min": min(v), "max": max(v)}
    off, on = float(np.median(times["clip_off"])), float(np.median(times["clip_on"]))
    print(json.dumps(dict(shape, leg=tag, steps_per_timing=a.steps, reps=a.reps, first_step_grad_norm=norm0,
                          clip_coef_after_warm_up=coef, ms_per_step={k: stat(v) for k, v in times.items()},
                          clip_on_minus_off_us=1e3 * (on - off),
                          spread_us=1e3 * max(max(v) - min(v) for v in times.values()))), flush=True)


def sage_leg():
    from gigl_amd.models import GraphSAGE
    eng = HipEngine(0)
    dev = eng.device
    args = argparse.Namespace(workload="products")
    n, d = bench.build_workload(eng, args)
    eng._graph_out = eng._graph  # (bidirectionalised: a node's out-neighbours are its in-neighbours)
    B, n_neg, fan, hid, emb = 2048, 512, [25, 10], args._workload[2], 128
    torch.manual_seed(0)
    model = GraphSAGE(d, hid, emb, num_layers=2, should_l2_normalize_embedding_layer_output=True).to(dev)
    gp = torch.Generator(device="cpu")
    gp.manual_seed(42)
    anchors = torch.randperm(n, generator=gp)[: POOL * B].view(POOL, B).to(torch.int32).to(dev)
    negs = torch.randint(0, n, (POOL, n_neg), generator=gp).to(torch.int32).to(dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    torch.cuda.set_stream(st)
    batches = lp_batches(eng, anchors, negs)
    st.synchronize()
    make = lambda **kw: NablpTrainPlan(eng, copy.deepcopy(model), B, 1, n_neg, fan, **HYPER, **kw)
    measure("sage", eng, make, batches, dict(nodes=n, feature_dim=d, hidden=hid, out=emb, anchors=B, negatives=n_neg, fanouts=fan))
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    eng.bind_stream(None)
    eng.close()


def gat_leg():
    from gigl_amd.models_attn import GAT
    eng = HipEngine(0)
    dev = eng.device
    n, d, fan, B, n_neg = 1 << a.gat_scale, 768, [25, 10], 1024, 512
    src, dst = bench.rmat_edges_gpu(a.gat_scale, a.gat_edges, seed=5, device=dev)
    mul = 0x9E3779B1  # (scatter the ids: hubs are not the low ids)
    src, dst = ((src * mul) % n).to(torch.int32), ((dst * mul) % n).to(torch.int32)
    eng.build_from_coo(n, src, dst, is_directed=True)
    eng.build_from_coo(n, dst, src, is_directed=True, out_graph=True)  # CSR by source: the positives' graph
    has_out = torch.bincount(src.long(), minlength=n) > 0
    del src, dst
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    x = torch.empty((n, d), device=dev, dtype=torch.float16)
    for i in range(0, n, 1 << 18):
        x[i:i + (1 << 18)] = (torch.randn((min(1 << 18, n - i), d), generator=g, device=dev) / 4).to(torch.float16)
    eng.load_features(x)
    del x
    torch.manual_seed(0)
    model = GAT(d, 128, 128, num_layers=2, heads=2, should_l2_normalize_embedding_layer_output=True).to(dev)
    gp = torch.Generator(device="cpu")
    gp.manual_seed(42)
    cand = torch.nonzero(has_out).view(-1)
    anchors = cand[torch.randint(0, cand.numel(), (POOL * B,), generator=gp).to(dev)].to(torch.int32).view(POOL, B)
    negs = torch.randint(0, n, (POOL, n_neg), generator=gp).to(torch.int32).to(dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    torch.cuda.set_stream(st)
    batches = lp_batches(eng, anchors, negs)
    st.synchronize()
    make = lambda **kw: GatNablpTrainPlan(eng, copy.deepcopy(model), B, 1, n_neg, fan, **HYPER, **kw)
    measure("gat", eng, make, batches, dict(nodes=n, edges=int(eng.n_edges), feature_dim=d, heads=2, hidden=128, out=128,
                                            anchors=B, negatives=n_neg, fanouts=fan))
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    eng.bind_stream(None)
    eng.close()


for leg in a.legs.split(","):
    {"sage": sage_leg, "gat": gat_leg}[leg]()
