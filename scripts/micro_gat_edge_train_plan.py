#!/usr/bin/env python3
"""Link-prediction TRAINING steps of an edge-featured GAT at the `gat-lp --train` shape of bench/gat_lp.py (768-wide fp16
rows, 2 heads x 128 -> 128, 1024 anchors + 1 positive each + 512 random negatives, fan-out [25, 10]) plus an fp32 edge
table of edge_dim 16, over one set of seeded batches in one process:
  A  the one-call plan with edge features (engine.GatEdgeNablpTrainPlan, next batch prefetched)
  B  the autograd step (hbm.ResidentGraph.train_graph with train_as_graph_data -> GAT._forward_graph -> torch.optim.Adam)
  C  the edge-free plan (engine.GatNablpTrainPlan) on the same batches (A / C = the cost of the edge terms)
The three alternate, each warmed up, `--steps` steps per timing ending in a device synchronise, `--reps` repetitions so that
the spread is visible; the first step's losses of A and B are compared first.  --conv gat (GATConv(edge_dim), the default)
or edge_attr_gat (the autograd loop's EdgeAttrGATConv backward needs layer widths that are multiples of 256: at this
shape B is then reported as unavailable).  --only-plan: plan steps alone (a kernel trace's run)."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gigl_amd.engine import GatEdgeNablpTrainPlan, GatNablpTrainPlan, HipEngine  # noqa: E402
from gigl_amd.hbm import ResidentGraph  # noqa: E402
from gigl_amd.models_attn import GAT  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=int, default=22)
ap.add_argument("--edges", type=int, default=48_000_000)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--negatives", type=int, default=512)
ap.add_argument("--fanouts", type=str, default="25,10")
ap.add_argument("--edge-dim", type=int, default=16)
ap.add_argument("--conv", type=str, default="gat", choices=["gat", "edge_attr_gat"])
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--autograd-steps", type=int, default=40, help="steps per timing of the (much slower) autograd loop")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--only-plan", action="store_true")
a = ap.parse_args()

eng = HipEngine(0)
dev = eng.device
n, d, fan, B, n_neg = 1 << a.scale, 768, [int(v) for v in a.fanouts.split(",")], a.batch, a.negatives
src, dst = bench.rmat_edges_gpu(a.scale, a.edges, seed=5, device=dev)
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
eng._set_edge_table(torch.randn((eng.n_edges, a.edge_dim), generator=g, device=dev) / 2)
torch.manual_seed(0)
kw = dict(num_layers=2, heads=2, should_l2_normalize_embedding_layer_output=True)
model = GAT(d, 128, 128, edge_dim=a.edge_dim, conv=a.conv, **kw).to(dev)
plain = GAT(d, 128, 128, **kw).to(dev)

pool = 16
gp = torch.Generator(device="cpu")
gp.manual_seed(42)
cand = torch.nonzero(has_out).view(-1)
anchors = cand[torch.randint(0, cand.numel(), (pool * B,), generator=gp).to(dev)].to(torch.int32).view(pool, B)
negs = torch.randint(0, n, (pool, n_neg), generator=gp).to(torch.int32).to(dev)
st = torch.cuda.Stream(device=dev)
torch.cuda.synchronize()
eng.bind_stream(st)
torch.cuda.set_stream(st)
batches = []
for i in range(pool):
    pos, cnt = eng.sample_positives(anchors[i], 1, sampling_seed=42)
    a2 = anchors[i].view(-1, 1)
    roots = torch.cat([a2, torch.where(cnt.view(-1, 1) > 0, pos.view(-1, 1), a2)], dim=1).reshape(-1)
    batches.append((roots.contiguous(), cnt.to(torch.int32).contiguous(), negs[i].contiguous()))
st.synchronize()

hyper = dict(temperature=0.07, remove_accidental_hits=True, lr=5e-3, weight_decay=1e-6)
plan = GatEdgeNablpTrainPlan(eng, copy.deepcopy(model), B, 1, n_neg, fan, **hyper)
plan_c = None if a.only_plan else GatNablpTrainPlan(eng, plain, B, 1, n_neg, fan, **hyper)


def plan_steps(p, k):
    last = None
    for i in range(k):
        j, jn = i % pool, (i + 1) % pool
        last = p.step(*batches[j], next_roots=(batches[jn][0], batches[jn][2]) if i + 1 < k else None)
    return last


def timed(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


first_plan = float(plan.step(*batches[0]).clone()[0])
assert np.isfinite(first_plan), "the first batch outgrew the plan's workspace"
if a.only_plan:
    plan_steps(plan, 8)
    t = timed(lambda k: plan_steps(plan, k), a.steps)
    print(json.dumps({"conv": a.conv, "edge_dim": a.edge_dim, "plan_ms_per_step": t, "steps": a.steps}), flush=True)
    plan.close()
    eng.close()
    sys.exit(0)

autograd, first_auto, why = None, None, None
try:
    ref = copy.deepcopy(model)
    ref.train()
    ref.engine = eng
    res = ResidentGraph.from_engine(eng, np.arange(n, dtype=np.int64), fan)
    res.train_as_graph_data, res.defer_x = True, True
    opt = torch.optim.Adam(ref.parameters(), lr=5e-3, weight_decay=1e-6)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_train_plan import _lp_loss_torch  # noqa: E402  (the retrieval loss on embeddings, in torch)

    def autograd(k):
        loss = None
        for i in range(k):
            roots, cnt, rn = batches[i % pool]
            embs = []
            for r in (roots, rn):
                gd, ri = res.train_graph(r)
                embs.append(ref(gd)[ri])
            loss = _lp_loss_torch(embs[0], embs[1], roots, cnt, rn, B, 1, 0.07)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        return loss
    ref0 = copy.deepcopy(ref.state_dict())
    first_auto = float(autograd(1))
    ref.load_state_dict(ref0)
except Exception as exc:  # noqa: BLE001 — a comparison figure only
    autograd, why = None, f"{type(exc).__name__}: {str(exc)[:200]}"

plan_steps(plan, 8)
plan_steps(plan_c, 8)
if autograd:
    autograd(3)
ta, tb, tc = [], [], []
for _ in range(a.reps):
    ta.append(timed(lambda k: plan_steps(plan, k), a.steps))
    if autograd:
        tb.append(timed(autograd, a.autograd_steps))
    tc.append(timed(lambda k: plan_steps(plan_c, k), a.steps))
stat = lambda v: None if not v else {"median": float(np.median(v)), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
print(json.dumps({
    "conv": a.conv, "edge_dim": a.edge_dim, "nodes": n, "edges": int(eng.n_edges), "anchors": B, "negatives": n_neg, "fanouts": fan,
    "steps_per_timing": a.steps, "autograd_steps_per_timing": a.autograd_steps if autograd else 0,
    "first_step_loss": {"plan": first_plan, "autograd": first_auto}, "autograd_unavailable": why,
    "plan_ms_per_step": stat(ta), "autograd_ms_per_step": stat(tb), "edge_free_plan_ms_per_step": stat(tc),
    "plan_not_slower_than_autograd_beyond_the_spread":
        None if not tb else float(np.median(ta)) <= float(np.median(tb)) + (max(tb) - min(tb)) + (max(ta) - min(ta)),
    "edge_terms_ratio": float(np.median(ta)) / float(np.median(tc))}), flush=True)
plan.close()
plan_c.close()
torch.cuda.synchronize()
torch.cuda.set_stream(torch.cuda.default_stream(dev))
eng.bind_stream(None)
eng.close()
