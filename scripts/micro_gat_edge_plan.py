#!/usr/bin/env python3
"""EdgeAttrGAT inference batches at BASELINE configs[4]'s encoder shape with edge features (RMAT graph of 2^22 nodes,
768 fp16 features, 2 heads x 128 -> 128, edge_dim 16, fan-out [15, 10], 1024 roots per batch), groups 1 and 16:
  A  the staged route: sample_khop + union_build + model(HipBatch) per batch (host-driven launches, a dense
     [cap_edges][16] edge array gathered per batch)
  B  the one-call plan with edge features, replayed as a hipGraph (GAT.make_plan + use_graph)
  C  the edge-free one-call GAT plan on the same batches (B / C = the cost of the edge terms)
A and B alternate in one process, five repetitions each over the same seeded batches, device-event times after a
warm-up; rows of A and B are compared at 1e-5 first."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gigl_amd.engine import HipEngine  # noqa: E402
from gigl_amd.models import HipBatch  # noqa: E402
from gigl_amd.models_attn import GAT  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=int, default=22)
ap.add_argument("--edges", type=int, default=48_000_000)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--edge-dim", type=int, default=16)
ap.add_argument("--batches", type=int, default=6, help="distinct seeded batch sets per repetition")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--groups", type=str, default="1,16")
a = ap.parse_args()

eng = HipEngine(0)
dev = eng.device
n, d, fan, b = 1 << a.scale, 768, [15, 10], a.batch
src, dst = bench.rmat_edges_gpu(a.scale, a.edges, seed=5, device=dev)
mul = 0x9E3779B1  # (scatter the ids: hubs are not the low ids)
eng.build_from_coo(n, ((src * mul) % n).to(torch.int32), ((dst * mul) % n).to(torch.int32), is_directed=True)
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
model = GAT(d, 128, 128, num_layers=2, heads=2, edge_dim=a.edge_dim, conv="edge_attr_gat").to(dev)
plain = GAT(d, 128, 128, num_layers=2, heads=2).to(dev)
st = torch.cuda.Stream(device=dev)
eng.bind_stream(st)
torch.cuda.set_stream(st)


def staged(roots, groups):
    outs = []
    for k in range(groups):
        part = roots[k * b:(k + 1) * b].contiguous()
        tree = eng.sample_khop(part, fan)
        u = eng.union_build(tree)
        outs.append(model(HipBatch(eng, tree, u))[u.root_local[:b].long()])
    return torch.cat(outs)


def timed(fn, sets):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for r in sets:
        fn(r)
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / len(sets)


for groups in [int(v) for v in a.groups.split(",")]:
    rg = torch.Generator().manual_seed(42 + groups)
    sets = [torch.randint(0, n, (b * groups,), generator=rg).to(torch.int32).to(dev) for _ in range(a.batches)]
    plan = model.make_plan(eng, b, fan, groups=groups)
    plan_c = plain.make_plan(eng, b, fan, groups=groups)
    over = torch.zeros(1, dtype=torch.int32, device=dev)
    want = staged(sets[0], groups)
    got = plan.run(sets[0])
    plan.overflow_add(over)
    err = float((got - want).abs().max())
    assert int(over.item()) == 0, "a batch outgrew the plan's workspace"
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-5), f"plan != staged: {err:.3e}"
    for p in (plan, plan_c):
        p.use_graph(True)
        for r in sets[:2]:  # captures, then replays
            p.run(r)
    for r in sets:  # warm-up of every timed shape
        staged(r, groups)
        plan.run(r)
        plan_c.run(r)
    torch.cuda.synchronize()
    ta, tb, tc = [], [], []
    for _ in range(a.reps):
        ta.append(timed(lambda r: staged(r, groups), sets))
        tb.append(timed(plan.run, sets))
        tc.append(timed(plan_c.run, sets))
    plan.overflow_add(over)
    assert int(over.item()) == 0
    med = lambda v: float(np.median(v))
    print(json.dumps({
        "groups": groups, "roots_per_call": b * groups, "max_abs_diff_plan_vs_staged": err,
        "staged_ms": {"median": med(ta), "min": min(ta), "max": max(ta), "spread": max(ta) - min(ta)},
        "plan_ms": {"median": med(tb), "min": min(tb), "max": max(tb), "spread": max(tb) - min(tb)},
        "edge_free_plan_ms": {"median": med(tc), "min": min(tc), "max": max(tc)},
        "plan_wins_by_more_than_the_staged_spread": med(ta) - med(tb) > max(ta) - min(ta),
        "edge_terms_ratio": med(tb) / med(tc)}), flush=True)
    plan.close()
    plan_c.close()
torch.cuda.synchronize()
torch.cuda.set_stream(torch.cuda.default_stream(dev))
eng.bind_stream(None)
eng.close()
