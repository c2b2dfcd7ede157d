#!/usr/bin/env python3
"""What the FeatureReconstruction task's decoder and loss cost, forward + backward: the fused route (gigl_amd.link_prediction.
feature_reconstruction_loss over csrc/reconstruct.hip: B root rows of work) against the same computation composed, as the
reference writes it, from what the project already has — gigl_linear over all N rows, the roots' rows zeroed, GraphConv as the
sum-aggregation gather over all rows plus gigl_linear (nn.sage_conv, aggr "sum"), the roots selected, torch ops for the loss,
autograd through all of it — on the same device and inputs: B in {512, 2048} roots, N = 16 B nodes, average in-degree 10 plus a
self loop each, (out, in) in {(128, 128), (256, 512)}, alpha 3.
One process, the two routes ALTERNATED: --reps timings each after a warm-up, --iters forward + backward passes per timing on
the host clock around a device synchronise; the spread (max - min) is reported next to the means.
One JSON line per shape, appended to --out (profiles/feature_reconstruction.txt)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--shapes", type=str, default="512x128x128,512x256x512,2048x128x128,2048x256x512")
ap.add_argument("--alpha", type=float, default=3.0)
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "feature_reconstruction.txt"))
a = ap.parse_args()


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    if not torch.cuda.is_available():
        raise SystemExit("micro_feature_reconstruction.py measures on the GPU; no device is visible")
    from gigl_amd.engine import default_engine
    from gigl_amd.link_prediction import feature_reconstruction_loss
    from gigl_amd.models_hetero import _linear
    from gigl_amd.nn import GraphData, sage_conv
    dev = torch.device("cuda:0")
    eng = default_engine(dev)
    stat = lambda v: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    for shape in a.shapes.split(","):
        b, out, d_in = (int(v) for v in shape.split("x"))
        n = 16 * b
        torch.manual_seed(b + out + d_in)
        ei = torch.cat((torch.randint(0, n, (2, 10 * n)), torch.arange(n).expand(2, n)), dim=1)
        graph = GraphData(x=torch.randn(n, d_in), edge_index=ei).to(dev)
        roots = torch.randperm(n)[:b].to(dev)
        enc = torch.randn(n, out).to(dev).requires_grad_(True)
        w_ed, w_rel, w_root = (torch.nn.Parameter((torch.randn(r, out) / out ** 0.5).to(dev)) for r in (out, d_in, d_in))
        b_rel = torch.nn.Parameter(0.1 * torch.randn(d_in).to(dev))
        params = [enc, w_ed, w_rel, w_root, b_rel]

        def composed():
            h = _linear(eng, enc, w_ed, None).index_fill(0, roots, 0.0)
            pred = sage_conv(h, w_rel, b_rel, w_root, eng, graph, False, "sum")[roots]
            return (1 - (F.normalize(graph.x[roots], dim=-1) * F.normalize(pred, dim=-1)).sum(-1)).pow(a.alpha).mean()

        fused = lambda: feature_reconstruction_loss(enc, graph.x, graph, roots, w_ed, w_rel, b_rel, a.alpha)

        def step(loss_fn):
            for p in params:
                p.grad = None
            loss_fn().backward()

        routes = {"fused": lambda: step(fused), "composed": lambda: step(composed)}
        for fn in routes.values():  # warm-up
            timed(fn, 3)
        diff = abs(float(fused().detach()) - float(composed().detach()))
        times = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, fn in routes.items():
                times[k].append(timed(fn, a.iters))
        line = json.dumps(dict(b=b, n=n, edges=int(ei.shape[1]), out=out, **{"in": d_in}, alpha=a.alpha, iters_per_timing=a.iters,
                               reps=a.reps, clock="host, device-synchronised", fwd_bwd_ms={k: stat(v) for k, v in times.items()},
                               speedup_of_means=stat(times["composed"])["mean"] / stat(times["fused"])["mean"],
                               loss_abs_diff=diff))
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


main()
