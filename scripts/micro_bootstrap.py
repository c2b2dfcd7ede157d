#!/usr/bin/env python3
"""What the bootstrap tasks' head and loss cost, forward + backward: the fused route (gigl_amd.link_prediction.
_FusedBootstrapHead over csrc/bootstrap.hip) against the same computation composed from what the other two-view tasks use —
_TwoViewTask._apply_head (two gigl_linear calls and a relu per view, autograd's backward through them) and torch ops for the
cosine terms — on the same device and inputs: rows and targets randn, the head's weights randn / sqrt(fan_in), n in {2048, 8192}
x out = hid in {128, 256}, BGRL and TBGRL (neg_lambda 0.12).
One process, the two routes ALTERNATED: --reps timings each after a warm-up, --iters forward + backward passes per timing on
the host clock around a device synchronise; the spread (max - min) is reported next to the means.
One JSON line per mode and shape, appended to --out (profiles/bootstrap.txt)."""
import argparse
import json
import math
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
ap.add_argument("--shapes", type=str, default="2048x128,2048x256,8192x128,8192x256")
ap.add_argument("--neg-lambda", type=float, default=0.12)
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "bootstrap.txt"))
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
        raise SystemExit("micro_bootstrap.py measures on the GPU; no device is visible")
    from gigl_amd.link_prediction import bootstrap_head_loss
    from gigl_amd.nablp_spec import _TwoViewTask
    dev = torch.device("cuda:0")
    lam = a.neg_lambda
    cos = F.cosine_similarity
    stat = lambda v: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        torch.manual_seed(n + d)
        task = _TwoViewTask(None, 0.0, 0.0, 0.0, 0.0, 0)  # (no encoder: only its head is used)
        task.head = torch.nn.Sequential(torch.nn.Linear(d, d), torch.nn.ReLU(), torch.nn.Linear(d, d)).to(dev)
        with torch.no_grad():
            for lin in (task.head[0], task.head[2]):
                lin.weight.copy_(torch.randn(d, d) / math.sqrt(d))
        e1, e2 = (torch.randn(n, d).to(dev).requires_grad_(True) for _ in range(2))
        y1, y2, yneg = (torch.randn(n, d).to(dev) for _ in range(3))

        def composed(neg):
            q1, q2 = task._apply_head(e1), task._apply_head(e2)
            if neg is None:
                return 2 - cos(q1, y2, dim=-1).mean() - cos(q2, y1, dim=-1).mean()
            return lam * (cos(q1, neg).mean() + cos(q2, neg).mean()) - (1 - lam) * (cos(q1, y2).mean() + cos(q2, y1).mean())

        def step(loss_fn, neg):
            e1.grad = e2.grad = None
            task.head.zero_grad(set_to_none=True)
            loss_fn(neg).backward()

        fused = lambda neg: bootstrap_head_loss(e1, e2, y1, y2, neg, task.head, lam)
        for mode, neg in (("bgrl", None), ("tbgrl", yneg)):
            routes = {"fused": lambda: step(fused, neg), "composed": lambda: step(composed, neg)}
            for fn in routes.values():  # warm-up
                timed(fn, 3)
            diff = abs(float(fused(neg)) - float(composed(neg)))
            times = {k: [] for k in routes}
            for _ in range(a.reps):
                for k, fn in routes.items():
                    times[k].append(timed(fn, a.iters))
            line = json.dumps(dict(loss=mode, n=n, out=d, hid=d, neg_lambda=lam, iters_per_timing=a.iters, reps=a.reps,
                                   clock="host, device-synchronised", fwd_bwd_ms={k: stat(v) for k, v in times.items()},
                                   speedup_of_means=stat(times["composed"])["mean"] / stat(times["fused"])["mean"],
                                   loss_abs_diff=diff))
            print(line, flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


main()
