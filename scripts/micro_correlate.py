#!/usr/bin/env python3
"""What the two correlation losses cost, forward + backward: the fused modules (gigl_amd.link_prediction.GBTLoss and
WhiteningDecorrelationLoss over csrc/correlate.hip) against the torch-op formulation of the reference's literal formulas
(standardise -> d x d products -> norms / masked squares, and autograd's backward) on the same device, rows randn * 3 with the
second view the first plus randn noise, n in {2048, 8192} x d in {128, 256}.
One process, the two routes ALTERNATED: --reps timings each after a warm-up, --iters forward + backward passes per timing on
the host clock around a device synchronise; the spread (max - min) is reported next to the means.
One JSON line per loss and shape, appended to --out (profiles/correlate.txt)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--shapes", type=str, default="2048x128,2048x256,8192x128,8192x256")
ap.add_argument("--lambd", type=float, default=1e-3)
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "correlate.txt"))
a = ap.parse_args()


def torch_gbt(z_a, z_b):
    n, d = z_a.shape
    za, zb = ((z - z.mean(dim=0)) / (z.std(dim=0) + 1e-15) for z in (z_a, z_b))
    c = za.T @ zb / n
    off = ~torch.eye(d, device=c.device).bool()
    return (1 - c.diagonal()).pow(2).sum() + c[off].pow(2).sum() / d


def torch_whitening(h1, h2, lambd):
    n, d = h1.shape
    z1, z2 = ((h - h.mean(0)) / h.std(0) for h in (h1, h2))
    iden = torch.eye(d, device=h1.device)
    norm = torch.linalg.matrix_norm
    return norm((z1 - z2) / n) + lambd * (norm(iden - z1.T @ z1 / n) + norm(iden - z2.T @ z2 / n))


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    if not torch.cuda.is_available():
        raise SystemExit("micro_correlate.py measures on the GPU; no device is visible")
    from gigl_amd.link_prediction import GBTLoss, WhiteningDecorrelationLoss
    dev = torch.device("cuda:0")
    gbt, wd = GBTLoss(), WhiteningDecorrelationLoss(lambd=a.lambd)
    losses = {"gbt": (lambda x, y: gbt(x, y)[0], torch_gbt),
              "whitening": (lambda x, y: wd(x, y, x.shape[0])[0], lambda x, y: torch_whitening(x, y, a.lambd))}
    stat = lambda v: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(n + d)
        h1 = 3 * torch.randn(n, d, generator=g)
        h2 = (h1 + torch.randn(n, d, generator=g)).to(dev).requires_grad_(True)
        h1 = h1.to(dev).requires_grad_(True)

        def step(loss_fn):
            h1.grad = h2.grad = None
            loss_fn(h1, h2).backward()

        for name, (fused, ops) in losses.items():
            routes = {"fused": lambda: step(fused), "torch_ops": lambda: step(ops)}
            for fn in routes.values():  # warm-up
                timed(fn, 3)
            diff = abs(float(fused(h1, h2)) - float(ops(h1, h2)))
            times = {k: [] for k in routes}
            for _ in range(a.reps):
                for k, fn in routes.items():
                    times[k].append(timed(fn, a.iters))
            line = json.dumps(dict(loss=name, n=n, d=d, lambd=a.lambd, iters_per_timing=a.iters, reps=a.reps,
                                   clock="host, device-synchronised", fwd_bwd_ms={k: stat(v) for k, v in times.items()},
                                   speedup_of_means=stat(times["torch_ops"])["mean"] / stat(times["fused"])["mean"],
                                   loss_abs_diff=diff))
            print(line, flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


main()
