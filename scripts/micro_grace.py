#!/usr/bin/env python3
"""What the GRACE contrastive loss costs, forward + backward: the fused module (gigl_amd.link_prediction.GRACELoss over
csrc/contrast.hip) against the torch-op formulation of the reference's formula (normalise -> three n x n cosine matrices ->
exp(. / T) -> row sums -> log, and autograd's backward) on the same device, rows randn (not normalised), n in {2048, 8192} x
d in {128, 256}, T = 0.5 (the literal formulation overflows at the reference task's default T = 0.001).
One process, the two routes ALTERNATED: --reps timings each after a warm-up, --iters forward + backward passes per timing on
the host clock around a device synchronise; the spread (max - min) is reported next to the means.  Also the MFMA rate of the
two entry points timed alone (gigl_grace_loss: prep + row log-sum-exps + fold; gigl_grace_loss_backward), from the operations
the kernels ISSUE, counted from the shape: six bf16 MFMA products per fp32 product, whole 64-row tiles and 32-wide K chunks
(forward: per view and row tile, two Gram tiles per column tile; backward: the same Gram tiles again per 128-column chunk,
and two second products over 64-column groups).  A rate over an entry point's time, not a kernel's share of peak.
One JSON line per shape, appended to --out (profiles/grace.txt)."""
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
ap.add_argument("--temperature", type=float, default=0.5)
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "grace.txt"))
a = ap.parse_args()


def torch_grace(h1, h2, t):
    x, y = (h / h.norm(dim=1, keepdim=True).clamp_min(1e-8) for h in (h1, h2))
    e11, e12, e22 = torch.exp(x @ x.t() / t), torch.exp(x @ y.t() / t), torch.exp(y @ y.t() / t)
    l1 = -torch.log(e12.diag() / (e11.sum(1) + e12.sum(1) - e11.diag()))
    l2 = -torch.log(e12.diag() / (e22.sum(1) + e12.sum(0) - e22.diag()))
    return ((l1 + l2) * 0.5).mean()


def mfma_flops(n, d):
    tiles, kc = -(-n // 64), -(-d // 32) * 32
    gram = 2 * 64 * 64 * kc * 6
    chunks = -(-d // 128)
    second = 2 * 64 * 64 * (-(-d // 64) * 64) * 6  # (all chunks' 64-column groups together)
    pairs = 2 * tiles * tiles * 2  # (view, row tile, column tile, own / other view)
    return pairs * gram, pairs * (chunks * gram + second)


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    if not torch.cuda.is_available():
        raise SystemExit("micro_grace.py measures on the GPU; no device is visible")
    from gigl_amd.engine import default_engine
    from gigl_amd.link_prediction import GRACELoss
    dev = torch.device("cuda:0")
    eng = default_engine(dev)
    fused = GRACELoss(temperature=a.temperature)
    stat = lambda v: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(n + d)
        h1 = torch.randn(n, d, generator=g).to(dev).requires_grad_(True)
        h2 = torch.randn(n, d, generator=g).to(dev).requires_grad_(True)

        def step(loss_fn):
            h1.grad = h2.grad = None
            loss_fn(h1, h2).backward()

        routes = {"fused": lambda: step(lambda x, y: fused(x, y)[0]),
                  "torch_ops": lambda: step(lambda x, y: torch_grace(x, y, a.temperature))}
        for fn in routes.values():  # warm-up
            timed(fn, 3)
        diff = abs(float(fused(h1, h2)[0]) - float(torch_grace(h1, h2, a.temperature)))
        times = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, fn in routes.items():
                times[k].append(timed(fn, a.iters))
        # the two entry points alone
        x, y = h1.detach(), h2.detach()
        _, na, nb, norm, lse = eng.grace_loss(x, y, a.temperature)
        one = torch.ones((), device=dev)
        t_f = [timed(lambda: eng.grace_loss(x, y, a.temperature), a.iters) for _ in range(a.reps)]
        t_b = [timed(lambda: eng.grace_loss_backward(na, nb, norm, lse, a.temperature, one), a.iters) for _ in range(a.reps)]
        f_f, f_b = mfma_flops(n, d)
        line = json.dumps(dict(n=n, d=d, temperature=a.temperature, iters_per_timing=a.iters, reps=a.reps,
                               clock="host, device-synchronised", fwd_bwd_ms={k: stat(v) for k, v in times.items()},
                               speedup_of_means=stat(times["torch_ops"])["mean"] / stat(times["fused"])["mean"],
                               loss_abs_diff=diff, forward_entry_ms=stat(t_f), backward_entry_ms=stat(t_b),
                               forward_issued_mfma_tflops=f_f / (min(t_f) * 1e-3) / 1e12,
                               backward_issued_mfma_tflops=f_b / (min(t_b) * 1e-3) / 1e12))
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


main()
