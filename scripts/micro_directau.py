#!/usr/bin/env python3
"""What the DirectAU uniformity loss costs, forward + backward: the fused modules (gigl_amd.link_prediction.UniformityLoss over
csrc/pairwise.hip) against the torch-op formulation of the same formula (pdist -> pow -> mul -> exp -> mean -> log and
autograd's backward) on the same device, rows L2-normalised, n in {2048, 8192} x d in {128, 256}.
One process, the two routes ALTERNATED: --reps timings each after a warm-up, --iters forward + backward passes per timing on
the host clock around a device synchronise; the spread (max - min) is reported next to the means.  Also the MFMA rate of the
two entry points timed alone (gigl_uniformity_loss: prep + pair sums + fold; gigl_uniformity_loss_backward), from the
operations the kernels ISSUE, counted from the shape: six bf16 MFMA products per fp32 product, whole 64-row tiles and 32-wide K
chunks (forward: the upper triangle of tile pairs; backward: every tile pair, the Gram tile again per 128-column chunk, and
the second product over 64-column groups).  A rate over an entry point's time, not a kernel's share of peak.
One JSON line per shape, appended to --out (profiles/directau.txt)."""
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
ap.add_argument("--temperature", type=float, default=2.0)
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "directau.txt"))
a = ap.parse_args()


def torch_uniformity(u, p, t):
    f = lambda x: torch.pdist(x, p=2).pow(2).mul(-t).exp().mean().log()
    return (f(u) + f(p)) / 2


def mfma_flops(n, d):
    tiles, kc = -(-n // 64), -(-d // 32) * 32
    gram = 2 * 64 * 64 * kc * 6
    fwd = tiles * (tiles + 1) // 2 * gram
    chunks = -(-d // 128)
    second = 2 * 64 * 64 * (-(-d // 64) * 64) * 6  # (all chunks' 64-column groups together)
    return fwd, tiles * tiles * (chunks * gram + second)


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    if not torch.cuda.is_available():
        raise SystemExit("micro_directau.py measures on the GPU; no device is visible")
    from gigl_amd.engine import default_engine
    from gigl_amd.link_prediction import UniformityLoss
    dev = torch.device("cuda:0")
    eng = default_engine(dev)
    fused = UniformityLoss(temperature=a.temperature)
    stat = lambda v: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(n + d)
        u = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1).to(dev).requires_grad_(True)
        p = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1).to(dev).requires_grad_(True)

        def step(loss_fn):
            u.grad = p.grad = None
            loss_fn(u, p).backward()

        routes = {"fused": lambda: step(fused), "torch_ops": lambda: step(lambda x, y: torch_uniformity(x, y, a.temperature))}
        for fn in routes.values():  # warm-up
            timed(fn, 3)
        diff = abs(float(fused(u, p)) - float(torch_uniformity(u, p, a.temperature)))
        times = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, fn in routes.items():
                times[k].append(timed(fn, a.iters))
        # the two entry points alone
        x = u.detach()
        _, xc, sq, s = eng.uniformity_loss(x, a.temperature)
        one = torch.ones((), device=dev)
        t_f = [timed(lambda: eng.uniformity_loss(x, a.temperature), a.iters) for _ in range(a.reps)]
        t_b = [timed(lambda: eng.uniformity_loss_backward(xc, sq, a.temperature, s, one), a.iters) for _ in range(a.reps)]
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
