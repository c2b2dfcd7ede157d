#!/usr/bin/env python3
"""What the hadamard_MLP decoder with one hidden layer costs, forward + backward: the fused route (gigl_amd.link_prediction.
hadamard_mlp_scores over csrc/hadamard.hip) against the composed one the deeper decoders keep (_DecoderMLP.pair_scores' fallback:
the candidates projected by the [Q h, D] query-scaled weights on gigl_linear, the rest in torch ops on [C Q, h] rows, autograd's
backward) on the same device and inputs: rows randn, weights randn / sqrt(fan_in), both biases, plain_last False, a random [Q, C]
weight on the scores.  --shapes QxCxDxh where both routes fit in memory, --fused-only where only the fused one is run.
One process, the two routes ALTERNATED: --reps timings each after a warm-up, --iters forward + backward passes per timing on
the host clock around a device synchronise; the spread (max - min) is reported next to the means.
One JSON line per shape, appended to --out (profiles/hadamard_decoder.txt)."""
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
ap.add_argument("--shapes", type=str, default="512x512x128x64,1024x1024x128x64,512x512x256x128,1024x1024x256x128")
ap.add_argument("--fused-only", type=str, default="2048x2560x128x64")
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "hadamard_decoder.txt"))
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
        raise SystemExit("micro_hadamard_decoder.py measures on the GPU; no device is visible")
    from gigl_amd.engine import default_engine
    from gigl_amd.link_prediction import DecoderType, LinkPredictionDecoder
    dev = torch.device("cuda:0")
    stat = lambda v: {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    shapes = [(s, True) for s in a.shapes.split(",") if s] + [(s, False) for s in a.fused_only.split(",") if s]
    for shape, both in shapes:
        nq, nc, d, h = (int(v) for v in shape.split("x"))
        torch.manual_seed(nq + nc + d + h)
        dec = LinkPredictionDecoder(DecoderType.hadamard_MLP, [d, h, 1], bias=True).to(dev)
        dec.engine = default_engine(dev)
        mlp = dec.mlp_decoder
        composed_mlp = type(mlp)([d, h, 1], bias=True, act_first=True).to(dev)  # (act_first: kept on the composed route)
        composed_mlp.load_state_dict(mlp.state_dict())
        q, c = (torch.randn(n, d).to(dev).requires_grad_(True) for n in (nq, nc))
        wgt = torch.randn(nq, nc).to(dev)

        def step(m):
            q.grad = c.grad = None
            m.zero_grad(set_to_none=True)
            (m.pair_scores(q, c, dec.engine) * wgt).sum().backward()

        routes = {"fused": lambda: step(mlp)}
        if both:
            routes["composed"] = lambda: step(composed_mlp)
        for fn in routes.values():  # warm-up
            timed(fn, 3)
        rec = dict(q=nq, c=nc, channels=[d, h, 1], iters_per_timing=a.iters, reps=a.reps, clock="host, device-synchronised")
        if both:
            with torch.no_grad():
                s1, s2 = mlp.pair_scores(q, c, dec.engine), composed_mlp.pair_scores(q, c, dec.engine)
            rec["scores_max_abs_diff"] = float((s1 - s2).abs().max())
        times = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, fn in routes.items():
                times[k].append(timed(fn, a.iters))
        rec["fwd_bwd_ms"] = {k: stat(v) for k, v in times.items()}
        if both:
            rec["speedup_of_means"] = stat(times["composed"])["mean"] / stat(times["fused"])["mean"]
        rec["torch_peak_memory_mb"] = torch.cuda.max_memory_allocated() / 2 ** 20
        torch.cuda.reset_peak_memory_stats()
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


main()
