#!/usr/bin/env python3
"""What hard-negative slots cost in the link-prediction training plan (engine.NablpTrainPlan(num_hard_negatives=H): the main
batch grows from 2 to 2 + H trees per anchor, the head from Q + n_rn to Q + b H + n_rn candidate columns), at the shape the
benchmark trains: bench/train.py's link-prediction leg — the products-shaped graph, GraphSAGE 100 -> 256 -> 128
L2-normalised, 2048 anchors + 1 positive each + 512 random negatives, fan-out [25, 10] — with H = 0 / 2 / 8 hard negatives
per anchor drawn from a label list in which every node has 8 entries (every slot filled: the worst case).
One process holds the three plans over the same seeded anchors from the same weights and times them ALTERNATELY: --steps
steps per timing between two HIP events on the plans' stream (next batch prefetched, as the trainer issues them), --reps
timings each after a warm-up, so that the spread is visible next to the differences.  H = 0 is the plan of
`bench.py --train --train-task lp`: the same launches.  One JSON line, appended to --out (profiles/lp_hard_negatives.txt)."""
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
from gigl_amd.engine import HipEngine, NablpTrainPlan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--hs", type=str, default="0,2,8")
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "lp_hard_negatives.txt"))
a = ap.parse_args()
HYPER = dict(temperature=0.07, remove_accidental_hits=True, lr=5e-3, weight_decay=1e-6)
POOL, LIST_DEGREE = 16, 8


def main():
    from gigl_amd.models import GraphSAGE
    hs = [int(h) for h in a.hs.split(",")]
    eng = HipEngine(0)
    dev = eng.device
    args = argparse.Namespace(workload="products")
    n, d = bench.build_workload(eng, args)
    eng._graph_out = eng._graph  # (bidirectionalised: a node's out-neighbours are its in-neighbours)
    rng = np.random.default_rng(7)
    eng.load_label_edges("neg", n, np.repeat(np.arange(n, dtype=np.int64), LIST_DEGREE), rng.integers(0, n, n * LIST_DEGREE))
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
    batches, plans = {}, {}
    for h in hs:
        batches[h] = []
        for i in range(POOL):
            roots, cnt = eng.nablp_main_roots(anchors[i], 1, h, sampling_seed=42, neg_label_edges="neg" if h else None)
            batches[h].append((roots, cnt if h else cnt[:B].contiguous(), negs[i].contiguous()))
        plans[h] = NablpTrainPlan(eng, copy.deepcopy(model), B, 1, n_neg, fan, num_hard_negatives=h, **HYPER)
    st.synchronize()

    def steps(h, k):
        p, bt = plans[h], batches[h]
        for i in range(k):
            j, jn = i % POOL, (i + 1) % POOL
            p.step(*bt[j], next_roots=(bt[jn][0], bt[jn][2]) if i + 1 < k else None)

    def timed(h, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(st)
        steps(h, k)
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    for h in hs:  # warm-up: eager step, captured step, replays
        first = float(plans[h].step(*batches[h][0]).clone()[0])
        assert np.isfinite(first), f"H={h}: the first batch outgrew the plan's workspace"
        steps(h, 8)
    times = {h: [] for h in hs}
    for _ in range(a.reps):
        for h in hs:
            times[h].append(timed(h, a.steps))
    filled = {h: float(batches[h][0][1][B:].float().mean()) if h else 0.0 for h in hs}
    for p in plans.values():
        p.close()
    stat = lambda v: {"median": float(np.median(v)), "min": min(v), "max": max(v)}
    line = json.dumps(dict(nodes=n, feature_dim=d, hidden=hid, out=emb, anchors=B, negatives=n_neg, fanouts=fan,
                           steps_per_timing=a.steps, reps=a.reps, hard_negatives_per_anchor_drawn=filled,
                           ms_per_step={f"H={h}": stat(v) for h, v in times.items()},
                           spread_us=1e3 * max(max(v) - min(v) for v in times.values())))
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
