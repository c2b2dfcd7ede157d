#!/usr/bin/env python3
"""What the job's task costs in the link-prediction training plan (engine.NablpTrainPlan(task=...): the head's three loss
launches are the retrieval loss' or gigl_lp_task_loss's Margin / Softmax ones — the same number of launches, Q (1 + H + n_rn)
floats read forward against Q C), at the shape the benchmark trains: bench/train.py's link-prediction leg — the
products-shaped graph, GraphSAGE 100 -> 256 -> 128 L2-normalised, 2048 anchors + 1 positive each + 512 random negatives,
fan-out [25, 10].
One process holds the three tasks' plans over the same seeded anchors from the same weights and times them ALTERNATELY:
--steps steps per timing between two HIP events on the plans' stream (next batch prefetched, as the trainer issues them),
--reps timings each after a warm-up, so that the spread is visible next to the differences.  Retrieval is the plan of
`bench.py --train --train-task lp`: the same launches.  Then the same Margin job on the AUTOGRAD loop — what `train_plan: off`
runs on the in-HBM route: HipBatch forward with autograd, the per-root score lists (nablp_spec._per_root_scores), the Margin
module over its padded matrices, torch.optim.Adam — --autograd-steps steps per timing on the host clock with a synchronise.
The ORDER in which a process creates the plans shows in the figures: the runtime maps a process's streams onto a few hardware
queues in creation order, each plan brings three streams of its own beside the caller's, and from the second plan on one of
them lands on the caller's queue — that plan's step loses some overlap (measured: the same plan is 0.08 ms slower created
second and 0.3 ms slower created third, whichever task it has).  So the script runs the alternation once per cyclic creation
order, each in a fresh child process (--no-rotate: this process, the order of --tasks), and reports per task the figure of
every position; position 0 — created first, as a job's only plan is — is the one to compare.
One JSON line, appended to --out (profiles/lp_tasks.txt)."""
import argparse
import copy
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--autograd-steps", type=int, default=4, help="0: skip the autograd loop")
ap.add_argument("--tasks", type=str, default="Retrieval,Margin,Softmax", help="a subset, e.g. for a kernel trace of one plan")
ap.add_argument("--no-rotate", action="store_true", help="measure in this process, plans created in the order of --tasks")
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "lp_tasks.txt"))
a = ap.parse_args()
HYPER = dict(temperature=0.07, remove_accidental_hits=True, lr=5e-3, weight_decay=1e-6, margin=0.5, softmax_temperature=0.07)
TASKS = tuple(a.tasks.split(","))
POOL = 16


def rotate():
    """one child per cyclic creation order (this process never opens the GPU) -> one line: per task, ms/step by position"""
    by_task = {t: {} for t in TASKS}
    spread, autograd, shape = 0.0, None, {}
    for k in range(len(TASKS)):
        order = TASKS[k:] + TASKS[:k]
        cmd = [sys.executable, os.path.abspath(__file__), "--no-rotate", "--tasks", ",".join(order), "--steps", str(a.steps), "--reps",
               str(a.reps), "--autograd-steps", str(a.autograd_steps if k == 0 else 0), "--out", os.devnull]
        d = json.loads(subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines()[-1])
        for pos, t in enumerate(order):
            by_task[t][f"created_{pos}"] = d["ms_per_step"][t]
        spread = max(spread, d["spread_us"])
        autograd = autograd or d["margin_autograd_loop_ms_per_step"]
        shape = {key: d[key] for key in ("nodes", "feature_dim", "hidden", "out", "anchors", "negatives", "fanouts", "steps_per_timing",
                                         "reps", "first_loss")}
    line = json.dumps(dict(shape, ms_per_step_by_creation_position=by_task, spread_us=spread,
                           margin_autograd_loop_ms_per_step=autograd))
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


def main():
    import bench
    from gigl_amd.engine import HipEngine, NablpTrainPlan
    from gigl_amd.models import GraphSAGE, HipBatch
    from gigl_amd.nablp_spec import Margin, NodeAnchorBasedLinkPredictionTaskInputs, _per_root_scores
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
    batches = []
    for i in range(POOL):
        roots, cnt = eng.nablp_main_roots(anchors[i], 1, 0, sampling_seed=42)
        batches.append((roots, cnt[:B].contiguous(), negs[i].contiguous()))
    plans = {t: NablpTrainPlan(eng, copy.deepcopy(model), B, 1, n_neg, fan, task=t, **HYPER) for t in TASKS}
    st.synchronize()

    def steps(t, k):
        p = plans[t]
        for i in range(k):
            j, jn = i % POOL, (i + 1) % POOL
            p.step(*batches[j], next_roots=(batches[jn][0], batches[jn][2]) if i + 1 < k else None)

    def timed(t, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(st)
        steps(t, k)
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    first = {}
    for t in TASKS:  # warm-up: eager step, captured step, replays
        first[t] = float(plans[t].step(*batches[0]).clone()[0])
        assert np.isfinite(first[t]), f"{t}: the first batch outgrew the plan's workspace"
        steps(t, 8)
    times = {t: [] for t in TASKS}
    for _ in range(a.reps):
        for t in TASKS:
            times[t].append(timed(t, a.steps))
    for p in plans.values():
        p.close()

    # ---- the Margin job on the autograd loop
    ref = copy.deepcopy(model).train()
    opt = torch.optim.Adam(ref.parameters(), lr=5e-3, weight_decay=1e-6)
    task = Margin(margin=HYPER["margin"])
    empty = torch.zeros((0,), dtype=torch.float32, device=dev)

    def autograd_step(i):
        roots, cnt, rn = batches[i % POOL]
        embs = []
        for r in (roots, rn):
            tree = eng.sample_khop(r, fan)
            u = eng.union_build(tree)
            embs.append(ref(HipBatch(eng, tree, u, train=True))[u.root_local[: r.numel()].long()])
        e = embs[0].view(B, 2, emb)
        query, n_pos = e[:, 0], cnt.tolist()
        pos_emb = e[:, 1][cnt > 0]
        scores = _per_root_scores(lambda q, c: q @ c.T, query, pos_emb, torch.zeros((0, emb), device=dev), n_pos, [0] * B,
                                  query @ embs[1].T, 0, empty)
        ti = NodeAnchorBasedLinkPredictionTaskInputs(main_batch=None, random_neg_batch=None, batch_embeddings=None,
                                                     batch_scores=scores)
        loss, pairs = task(ti, device=dev)
        loss = loss / max(int(pairs), 1)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    for i in range(2 if a.autograd_steps else 0):
        autograd_step(i)
    autograd = []
    for _ in range(a.reps if a.autograd_steps else 0):
        st.synchronize()
        t1 = time.perf_counter()
        for i in range(a.autograd_steps):
            autograd_step(i)
        st.synchronize()
        autograd.append((time.perf_counter() - t1) / a.autograd_steps * 1e3)

    stat = lambda v: {"median": float(np.median(v)), "min": min(v), "max": max(v)}
    line = json.dumps(dict(nodes=n, feature_dim=d, hidden=hid, out=emb, anchors=B, negatives=n_neg, fanouts=fan,
                           steps_per_timing=a.steps, reps=a.reps, first_loss=first,
                           ms_per_step={t: stat(v) for t, v in times.items()},
                           spread_us=1e3 * max(max(v) - min(v) for v in times.values()),
                           margin_autograd_loop_ms_per_step=dict(stat(autograd), steps_per_timing=a.autograd_steps,
                                                                 clock="host, synchronised") if autograd else None))
    print(line, flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    eng.bind_stream(None)
    eng._graph_out = None  # (an alias of the main graph: freed once)
    eng.close()


main() if a.no_rotate else rotate()
