"""keyed (TopK / RandomWeighted) vs uniform frontier expansion over the SAME frontier: gigl_expand_frontier_keyed vs
gigl_expand_frontier on a DBLP-sized typed graph (one hop of an op DAG over a realistic frontier) and on a hub-heavy
frontier.  Prints µs per call (device events), the bytes a keyed op must read (sum of the frontier rows' degrees x 8 B:
col + weight) over that time as a fraction of the 8 TB/s HBM peak, and the frontier's degree bins.
usage (GPU box): python scripts/micro_keyed_expand.py [n_authors n_papers edges_per_type]
kernel times: rocprofv3 --kernel-trace --stats -d <out> -- python scripts/micro_keyed_expand.py"""
import sys

import numpy as np
import torch

from gigl_amd._lib import SAMPLE_RANDOM_WEIGHTED, SAMPLE_TOPK
from gigl_amd.graphdb_sampler import INCOMING, EdgeType, HipGraphDBSampler

HBM_PEAK = 8.0e12
na, npp, ne = (int(v) for v in (sys.argv[1:4] + ["500000", "1000000", "8000000"])[:3])
rng = np.random.default_rng(0)
a2p = EdgeType("author", "writes", "paper")
src = (na * rng.random(ne) ** 2).astype(np.uint32)  # skewed authors: the busiest wrote ~ne / sqrt(na) papers
dst = rng.integers(0, npp, ne).astype(np.uint32)
w = rng.random(ne).astype(np.float32)
s = HipGraphDBSampler({"author": 0, "paper": 1}, {"author": na, "paper": npp}, {a2p: (src, dst)}, {a2p: 0},
                      edge_key_columns={a2p: {"w": w}})
eng = s.engine
deg_out = np.bincount(src, minlength=na)  # (upper bound of the distinct row lengths: repeats are rare here)


def frontier(kind: str, m: int):
    if kind == "dblp":  # hop 2 of a paper-rooted DAG: the authors of sampled papers (degree-weighted)
        return src[rng.integers(0, ne, m)]
    hubs = np.argsort(deg_out)[-64:].astype(np.uint32)  # hub-heavy: the 64 busiest authors in a quarter of the slots
    v = rng.integers(0, na, m).astype(np.uint32)
    on = rng.random(m) < 0.25
    v[on] = rng.choice(hubs, int(on.sum()))
    return v


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


label = s._key(a2p, "OUTGOING")
col = s.key_column(a2p, "OUTGOING", "w")
for kind, m in (("dblp", 40960), ("dblp", 409600), ("hubs", 40960)):
    nodes = frontier(kind, m)
    ksums = rng.integers(0, 2**31, m).astype(np.int32)
    nd = torch.from_numpy(nodes.view(np.int32)).to(eng.device)
    kd = torch.from_numpy(ksums).to(eng.device)
    d = deg_out[nodes].astype(np.int64)
    bytes_ = int(d.sum()) * 8
    for f in (10, 64, 256):
        bins = {"<=f": int((d <= f).sum()), "f<n<=64": int(((d > f) & (d <= 64)).sum()),
                ">64": int(((d > f) & (d > 64)).sum())}
        heavy_share = float(d[(d > f) & (d > 64)].sum()) / max(float(d.sum()), 1.0)
        t_u = timed(lambda: eng.expand_frontier(nd, kd, f, 42, 1, label_edges=label))
        t_t = timed(lambda: eng.expand_frontier_keyed(nd, kd, f, 42, SAMPLE_TOPK, col, label))
        t_w = timed(lambda: eng.expand_frontier_keyed(nd, kd, f, 42, SAMPLE_RANDOM_WEIGHTED, col, label))
        print(f"{kind:5s} m={m:7d} f={f:4d} sum_deg={int(d.sum()):10d}  uniform {t_u:9.1f} us  topk {t_t:9.1f} us "
              f"({bytes_ / (t_t * 1e-6) / HBM_PEAK:5.3f} of HBM peak)  random_weighted {t_w:9.1f} us "
              f"({bytes_ / (t_w * 1e-6) / HBM_PEAK:5.3f})  bins {bins}  heavy rows' share of sum_deg {heavy_share:.2f}",
              flush=True)
s.close()
