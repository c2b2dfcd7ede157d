"""gigl_lp_rank_metrics (csrc/loss.hip: MRR and hits@k of a score matrix, one wave per anchor, summed on the device) through
the C ABI against a numpy fp64 restatement of base._positive_ranks / hit_rate_at_k / mean_reciprocal_rank written here: the
rank of a positive is one more than the number of VALID negatives that score strictly higher, an anchor adds the means over
its positives, anchors without a positive add nothing.  Counts are exact; sums are within 1e-9 (both sides are fp64 sums of
a few terms of size <= 1, only the order differs)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gigl_amd._lib import (LP_EVAL_BATCHES, LP_EVAL_HITS0, LP_EVAL_LEN, LP_EVAL_LOSS_SUM, LP_EVAL_MRR_SUM,
                           LP_EVAL_RANK_NODES)

B, P = 5, 3
POS_CNT = [3, 0, 1, 2, 3]
KS = [1, 5, 10, 50, 100, 500]


@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _reference(scores, pos_cnt, n_neg, neg_col0, neg_valid, ks):
    """-> (mrr sum, ranked anchors, hits sums) in fp64"""
    mrr, nodes, hits = 0.0, 0, np.zeros(len(ks), np.float64)
    s = scores.astype(np.float64)
    keep = np.ones(n_neg, bool) if neg_valid is None else neg_valid.astype(bool)
    for i in range(B):
        p = min(int(pos_cnt[i]), P)
        if p <= 0:
            continue
        ranks = []
        for j in range(p):
            q = i * P + j
            negs = s[q, neg_col0:neg_col0 + n_neg][keep]
            ranks.append(1 + int((negs > s[q, q]).sum()))
        ranks = np.asarray(ranks, np.float64)
        mrr += float((1.0 / ranks).mean())
        hits += np.asarray([(ranks <= k).mean() for k in ks])
        nodes += 1
    return mrr, nodes, hits


def _scores(n_neg, seed):
    """[Q][ld] scores with ld > Q + n_neg; some negatives TIE with the row's positive exactly, one is -inf; the columns
    beyond the negatives hold large values that must never be read as negatives"""
    rng = np.random.default_rng(seed)
    Q = B * P
    ld = Q + n_neg + 3
    # a coarse grid: many exact ties among the fp32 values
    s = (rng.integers(-8, 9, (Q, ld)) / 8.0).astype(np.float32)
    s[:, Q + n_neg:] = 100.0
    for q in range(Q):
        if n_neg >= 1:
            s[q, Q + (q % n_neg)] = s[q, q]  # a tie with the positive: not counted
        if n_neg >= 2:
            s[q, Q + ((q + 1) % n_neg)] = -np.inf
    return s, ld


def _run(eng, s, ld, n_neg, neg_valid, acc, ks=KS, pos_cnt=POS_CNT):
    dev = eng.device
    sd = torch.from_numpy(s).to(dev)
    pc = torch.tensor(pos_cnt, dtype=torch.int32, device=dev)
    nv = None if neg_valid is None else torch.from_numpy(neg_valid.astype(np.int32)).to(dev)
    ks_arr = (C.c_int32 * len(ks))(*ks)
    torch.cuda.synchronize()  # (the inputs were written on torch's stream, the call runs on the engine's)
    rc = eng._lib.gigl_lp_rank_metrics(eng._ctx, C.c_void_p(sd.data_ptr()), ld, B, P, C.c_void_p(pc.data_ptr()), n_neg, B * P,
                                       C.c_void_p(nv.data_ptr()) if nv is not None else None, ks_arr, len(ks),
                                       C.c_void_p(acc.data_ptr()))
    eng.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("n_neg", [0, 1, 63, 64, 70])
@pytest.mark.parametrize("masked", [False, True])
def test_rank_metrics_equal_the_numpy_restatement(eng, n_neg, masked):
    s, ld = _scores(n_neg, seed=n_neg)
    neg_valid = (np.arange(n_neg) % 2 == 0) if masked else None  # every other negative invalid
    mrr, nodes, hits = _reference(s, POS_CNT, n_neg, B * P, neg_valid, KS)
    assert nodes == 4
    acc = torch.zeros(LP_EVAL_LEN, dtype=torch.float64, device=eng.device)
    assert _run(eng, s, ld, n_neg, neg_valid, acc) == 0
    a = acc.cpu().numpy()
    print(f"n_neg={n_neg} masked={masked}: mrr sum {a[LP_EVAL_MRR_SUM]!r} vs {mrr!r}, hits sums "
          f"{a[LP_EVAL_HITS0:LP_EVAL_HITS0 + len(KS)]} vs {hits}")
    assert a[LP_EVAL_RANK_NODES] == nodes
    assert a[LP_EVAL_LOSS_SUM] == 0 and a[LP_EVAL_BATCHES] == 0 and (a[LP_EVAL_HITS0 + len(KS):] == 0).all()
    assert abs(a[LP_EVAL_MRR_SUM] - mrr) <= 1e-9
    np.testing.assert_allclose(a[LP_EVAL_HITS0:LP_EVAL_HITS0 + len(KS)], hits, rtol=0, atol=1e-9)
    beyond = [i for i, k in enumerate(KS) if k >= 1 + n_neg]  # a k beyond 1 + #negatives is always a hit
    assert all(abs(a[LP_EVAL_HITS0 + i] - nodes) <= 1e-9 for i in beyond)
    # a second call ADDS into the (non-zero) accumulators; two calls on the same input give identical bits
    run1 = acc.clone()
    acc[LP_EVAL_LOSS_SUM] = 3.5
    first = acc.clone()
    assert _run(eng, s, ld, n_neg, neg_valid, acc) == 0
    delta = (acc - first).cpu().numpy()
    a2 = acc.cpu().numpy()
    assert a2[LP_EVAL_LOSS_SUM] == 3.5 and a2[LP_EVAL_RANK_NODES] == 2 * nodes
    assert abs(a2[LP_EVAL_MRR_SUM] - 2 * mrr) <= 1e-9
    np.testing.assert_allclose(a2[LP_EVAL_HITS0:LP_EVAL_HITS0 + len(KS)], 2 * hits, rtol=0, atol=1e-9)
    assert abs(delta[LP_EVAL_MRR_SUM] - mrr) <= 1e-9
    again = torch.zeros(LP_EVAL_LEN, dtype=torch.float64, device=eng.device)
    assert _run(eng, s, ld, n_neg, neg_valid, again) == 0
    assert torch.equal(again.view(torch.int64), run1.view(torch.int64))


@pytest.mark.gpu
def test_rank_metrics_reject_bad_ks(eng):
    s, ld = _scores(8, seed=1)
    acc = torch.zeros(LP_EVAL_LEN, dtype=torch.float64, device=eng.device)
    assert _run(eng, s, ld, 8, None, acc, ks=[1, 0]) == -1          # GIGL_E_INVALID_ARG: k < 1
    assert _run(eng, s, ld, 8, None, acc, ks=list(range(1, 10))) == -1  # more than GIGL_LP_EVAL_MAX_KS
    assert (acc.cpu().numpy() == 0).all()
