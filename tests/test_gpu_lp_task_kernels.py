"""The Margin and Softmax tasks' kernels over designed score matrices (gigl_lp_task_loss / gigl_lp_task_loss_backward,
csrc/loss.hip; the contract is in include/gigl_hip.h), without a graph: the plan's head calls the same launchers.

Reference: `_restate` below, an fp64 numpy restatement of the header's formulas written for this file (not the package's
Margin / Softmax modules).  Bounds, the project's own: the loss within 1e-5 of the reference's, relative; the gradient within
1e-4 of the reference's largest element; a reference of exactly 0 (no negatives, no valid row) must be met exactly.

Every entry of the score matrix that the contract says takes NO part is NaN here — the rows' padding beyond C, invalid rows,
invalid negatives' columns, the positives' block off the diagonal, the other anchors' hard negatives — so a kernel that
reads one of them into a sum shows up as a NaN, not as an error in the seventh digit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN, TEMP = 0.3, 0.07
E_INVALID_ARG = -1

# (b, P, H, n_rn, ld - C)
SHAPES = [(1, 1, 0, 1, 0), (1, 1, 0, 0, 0), (3, 2, 3, 5, 7), (5, 1, 1, 63, 0), (5, 1, 1, 64, 0), (5, 1, 1, 65, 0),
          (4, 3, 2, 255, 0), (4, 3, 2, 257, 0), (2, 1, 0, 1029, 3)]


@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _design(b, P, H, n_rn, pad, seed, values=None):
    """-> (scores [Q, C + pad] float32, pos_cnt int32, valid int32 [C], cases): counts per anchor in the order (fewer than P
    positives, all H hard negatives), (0 positives, fewer than H), (all P, 0 hard negatives), ...; the LAST anchor of a batch
    of two or more is absent; about a fifth of the random negatives' columns are invalid, the span's first and last among
    them when it has five or more.  valid is what the plan's lp_pack_kernel would write for these counts.  Scores are
    multiples of 1 / 64 in [-2, 2] (or drawn from `values`); what takes no part is NaN."""
    rng = np.random.default_rng(seed)
    Q, R0 = b * P, b * (P + H)
    Cn = R0 + n_rn
    present = np.ones(b, dtype=bool)
    if b >= 2:
        present[-1] = False
    pos = np.array([[max(P - 1, 1), 0, P][i % 3] for i in range(b)]) * present
    hard = np.array([[H, H // 2, 0][i % 3] for i in range(b)]) * present
    valid = np.zeros(Cn, dtype=np.int32)
    for i in range(b):
        valid[i * P:i * P + pos[i]] = 1
        valid[Q + i * H:Q + i * H + hard[i]] = 1
    rn_ok = rng.random(n_rn) >= 0.2
    if n_rn >= 5:
        rn_ok[[0, n_rn - 1, n_rn // 2]] = False
    elif n_rn:
        rn_ok[:] = True
    valid[R0:] = rn_ok
    draw = (lambda size: rng.integers(-128, 129, size) / 64.0) if values is None else (lambda size: rng.choice(values, size))
    s = np.full((Q, Cn + pad), np.nan, dtype=np.float32)
    for q in range(Q):
        i = q // P
        if not valid[q]:
            continue
        s[q, q] = draw(1)[0]
        cols = np.concatenate([Q + i * H + np.flatnonzero(valid[Q + i * H:Q + (i + 1) * H]), R0 + np.flatnonzero(valid[R0:])])
        s[q, cols] = draw(cols.size)
    cases = set()
    for i in range(b):
        if not present[i]:
            cases.add("absent anchor")
            continue
        cases.add("0 positives" if pos[i] == 0 else "fewer positives" if pos[i] < P else "all positives")
        if H:
            cases.add("0 hard" if hard[i] == 0 else "fewer hard" if hard[i] < H else "all hard")
    if n_rn and not rn_ok.all():
        cases.add("invalid random negative")
    cnt = np.concatenate([pos, hard]) if H else pos
    return s, cnt.astype(np.int32), valid, cases


def _restate(kind, param, w, s, b, P, H, n_rn, valid):
    """the header's formulas in fp64 -> (loss, valid rows, normaliser, dscores [Q, C], used [Q, C] bool: Neg(q) and q itself,
    smallest |m - pos + neg| over the pairs (Margin))"""
    Q, R0 = b * P, b * (P + H)
    Cn = R0 + n_rn
    param = float(np.float32(param))  # (the library is handed a float)
    w = float(np.float32(w))
    x = s[:, :Cn].astype(np.float64)
    d = np.zeros((Q, Cn))
    used = np.zeros((Q, Cn), dtype=bool)
    rows, pairs, total, kink = 0, 0, 0.0, np.inf
    per_row = []
    for q in range(Q):
        if not valid[q]:
            continue
        i = q // P
        neg = np.concatenate([Q + i * H + np.flatnonzero(valid[Q + i * H:Q + (i + 1) * H]), R0 + np.flatnonzero(valid[R0:])])
        rows += 1
        pairs += neg.size
        used[q, q] = True
        used[q, neg] = True
        per_row.append((q, neg))
    for q, neg in per_row:
        pos = x[q, q]
        if kind == "Margin":
            h = param - pos + x[q, neg]
            if neg.size:
                kink = min(kink, float(np.abs(h).min()))
            total += float(np.maximum(h, 0.0).sum())
            act = h >= 0.0
            d[q, neg] = w * act / max(pairs, 1)
            d[q, q] = -w * act.sum() / max(pairs, 1)
        else:
            v = np.concatenate([[pos], x[q, neg]]) / param
            m = v.max()
            lse = m + np.log(np.exp(v - m).sum())
            total += lse - v[0]
            p = np.exp(v - lse)
            d[q, neg] = w * p[1:] / (param * max(rows, 1))
            d[q, q] = w * (p[0] - 1.0) / (param * max(rows, 1))
    norm = pairs if kind == "Margin" else rows
    return w * total / max(norm, 1), rows, norm, d, used, kink


def _run(eng, kind, param, w, s, b, P, H, n_rn, cnt, valid, with_cnt=True):
    dev = eng.device
    st = torch.from_numpy(s).to(dev)
    out3, row_a, row_b, d = eng.lp_task_loss(kind, param, w, st, b, P, H, n_rn,
                                             torch.from_numpy(cnt).to(dev) if with_cnt else None, torch.from_numpy(valid).to(dev))
    eng.synchronize()
    return out3.cpu().numpy(), row_a.cpu().numpy(), row_b.cpu().numpy(), d.cpu().numpy()


def _check(tag, got3, got_d, want):
    loss, rows, norm, d, used, _ = want
    print(f"{tag}: loss {float(got3[0])!r} want {float(loss)!r} rel {abs(float(got3[0]) - loss) / max(abs(loss), 1e-300):.2e}; rows {got3[1]} norm "
          f"{got3[2]}; gradient error {np.abs(got_d - d).max() / max(np.abs(d).max(), 1e-300):.2e} of the largest element")
    assert got3[1] == rows and got3[2] == norm, tag
    if loss == 0.0:
        assert got3[0] == 0.0, tag
    else:
        assert abs(got3[0] - loss) <= 1e-5 * abs(loss), tag
    assert np.isfinite(got_d).all(), tag
    assert not got_d[~used].any(), f"{tag}: a column outside Neg(q) and q, or an invalid row, has a gradient"
    if not d.any():
        assert not got_d.any(), tag
    else:
        assert np.abs(got_d - d).max() <= 1e-4 * np.abs(d).max(), tag


def test_the_designed_batches_hold_every_case():
    """from the inputs: every batch of two or more anchors has an absent one; the batches with three or more have an anchor
    without a positive, and — where P >= 2 / H >= 2 make it possible — one with fewer than P positives and hard-negative
    counts of 0 (four or more anchors: a present one's), fewer than H and H; every batch with five or more random negatives
    has invalid ones.  (One or two anchors cannot hold all of it; the union over the shapes does.)"""
    seen = set()
    for k, (b, P, H, n_rn, pad) in enumerate(SHAPES):
        cases = _design(b, P, H, n_rn, pad, seed=k)[3]
        seen |= cases
        if b >= 2:
            assert "absent anchor" in cases
        if b >= 3:
            assert "0 positives" in cases
            if P >= 2:
                assert "fewer positives" in cases
            if H >= 1:
                assert "all hard" in cases
                if b >= 4:  # (of three anchors two are present: the third count of 0 is the absent anchor's)
                    assert "0 hard" in cases
            if H >= 2:
                assert "fewer hard" in cases
        if n_rn >= 5:
            assert "invalid random negative" in cases
    assert seen == {"absent anchor", "0 positives", "fewer positives", "all positives", "0 hard", "fewer hard", "all hard",
                    "invalid random negative"}


@pytest.mark.parametrize("kind,param", [("Margin", MARGIN), ("Softmax", TEMP)])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_loss_and_gradient_against_the_fp64_restatement(eng, kind, param, shape):
    """every shape of the issue's table, both tasks, weight 0.75.  Margin: on the grid every m - pos + neg is at least 3.1e-3
    from zero (asserted, no pair left out), so the active set is the reference's.  Also: a second call gives the same bits;
    pos_cnt == NULL (valid alone decides) gives the same bits; weight 0.5 x gives EXACTLY half of every loss and gradient
    word — bit for bit, not within an ulp: the weight enters each result through one scale word (w / N, w / (T R), w x the
    fp64 sum) and halving a float is exact, so every later rounding happens on exactly halved operands."""
    b, P, H, n_rn, pad = shape
    s, cnt, valid, _ = _design(b, P, H, n_rn, pad, seed=SHAPES.index(shape))
    w = 0.75
    want = _restate(kind, param, w, s, b, P, H, n_rn, valid)
    if kind == "Margin" and want[2] > 0:
        assert want[5] >= 3.1e-3, want[5]
    got3, ra, rb, d = _run(eng, kind, param, w, s, b, P, H, n_rn, cnt, valid)
    _check(f"{kind} {shape}", got3, d, want)
    if n_rn == 0:  # no negatives at all: loss 0, no gradient
        assert got3[0] == 0.0 and not d.any() and want[0] == 0.0
    again = _run(eng, kind, param, w, s, b, P, H, n_rn, cnt, valid)
    for x, y in zip((got3, ra, rb, d), again):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    bare = _run(eng, kind, param, w, s, b, P, H, n_rn, cnt, valid, with_cnt=False)
    assert np.array_equal(bare[0].view(np.uint32), got3.view(np.uint32)) and np.array_equal(bare[3].view(np.uint32), d.view(np.uint32))
    half3, _, _, half_d = _run(eng, kind, param, w / 2, s, b, P, H, n_rn, cnt, valid)
    assert np.array_equal((half_d * np.float32(2)).view(np.uint32), d.view(np.uint32))
    assert np.float32(half3[0] * np.float32(2)).view(np.uint32) == got3[:1].view(np.uint32)[0]


def test_margin_at_the_exact_kink_follows_clamp_min(eng):
    """m = 0.25, pos = 0.5, neg = 0.25: m - pos + neg is exactly 0 in fp32.  torch's margin_ranking_loss differentiates
    through clamp_min, whose gradient at 0 is 1: loss 0, -w / N on the positive, +w / N on the negative (N = 1)"""
    s = np.array([[0.5, 0.25]], dtype=np.float32)
    w = 0.75
    got3, _, rb, d = _run(eng, "Margin", 0.25, w, s, 1, 1, 0, 1, np.array([1], np.int32), np.array([1, 1], np.int32))
    assert got3.tolist() == [0.0, 1.0, 1.0] and rb.tolist() == [1.0]
    assert d.tolist() == [[-w, w]]


def test_softmax_with_extreme_logits_is_finite_and_within_bounds(eng):
    """scores +-40 at T = 0.07 (logits +-571: exp overflows fp32 without the running maximum)"""
    b, P, H, n_rn, pad = 4, 3, 2, 257, 0
    s, cnt, valid, _ = _design(b, P, H, n_rn, pad, seed=21, values=np.array([-40.0, 40.0]))
    want = _restate("Softmax", TEMP, 1.0, s, b, P, H, n_rn, valid)
    got3, _, _, d = _run(eng, "Softmax", TEMP, 1.0, s, b, P, H, n_rn, cnt, valid)
    assert np.isfinite(got3).all() and np.isfinite(want[0]) and want[0] > 100.0
    _check("Softmax +-40", got3, d, want)


def test_invalid_arguments_are_refused(eng):
    from gigl_amd._lib import LP_TASKS
    import ctypes as C
    dev = eng.device
    b, P, H, n_rn = 2, 1, 1, 3
    Cn = b * (P + H) + n_rn
    s = torch.zeros((b * P, Cn), dtype=torch.float32, device=dev)
    valid = torch.ones(Cn, dtype=torch.int32, device=dev)
    ra, rb, o3 = (torch.zeros(4, dtype=torch.float32, device=dev) for _ in range(3))
    d = torch.zeros((b * P, Cn), dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def fwd(kind, param, weight, ld=Cn):
        return eng._lib.gigl_lp_task_loss(eng._ctx, kind, param, weight, p(s), ld, b, P, H, n_rn, None, p(valid), p(ra), p(rb), p(o3))

    def bwd(kind, param, weight, ld=Cn):
        return eng._lib.gigl_lp_task_loss_backward(eng._ctx, kind, param, weight, p(s), ld, b, P, H, n_rn, None, p(valid), p(ra),
                                                   p(rb), p(o3), p(d))
    M, S, R = LP_TASKS["Margin"], LP_TASKS["Softmax"], LP_TASKS["Retrieval"]
    inf, nan = float("inf"), float("nan")
    for call in (fwd, bwd):
        assert call(M, 0.3, 1.0) == 0 and call(S, 0.07, 2.5) == 0 and call(M, -1.0, 1e-3) == 0
        for bad in ((S, 0.0, 1.0), (S, -0.07, 1.0), (S, nan, 1.0), (S, inf, 1.0), (M, nan, 1.0), (M, inf, 1.0), (M, -inf, 1.0),
                    (M, 0.3, 0.0), (M, 0.3, -1.0), (M, 0.3, inf), (S, 0.07, nan), (7, 0.3, 1.0), (-1, 0.3, 1.0), (R, 0.07, 1.0)):
            assert call(*bad) == E_INVALID_ARG, bad
        assert call(M, 0.3, 1.0, ld=Cn - 1) == E_INVALID_ARG
    eng.synchronize()
