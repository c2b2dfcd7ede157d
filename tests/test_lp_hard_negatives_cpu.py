"""The host-side index arithmetic of hard negatives in the link-prediction plans, on the CPU: the positions of the real
positives / hard negatives in the anchor-major root list (hbm.nablp_label_rows) against a loop, and the padding of a short
batch to a plan's capacity (engine.pad_lp_batch — what NablpTrainPlan._padded calls) with the count list's two halves
padded separately."""
import numpy as np
import pytest
import torch


@pytest.mark.parametrize("P,H", [(1, 0), (2, 3), (1, 1), (3, 2)])
def test_label_rows_against_a_loop(P, H):
    from gigl_amd.hbm import nablp_label_rows
    rng = np.random.default_rng(P * 10 + H)
    for b in (1, 2, 7, 40):
        n_pos, n_neg = rng.integers(0, P + 1, b), rng.integers(0, H + 1, b)
        T = 1 + P + H
        want_p = [i * T + 1 + j for i in range(b) for j in range(int(n_pos[i]))]
        want_n = [i * T + 1 + P + k for i in range(b) for k in range(int(n_neg[i]))]
        got_p, got_n = nablp_label_rows(n_pos, n_neg, P, H)
        assert got_p.dtype == np.int64 and got_n.dtype == np.int64
        assert got_p.tolist() == want_p and got_n.tolist() == want_n
    got_p, got_n = nablp_label_rows(np.zeros(3, np.int64), np.zeros(3, np.int64), P, H)
    assert got_p.size == 0 and got_n.size == 0


def test_padding_keeps_the_two_count_halves_apart():
    from gigl_amd.engine import pad_lp_batch
    b, P, H, n_rn = 5, 2, 3, 4
    T = 1 + P + H
    roots = torch.arange(3 * T, dtype=torch.int32)
    cnt = torch.tensor([2, 1, 0, 3, 0, 2], dtype=torch.int32)  # (positives of 3 anchors, then their hard negatives)
    rn = torch.tensor([7, 8], dtype=torch.int32)
    r2, c2, n2 = pad_lp_batch(roots, cnt, rn, b, P, H, n_rn)
    assert r2.tolist() == list(range(3 * T)) + [-1] * (2 * T)
    assert c2.tolist() == [2, 1, 0, 0, 0, 3, 0, 2, 0, 0] and c2.dtype == torch.int32
    assert n2.tolist() == [7, 8, -1, -1]
    # a full batch is handed through; the next batch's roots are padded without counts
    full = torch.arange(b * T, dtype=torch.int32)
    cf = torch.arange(2 * b, dtype=torch.int32)
    r3, c3, n3 = pad_lp_batch(full, cf, torch.arange(n_rn, dtype=torch.int32), b, P, H, n_rn)
    assert torch.equal(r3, full) and torch.equal(c3, cf) and n3.numel() == n_rn
    r4, c4, _ = pad_lp_batch(roots, None, rn, b, P, H, n_rn)
    assert r4.numel() == b * T and c4 is None


def test_padding_without_hard_negatives_is_one_count_per_anchor():
    from gigl_amd.engine import pad_lp_batch
    roots = torch.arange(4, dtype=torch.int32)  # 2 anchors x (1 + 1)
    r, c, n = pad_lp_batch(roots, torch.tensor([1, 0], dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 3, 1, 0, 2)
    assert r.tolist() == [0, 1, 2, 3, -1, -1] and c.tolist() == [1, 0, 0] and n.tolist() == [-1, -1]
    with pytest.raises(AssertionError):
        pad_lp_batch(roots, torch.tensor([1, 0, 0, 0], dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 3, 1, 0, 2)
