"""NablpTrainPlan.evaluate of a plan with hard-negative slots (H = 2) against the CPU restatement of the trainer's
validate(): the pattern, cases and width conditions of tests/test_gpu_lp_eval_plan.py::
test_plan_evaluation_against_the_cpu_restatement.  The loss has the hard-negative columns in it; the ranks are taken against
the RANDOM negatives only, as the reference's validate does (node_anchor_based_link_prediction_modeling_task_spec.py:
537-542: hit_rate_at_k / mean_reciprocal_rank over pos_scores and random_neg_scores) — hard negatives leave them alone."""
import numpy as np
import pytest
import torch

import oracle
from helpers import rmat_edges
from oracle import gnn_ref

pytestmark = pytest.mark.gpu

KS = [1, 5, 10, 50, 100, 500]
FAN = [10, 5]
TEMP = 0.07
H = 2


@pytest.fixture(scope="module")
def setup():
    """the graph of tests/test_gpu_lp_eval_plan.py's `setup` (its cases' intervals are narrow on it), plus a hard-negative
    list in which node i has i % (H + 2) entries"""
    from gigl_amd.engine import HipEngine
    s, d = rmat_edges(13, 150000, seed=8)
    n = 1 << 13
    rowptr, col = oracle.build_csc(n, s, d, is_directed=False)
    x = (np.random.default_rng(0).standard_normal((n, 100)) / 4).astype(np.float32)
    eng = HipEngine(0)
    eng.load_csc(rowptr, col)
    eng.load_features(x)
    dst = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rowptr).astype(np.int64))
    eng.build_from_coo(n, dst, col.astype(np.uint32), is_directed=True, out_graph=True)
    rng = np.random.default_rng(1)
    deg = np.arange(n) % (H + 2)
    eng.load_label_edges("neg", n, np.repeat(np.arange(n), deg), rng.integers(0, n, int(deg.sum())))
    yield eng, rowptr, col, x, n
    eng.close()


def _lp_batches(eng, n, b, P, n_rn, steps, seed):
    """that file's batches — the same anchors and random negatives from the same seed — with the hard-negative slots"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        anchors = torch.from_numpy(rng.permutation(n)[:b].astype(np.uint32).view(np.int32)).to(eng.device)
        roots, cnt = eng.nablp_main_roots(anchors, P, H, sampling_seed=42, neg_label_edges="neg")
        rn = torch.from_numpy(rng.permutation(n)[:n_rn].astype(np.uint32).view(np.int32)).to(eng.device)
        out.append((roots, cnt, rn))
    return out


def _short(batch, b, T, anchors=30, negatives=20):
    return (batch[0][: T * anchors].contiguous(), batch[1].view(2, b)[:, :anchors].reshape(-1).contiguous(),
            batch[2][:negatives].contiguous())


def _lp_loss_torch(emb_main, emb_rn, roots, cnt, rn, b, P, temperature):
    """infer_task_inputs + Retrieval on embeddings (utils/infer.py; loss.py:209-331): repeated queries x cat(positives,
    hard negatives — ragged —, random negatives), the same-query mask over the positives' block, the accidental-hit mask
    over every column, summed cross-entropy / query rows"""
    T = 1 + P + H
    ids = (roots.to(torch.int64) & 0xFFFFFFFF).view(b, T)
    kp, kn = cnt.to(torch.int64).view(2, b)
    base = torch.arange(b).view(-1, 1) * T
    slot_p, slot_h = torch.arange(P).view(1, P), torch.arange(H).view(1, H)
    ok_p, ok_h = (slot_p < kp.view(-1, 1)).reshape(-1), (slot_h < kn.view(-1, 1)).reshape(-1)
    q_rows = base.expand(-1, P).reshape(-1)[ok_p]
    p_rows = (base + 1 + slot_p).reshape(-1)[ok_p]
    h_rows = (base + 1 + P + slot_h).reshape(-1)[ok_h]
    scores = emb_main[q_rows] @ torch.cat([emb_main[p_rows], emb_main[h_rows], emb_rn]).T / temperature
    qid = ids.reshape(-1)[q_rows]
    cid = torch.cat([ids.reshape(-1)[p_rows], ids.reshape(-1)[h_rows], rn.to(torch.int64) & 0xFFFFFFFF])
    Q, Cn = scores.shape
    eye = torch.zeros((Q, Cn), dtype=torch.bool)
    eye[torch.arange(Q), torch.arange(Q)] = True
    same_q = torch.zeros_like(eye)
    same_q[:, :Q] = qid.view(-1, 1) == qid.view(1, -1)
    hit = cid.view(1, -1) == cid[:Q].view(-1, 1)
    masked = scores.masked_fill((same_q | hit) & ~eye, torch.finfo(torch.float32).min)
    return torch.nn.functional.cross_entropy(masked, torch.arange(Q), reduction="sum") / max(Q, 1)


def _cpu_embeddings(kind, rowptr, col, x, params, roots, heads):
    r_h = roots.cpu().numpy().view(np.uint32)
    nbr, _ = oracle.sample_khop(rowptr, col, r_h, FAN, canonical=True)
    u = oracle.union_build(r_h, FAN, nbr)
    ei = gnn_ref.union_edge_index(u["rowptr"], u["col"])
    h = torch.from_numpy(x[u["nodes"].astype(np.int64)])
    if kind == "sage":
        h = gnn_ref.graphsage_forward(h, ei, params, 2)
    else:
        for l, hd in enumerate((heads, 1)):
            p = f"conv_layers.{l}."
            h = gnn_ref.gat_conv(h, ei, params[p + "lin.weight"], params[p + "att_src"], params[p + "att_dst"],
                                 params[p + "bias"], hd)
            if l == 0:
                h = torch.relu(h)
    h = torch.nn.functional.normalize(h, p=2, dim=1)
    return h[torch.from_numpy(u["root_local"].astype(np.int64))]


def _rank_sums(pos, negs, shift):
    """(mean 1 / rank, [mean rank <= k]) of one anchor with ranks 1 + #{neg > pos + shift}"""
    ranks = 1 + (negs.reshape(1, -1) > (pos.reshape(-1, 1) + shift)).sum(axis=1)
    return float((1.0 / ranks).mean()), np.asarray([(ranks <= k).mean() for k in KS])


def _cpu_pass(kind, rowptr, col, x, params, batches, P, heads, delta):
    """validate() restated on the CPU -> (loss, {"mrr": (lo, hi), "hits": (lo [k], hi [k])}, ranked anchors): the rank
    metrics — against the random negatives only — as an interval: scores may differ by delta between two correct fp32
    forwards, so a near-tie may flip"""
    T = 1 + P + H
    losses, nodes = [], 0
    mrr, hits = np.zeros(2), np.zeros((2, len(KS)))
    with torch.no_grad():
        for roots, cnt, rn in batches:
            em = _cpu_embeddings(kind, rowptr, col, x, params, roots, heads)
            er = _cpu_embeddings(kind, rowptr, col, x, params, rn, heads)
            na = cnt.numel() // 2
            losses.append(float(_lp_loss_torch(em, er, roots.cpu(), cnt.cpu(), rn.cpu(), na, P, TEMP)))
            e64, r64 = em.double().numpy().reshape(na, T, -1), er.double().numpy()
            for i, c in enumerate(cnt.cpu().tolist()[:na]):
                p = min(c, P)
                if p <= 0:
                    continue
                nodes += 1
                pos, negs = e64[i, 1:1 + p] @ e64[i, 0], r64 @ e64[i, 0]
                for side, shift in enumerate((-delta, +delta)):  # worst case, best case
                    m, h = _rank_sums(pos, negs, shift)
                    mrr[side] += m
                    hits[side] += h
    return float(np.mean(losses)), {"mrr": tuple(mrr / max(nodes, 1)), "hits": tuple(hits / max(nodes, 1))}, nodes


def _models(kind):
    """(constructor of the model, plan class, heads of the first layer, embedding width)"""
    from gigl_amd.engine import GatNablpTrainPlan, NablpTrainPlan
    from gigl_amd.models import GraphSAGE
    from gigl_amd.models_attn import GAT
    if kind == "sage":
        make = lambda: GraphSAGE(100, 32, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True)
        return make, NablpTrainPlan, 1, 16
    make = lambda: GAT(100, 16, 32, num_layers=2, heads=2, should_l2_normalize_embedding_layer_output=True)
    return make, GatNablpTrainPlan, 2, 32


CPU_CASES = [("sage", 48, 2, 70, 11), ("gat", 48, 1, 32, 19)]  # (kind, b, P, n_rn, batch seed): that test's


@pytest.mark.parametrize("kind,b,P,n_rn,seed", CPU_CASES)
def test_plan_evaluation_with_hard_negatives_against_the_cpu_restatement(setup, kind, b, P, n_rn, seed):
    eng, rowptr, col, x, n = setup
    make, cls, heads, d = _models(kind)
    batches = _lp_batches(eng, n, b, P, n_rn, 2, seed=seed)
    assert all(set(c[b:].tolist()) == set(range(H + 1)) for _, c, _ in batches)  # (anchors with 0 .. H hard negatives)
    batches[-1] = _short(batches[-1], b, 1 + P + H)
    torch.manual_seed(6)
    model = make()
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    # unit rows, each within the project's 1e-5 forward bound: |<a, b> - <a', b'>| <= 2 sqrt(d) 1e-5
    delta = 2.0 * np.sqrt(d) * 1e-5
    want_loss, want, nodes = _cpu_pass(kind, rowptr, col, x, params, batches, P, heads, delta)
    widths = (want["mrr"][1] - want["mrr"][0], (want["hits"][1] - want["hits"][0]).max())
    print(f"{kind}: CPU loss {want_loss!r}, {nodes} ranked anchors, MRR in {want['mrr']}, hits in {want['hits']}, widths {widths}")
    # the intervals must be narrow, or being inside them says nothing
    assert nodes > 0 and widths[0] <= 2e-3 and widths[1] <= 0.04, widths
    lib = model.to(eng.device)
    st = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    try:
        plan = cls(eng, lib, b, P, n_rn, FAN, temperature=TEMP, lr=5e-3, weight_decay=1e-6, num_hard_negatives=H)
        with torch.cuda.stream(st):
            got = plan.evaluate(batches, KS)
            again = plan.evaluate(batches, KS)  # (the graph part is replayed from its captured graph from the second call on)
        steps = plan.adam_steps()
        plan.close()
    finally:
        eng.bind_stream(torch.cuda.current_stream(eng.device))
    print(f"{kind}: plan {got}")
    assert got["batches"] == 2 and got["rank_nodes"] == nodes and steps == 0
    np.testing.assert_allclose(got["loss"], want_loss, rtol=1e-4, atol=1e-5)
    assert want["mrr"][0] - 1e-6 <= got["mrr"] <= want["mrr"][1] + 1e-6, (got["mrr"], want["mrr"])
    for i, k in enumerate(KS):
        assert want["hits"][0][i] - 1e-6 <= got["hits"][i] <= want["hits"][1][i] + 1e-6, (k, got["hits"][i], want["hits"])
    assert again["batches"] == 2 and again["rank_nodes"] == nodes
    np.testing.assert_allclose(again["loss"], want_loss, rtol=1e-4, atol=1e-5)
    assert want["mrr"][0] - 1e-6 <= again["mrr"] <= want["mrr"][1] + 1e-6
