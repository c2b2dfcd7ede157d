"""gigl_nablp_train_plan_eval / NablpTrainPlan.evaluate (one library call per evaluation batch, one host read per pass)
against the CPU restatement of the trainer's validate() — oracle sample -> collate -> fp32 forward of both batches ->
normalise -> scores -> retrieval loss, and per anchor the ranks of its positives among the random negatives — and the
contract of the call: it trains nothing, keeps an announced batch, leaves the captured training graphs valid, and a pass
that overflows a regular plan's workspace is redone in a wide one."""
import numpy as np
import pytest
import torch

import oracle
from helpers import assert_adam_state, rmat_edges
from oracle import gnn_ref

KS = [1, 5, 10, 50, 100, 500]
FAN = [10, 5]
TEMP = 0.07


@pytest.fixture(scope="module")
def setup():
    """the graph of tests/test_gpu_train_plan.py's `setup`, with its out-graph (the positives are drawn from it)"""
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
    yield eng, rowptr, col, x, n
    eng.close()


def _lp_batches(eng, n, b, P, n_rn, steps, seed):
    """main roots (anchor-major: anchor + its P positive slots, a missing positive repeats the anchor), positives per
    anchor and random-negative roots of `steps` batches, drawn as the trainer's in-HBM route draws them"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        anchors = torch.from_numpy(rng.permutation(n)[:b].astype(np.uint32).view(np.int32)).to(eng.device)
        pos, cnt = eng.sample_positives(anchors, P, sampling_seed=42)
        ar = torch.arange(P, device=eng.device).view(1, P)
        a2 = anchors.view(-1, 1)
        grouped = torch.where(ar < cnt.view(-1, 1), pos.view(-1, P), a2.expand(-1, P))
        roots = torch.cat([a2, grouped], dim=1).reshape(-1).contiguous()
        rn = torch.from_numpy(rng.permutation(n)[:n_rn].astype(np.uint32).view(np.int32)).to(eng.device)
        out.append((roots, cnt.to(torch.int32).contiguous(), rn))
    return out


def _short(batch, T, anchors=30, negatives=20):
    return (batch[0][: T * anchors].contiguous(), batch[1][:anchors].contiguous(), batch[2][:negatives].contiguous())


def _lp_loss_torch(emb_main, emb_rn, roots, cnt, rn, b, P, temperature):
    """infer_task_inputs + Retrieval on embeddings (utils/infer.py; loss.py:209-331): repeated queries x cat(positives,
    random negatives), the same-query and accidental-hit masks, summed cross-entropy / query rows"""
    T = 1 + P
    ids = (roots.to(torch.int64) & 0xFFFFFFFF).view(b, T)
    slot = torch.arange(P).view(1, P)
    ok = (slot < cnt.to(torch.int64).view(-1, 1)).reshape(-1)
    q_rows = (torch.arange(b) * T).repeat_interleave(P)[ok]
    p_rows = (torch.arange(b).view(-1, 1) * T + 1 + slot).reshape(-1)[ok]
    rq, pos = emb_main[q_rows], emb_main[p_rows]
    scores = rq @ torch.cat([pos, emb_rn]).T / temperature
    qid = ids[:, 0].repeat_interleave(P)[ok]
    cid = torch.cat([ids.reshape(-1)[p_rows], rn.to(torch.int64) & 0xFFFFFFFF])
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
    metrics as an interval — scores may differ by delta between two correct fp32 forwards, so a near-tie may flip"""
    T = 1 + P
    losses, nodes = [], 0
    mrr, hits = np.zeros(2), np.zeros((2, len(KS)))
    with torch.no_grad():
        for roots, cnt, rn in batches:
            em = _cpu_embeddings(kind, rowptr, col, x, params, roots, heads)
            er = _cpu_embeddings(kind, rowptr, col, x, params, rn, heads)
            na = cnt.numel()
            losses.append(float(_lp_loss_torch(em, er, roots.cpu(), cnt.cpu(), rn.cpu(), na, P, TEMP)))
            e64, r64 = em.double().numpy().reshape(na, T, -1), er.double().numpy()
            for i, c in enumerate(cnt.cpu().tolist()):
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


# (kind, b, P, n_rn, batch seed): GraphSAGE 100 -> 32 -> 16 with two positive slots per anchor; the GAT plan at the shape of
# test_library_gat_link_prediction_step_against_the_cpu_restatement.  The batch seeds are ones for which the CPU intervals
# below are narrow enough to check something (asserted from the CPU values alone; of the seeds 11, 13, 17, 19, 23 all do for
# GraphSAGE, 17, 19 and 23 for the GAT — widths up to 6.4e-4 / 7.6e-3 and 2.0e-4 / 0).
CPU_CASES = [("sage", 48, 2, 70, 11), ("gat", 48, 1, 32, 19)]


def cpu_case(setup, kind, b, P, n_rn, seed):
    eng, rowptr, col, x, n = setup
    make, cls, heads, d = _models(kind)
    batches = _lp_batches(eng, n, b, P, n_rn, 2, seed=seed)
    batches[-1] = _short(batches[-1], 1 + P)
    torch.manual_seed(6)
    model = make()
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    # unit rows, each within the project's 1e-5 forward bound: |<a, b> - <a', b'>| <= 2 sqrt(d) 1e-5
    delta = 2.0 * np.sqrt(d) * 1e-5
    want_loss, want, nodes = _cpu_pass(kind, rowptr, col, x, params, batches, P, heads, delta)
    widths = (want["mrr"][1] - want["mrr"][0], (want["hits"][1] - want["hits"][0]).max())
    return batches, model, cls, want_loss, want, nodes, widths


@pytest.mark.gpu
@pytest.mark.parametrize("kind,b,P,n_rn,seed", CPU_CASES)
def test_plan_evaluation_against_the_cpu_restatement(setup, kind, b, P, n_rn, seed):
    eng = setup[0]
    batches, model, cls, want_loss, want, nodes, widths = cpu_case(setup, kind, b, P, n_rn, seed)
    print(f"{kind}: CPU loss {want_loss!r}, {nodes} ranked anchors, MRR in {want['mrr']}, hits in {want['hits']}, widths {widths}")
    # the intervals must be narrow, or being inside them says nothing
    assert nodes > 0 and widths[0] <= 2e-3 and widths[1] <= 0.04, widths
    lib = model.to(eng.device)
    st = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    try:
        plan = cls(eng, lib, b, P, n_rn, FAN, temperature=TEMP, lr=5e-3, weight_decay=1e-6)
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


@pytest.mark.gpu
@pytest.mark.parametrize("kind,b,P,n_rn", [("sage", 128, 1, 64), ("gat", 96, 1, 40)])
def test_evaluation_leaves_training_alone(setup, kind, b, P, n_rn):
    """6 steps with prefetch (one step announces a batch that is then not the one trained on), an evaluation pass of two
    batches after steps 2 and 4 — step 2 announced its next batch — against the same 6 steps without: same loss history,
    same Adam state, same step count"""
    eng, rowptr, col, x, n = setup
    make, cls, heads, d = _models(kind)
    steps = 6
    batches = _lp_batches(eng, n, b, P, n_rn, steps, seed=5)
    evals = _lp_batches(eng, n, b, P, n_rn, 2, seed=21)
    evals[-1] = _short(evals[-1], 1 + P)

    def run(with_evals):
        torch.manual_seed(4)
        lib = make().to(eng.device)
        st = torch.cuda.Stream(device=eng.device)
        torch.cuda.synchronize()
        eng.bind_stream(st)
        try:
            plan = cls(eng, lib, b, P, n_rn, FAN, temperature=TEMP, remove_accidental_hits=True, lr=5e-3, weight_decay=1e-6)
            got, passes = [], []
            with torch.cuda.stream(st):
                for i, (roots, cnt, rn) in enumerate(batches):
                    nxt = None
                    if i + 1 < steps and i % 4 != 2:
                        j = i + 1 if i != 4 else 0  # (step 4 announces the wrong batch)
                        nxt = (batches[j][0], batches[j][2])
                    got.append(plan.step(roots, cnt, rn, next_roots=nxt).clone())
                    if with_evals and i in (1, 3):
                        assert nxt is not None
                        passes.append(plan.evaluate(evals, KS))
            eng.synchronize()
            n_steps = plan.adam_steps()
            plan.store(lib)
            moments = plan.moments()
            plan.close()
        finally:
            eng.bind_stream(torch.cuda.current_stream(eng.device))
        return [float(v[0]) for v in got], lib, moments, n_steps, passes

    want, lib0, mom0, steps0, _ = run(False)
    got, lib1, mom1, steps1, passes = run(True)
    print(f"{kind}: losses with evaluation passes {got} vs without {want}; passes {passes}")
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)
    assert steps1 == steps0 == steps
    # (the GAT plan hands out its moments flat)
    flat = (lambda sd: {k: v.reshape(-1) for k, v in sd.items()}) if kind == "gat" else (lambda sd: sd)
    assert_adam_state(f"{kind} plan with evaluation passes vs without", flat(lib1.state_dict()), mom1, flat(lib0.state_dict()),
                      mom0, tol_m=1e-4, tol_v=1e-4, tol_p=1e-4)
    assert len(passes) == 2
    for m in passes:
        assert m["batches"] == 2 and m["rank_nodes"] > 0 and np.isfinite([m["loss"], m["mrr"], *m["hits"]]).all()
    assert passes[0]["loss"] != passes[1]["loss"]  # (the second pass saw the parameters two steps later)


@pytest.mark.gpu
def test_evaluation_grows_a_plan_whose_workspace_overflows():
    """a graph of 4096 nodes with fan-outs (2, 50), as tests/test_gpu_overflow.py builds it: roots are each other's sampled
    neighbours, a regular plan's workspace overflows — evaluate() grows the plan, redoes the pass, and returns what a plan
    that was wide from the start returns"""
    from gigl_amd.engine import HipEngine, NablpTrainPlan
    from gigl_amd.models import GraphSAGE
    N, E, fan, d = 4096, 60_000, [2, 50], 64
    src, dst = rmat_edges(15, E, 7)
    src, dst = (src.astype(np.int64) * 0x9E3779B1) % N, (dst.astype(np.int64) * 0x9E3779B1) % N
    keep = src != dst
    rowptr, col = oracle.build_csc(N, src[keep].astype(np.uint32), dst[keep].astype(np.uint32), is_directed=False)
    x = (np.random.default_rng(3).standard_normal((N, d)) / 4).astype(np.float32)
    b, P, n_rn = 48, 1, 32
    eng = HipEngine(0)
    try:
        eng.load_csc(rowptr, col)
        eng.load_features(x)
        dst_rows = np.repeat(np.arange(N, dtype=np.uint32), np.diff(rowptr).astype(np.int64))
        eng.build_from_coo(N, dst_rows, col.astype(np.uint32), is_directed=True, out_graph=True)
        batches = _lp_batches(eng, N, b, P, n_rn, 3, seed=11)
        over = []
        for roots, _, _ in batches:
            r_h = roots.cpu().numpy().view(np.uint32)
            u = oracle.union_build(r_h, fan, oracle.sample_khop(rowptr, col, r_h, fan, canonical=True)[0])
            over.append(int(u["meta"][3]) > r_h.size * (1 + fan[0]))
        assert any(over), over
        torch.manual_seed(6)
        lib = GraphSAGE(d, 32, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)
        st = torch.cuda.Stream(device=eng.device)
        torch.cuda.synchronize()
        eng.bind_stream(st)
        with torch.cuda.stream(st):
            plan = NablpTrainPlan(eng, lib, b, P, n_rn, fan, temperature=TEMP)
            got = plan.evaluate(batches, KS)
            assert plan.wide and plan.overflow_redone == 1 and plan.eval_overflowed == 0
            plan.close()
            wide = NablpTrainPlan(eng, lib, b, P, n_rn, fan, temperature=TEMP)
            wide.grow()
            want = wide.evaluate(batches, KS)
            assert wide.eval_overflowed == 0 and not hasattr(wide, "overflow_redone")
            wide.close()
        eng.bind_stream(torch.cuda.current_stream(eng.device))
        print("evaluation after growing:", got, "vs a wide plan's:", want)
        assert got["batches"] == want["batches"] == 3 and got["rank_nodes"] == want["rank_nodes"] > 0
        assert np.isfinite([got["loss"], got["mrr"], *got["hits"]]).all()
        # (the same kernels over the same inputs; only the order of the fp32 atomics inside a forward may differ)
        np.testing.assert_allclose([got["loss"], got["mrr"], *got["hits"]], [want["loss"], want["mrr"], *want["hits"]],
                                   rtol=1e-6, atol=0)
    finally:
        eng.close()
