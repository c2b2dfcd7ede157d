"""Hard negatives in the library's link-prediction training plans (gigl_ctx_set_lp_hard_negatives, gigl_nablp_main_roots;
csrc/pipeline.hip, csrc/sample.hip): the main batch has T = 1 + P + H roots per anchor, the candidates are
cat(positives, hard negatives, random negatives) as in the reference's infer_task_inputs (utils/infer.py), every query row
is scored against all of them, the same-query mask covers the positives' block and the accidental-hit mask every column.

Checked against the torch composition the root assembler replaces (bit-exact), against the autograd step at equal weights,
against the CPU restatement (oracle sample -> collate -> fp32 forward -> ragged loss -> autograd -> Adam), and — H = 0 —
against the plan as it was, bit for bit.  The graph has 390 nodes (five of them without an edge) and no node has more than
f0 = 10 neighbours: the first hop then takes every neighbour of a root, so the nodes of level <= 1 are the roots and their
neighbours — at most b (1 + f0) rows whichever roots a batch has.  That is the static bound of a regular plan's workspace
AND of the autograd forward over a HipBatch these tests compare with (models.GraphSAGE._forward_union_autograd sizes its
buffers by it and runs the device's row count): a batch of five random-negative roots on a denser graph leaves it."""
import numpy as np
import pytest
import torch

import oracle
from helpers import assert_adam_state, torch_adam_moments
from oracle import gnn_ref

pytestmark = pytest.mark.gpu

N, N_ISOLATED, FAN, TEMP = 390, 5, [10, 5], 0.07


def _engine(x):
    from gigl_amd.engine import HipEngine
    rng = np.random.default_rng(8)
    m = N - N_ISOLATED  # (the last N_ISOLATED nodes have no edge: anchors without a positive)
    # four permutations' edges i -> perm(i), both directions: at most 8 neighbours per node
    s = np.tile(np.arange(m), 4).astype(np.uint32)
    d = np.concatenate([rng.permutation(m) for _ in range(4)]).astype(np.uint32)
    rowptr, col = oracle.build_csc(N, s, d, is_directed=False)
    assert int(np.diff(rowptr).max()) <= FAN[0] and int(np.diff(rowptr)[:m].min()) >= 2
    eng = HipEngine(0)
    eng.load_csc(rowptr, col)
    eng.load_features(x)
    dst = np.repeat(np.arange(N, dtype=np.uint32), np.diff(rowptr).astype(np.int64))
    eng.build_from_coo(N, dst, col.astype(np.uint32), is_directed=True, out_graph=True)  # (out-edges = reversed in-edges)
    return eng, rowptr, col


@pytest.fixture(scope="module")
def setup():
    x = (np.random.default_rng(0).standard_normal((N, 100)) / 4).astype(np.float32)
    eng, rowptr, col = _engine(x)
    yield eng, rowptr, col, x, N
    eng.close()


def _i32(a, dev):
    return torch.from_numpy(np.asarray(a).astype(np.uint32).view(np.int32)).to(dev)


def _torch_main_roots(eng, anchors, P, H, neg_list):
    """the composition gigl_nablp_main_roots replaces: two sample_positives (counters 3 / 4), where / cat"""
    a2 = anchors.view(-1, 1)
    pos, cnt = eng.sample_positives(anchors, P, sampling_seed=42)
    cols = [a2, torch.where(torch.arange(P, device=eng.device).view(1, P) < cnt.view(-1, 1), pos.view(-1, P), a2.expand(-1, P))]
    ncnt = torch.zeros_like(cnt)
    if H:
        if neg_list is not None:
            neg, ncnt = eng.sample_positives(anchors, H, sampling_seed=42, counter=4, label_edges=neg_list)
            cols.append(torch.where(torch.arange(H, device=eng.device).view(1, H) < ncnt.view(-1, 1), neg.view(-1, H),
                                    a2.expand(-1, H)))
        else:
            cols.append(a2.expand(-1, H))
    return torch.cat(cols, dim=1).reshape(-1).contiguous(), torch.cat([cnt, ncnt]).to(torch.int32)


@pytest.mark.parametrize("P,H", [(1, 0), (2, 3), (1, 1)])
def test_main_roots_equal_the_torch_composition(setup, P, H):
    """gigl_nablp_main_roots, bit for bit: node i has i % (H + 2) hard negatives (counts 0 .. H and one over), one anchor of
    the batch is absent (0xFFFFFFFF: a row of 0xFFFFFFFF, counts 0), and without a hard-negative list every such slot is empty"""
    eng, rowptr, col, x, n = setup
    rng = np.random.default_rng(3)
    deg = np.arange(n) % (H + 2)
    src = np.repeat(np.arange(n), deg)
    dst = np.concatenate([rng.permutation(n)[:k] for k in deg]) if src.size else src
    eng.load_label_edges("neg_roots", n, src, dst)
    ids = rng.permutation(n)[:75].astype(np.int64)
    ids[17] = 0xFFFFFFFF
    ids[40] = n - 1  # (no out-edge: no positive)
    anchors = _i32(ids, eng.device)
    for neg_list in ("neg_roots", None):
        want_r, want_c = _torch_main_roots(eng, anchors, P, H, neg_list)
        got_r, got_c = eng.nablp_main_roots(anchors, P, H, sampling_seed=42, neg_label_edges=neg_list)
        eng.synchronize()
        assert got_r.dtype == torch.int32 and got_c.dtype == torch.int32
        assert torch.equal(got_r, want_r) and torch.equal(got_c, want_c), (P, H, neg_list)
        T = 1 + P + H
        assert got_r.view(-1, T)[17].tolist() == [-1] * T and got_c.view(2, -1)[:, 17].tolist() == [0, 0]
        assert int(got_c[40]) == 0
        if H and neg_list:
            k = got_c.view(2, -1)[1].cpu().numpy()
            real = ids != 0xFFFFFFFF
            assert np.array_equal(k[real], np.minimum(deg[ids[real]], H)) and set(k.tolist()) == set(range(H + 1))
            assert (deg[ids[real]] == H + 1).any()
        else:
            assert int(got_c.view(2, -1)[1].abs().sum()) == 0


def test_the_setting_refuses_what_it_cannot_hold(setup):
    from gigl_amd._lib import GIGL_MAX_FANOUT
    eng = setup[0]
    lib = eng._lib
    assert lib.gigl_ctx_set_lp_hard_negatives(eng._ctx, -1) != 0
    assert lib.gigl_ctx_set_lp_hard_negatives(eng._ctx, GIGL_MAX_FANOUT + 1) != 0
    assert lib.gigl_ctx_set_lp_hard_negatives(eng._ctx, GIGL_MAX_FANOUT) == 0
    assert lib.gigl_ctx_set_lp_hard_negatives(eng._ctx, 0) == 0


def _designed_batches(eng, n, b, P, H, n_rn, steps, seed, list_name):
    """`steps` batches (main roots [b T], counts [2 b], random negatives) whose hard-negative list is BUILT so that the
    batches hold every case the head has to tell apart — asserted below from the batches themselves:
    an anchor with 0 hard negatives, one with fewer than H, one with all H, an anchor WITHOUT a positive that has hard
    negatives, a hard negative that is its own row's positive (an accidental hit: excluded from that row), one that is
    another anchor's positive (stays a candidate), one equal to a random negative of the batch."""
    rng = np.random.default_rng(seed)
    anchors = [rng.permutation(n - N_ISOLATED)[:b] for _ in range(steps)]
    rns = [rng.permutation(n)[:n_rn] for _ in range(steps)]
    anchors[1][0] = n - 1  # (an isolated node: no positive, H hard negatives)
    pos_all, cnt_all = eng.sample_positives(_i32(np.arange(n), eng.device), P, sampling_seed=42)
    pos_all, cnt_all = pos_all.view(n, P).cpu().numpy().view(np.uint32).astype(np.int64), cnt_all.cpu().numpy()
    lists = {v: rng.permutation(n)[: v % (H + 2)].tolist() for v in range(n)}  # (0 .. H + 1 hard negatives per node)
    a0, a1, a2 = (int(v) for v in anchors[0][:3])
    a3 = next(int(v) for v in anchors[0][3:] if cnt_all[v] > 0 and pos_all[v, 0] not in pos_all[a2, :cnt_all[a2]])
    assert cnt_all[a1] > 0 and H >= 2
    lists[a0] = []
    lists[a1] = [int(pos_all[a1, 0])]
    fill = [int(v) for v in rng.permutation(n) if v not in (pos_all[a3, 0], rns[0][0])]
    lists[a2] = [int(pos_all[a3, 0]), int(rns[0][0])] + fill[: H - 2]
    lists[n - 1] = [int(v) for v in anchors[1][1:1 + H]]
    assert len(set(lists[a2])) == H
    src = np.concatenate([np.full(len(v), k, dtype=np.int64) for k, v in lists.items()])
    dst = np.concatenate([np.asarray(v, dtype=np.int64) for v in lists.values()])
    eng.load_label_edges(list_name, n, src, dst)
    out = []
    for a, rn in zip(anchors, rns):
        roots, cnt = eng.nablp_main_roots(_i32(a, eng.device), P, H, sampling_seed=42, neg_label_edges=list_name)
        out.append((roots, cnt, _i32(rn, eng.device)))
    eng.synchronize()
    # ---- the cases, read back from the batches
    T = 1 + P + H
    seen = set()
    for roots, cnt, rn in out:
        ids = (roots.cpu().numpy().view(np.uint32).astype(np.int64)).reshape(b, T)
        kp, kn = cnt.cpu().numpy().reshape(2, b)
        rn_ids = set(rn.cpu().numpy().view(np.uint32).astype(np.int64).tolist())
        pos_of = [set(ids[i, 1:1 + kp[i]].tolist()) for i in range(b)]
        for i in range(b):
            hard = ids[i, 1 + P:1 + P + kn[i]].tolist()
            assert len(hard) == min(len(lists[int(ids[i, 0])]), H) and set(hard) <= set(lists[int(ids[i, 0])])
            seen.add("none" if kn[i] == 0 else "all" if kn[i] == H else "fewer")
            if kp[i] == 0 and kn[i] > 0:
                seen.add("anchor without a positive")
            for h in hard:
                if h in pos_of[i]:
                    seen.add("own positive")
                if any(h in pos_of[j] for j in range(b) if j != i) and h not in pos_of[i]:
                    seen.add("another anchor's positive")
                if h in rn_ids:
                    seen.add("a random negative")
    assert seen == {"none", "fewer", "all", "anchor without a positive", "own positive", "another anchor's positive",
                    "a random negative"}, seen
    return out


def _lp_loss_torch(emb_main, emb_rn, roots, cnt, rn, b, P, H, temperature):
    """infer_task_inputs + Retrieval on embeddings, in torch (utils/infer.py; loss.py:209-331): repeated queries x
    cat(positives, hard negatives, random negatives) — the hard negatives RAGGED, as the reference concatenates them —
    the same-query mask over the positives' block, the accidental-hit mask over every column, CE / rows"""
    T, dev = 1 + P + H, roots.device
    ids = (roots.to(torch.int64) & 0xFFFFFFFF).view(b, T)
    kp, kn = cnt.to(torch.int64).view(2, b)
    base = torch.arange(b, device=dev).view(-1, 1) * T
    slot_p, slot_h = torch.arange(P, device=dev).view(1, P), torch.arange(H, device=dev).view(1, H)
    ok_p, ok_h = (slot_p < kp.view(-1, 1)).reshape(-1), (slot_h < kn.view(-1, 1)).reshape(-1)
    q_rows = base.expand(-1, P).reshape(-1)[ok_p]
    p_rows = (base + 1 + slot_p).reshape(-1)[ok_p]
    h_rows = (base + 1 + P + slot_h).reshape(-1)[ok_h]
    rq = emb_main[q_rows]
    cand = torch.cat([emb_main[p_rows], emb_main[h_rows], emb_rn])
    scores = rq @ cand.T / temperature
    qid = ids.reshape(-1)[q_rows]
    cid = torch.cat([ids.reshape(-1)[p_rows], ids.reshape(-1)[h_rows], rn.to(torch.int64) & 0xFFFFFFFF])
    Q, Cn = scores.shape
    eye = torch.zeros((Q, Cn), dtype=torch.bool, device=dev)
    eye[torch.arange(Q), torch.arange(Q)] = True
    same_q = torch.zeros_like(eye)
    same_q[:, :Q] = qid.view(-1, 1) == qid.view(1, -1)
    hit = cid.view(1, -1) == cid[:Q].view(-1, 1)
    masked = scores.masked_fill((same_q | hit) & ~eye, torch.finfo(torch.float32).min)
    return torch.nn.functional.cross_entropy(masked, torch.arange(Q, device=dev), reduction="sum") / max(Q, 1)


def _plan_run(eng, plan, batches, prefetch=False):
    """the batches through plan.step on a stream of its own -> ([loss], [rows])"""
    st = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    try:
        got = []
        with torch.cuda.stream(st):
            for i, (roots, cnt, rn) in enumerate(batches):  # (eager once, captured on the second step, replayed from then on)
                nxt = None
                if prefetch and i + 1 < len(batches) and i % 4 != 2:
                    j = i + 1 if i != 4 else 0  # (step 4 announces the wrong batch)
                    nxt = (batches[j][0], batches[j][2])
                got.append(plan.step(roots, cnt, rn, next_roots=nxt).clone())
        eng.synchronize()
    finally:
        eng.bind_stream(torch.cuda.current_stream(eng.device))
    return [float(v[0]) for v in got], [float(v[1]) for v in got]


@pytest.mark.parametrize("dims,b,P,H,n_rn,prefetch", [((100, 32, 16), 6, 2, 3, 5, False), ((100, 32, 70), 48, 1, 2, 32, True)])
def test_step_with_hard_negatives_equals_the_autograd_step(setup, dims, b, P, H, n_rn, prefetch):
    """the pattern of test_library_link_prediction_step_equals_the_autograd_step with hard-negative columns: 8 steps, the
    loss history at rtol 2e-5 / atol 2e-6, Adam's state at 1e-4 (that test's bounds for the normalised encoder), rows = the
    positives that took part.  The second case has an embedding width that is no multiple of 64 (the unpack keeps 8 columns
    per lane) and announces most batches ahead."""
    from gigl_amd.engine import NablpTrainPlan
    from gigl_amd.models import GraphSAGE, HipBatch
    eng, rowptr, col, x, n = setup
    steps = 8
    batches = _designed_batches(eng, n, b, P, H, n_rn, steps, seed=5, list_name="neg_step")
    torch.manual_seed(4)
    kw = dict(num_layers=2, should_l2_normalize_embedding_layer_output=True)
    ref = GraphSAGE(*dims, **kw).to(eng.device)
    lib = GraphSAGE(*dims, **kw).to(eng.device)
    lib.load_state_dict(ref.state_dict())
    ref.train()
    opt = torch.optim.Adam(ref.parameters(), lr=5e-3, weight_decay=1e-6, foreach=False)
    want = []
    for roots, cnt, rn in batches:
        embs = []
        for r in (roots, rn):
            tree = eng.sample_khop(r, FAN)
            u = eng.union_build(tree)
            embs.append(ref(HipBatch(eng, tree, u, train=True))[u.root_local[: r.numel()].long()])
        loss = _lp_loss_torch(embs[0], embs[1], roots, cnt, rn, b, P, H, TEMP)
        opt.zero_grad()
        loss.backward()
        opt.step()
        want.append(float(loss))
    plan = NablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, remove_accidental_hits=True, lr=5e-3, weight_decay=1e-6,
                          num_hard_negatives=H)
    got, rows = _plan_run(eng, plan, batches, prefetch)
    plan.store(lib)
    moments = plan.moments()
    plan.close()
    print(f"H={H}: plan losses {got} autograd losses {want}")
    assert rows == [float(int(c[:b].clamp(max=P).sum())) for _, c, _ in batches]
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)
    assert_adam_state("hard-negative plan vs autograd", lib.state_dict(), moments, ref.state_dict(),
                      torch_adam_moments(opt, dict(ref.named_parameters())), tol_m=1e-4, tol_v=1e-4, tol_p=1e-4)


def test_step_with_hard_negatives_against_the_cpu_restatement(setup):
    """the pattern of test_library_link_prediction_step_against_the_cpu_restatement over the T-root list: oracle sample ->
    collate -> fp32 forward (gnn_ref) -> normalise -> the ragged loss -> torch autograd -> Adam; 4 steps, the last batch
    short in anchors AND in random negatives"""
    from gigl_amd.engine import NablpTrainPlan
    from gigl_amd.models import GraphSAGE
    eng, rowptr, col, x, n = setup
    b, P, H, n_rn, steps = 48, 1, 2, 32, 4
    T = 1 + P + H
    batches = _designed_batches(eng, n, b, P, H, n_rn, steps, seed=11, list_name="neg_cpu")
    r_, c_, rn_ = batches[-1]
    batches[-1] = (r_[: T * 30].contiguous(), c_.view(2, b)[:, :30].reshape(-1).contiguous(), rn_[:20].contiguous())
    torch.manual_seed(6)
    model = GraphSAGE(100, 32, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True)
    params = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(list(params.values()), lr=5e-3, weight_decay=1e-6, foreach=False)
    want = []
    for roots, cnt, rn in batches:
        embs = []
        for r in (roots, rn):
            r_h = r.cpu().numpy().view(np.uint32)
            nbr, _ = oracle.sample_khop(rowptr, col, r_h, FAN, canonical=True)
            u = oracle.union_build(r_h, FAN, nbr)
            ei = gnn_ref.union_edge_index(u["rowptr"], u["col"])
            out = gnn_ref.graphsage_forward(torch.from_numpy(x[u["nodes"].astype(np.int64)]), ei, params, 2)
            out = torch.nn.functional.normalize(out, p=2, dim=1)
            embs.append(out[torch.from_numpy(u["root_local"].astype(np.int64))])
        loss = _lp_loss_torch(embs[0], embs[1], roots.cpu(), cnt.cpu(), rn.cpu(), cnt.numel() // 2, P, H, TEMP)
        opt.zero_grad()
        loss.backward()
        opt.step()
        want.append(float(loss))
    lib = GraphSAGE(100, 32, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)
    lib.load_state_dict(model.state_dict())
    plan = NablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, lr=5e-3, weight_decay=1e-6, num_hard_negatives=H)
    got, _ = _plan_run(eng, plan, batches)
    plan.store(lib)
    moments = plan.moments()
    plan.close()
    print(f"plan losses {got} CPU losses {want}")
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)
    assert_adam_state("hard-negative plan vs the CPU restatement", lib.state_dict(), moments, params,
                      torch_adam_moments(opt, params), tol_m=1e-3, tol_v=1e-3, tol_p=1e-4)


def test_gat_step_with_hard_negatives_equals_the_autograd_step(setup):
    """the GAT kind (gigl_gat_nablp_train_plan_create shares the head) at the smallest shape of GAT_LP_STEP_CASES — four
    heads of 8, 16 out, not normalised, fp32 — against the autograd step over device-built batch graphs, at the bounds of
    test_library_gat_link_prediction_step_equals_the_autograd_step for that case: losses rtol 1e-3 / atol 1e-5, Adam's
    state 1e-3 / 1e-3 / 1e-4"""
    from gigl_amd.engine import GatNablpTrainPlan
    from gigl_amd.hbm import ResidentGraph
    from gigl_amd.models_attn import GAT
    _, rowptr, col, x, n = setup
    eng, _, _ = _engine(x)  # (an engine of its own: ResidentGraph.from_engine borrows it)
    try:
        b, P, H, n_rn, steps = 24, 1, 2, 16, 6
        batches = _designed_batches(eng, n, b, P, H, n_rn, steps, seed=9, list_name="neg_gat")
        torch.manual_seed(6)
        kw = dict(num_layers=2, heads=4, should_l2_normalize_embedding_layer_output=False)
        ref = GAT(100, 8, 16, **kw).to(eng.device)
        lib = GAT(100, 8, 16, **kw).to(eng.device)
        lib.load_state_dict(ref.state_dict())
        ref.train()
        ref.engine = eng
        res = ResidentGraph.from_engine(eng, np.arange(n, dtype=np.int64), FAN)
        res.train_as_graph_data, res.defer_x = True, True
        opt = torch.optim.Adam(ref.parameters(), lr=5e-3, weight_decay=1e-6, foreach=False)
        want = []
        for roots, cnt, rn in batches:
            embs = []
            for r in (roots, rn):
                g, ri = res.train_graph(r)
                embs.append(ref(g)[ri])
            loss = _lp_loss_torch(embs[0], embs[1], roots, cnt, rn, b, P, H, TEMP)
            opt.zero_grad()
            loss.backward()
            opt.step()
            want.append(float(loss))
        plan = GatNablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, remove_accidental_hits=True, lr=5e-3,
                                 weight_decay=1e-6, num_hard_negatives=H)
        got, rows = _plan_run(eng, plan, batches, prefetch=True)
        plan.store(lib)
        moments = plan.moments()
        plan.close()
        print(f"GAT, H={H}: plan losses {got} autograd losses {want}")
        assert rows == [float(int(c[:b].clamp(max=P).sum())) for _, c, _ in batches]
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-5)
        flat = lambda sd: {k: v.reshape(-1) for k, v in sd.items()}
        assert_adam_state("GAT hard-negative plan vs autograd", flat(lib.state_dict()), moments, flat(ref.state_dict()),
                          {k: (m.reshape(-1), v.reshape(-1)) for k, (m, v) in
                           torch_adam_moments(opt, dict(ref.named_parameters())).items()},
                          tol_m=1e-3, tol_v=1e-3, tol_p=1e-4)
    finally:
        eng.close()


def _plain_batches(eng, n, b, P, n_rn, steps, seed):
    """batches without hard negatives in which no node is a root more than twice (anchors and their positives): the roots'
    output gradients are added with atomics, and only a sum of up to two terms is the same bits in either order"""
    rng = np.random.default_rng(seed)
    pos_all, cnt_all = eng.sample_positives(_i32(np.arange(n), eng.device), P, sampling_seed=42)
    pos_all, cnt_all = pos_all.view(n, P).cpu().numpy().view(np.uint32).astype(np.int64), cnt_all.cpu().numpy()
    out = []
    for _ in range(steps):
        times, anchors = {}, []
        for a in rng.permutation(n).tolist():
            mine = [a] + pos_all[a, :cnt_all[a]].tolist()
            if all(times.get(v, 0) + mine.count(v) <= 2 for v in mine):
                anchors.append(a)
                for v in mine:
                    times[v] = times.get(v, 0) + 1
            if len(anchors) == b:
                break
        assert len(anchors) == b
        roots, cnt = eng.nablp_main_roots(_i32(anchors, eng.device), P, 0, sampling_seed=42)
        out.append((roots, cnt[:b].contiguous(), _i32(rng.permutation(n)[:n_rn], eng.device)))
    return out


def _matching_runs(kinds):
    """the GraphSAGE plan WITHOUT hard negatives over the same 4 batches from the same weights, once per entry of `kinds`:
    "plain" (created without the call), "zero" (after gigl_ctx_set_lp_hard_negatives(ctx, 0)), "after_two" (after a plan with
    H = 2 of the same engine was used, grown and closed) -> {kind: (losses, rows, parameters)}, and the batches.
    The graph is a perfect matching — every node has ONE neighbour — and no node is a root more than twice.  The step
    leaves the order of two kinds of float sums open: the roots' gradient rows (atomics, one term per root that is the
    node) and a hidden row's gradient, which starts from the row's own term and adds the rows of its transposed list in the
    list's order (filled with atomics: gather_mean_backward's transposed kernel).  Here both have two terms at the most — on
    a ring the second has three, and two runs of one plan differ in the last bits — and two terms add up to the same bits in
    either order."""
    from gigl_amd.engine import HipEngine, NablpTrainPlan
    from gigl_amd.models import GraphSAGE
    n, b, P, n_rn = 384, 48, 1, 32
    rng = np.random.default_rng(8)
    pairs = rng.permutation(n).astype(np.uint32).reshape(-1, 2)
    rowptr, col = oracle.build_csc(n, pairs[:, 0], pairs[:, 1], is_directed=False)
    assert np.diff(rowptr).tolist() == [1] * n
    eng = HipEngine(0)
    try:
        eng.load_csc(rowptr, col)
        eng.load_features((rng.standard_normal((n, 100)) / 4).astype(np.float32))
        dst = np.arange(n, dtype=np.uint32)
        eng.build_from_coo(n, dst, col.astype(np.uint32), is_directed=True, out_graph=True)
        batches = _plain_batches(eng, n, b, P, n_rn, 4, seed=13)
        torch.manual_seed(4)
        init = GraphSAGE(100, 32, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True).state_dict()

        def explicit_zero():
            assert eng._lib.gigl_ctx_set_lp_hard_negatives(eng._ctx, 0) == 0

        def a_plan_with_two_came_first():
            deg = np.arange(n) % 4  # (0 .. 3 hard negatives per node, two slots)
            eng.load_label_edges("neg_leak", n, np.repeat(np.arange(n), deg), rng.integers(0, n, int(deg.sum())))
            hard = []
            for _ in range(2):
                roots, cnt = eng.nablp_main_roots(_i32(rng.permutation(n)[:b], eng.device), P, 2, sampling_seed=42,
                                                  neg_label_edges="neg_leak")
                hard.append((roots, cnt, _i32(rng.permutation(n)[:n_rn], eng.device)))
            other = GraphSAGE(100, 32, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)
            plan = NablpTrainPlan(eng, other, b, P, n_rn, FAN, temperature=TEMP, lr=5e-3, weight_decay=1e-6, num_hard_negatives=2)
            losses, _ = _plan_run(eng, plan, hard)
            plan.grow()  # (the re-created wide plan has the slots too: it takes the same batches)
            losses += _plan_run(eng, plan, hard)[0]
            plan.close()
            assert np.isfinite(losses).all() and int(hard[0][1][b:].sum()) > 0

        out = {}
        for kind in kinds:
            lib = GraphSAGE(100, 32, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)
            lib.load_state_dict(init)
            {"plain": lambda: None, "zero": explicit_zero, "after_two": a_plan_with_two_came_first}[kind.split("#")[0]]()
            plan = NablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, lr=5e-3, weight_decay=1e-6)
            got, rows = _plan_run(eng, plan, batches)
            plan.store(lib)
            plan.close()
            out[kind] = (got, rows, {k: v.clone() for k, v in lib.state_dict().items()})
        return out, batches, P
    finally:
        eng.close()


def test_no_hard_negatives_is_the_plan_as_it_was_bit_for_bit():
    """H = 0: a plan created after gigl_ctx_set_lp_hard_negatives(ctx, 0) and one created without the call give BIT-EQUAL
    loss histories and parameters over the same 4 batches — and so does one created after a plan with H = 2 of the same
    engine was used, grown and closed: the setting does not outlive the create call it was made for (a plan that had kept
    the two slots would read 2 b counts and 4 b roots out of these buffers).  On a general graph two runs of ONE plan differ
    in the last bits (_matching_runs says where the order of a float sum is open; measured: a ring leaves parameters 4e-7
    apart), so the graph is one on which they do not: the plan created without the call is run twice and must repeat itself
    too, or the comparison would say nothing."""
    runs, batches, P = _matching_runs(["plain", "zero", "after_two", "plain#again"])
    base = runs["plain"]
    assert np.isfinite(base[0]).all() and base[1] == [float(int(c.clamp(max=P).sum())) for _, c, _ in batches]
    diff = lambda x: max(float((x[2][k] - v).abs().max()) for k, v in base[2].items())
    print({kind: (r[0] == base[0], diff(r)) for kind, r in runs.items()})
    for kind in ("plain#again", "zero", "after_two"):
        other = runs[kind]
        assert other[1] == base[1], kind
        assert other[0] == base[0], kind
        for k in base[2]:
            assert torch.equal(other[2][k], base[2][k]), (kind, k)


def test_gradients_reach_a_hard_negatives_rows():
    """one anchor whose ONLY connection to node v is a hard-negative edge (v is in no tree of the batch but its own): after one
    step gigl_nablp_train_plan_grads equals autograd's to 1e-4 of the largest element (the project's gradient bound), and
    the same step with that column masked (its count 0) gives a DIFFERENT first-layer gradient — the path is live"""
    from gigl_amd.engine import HipEngine, NablpTrainPlan
    from gigl_amd.models import GraphSAGE, HipBatch
    rng = np.random.default_rng(2)
    n = 64
    # two components: nodes 0..31 (the anchor's side, the random negatives) and 32..63 (v's side); at most f0 neighbours
    # per node (three permutations' edges on each side), so that the autograd forward's static row bound holds
    half = np.arange(32)
    s = np.concatenate([np.tile(half, 3), np.tile(half + 32, 3)]).astype(np.uint32)
    d = np.concatenate([rng.permutation(32) for _ in range(3)] + [32 + rng.permutation(32) for _ in range(3)]).astype(np.uint32)
    rowptr, col = oracle.build_csc(n, s, d, is_directed=False)
    assert int(np.diff(rowptr).max()) <= FAN[0]
    x = (rng.standard_normal((n, 100)) / 4).astype(np.float32)
    eng = HipEngine(0)
    try:
        eng.load_csc(rowptr, col)
        eng.load_features(x)
        dst = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rowptr).astype(np.int64))
        eng.build_from_coo(n, dst, col.astype(np.uint32), is_directed=True, out_graph=True)
        anchor = int(np.flatnonzero(np.diff(rowptr)[:32] > 0)[0])
        v = 32 + int(np.flatnonzero(np.diff(rowptr)[32:] > 0)[0])
        eng.load_label_edges("neg_one", n, np.array([anchor]), np.array([v]))
        b, P, H, n_rn = 1, 1, 1, 4
        roots, cnt = eng.nablp_main_roots(_i32([anchor], eng.device), P, H, sampling_seed=42, neg_label_edges="neg_one")
        rn = _i32(rng.permutation(32)[:n_rn], eng.device)
        eng.synchronize()
        assert cnt.tolist() == [1, 1] and (roots.cpu().numpy().view(np.uint32)[[0, 2]]).tolist() == [anchor, v]
        torch.manual_seed(4)
        kw = dict(num_layers=2, should_l2_normalize_embedding_layer_output=True)
        ref = GraphSAGE(100, 32, 16, **kw).to(eng.device)
        init = {k: t.clone() for k, t in ref.state_dict().items()}
        grads = {}
        for tag, c in (("live", cnt), ("masked", torch.tensor([1, 0], dtype=torch.int32, device=eng.device))):
            embs = []
            for r in (roots, rn):
                tree = eng.sample_khop(r, FAN)
                u = eng.union_build(tree)
                embs.append(ref(HipBatch(eng, tree, u, train=True))[u.root_local[: r.numel()].long()])
            ref.zero_grad()
            _lp_loss_torch(embs[0], embs[1], roots, c, rn, b, P, H, TEMP).backward()
            want = [torch.cat([cv.lin_l.weight.grad, cv.lin_r.weight.grad], dim=1).clone() for cv in ref.conv_layers]
            lib = GraphSAGE(100, 32, 16, **kw).to(eng.device)
            lib.load_state_dict(init)
            plan = NablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, lr=5e-3, weight_decay=1e-6, num_hard_negatives=H)
            plan.grow()  # (three roots of a 64-node graph: the worst-case workspace; the grown plan keeps the slot)
            st = torch.cuda.Stream(device=eng.device)
            torch.cuda.synchronize()
            eng.bind_stream(st)
            try:
                with torch.cuda.stream(st):
                    loss = plan.step(roots, c, rn).clone()
                    got = [plan.grads(l)[0] for l in range(2)]
                eng.synchronize()
            finally:
                eng.bind_stream(torch.cuda.current_stream(eng.device))
            plan.close()
            assert np.isfinite(float(loss[0])) and float(loss[1]) == 1.0
            for l in range(2):
                err = float((got[l] - want[l]).abs().max()) / float(want[l].abs().max())
                print(f"{tag}: layer {l} gradient error {err:.2e} of the largest element")
                assert err <= 1e-4, (tag, l, err)
            grads[tag] = got
        diff = float((grads["live"][0] - grads["masked"][0]).abs().max()) / float(grads["live"][0].abs().max())
        print(f"first-layer gradient, live against masked: {diff:.2e} of the largest element")
        assert diff > 1e-2
    finally:
        eng.close()
