"""The link-prediction training step of an edge-featured GAT as one library call (engine.GatEdgeNablpTrainPlan,
gigl_gat_nablp_train_plan_set_edge_features): GATConv(edge_dim) and EdgeAttrGATConv (shared / separate message weight)
over the resident edge table read in place — against the CPU restatement (oracle sample -> union -> gnn_ref.gat_conv over
the whole union -> normalise -> retrieval loss -> torch autograd -> torch.optim.Adam) and against the autograd step over
the same batches.  Graph and tables: the recipe of tests/test_gpu_gat_edge_plan.py (RMAT with added self loops, a shuffled
COO edge table)."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from helpers import assert_adam_state, torch_adam_moments
from oracle import gnn_ref
from test_gpu_gat_edge_plan import _csc_positions, _engine, _graph
from test_gpu_train_plan import _lp_loss_torch

pytestmark = pytest.mark.gpu
FAN, TEMP, P = [10, 5], 0.07, 1
EDGE_NAMES = ("lin_edge.weight", "att_edge", "lin_edge_message.weight")


def _batches(eng, n, rowptr, b, n_rn, steps, seed):
    """as test_gpu_train_plan._lp_batches (anchor-major main roots, positives per anchor, random-negative roots), with the
    self-loop nodes of lowest in-degree (the graph's nodes 0..99 carry one) among every batch's anchors and negatives, so
    that every batch union holds a self edge: the removal / mean-attribute path of both layers"""
    rng = np.random.default_rng(seed)
    loops = np.argsort(np.diff(rowptr)[:100], kind="stable")[:8]
    out = []
    for _ in range(steps):
        perm = rng.permutation(n)
        perm = perm[~np.isin(perm, loops)]
        a_ids = np.concatenate([loops[:4], perm[:b - 4]])
        r_ids = np.concatenate([loops[4:], perm[b:b + n_rn - 4]])
        anchors = torch.from_numpy(a_ids.astype(np.uint32).view(np.int32)).to(eng.device)
        pos, cnt = eng.sample_positives(anchors, P, sampling_seed=42)
        ar = torch.arange(P, device=eng.device).view(1, P)
        a2 = anchors.view(-1, 1)
        grouped = torch.where(ar < cnt.view(-1, 1), pos.view(-1, P), a2.expand(-1, P))
        roots = torch.cat([a2, grouped], dim=1).reshape(-1).contiguous()
        rn = torch.from_numpy(r_ids.astype(np.uint32).view(np.int32)).to(eng.device)
        out.append((roots, cnt.to(torch.int32).contiguous(), rn))
    return out


def _setup(d, dtype, de):
    n, rowptr, col = _graph()
    eng, x, efeat = _engine(n, rowptr, col, d, dtype, de)
    dst = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rowptr).astype(np.int64))
    eng.build_from_coo(n, dst, col.astype(np.uint32), is_directed=True, out_graph=True)  # (the positives' out-graph)
    return eng, n, rowptr, col, x, efeat


def _model(d, hid, out, heads, de, conv, share, seed):
    from gigl_amd.models_attn import GAT
    torch.manual_seed(seed)
    model = GAT(d, hid, out, num_layers=2, heads=heads, edge_dim=de, conv=conv, share_edge_att_message_weight=share,
                should_l2_normalize_embedding_layer_output=True)
    with torch.no_grad():
        for c in model.conv_layers:
            c.bias.normal_(0, 0.1)
    return model


def _restatement(params, opt, conv, share, heads, rowptr, col, x, efeat, batches, dtype=torch.float32):
    """the step on the CPU, per batch: oracle.sample_khop(canonical) -> oracle.union_build -> gnn_ref.gat_conv over the
    WHOLE union for both layers (the edge rows looked up as test_gpu_gat_edge_plan._oracle_rows does) -> normalise ->
    _lp_loss_torch -> autograd -> Adam.  -> (losses, self edges per batch union, the first step's gradients by name)"""
    losses, self_edges, first = [], [], None
    for roots, cnt, rn in batches:
        embs = []
        for r in (roots, rn):
            r_h = r.cpu().numpy().view(np.uint32)
            nbr, _ = oracle.sample_khop(rowptr, col, r_h, FAN, canonical=True)
            u = oracle.union_build(r_h, FAN, nbr)
            ei = gnn_ref.union_edge_index(u["rowptr"], u["col"])
            nodes = np.asarray(u["nodes"]).astype(np.int64)
            pos = _csc_positions(rowptr, col, nodes[ei[0].numpy()], nodes[ei[1].numpy()])
            assert (pos >= 0).all()
            ea = torch.from_numpy(efeat[pos]).to(dtype)
            self_edges.append(int((ei[0] == ei[1]).sum()))
            h = torch.from_numpy(x[nodes].astype(np.float32)).to(dtype)
            for l, hd in enumerate((heads, 1)):
                p = f"conv_layers.{l}."
                w_msg = None
                if conv == "edge_attr_gat":
                    w_msg = params[p + "lin_edge.weight"] if share else params[p + "lin_edge_message.weight"]
                h = gnn_ref.gat_conv(h, ei, params[p + "lin.weight"], params[p + "att_src"], params[p + "att_dst"],
                                     params[p + "bias"], hd, edge_attr=ea, w_edge=params[p + "lin_edge.weight"],
                                     att_edge=params[p + "att_edge"], w_edge_msg=w_msg)
                if l == 0:
                    h = torch.relu(h)
            h = torch.nn.functional.normalize(h, p=2, dim=1)
            embs.append(h[torch.from_numpy(u["root_local"].astype(np.int64))])
        loss = _lp_loss_torch(embs[0], embs[1], roots.cpu(), cnt.cpu(), rn.cpu(), cnt.numel(), P, TEMP)
        opt.zero_grad()
        loss.backward()
        if first is None:
            first = {k: v.grad.detach().clone() for k, v in params.items()}
        opt.step()
        losses.append(float(loss))
    return losses, self_edges, first


def _plan_grads_by_name(plan):
    out = {}
    for l in range(2):
        for name, t in zip(("lin.weight", "att_src", "att_dst", "bias") + EDGE_NAMES, plan.grads(l)):
            if t is not None:
                out[f"conv_layers.{l}.{name}"] = t
    return out


@pytest.mark.parametrize("conv,share,heads,d,dtype,hid,out,de,prefetch", [
    ("gat", True, 2, 100, np.float16, 16, 32, 16, False),
    ("edge_attr_gat", True, 4, 100, np.float32, 8, 24, 3, True),
    ("edge_attr_gat", False, 1, 260, np.float32, 32, 16, 64, False),
    ("edge_attr_gat", False, 2, 320, np.float16, 16, 40, 16, True),
    ("gat", True, 4, 100, np.float32, 8, 16, 64, True),
    ("edge_attr_gat", True, 1, 100, np.float16, 16, 32, 3, False)])
def test_edge_plan_step_against_the_cpu_restatement(conv, share, heads, d, dtype, hid, out, de, prefetch):
    """four steps, the last batch short (fewer anchors and negatives than the plan's capacity: padded and masked), through
    step and through step2 with the next batch prefetched.  The bars are the edge-free GAT plan's
    (test_library_gat_link_prediction_step_against_the_cpu_restatement): losses rtol 1e-4 / atol 1e-5, Adam's moments 1e-3
    and the determined parameters 1e-4 over EVERY tensor, lin_edge.weight / att_edge / lin_edge_message.weight included.
    A shared message weight (lin_edge.weight used twice) is ONE tensor: its displacement equals the restatement's, not
    twice it."""
    from gigl_amd.engine import GatEdgeNablpTrainPlan
    eng, n, rowptr, col, x, efeat = _setup(d, dtype, de)
    try:
        b, n_rn, steps = 48, 32, 4
        batches = _batches(eng, n, rowptr, b, n_rn, steps, seed=13 + de)
        batches[-1] = (batches[-1][0][: 2 * 30].contiguous(), batches[-1][1][:30].contiguous(), batches[-1][2][:20].contiguous())
        model = _model(d, hid, out, heads, de, conv, share, seed=8 + heads)
        start = {k: v.detach().clone() for k, v in model.state_dict().items()}
        params = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
        opt = torch.optim.Adam(list(params.values()), lr=5e-3, weight_decay=1e-6, foreach=False)
        want, self_edges, first = _restatement(params, opt, conv, share, heads, rowptr, col, x, efeat, batches)
        assert min(self_edges) >= 1, self_edges  # every batch union exercises the self-loop removal / mean attribute
        for k, g in first.items():  # (checked on the CPU: the restatement is differentiable in every edge tensor)
            assert torch.isfinite(g).all() and float(g.abs().max()) > 0, k
        lib = _model(d, hid, out, heads, de, conv, share, seed=8 + heads).to(eng.device)
        lib.load_state_dict(start)
        st = torch.cuda.Stream(device=eng.device)
        torch.cuda.synchronize()
        eng.bind_stream(st)
        plan = GatEdgeNablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, lr=5e-3, weight_decay=1e-6)
        got = []
        with torch.cuda.stream(st):
            for i, bt in enumerate(batches):
                nxt = (batches[i + 1][0], batches[i + 1][2]) if prefetch and i + 1 < steps else None
                got.append(plan.step(*bt, next_roots=nxt).clone())
                if i == 0:
                    grads, again = _plan_grads_by_name(plan), _plan_grads_by_name(plan)
        eng.synchronize()
        got = [float(v[0]) for v in got]
        plan.store(lib)
        moments = plan.moments()
        plan.close()
        eng.bind_stream(torch.cuda.current_stream(eng.device))
        print(f"{conv} share={share} H={heads} De={de}: losses", got, "vs", want, "| self edges", self_edges)
        assert np.isfinite(got).all()  # (no step overflowed: an overflowing batch reports NaN and trains nothing)
        assert set(grads) == set(first)
        errs = {}
        for k in first:
            assert torch.equal(grads[k], again[k]), k  # (asking twice adds nothing twice)
            gk = grads[k].cpu().reshape(-1)
            assert torch.isfinite(gk).all() and float(gk.abs().max()) > 0, k
            errs[k] = float((gk - first[k].reshape(-1)).abs().max()) / (float(first[k].abs().max()) + 1e-12)
        print("first-step gradients vs the restatement (max |err| / max |grad|):", {k: f"{v:.2e}" for k, v in errs.items()})
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)
        flat = lambda sd: {k: v.reshape(-1) for k, v in sd.items()}
        assert_adam_state("edge GAT link-prediction plan vs the CPU restatement", flat(lib.state_dict()), moments, flat(params),
                          {k: (m.reshape(-1), v.reshape(-1)) for k, (m, v) in torch_adam_moments(opt, params).items()},
                          tol_m=1e-3, tol_v=1e-3, tol_p=1e-4)
        assert all(f"conv_layers.{l}.{nm}" in moments for l in range(2) for nm in EDGE_NAMES[:2])
        assert (f"conv_layers.0.{EDGE_NAMES[2]}" in moments) == (conv == "edge_attr_gat" and not share)
        if conv == "edge_attr_gat" and share:  # one update per step: the displacement is the restatement's, not twice it
            for l in range(2):
                k = f"conv_layers.{l}.lin_edge.weight"
                moved = float((lib.state_dict()[k].cpu() - start[k]).norm())
                moved_ref = float((params[k].detach() - start[k]).norm())
                print(f"{k}: moved {moved:.6f}, the restatement {moved_ref:.6f}")
                assert moved_ref > 0 and abs(moved / moved_ref - 1.0) < 0.01
    finally:
        eng.close()


EDGE_STEP_CASES = [("gat", True, 4, 100, np.float32, 8, 32, 3), ("edge_attr_gat", True, 2, 768, np.float16, 128, 256, 16),
                   ("edge_attr_gat", False, 1, 320, np.float32, 256, 256, 64)]


@pytest.mark.parametrize("conv,share,heads,d,dtype,hid,out,de", EDGE_STEP_CASES)
def test_edge_plan_unforked_step_equals_the_autograd_step(monkeypatch, conv, share, heads, d, dtype, hid, out, de):
    """the same step, same body and bars, with GIGL_LP_FORK=0 (read at every create): both encodes one after the other on
    the caller's stream, d v and the message weights' gradients accumulated in one place"""
    monkeypatch.setenv("GIGL_LP_FORK", "0")
    test_edge_plan_step_equals_the_autograd_step(conv, share, heads, d, dtype, hid, out, de)


@pytest.mark.parametrize("conv,share,heads,d,dtype,hid,out,de", EDGE_STEP_CASES)
def test_edge_plan_step_equals_the_autograd_step(conv, share, heads, d, dtype, hid, out, de):
    """against the autograd step over the same batches (hbm.ResidentGraph.train_graph with train_as_graph_data ->
    GAT._forward_graph: dense per-batch attributes, every source row projected): all first-step gradients, the three edge
    tensors per layer included, max |err| / max |grad| < 2e-4 — the edge-free GAT plan test's bar — then the loss history
    with prefetch.  (EdgeAttrGATConv's autograd backward is built for layer widths that are multiples of 256: those cases
    run 2 x 128 / 256 and 256 / 256 channels.)"""
    from gigl_amd.engine import GatEdgeNablpTrainPlan
    from gigl_amd.hbm import ResidentGraph
    eng, n, rowptr, col, x, efeat = _setup(d, dtype, de)
    try:
        b, n_rn, steps = 96, 40, 4
        batches = _batches(eng, n, rowptr, b, n_rn, steps, seed=9)
        ref = _model(d, hid, out, heads, de, conv, share, seed=6).to(eng.device)
        lib = _model(d, hid, out, heads, de, conv, share, seed=6).to(eng.device)
        lib.load_state_dict(ref.state_dict())
        ref.train()
        ref.engine = eng
        res = ResidentGraph.from_engine(eng, np.arange(n, dtype=np.int64), FAN)
        res.train_as_graph_data, res.defer_x = True, True
        opt = torch.optim.Adam(ref.parameters(), lr=5e-3, weight_decay=1e-6, foreach=False)
        want, first = [], None
        for roots, cnt, rn in batches:
            embs = []
            for r in (roots, rn):
                g, ri = res.train_graph(r)
                assert g.edge_attr is not None
                embs.append(ref(g)[ri])
            loss = _lp_loss_torch(embs[0], embs[1], roots, cnt, rn, b, P, TEMP)
            opt.zero_grad()
            loss.backward()
            if first is None:
                first = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
            opt.step()
            want.append(float(loss))
        st = torch.cuda.Stream(device=eng.device)
        torch.cuda.synchronize()
        eng.bind_stream(st)
        plan = GatEdgeNablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, remove_accidental_hits=True, lr=5e-3,
                                     weight_decay=1e-6)
        got = []
        with torch.cuda.stream(st):
            for i, (roots, cnt, rn) in enumerate(batches):
                nxt = (batches[i + 1][0], batches[i + 1][2]) if i + 1 < steps and i != 2 else None
                got.append(plan.step(roots, cnt, rn, next_roots=nxt).clone())
                if i == 0:
                    grads, again = _plan_grads_by_name(plan), _plan_grads_by_name(plan)
        eng.synchronize()
        plan.close()
        eng.bind_stream(torch.cuda.current_stream(eng.device))
        got = [float(v[0]) for v in got]
        assert np.isfinite(got).all() and set(grads) == set(first)
        errs = {}
        for k, w_ in first.items():
            assert torch.equal(grads[k], again[k]), k
            assert float(grads[k].abs().max()) > 0, k
            errs[k] = float((grads[k].reshape(-1) - w_.reshape(-1)).abs().max()) / (float(w_.abs().max()) + 1e-12)
        print("edge GAT plan vs autograd: first-step gradient errors (max |err| / max |grad|):",
              {k: f"{v:.2e}" for k, v in errs.items()}, "| losses", got, "vs", want)
        assert max(errs.values()) < 2e-4 and abs(got[0] - want[0]) < 1e-4 * abs(want[0]), (errs, got[0], want[0])
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)
    finally:
        eng.close()


def test_edge_plan_survives_growing_onto_wide_workspaces():
    """grow() re-creates the plan — the setter runs again on the new handle — and adopts the moments, the edge tensors'
    included: the steps after it continue the run of a plan that never grew"""
    from gigl_amd.engine import GatEdgeNablpTrainPlan
    eng, n, rowptr, col, x, efeat = _setup(100, np.float32, 6)
    try:
        b, n_rn, steps = 48, 32, 4
        batches = _batches(eng, n, rowptr, b, n_rn, steps, seed=3)
        runs = []
        for grow_after in (None, 1):
            lib = _model(100, 16, 32, 2, 6, "edge_attr_gat", False, seed=4).to(eng.device)
            plan = GatEdgeNablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, lr=5e-3, weight_decay=1e-6)
            losses = []
            for i, bt in enumerate(batches):
                losses.append(float(plan.step(*bt)[0]))
                if grow_after is not None and i == grow_after:
                    plan.grow()
                    assert plan.wide
            moments = plan.moments()
            plan.store(lib)
            plan.close()
            runs.append((losses, moments, {k: v.clone() for k, v in lib.state_dict().items()}))
        (l0, m0, p0), (l1, m1, p1) = runs
        assert np.isfinite(l0).all()
        np.testing.assert_allclose(l1, l0, rtol=1e-4, atol=1e-5)  # (the wide workspaces number the union's nodes differently)
        for k in m0:
            for a, c in zip(m0[k], m1[k]):
                assert float((a - c).abs().max()) <= 1e-3 * float(a.abs().max()), k
        assert any("lin_edge_message.weight" in k for k in m0)
    finally:
        eng.close()


def test_edge_plan_error_behaviour():
    """the setter after a step, on a GraphSAGE plan, with a 65-wide or an fp16 edge table; a model with edge_dim on an engine
    without a table"""
    from gigl_amd import _lib
    from gigl_amd._lib import GiglError
    from gigl_amd.engine import GatEdgeNablpTrainPlan, GatNablpTrainPlan, HipEngine, NablpTrainPlan
    from gigl_amd.models import GraphSAGE
    from gigl_amd.models_attn import GAT
    eng, n, rowptr, col, x, efeat = _setup(100, np.float32, 6)
    try:
        b, n_rn = 48, 32
        batches = _batches(eng, n, rowptr, b, n_rn, 1, seed=3)
        lib = _model(100, 16, 32, 2, 6, "gat", True, seed=4).to(eng.device)
        plan = GatEdgeNablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP)
        arr = lambda ts: (C.c_void_p * 2)(*[(t.data_ptr() if t is not None else None) for t in ts])
        setter = eng._lib.gigl_gat_nablp_train_plan_set_edge_features
        args = (eng._efeat_handle, arr(plan.w_edge), arr(plan.att_edge), arr(plan.w_edge_msg))
        assert setter(plan._plan, *args) == -1  # (set once: the constructor did)
        assert np.isfinite(float(plan.step(*batches[0])[0]))
        eng.synchronize()
        assert setter(plan._plan, *args) == -1  # GIGL_E_INVALID_ARG after the first step
        plan.close()
        # the edge-free GAT plan takes the setter before its first step, not after; a GraphSAGE plan never does
        sage = NablpTrainPlan(eng, GraphSAGE(100, 16, 8, num_layers=2).to(eng.device), b, P, n_rn, FAN)
        assert setter(sage._plan, *args) == -1
        sage.close()
        # an fp16 edge table / a 65-wide one: GIGL_E_UNSUPPORTED out of the constructor
        good = eng._efeat_handle
        half = torch.zeros((len(col), 6), dtype=torch.float16, device=eng.device)
        h16 = C.c_void_p()
        _lib.check(eng._lib.gigl_features_load(eng._ctx, half.shape[0], half.shape[1], _lib.DTYPE_F16, C.c_void_p(half.data_ptr()),
                                               _lib.LOC_DEVICE, C.byref(h16)), eng._ctx)
        eng._efeat_handle = h16
        try:
            with pytest.raises(GiglError) as e:
                GatEdgeNablpTrainPlan(eng, lib, b, P, n_rn, FAN)
            assert e.value.code == -4
        finally:
            eng._efeat_handle = good
            eng._lib.gigl_features_destroy(h16)
        eng._set_edge_table(torch.zeros((len(col), 65), dtype=torch.float32, device=eng.device))
        wide = GAT(100, 16, 32, num_layers=2, heads=2, edge_dim=65).to(eng.device)
        with pytest.raises(NotImplementedError):  # (the predicate refuses it before the library is asked)
            GatEdgeNablpTrainPlan(eng, wide, b, P, n_rn, FAN)
        h = C.c_void_p()
        edge_free = GAT(100, 16, 32, num_layers=2, heads=2).to(eng.device)
        bare = GatNablpTrainPlan(eng, edge_free, b, P, n_rn, FAN)
        w65 = [torch.zeros((32, 65), device=eng.device), torch.zeros((32, 65), device=eng.device)]
        a65 = [torch.zeros(32, device=eng.device), torch.zeros(32, device=eng.device)]
        assert setter(bare._plan, eng._efeat_handle, arr(w65), arr(a65), None) == -4  # GIGL_E_UNSUPPORTED: De = 65
        bare.close()
    finally:
        eng.close()
    # a model with edge_dim on an engine without an edge table raises (no fallback)
    n, rowptr, col = _graph()
    eng = HipEngine(0)
    try:
        eng.load_csc(rowptr, col)
        eng.load_features(np.zeros((n, 100), np.float32))
        model = GAT(100, 16, 32, num_layers=2, heads=2, edge_dim=6).to(eng.device)
        with pytest.raises(RuntimeError, match="edge table"):
            GatEdgeNablpTrainPlan(eng, model, 48, P, 32, FAN)
    finally:
        eng.close()
