"""Gradient-norm clipping and the ConstantLR warm-up inside the link-prediction training plans
(gigl_nablp_train_plan_set_clip_grad_norm / _set_constant_lr / _grad_norm; engine.NablpTrainPlan, GatNablpTrainPlan,
GatEdgeNablpTrainPlan with clip_grad_norm / lr_factor / lr_total_iters): what the reference's loop does between backward
and the scheduler's step (node_anchor_based_link_prediction_modeling_task_spec.py:401-406) — clip_grad_norm_ over all
parameters, optimizer.step, lr_scheduler.step — against the plan's own unclipped gradients, against the autograd loop
with torch's clip_grad_norm_ / ConstantLR, and against plans without the knobs.  Graph and batches: the recipe of
tests/test_gpu_train_plan.py (RMAT scale 13, 100-wide rows)."""
import math

import numpy as np
import pytest
import torch

import oracle
from helpers import adam_state_errors, assert_adam_state, rmat_edges, torch_adam_moments

pytestmark = pytest.mark.gpu
FAN, TEMP, LR, WD = [10, 5], 0.07, 5e-3, 1e-6
BETA1, BETA2 = np.float32(0.9), np.float32(0.999)
SAGE_SHAPE = ((100, 32, 16), 128, 1, 64)  # dims, b, P, random negatives: test_gpu_train_plan's smallest normalised case


@pytest.fixture(scope="module")
def setup():
    from gigl_amd.engine import HipEngine
    s, d = rmat_edges(13, 150000, seed=8)
    n = 1 << 13
    rowptr, col = oracle.build_csc(n, s, d, is_directed=False)
    x = (np.random.default_rng(0).standard_normal((n, 100)) / 4).astype(np.float32)
    eng = HipEngine(0)
    eng.load_csc(rowptr, col)
    eng.load_features(x)
    dst = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rowptr).astype(np.int64))
    eng.build_from_coo(n, dst, col.astype(np.uint32), is_directed=True, out_graph=True)  # (out-edges = reversed in-edges)
    yield eng, rowptr, col, x, n
    eng.close()


def _lp_batches(eng, n, b, P, n_rn, steps, seed):
    """as tests/test_gpu_train_plan._lp_batches: main roots (anchor-major: anchor + its P positive slots, a missing positive
    repeats the anchor), positives per anchor and random-negative roots of `steps` batches"""
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


def _lp_loss_torch(emb_main, emb_rn, roots, cnt, rn, b, P, temperature):
    """as tests/test_gpu_train_plan._lp_loss_torch: infer_task_inputs + Retrieval on embeddings, in torch"""
    T = 1 + P
    ids = (roots.to(torch.int64) & 0xFFFFFFFF).view(b, T)
    k = cnt.to(torch.int64)
    slot = torch.arange(P, device=roots.device).view(1, P)
    ok = (slot < k.view(-1, 1)).reshape(-1)
    q_rows = (torch.arange(b, device=roots.device) * T).repeat_interleave(P)[ok]
    p_rows = (torch.arange(b, device=roots.device).view(-1, 1) * T + 1 + slot).reshape(-1)[ok]
    rq, pos = emb_main[q_rows], emb_main[p_rows]
    cand = torch.cat([pos, emb_rn])
    scores = rq @ cand.T / temperature
    qid = ids[:, 0].repeat_interleave(P)[ok]
    cid = torch.cat([ids.reshape(-1)[p_rows], rn.to(torch.int64) & 0xFFFFFFFF])
    Q, Cn = scores.shape
    eye = torch.zeros((Q, Cn), dtype=torch.bool, device=scores.device)
    eye[torch.arange(Q), torch.arange(Q)] = True
    same_q = torch.zeros_like(eye)
    same_q[:, :Q] = qid.view(-1, 1) == qid.view(1, -1)
    hit = cid.view(1, -1) == cid[:Q].view(-1, 1)
    masked = scores.masked_fill((same_q | hit) & ~eye, torch.finfo(torch.float32).min)
    return torch.nn.functional.cross_entropy(masked, torch.arange(Q, device=scores.device), reduction="sum") / max(Q, 1)


# ---- running plans

def _run(eng, plan, batches, prefetch=False, after_step=None):
    """the batches through plan.step on a stream of their own (the first call runs eagerly, the second is captured, later ones
    replay); prefetch: most steps announce the next batch, some do not, step 4 announces the wrong one.  -> losses"""
    st = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    got = []
    try:
        with torch.cuda.stream(st):
            for i, (roots, cnt, rn) in enumerate(batches):
                nxt = None
                if prefetch and i + 1 < len(batches) and i % 4 != 2:
                    j = i + 1 if i != 4 else 0
                    nxt = (batches[j][0], batches[j][2])
                got.append(plan.step(roots, cnt, rn, next_roots=nxt).clone())
                if after_step is not None:
                    after_step(i)
        eng.synchronize()
    finally:
        eng.bind_stream(torch.cuda.current_stream(eng.device))
    return [float(v[0]) for v in got]


def _sage_grads_by_name(plan):
    out = {}
    for l in range(len(plan.w)):
        gw, gb = plan.grads(l)
        d = int(gw.shape[1]) // 2
        out[f"conv_layers.{l}.lin_l.weight"], out[f"conv_layers.{l}.lin_r.weight"] = gw[:, :d], gw[:, d:]
        if gb is not None:
            out[f"conv_layers.{l}.lin_l.bias"] = gb
    return out


def _gat_grads_by_name(plan):
    out = {}
    for l in range(2):
        for name, t in zip(("lin.weight", "att_src", "att_dst", "bias"), plan.grads(l)):
            if t is not None:
                out[f"conv_layers.{l}.{name}"] = t
    return out


def _host_norm(grads):
    """sqrt(sum g^2) over every tensor, fp64 on the host"""
    return math.sqrt(sum(float((g.detach().cpu().double() ** 2).sum()) for g in grads.values()))


def _snap(eng, plan):
    """the GraphSAGE plan's trained state, cloned and keyed like the model's state dict: (parameters, Adam's moments)"""
    eng.synchronize()
    params = {}
    for l, (w, b) in enumerate(zip(plan.w, plan.bias)):
        d = int(w.shape[1]) // 2
        params[f"conv_layers.{l}.lin_l.weight"], params[f"conv_layers.{l}.lin_r.weight"] = w[:, :d].clone(), w[:, d:].clone()
        if b is not None:
            params[f"conv_layers.{l}.lin_l.bias"] = b.clone()
    return params, {k: (m.clone(), v.clone()) for k, (m, v) in plan.moments().items()}


def _identical(a, b):
    """two _snap()s hold the same bits: every parameter, every moment"""
    return all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and \
        all(torch.equal(x, y) for k in a[1] for x, y in zip(a[1][k], b[1][k]))


def _run_diff(losses_a, snaps_a, losses_b, snaps_b):
    """ONE figure for how far two runs are apart, in relative units: the largest of the steps' |loss difference| / loss and of
    their states' differences as the project compares trained states (helpers.adam_state_errors: Adam's moments on every
    element and the parameters on the determined set, each over the tensor's largest value — the raw parameter of an element
    whose gradient is rounding noise moves by up to lr per step in either direction and says nothing)"""
    fig = max(abs(x - y) / abs(x) for x, y in zip(losses_a, losses_b))
    for a, b in zip(snaps_a, snaps_b):
        for k, (em, ev, ep, _) in adam_state_errors(b[0], b[1], a[0], a[1]).items():
            fig = max(fig, em, ev, ep / (float(a[0][k].abs().max()) + 1e-30))
    return fig


# ---- 1, 2: norm, coefficient and the clipped first step against the plan's own unclipped gradients

def _check_first_clipped_step(tag, eng, make_plan, grads_by_name, start, batch, wd):
    """an unclipped first step measures the norm; a plan clipping at HALF of it then reports that norm and coef ~ 0.5
    (1e-6 relative: fp32 gradients, fp64 accumulation), and — the moments start from zero — leaves exp_avg = (1 - beta1)
    (coef g + wd w0), exp_avg_sq = (1 - beta2) (...)^2 of the host's fp32 evaluation (2e-6 of each tensor's largest value)"""
    plan = make_plan(0.0)
    _run(eng, plan, [batch])
    norm0 = _host_norm(grads_by_name(plan))
    plan.close()
    assert norm0 > 0
    max_norm = 0.5 * norm0
    plan = make_plan(max_norm)
    _run(eng, plan, [batch])
    grads = grads_by_name(plan)
    got_norm, got_coef = plan.grad_norm()
    moments = plan.moments()
    plan.close()
    assert set(grads) == set(moments), (sorted(grads), sorted(moments))  # every trained tensor, once
    norm = _host_norm(grads)
    coef = min(1.0, max_norm / (norm + 1e-6))
    print(f"{tag}: total_norm {got_norm!r} vs the host's {norm!r}, coef {got_coef!r} vs {coef!r}")
    assert coef < 0.9
    assert abs(got_norm - norm) <= 1e-6 * norm and abs(got_coef - coef) <= 1e-6 * coef, (got_norm, norm, got_coef, coef)
    worst = (0.0, 0.0)
    for k, g in grads.items():
        g32 = g.detach().cpu().numpy().reshape(-1).astype(np.float32)
        w0 = start[k].detach().cpu().numpy().reshape(-1).astype(np.float32)
        gr = np.float32(coef) * g32 + np.float32(wd) * w0
        want_m = (np.float32(1) - BETA1) * gr
        want_v = (np.float32(1) - BETA2) * gr * gr
        m, v = (t.detach().cpu().numpy().reshape(-1) for t in moments[k])
        em = float(np.abs(m - want_m).max()) / float(np.abs(want_m).max())
        ev = float(np.abs(v - want_v).max()) / float(np.abs(want_v).max())
        worst = (max(worst[0], em), max(worst[1], ev))
        assert em <= 2e-6 and ev <= 2e-6, (tag, k, em, ev)
    print(f"{tag}: first clipped step, exp_avg {worst[0]:.2e} exp_avg_sq {worst[1]:.2e} of the tensors' largest")


def test_norm_and_coefficient_of_the_sage_plan(setup):
    """(weight decay 1e-2, not the trainer's 1e-6: clipping AFTER the decay had joined would move exp_avg by (1 - coef) wd w,
    which only a decay of this size lifts above the 2e-6 bar)"""
    from gigl_amd.engine import NablpTrainPlan
    from gigl_amd.models import GraphSAGE
    eng, rowptr, col, x, n = setup
    b, P, n_rn, wd = 48, 1, 32, 1e-2
    batch = _lp_batches(eng, n, b, P, n_rn, 1, seed=21)[0]
    torch.manual_seed(4)
    lib = GraphSAGE(100, 32, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)
    start = {k: v.detach().clone() for k, v in lib.state_dict().items()}
    make = lambda c: NablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, lr=LR, weight_decay=wd, clip_grad_norm=c)
    _check_first_clipped_step("GraphSAGE plan", eng, make, _sage_grads_by_name, start, batch, wd)


def test_norm_and_coefficient_of_the_gat_plan(setup):
    """two heads: W0 / b0 enter Adam as a slice per head (a slice counted twice would raise the norm), the second layer's
    attention vectors and bias have a second source from the forked encode (left out, it would lower it)"""
    from gigl_amd.engine import GatNablpTrainPlan, HipEngine
    from gigl_amd.models_attn import GAT
    _, rowptr, col, x, n = setup
    eng = HipEngine(0)
    try:
        eng.load_csc(rowptr, col)
        eng.load_features(x)
        dst = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rowptr).astype(np.int64))
        eng.build_from_coo(n, dst, col.astype(np.uint32), is_directed=True, out_graph=True)
        b, P, n_rn, wd = 48, 1, 32, 1e-2
        batch = _lp_batches(eng, n, b, P, n_rn, 1, seed=13)[0]
        torch.manual_seed(8)
        lib = GAT(100, 16, 32, num_layers=2, heads=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)
        with torch.no_grad():
            for c in lib.conv_layers:
                c.bias.normal_(0, 0.1)
        start = {k: v.detach().clone() for k, v in lib.state_dict().items()}
        make = lambda c: GatNablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, lr=LR, weight_decay=wd, clip_grad_norm=c)
        _check_first_clipped_step("GAT plan", eng, make, _gat_grads_by_name, start, batch, wd)
    finally:
        eng.close()


def test_norm_and_coefficient_of_the_edge_featured_gat_plan():
    """EdgeAttrGATConv with the SHARED message weight (lin_edge.weight used twice: one tensor to torch, one Adam entry, one
    share of the norm), the smallest shape of tests/test_gpu_gat_edge_train_plan.py; grads() covers the edge tensors"""
    from gigl_amd.engine import GatEdgeNablpTrainPlan
    from test_gpu_gat_edge_train_plan import _batches, _model, _plan_grads_by_name, _setup
    heads, d, dtype, hid, out, de = 1, 100, np.float16, 16, 32, 3
    eng, n, rowptr, col, x, efeat = _setup(d, dtype, de)
    try:
        b, n_rn, wd = 48, 32, 1e-2
        batch = _batches(eng, n, rowptr, b, n_rn, 1, seed=13 + de)[0]
        lib = _model(d, hid, out, heads, de, "edge_attr_gat", True, seed=8 + heads).to(eng.device)
        start = {k: v.detach().clone() for k, v in lib.state_dict().items()}
        make = lambda c: GatEdgeNablpTrainPlan(eng, lib, b, 1, n_rn, FAN, temperature=TEMP, lr=LR, weight_decay=wd, clip_grad_norm=c)
        _check_first_clipped_step("edge-featured GAT plan", eng, make, _plan_grads_by_name, start, batch, wd)
    finally:
        eng.close()


# ---- 3: a clipped run against autograd with torch's clip_grad_norm_

def _autograd_run(params, embed, batches, b, P, max_norm=None, sched=None, lr=LR):
    """the autograd loop of tests/test_gpu_train_plan.py with clip_grad_norm_ before opt.step() (max_norm None: the norm is
    only measured) and, sched = (factor, total_iters), ConstantLR stepped after it.  embed(roots) -> the roots' embeddings.
    -> (losses, the norm of every step, the optimiser)"""
    params = list(params)
    opt = torch.optim.Adam(params, lr=lr, weight_decay=WD, foreach=False)
    scheduler = torch.optim.lr_scheduler.ConstantLR(opt, factor=sched[0], total_iters=sched[1]) if sched else None
    losses, norms = [], []
    for roots, cnt, rn in batches:
        loss = _lp_loss_torch(embed(roots), embed(rn), roots, cnt, rn, b, P, TEMP)
        opt.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm if max_norm is not None else float("inf"),
                                                          foreach=False)))
        opt.step()
        if scheduler is not None:
            scheduler.step()
        losses.append(float(loss.detach()))
    return losses, norms, opt


def _sage_embed(eng, model):
    from gigl_amd.models import HipBatch

    def embed(r):
        tree = eng.sample_khop(r, FAN)
        u = eng.union_build(tree)
        return model(HipBatch(eng, tree, u, train=True))[u.root_local[: r.numel()].long()]
    return embed


def _sage_models(eng, dims, seed=4):
    from gigl_amd.models import GraphSAGE
    torch.manual_seed(seed)
    mk = lambda: GraphSAGE(dims[0], dims[1], dims[2], num_layers=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)
    first = mk()
    out = [first]
    for _ in range(2):
        m = mk()
        m.load_state_dict(first.state_dict())
        out.append(m)
    return out


def test_clipped_sage_run_equals_autograd_with_clip_grad_norm(setup):
    """8 steps, prefetch on some, clipping active at every one; the bounds are those of the unclipped comparison of this shape
    (test_library_link_prediction_step_equals_the_autograd_step, normalised: losses rtol 2e-5 / atol 2e-6, moments and
    determined parameters 1e-4); the last step's norm and coef agree to the moments' bound"""
    from gigl_amd.engine import NablpTrainPlan
    eng, rowptr, col, x, n = setup
    dims, b, P, n_rn = SAGE_SHAPE
    batches = _lp_batches(eng, n, b, P, n_rn, 8, seed=5)
    dry, ref, lib = _sage_models(eng, dims)
    dry.train()
    ref.train()
    _, dry_norms, _ = _autograd_run(dry.parameters(), _sage_embed(eng, dry), batches, b, P)
    max_norm = 0.25 * min(dry_norms)
    want, norms, opt = _autograd_run(ref.parameters(), _sage_embed(eng, ref), batches, b, P, max_norm=max_norm)
    assert min(norms) > max_norm, (norms, max_norm)  # clipping is active at every step
    plan = NablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, lr=LR, weight_decay=WD, clip_grad_norm=max_norm)
    got = _run(eng, plan, batches, prefetch=True)
    got_norm, got_coef = plan.grad_norm()
    plan.store(lib)
    moments = plan.moments()
    plan.close()
    want_coef = min(1.0, max_norm / (norms[-1] + 1e-6))
    print(f"clipped GraphSAGE run: max_norm {max_norm:.6f}, autograd norms {norms}, last norm {got_norm!r} coef {got_coef!r} "
          f"vs {norms[-1]!r} {want_coef!r}; loss errors {[abs(g - w) / abs(w) for g, w in zip(got, want)]}")
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)
    assert_adam_state("clipped link-prediction plan vs autograd", lib.state_dict(), moments, ref.state_dict(),
                      torch_adam_moments(opt, dict(ref.named_parameters())), tol_m=1e-4, tol_v=1e-4, tol_p=1e-4)
    assert abs(got_norm - norms[-1]) <= 1e-4 * norms[-1] and abs(got_coef - want_coef) <= 1e-4 * want_coef


def test_clipped_gat_run_equals_autograd_with_clip_grad_norm(setup):
    """the same for the heads = 2 GAT plan, against the autograd step of
    test_library_gat_link_prediction_step_equals_the_autograd_step and with its figures (normalised: losses rtol 1e-4 /
    atol 1e-5, moments 1e-3, determined parameters 1e-4)"""
    from gigl_amd.engine import GatNablpTrainPlan, HipEngine
    from gigl_amd.hbm import ResidentGraph
    from gigl_amd.models_attn import GAT
    _, rowptr, col, x, n = setup
    eng = HipEngine(0)
    try:
        eng.load_csc(rowptr, col)
        eng.load_features(x)
        dst = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rowptr).astype(np.int64))
        eng.build_from_coo(n, dst, col.astype(np.uint32), is_directed=True, out_graph=True)
        b, P, n_rn = 96, 1, 40
        batches = _lp_batches(eng, n, b, P, n_rn, 8, seed=9)
        torch.manual_seed(6)
        mk = lambda: GAT(100, 16, 32, num_layers=2, heads=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)
        dry, ref, lib = mk(), mk(), mk()
        ref.load_state_dict(dry.state_dict())
        lib.load_state_dict(dry.state_dict())
        res = ResidentGraph.from_engine(eng, np.arange(n, dtype=np.int64), FAN)
        res.train_as_graph_data, res.defer_x = True, True

        def embed_with(model):
            model.train()
            model.engine = eng

            def embed(r):
                g, ri = res.train_graph(r)
                return model(g)[ri]
            return embed
        _, dry_norms, _ = _autograd_run(dry.parameters(), embed_with(dry), batches, b, P)
        max_norm = 0.25 * min(dry_norms)
        want, norms, opt = _autograd_run(ref.parameters(), embed_with(ref), batches, b, P, max_norm=max_norm)
        assert min(norms) > max_norm, (norms, max_norm)
        plan = GatNablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, lr=LR, weight_decay=WD, clip_grad_norm=max_norm)
        got = _run(eng, plan, batches, prefetch=True)
        got_norm, got_coef = plan.grad_norm()
        plan.store(lib)
        moments = plan.moments()
        plan.close()
        want_coef = min(1.0, max_norm / (norms[-1] + 1e-6))
        print(f"clipped GAT run: max_norm {max_norm:.6f}, autograd norms {norms}, last norm {got_norm!r} coef {got_coef!r} vs "
              f"{norms[-1]!r} {want_coef!r}; loss errors {[abs(g - w) / abs(w) for g, w in zip(got, want)]}")
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)
        flat = lambda sd: {k: v.reshape(-1) for k, v in sd.items()}
        assert_adam_state("clipped GAT link-prediction plan vs autograd", flat(lib.state_dict()), moments, flat(ref.state_dict()),
                          {k: (m.reshape(-1), v.reshape(-1)) for k, (m, v) in
                           torch_adam_moments(opt, dict(ref.named_parameters())).items()}, tol_m=1e-3, tol_v=1e-3, tol_p=1e-4)
        assert abs(got_norm - norms[-1]) <= 1e-3 * norms[-1] and abs(got_coef - want_coef) <= 1e-3 * want_coef
    finally:
        eng.close()


# ---- 4, 5, 6: against plans without the knobs

@pytest.fixture(scope="module")
def plain_runs(setup):
    """the GraphSAGE plan WITHOUT clipping or schedule, twice over the same six batches from the same weights: its state after
    every step (the second run also asks for the gradients after every step, whose norms it returns) — the references of the
    tests below, and their own run-to-run repeatability"""
    from gigl_amd.engine import NablpTrainPlan
    eng, rowptr, col, x, n = setup
    dims, b, P, n_rn = SAGE_SHAPE
    batches = _lp_batches(eng, n, b, P, n_rn, 6, seed=5)
    models = _sage_models(eng, dims)
    runs, norms = [], []
    for k in range(2):
        plan = NablpTrainPlan(eng, models[0], b, P, n_rn, FAN, temperature=TEMP, lr=LR, weight_decay=WD)
        snaps = []

        def after(i):
            if k == 1:
                norms.append(_host_norm(_sage_grads_by_name(plan)))
            snaps.append(_snap(eng, plan))
        losses = _run(eng, plan, batches, after_step=after)
        plan.close()
        runs.append((losses, snaps))
    (l0, s0), (l1, s1) = runs
    identical = l0 == l1 and all(_identical(a, c) for a, c in zip(s0, s1))
    figs = [_run_diff(l0[:k], s0[:k], l1[:k], s1[:k]) for k in range(1, 7)]
    print(f"plain GraphSAGE plan, two runs: bit-identical {identical}; largest difference over the first k = 1..6 steps "
          f"{[f'{v:.3e}' for v in figs]}; gradient norms {norms}")
    return dict(batches=batches, model=models[0], losses=l0, snaps=s0, norms=norms, identical=identical, rep=figs)


def _assert_same_run(tag, plain, losses, snaps, upto):
    """steps < upto of a run equal the plain runs': bit for bit where those repeat bit for bit, else within four times the
    largest difference the two plain runs showed over the same steps (_run_diff's figure)"""
    same = losses[:upto] == plain["losses"][:upto] and all(_identical(a, c) for a, c in zip(plain["snaps"][:upto], snaps[:upto]))
    fig = _run_diff(plain["losses"][:upto], plain["snaps"][:upto], losses[:upto], snaps[:upto])
    print(f"{tag}: vs the plain plan over {upto} steps: bit-identical {same}, largest difference {fig:.3e} "
          f"(the plain runs' own: {plain['rep'][upto - 1]:.3e})")
    if plain["identical"]:
        assert same, (tag, fig)
    else:
        assert fig <= 4 * plain["rep"][upto - 1], (tag, fig, plain["rep"][upto - 1])


def _sage_plan_run(setup, plain, steps, lr=LR, **knobs):
    from gigl_amd.engine import NablpTrainPlan
    eng = setup[0]
    dims, b, P, n_rn = SAGE_SHAPE
    plan = NablpTrainPlan(eng, plain["model"], b, P, n_rn, FAN, temperature=TEMP, lr=lr, weight_decay=WD, **knobs)
    snaps, seen = [], []

    def after(i):
        if knobs.get("clip_grad_norm"):
            seen.append(plan.grad_norm())
        snaps.append(_snap(eng, plan))
    losses = _run(eng, plan, plain["batches"][:steps], after_step=after)
    plan.close()
    return losses, snaps, seen


def test_clipping_that_never_bites_changes_nothing(setup, plain_runs):
    """max_norm = 1e6 x the largest norm of the run: coef is 1.0 at every step and g * 1.0f is exact, so five steps leave the
    state of the plan that does not clip: bit for bit if the plain plan repeats itself bit for bit.  It does not — measured,
    two plain runs over these five steps end 2.4e-6 of a tensor's largest value apart in a raw parameter and 5.6e-7 in a
    moment, their losses equal (the step's float atomics: the roots' gradient rows, the transposed lists' order) — so the
    bound is four times the two plain runs' own largest difference.  (The clipped kernel's float instructions are the
    unclipped kernel's plus the one multiply; a run clipped at 1e6 x the norm was 1.2e-5 / 7.2e-7 / 0 away.)"""
    losses, snaps, seen = _sage_plan_run(setup, plain_runs, 5, clip_grad_norm=1e6 * max(plain_runs["norms"]))
    assert all(c == 1.0 for _, c in seen), seen
    for (got, _), want in zip(seen, plain_runs["norms"]):  # (and the norm pass measures what the plain plan's grads() hold)
        assert abs(got - want) <= 1e-6 * want, (got, want)
    _assert_same_run("clipping at 1e6 x the norm", plain_runs, losses, snaps, 5)


def test_constant_lr_warm_up(setup, plain_runs):
    """ConstantLR(factor 0.25, total_iters 3): steps 1-3 are those of a plan created with lr = 0.25 x base (bit for bit, the
    product being exact), step 6 is NOT that plan's — and is autograd's with torch.optim.lr_scheduler.ConstantLR stepped
    after the optimiser, within the bounds of the plan-vs-autograd comparison of this shape"""
    eng, rowptr, col, x, n = setup
    dims, b, P, n_rn = SAGE_SHAPE
    low_l, low_s, _ = _sage_plan_run(setup, plain_runs, 6, lr=0.25 * LR)
    got_l, got_s, _ = _sage_plan_run(setup, plain_runs, 6, lr_factor=0.25, lr_total_iters=3)
    # (the same kernels at another lr: the yardstick is the plain plan's repeatability over as many steps)
    low = dict(plain_runs, losses=low_l, snaps=low_s)
    _assert_same_run("warm-up steps vs lr = 0.25 x base", low, got_l, got_s, 3)
    apart = _run_diff(low_l[5:6], low_s[5:6], got_l[5:6], got_s[5:6])
    assert apart > 1e-3, apart  # three steps at four times the learning rate
    _, ref, lib = _sage_models(eng, dims)
    ref.train()
    want, _, opt = _autograd_run(ref.parameters(), _sage_embed(eng, ref), plain_runs["batches"], b, P, sched=(0.25, 3))
    from gigl_amd.engine import NablpTrainPlan
    plan = NablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, lr=LR, weight_decay=WD, lr_factor=0.25, lr_total_iters=3)
    got = _run(eng, plan, plain_runs["batches"], prefetch=True)
    plan.store(lib)
    moments = plan.moments()
    plan.close()
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)
    assert_adam_state("ConstantLR plan vs autograd", lib.state_dict(), moments, ref.state_dict(),
                      torch_adam_moments(opt, dict(ref.named_parameters())), tol_m=1e-4, tol_v=1e-4, tol_p=1e-4)


def test_both_knobs_survive_grow(setup, plain_runs):
    """step, grow() (the plan is re-created with wide workspaces and adopts the optimiser state), step, step — against a twin
    that never grew.  The wide workspaces number the batch's nodes differently, so that a grown plan does not repeat a
    regular one bit for bit whatever its optimiser does: the run-to-run figure the bound is four times of is taken from the
    same pair WITHOUT the knobs (a plain plan grown after its first step against the plain runs).  total_iters = 2: the
    third step runs at the full learning rate only if the grown plan's schedule went on counting from where it stood."""
    from gigl_amd.engine import NablpTrainPlan
    eng, rowptr, col, x, n = setup
    dims, b, P, n_rn = SAGE_SHAPE
    batches = plain_runs["batches"][:3]
    knobs = dict(clip_grad_norm=0.5 * min(plain_runs["norms"]), lr_factor=0.25, lr_total_iters=2)

    def run(grow, **kw):
        plan = NablpTrainPlan(eng, plain_runs["model"], b, P, n_rn, FAN, temperature=TEMP, lr=LR, weight_decay=WD, **kw)
        seen = []

        def after(i):
            if kw:
                seen.append(plan.grad_norm())
            if grow and i == 0:
                plan.grow()
                assert plan.wide
        losses = _run(eng, plan, batches, after_step=after)
        snap = _snap(eng, plan)
        plan.close()
        return losses[2:], [snap], seen
    base_l, base_s, _ = run(True)
    r = _run_diff(plain_runs["losses"][2:3], plain_runs["snaps"][2:3], base_l, base_s)
    twin_l, twin_s, twin_seen = run(False, **knobs)
    got_l, got_s, seen = run(True, **knobs)
    d = _run_diff(twin_l, twin_s, got_l, got_s)
    print(f"grown vs never grown after 3 steps: plain plan {r:.3e}; with both knobs {d:.3e}; norm / coef per step {seen} vs "
          f"{twin_seen}")
    assert all(c < 1.0 for _, c in seen), seen  # the re-created plan still clips
    # the schedule: a counter that started again would keep step 3 at lr / 4 — a quarter of the twin's last displacement
    low_l, low_s, _ = run(False, **dict(knobs, lr_total_iters=3))
    assert _run_diff(low_l, low_s, twin_l, twin_s) > 1e-4
    assert r > 0 and d <= 4 * r, (d, r)


# ---- 7: the setters' errors

def test_setter_errors(setup):
    from gigl_amd._lib import GiglError
    from gigl_amd.engine import NablpTrainPlan
    from gigl_amd.models import GraphSAGE
    eng, rowptr, col, x, n = setup
    b, P, n_rn = 48, 1, 32
    batch = _lp_batches(eng, n, b, P, n_rn, 1, seed=3)[0]
    lib = GraphSAGE(100, 32, 16, num_layers=2).to(eng.device)
    mk = lambda **kw: NablpTrainPlan(eng, lib, b, P, n_rn, FAN, temperature=TEMP, **kw)
    for bad in (dict(clip_grad_norm=-1.0), dict(clip_grad_norm=float("nan")), dict(clip_grad_norm=float("inf")),
                dict(lr_factor=0.0), dict(lr_factor=1.5), dict(lr_factor=float("nan")), dict(lr_factor=0.5, lr_total_iters=-1),
                dict(lr_total_iters=-1)):
        with pytest.raises(GiglError) as e:
            mk(**bad)
        assert e.value.code == -1, bad  # GIGL_E_INVALID_ARG
    plan = mk()
    lib_ = eng._lib
    assert lib_.gigl_nablp_train_plan_set_clip_grad_norm(plan._plan, 0.0) == -1  # (the C entry point takes no "off")
    assert lib_.gigl_nablp_train_plan_set_clip_grad_norm(plan._plan, -2.0) == -1
    assert lib_.gigl_nablp_train_plan_set_constant_lr(plan._plan, 0.0, 3) == -1
    assert lib_.gigl_nablp_train_plan_set_constant_lr(plan._plan, 1.5, 3) == -1
    assert lib_.gigl_nablp_train_plan_set_constant_lr(plan._plan, 0.5, -1) == -1
    with pytest.raises(GiglError):  # a plan that does not clip computes no norm
        plan.grad_norm()
    assert lib_.gigl_nablp_train_plan_set_clip_grad_norm(plan._plan, 1.0) == 0  # before the first step: taken
    assert lib_.gigl_nablp_train_plan_set_constant_lr(plan._plan, 0.5, 2) == 0
    assert np.isfinite(_run(eng, plan, [batch])[0])
    norm, coef = plan.grad_norm()
    assert norm > 0 and 0 < coef <= 1
    assert lib_.gigl_nablp_train_plan_set_clip_grad_norm(plan._plan, 1.0) == -1  # after it: the step is captured
    assert lib_.gigl_nablp_train_plan_set_constant_lr(plan._plan, 0.5, 2) == -1
    for knobs in ((1.0, 1.0, 0), (0.0, 0.5, 2)):  # ... and through the plan object: GiglError
        plan._optim_knobs = knobs
        with pytest.raises(GiglError):
            plan._apply_optim_knobs(plan._plan)
    plan.close()
