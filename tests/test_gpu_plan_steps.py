"""The one-call plan's step list (csrc/pipeline.hip plan_build_steps): the segments of a profiled replay follow the kernel
ids the steps' launchers record under, and every setter that changes what a plan runs drops the captured graphs and
rebuilds the list.  640-node graph of sage_plan_cases.py, 64 roots, fan-outs [5, 3]; every comparison is bit for bit (the
plan's forward is deterministic: replay and eager issue the same launches in the same order)."""
import numpy as np
import pytest
import torch

import sage_plan_cases as sc
from gigl_amd import _lib

pytestmark = pytest.mark.gpu
B, FAN, D_IN = 64, [5, 3], 36
REPLAYS = 6


@pytest.fixture()
def eng():
    """an engine over the graph and a table, bound to a created stream (the legacy default stream cannot be captured)"""
    from gigl_amd.engine import HipEngine
    rowptr, col, _ = sc.graph("main")
    e = HipEngine(0)
    e.load_csc(rowptr, col)
    e.load_features((np.random.default_rng(7).standard_normal((sc.N_NODES, D_IN)) / 4).astype(np.float32))
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=e.device)
    e.bind_stream(st)
    torch.cuda.set_stream(st)
    try:
        yield e
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream(e.device))
        e.close()


def _roots(e):
    return torch.from_numpy(sc.roots_of("groups").view(np.int32)).to(e.device)


def _sage_weights(e, hidden, n_out, seed):
    g = torch.Generator().manual_seed(seed)
    dims = [D_IN, hidden, n_out]
    ws = [(torch.randn(dims[l + 1], 2 * dims[l], generator=g) / (2 * dims[l]) ** 0.5).to(e.device) for l in range(2)]
    bs = [(torch.randn(dims[l + 1], generator=g) * 0.1).to(e.device) for l in range(2)]
    return ws, bs


def _make(e, family):
    """-> a factory of identically configured plans of the family"""
    if family == "gat":
        from gigl_amd.models_attn import GAT
        torch.manual_seed(3)
        model = GAT(D_IN, 16, 24, num_layers=2, heads=2).to(e.device)  # heads [2, 1]
        return lambda: model.make_plan(e, B, FAN)
    ws, bs = _sage_weights(e, 256 if family == "sage_fused" else 64, 47, seed=5)
    return lambda: e.make_sage_plan(ws, bs, B, FAN)


@pytest.mark.parametrize("family", ["sage_fused", "sage_apart", "gat"])
@pytest.mark.parametrize("kernel", ["gather_mean", "linear"])
def test_profiled_replay_times_every_launch_of_the_family(eng, family, kernel):
    """with one kernel family profiled, a replayed plan equals the eager plan bit for bit, and profile_read reports exactly
    replays x (the launches of that family in ONE eager run, as the eager plan's own profile_read counts them) with a
    measured time: every launcher that records under the family's id sits in an eager segment, none inside a captured
    graph (a GAT plan's layers >= 1 project with gigl_linear and attend with a gather-family kernel)"""
    make = _make(eng, family)
    eager, replayed = make(), make()
    try:
        assert eager.fused_layers() == (family == "sage_fused")
        roots = _roots(eng)
        eager.run(roots)  # (whatever only a first run launches stays out of the count)
        eng.profile_enable([kernel], 64)
        want = eager.run(roots).clone()
        _, per_run = eng.profile_read(kernel)
        assert per_run >= 1 and bool(torch.isfinite(want).all())
        replayed.use_graph(True)
        assert torch.equal(replayed.run(roots), want)  # captures (its own eager run is untimed)
        eng.profile_reset()
        for i in range(REPLAYS):
            assert torch.equal(replayed.run(roots), want), i
        replayed.flush_profile()
        ms, launches = eng.profile_read(kernel)
        print(f"{family} {kernel}: {per_run} launches per eager run, {launches} over {REPLAYS} replays, {ms:.4f} ms")
        assert launches == REPLAYS * per_run
        assert ms > 0
    finally:
        eng.profile_enable([], 0)
        eager.close()
        replayed.close()


def test_reconfigured_captured_plan_equals_a_fresh_eager_plan(eng):
    """one captured SAGE plan through every setter that changes what it runs: after each, the next run (which captures
    again) and the one after it (a replay) equal a freshly created eager plan configured the same way, bit for bit"""
    lib, ctx = eng._lib, eng._ctx
    ws, bs = _sage_weights(eng, 256, 47, seed=5)
    ws2, bs2 = _sage_weights(eng, 256, 47, seed=6)
    proj = eng.project_features(ws[0])
    roots = _roots(eng)
    side = torch.cuda.Stream(device=eng.device)
    plan = eng.make_sage_plan(ws, bs, B, FAN)
    plan.use_graph(True)

    def check_against(fresh, change, what):
        try:
            want = fresh.run(roots).clone()
        finally:
            fresh.close()
        plan.run(roots)  # (still the old configuration: captured under the arena as the fresh plan left it)
        change()
        for turn in ("capture", "replay"):
            assert torch.equal(plan.run(roots), want), (what, turn)
        return want

    try:
        assert plan.fused_layers()
        base = check_against(eng.make_sage_plan(ws, bs, B, FAN), lambda: None, "as created")
        summed = check_against(eng.make_sage_plan(ws, bs, B, FAN, aggr="sum"),
                               lambda: _lib.check(lib.gigl_sage_plan_set_aggr(plan._plan, _lib.AGGR["sum"]), ctx), "set_aggr")
        assert not torch.equal(summed, base)
        fresh = eng.make_sage_plan(ws, bs, B, FAN, aggr="sum")
        fresh.set_projected_input(proj)
        check_against(fresh, lambda: plan.set_projected_input(proj), "set_projected_input")
        assert not plan.fused_layers()
        back = check_against(eng.make_sage_plan(ws, bs, B, FAN, aggr="sum"), lambda: plan.set_projected_input(None),
                             "set_projected_input(None)")
        assert plan.fused_layers() and torch.equal(back, summed)
        check_against(eng.make_sage_plan(ws, bs, B // 2, FAN, groups=2, aggr="sum"),
                      lambda: _lib.check(lib.gigl_sage_plan_set_groups(plan._plan, B // 2), ctx), "set_groups")
        moved = check_against(eng.make_sage_plan(ws2, bs2, B // 2, FAN, groups=2, aggr="sum"),
                              lambda: plan.set_weights(ws2, bs2), "set_weights")
        assert not torch.equal(moved, summed)
        check_against(eng.make_sage_plan(ws2, bs2, B // 2, FAN, groups=2, aggr="sum"),
                      lambda: plan.set_graph_stream(side), "set_graph_stream")
        check_against(eng.make_sage_plan(ws2, bs2, B // 2, FAN, groups=2, aggr="sum"),
                      lambda: plan.set_graph_stream(None), "set_graph_stream(None)")
    finally:
        torch.cuda.synchronize()
        plan.close()
