"""The GCN inference plan (gigl_gcn_plan_*, csrc/pipeline.hip + csrc/agg.hip's gcn_layer_rows_kernel and
gcn_root_layer_kernel) through engine.GcnPlan against a FLOAT64 restatement of TwoLayerGCN's eval-time forward over the
oracle's union graph — cases, batches, references and the bound in tests/gcn_infer_cases.py.

Every shape runs four ways — layer 1 aggregate-first or over the projected table, layer 2 fused into the roots' rows or as
gather + projection + copy — each against the float64 rows, bound max(1e-5, 4 x the float32 restatement's error), over every
element; fused_root() must report what ran.  Tree and union graph of the plan are bit-exact against the oracle.  Two runs,
eager against hipGraph replay, and groups = 4 x 16 roots against four plans of 16 roots are bit-identical.  New weights with
a recomputed projection give the new reference; a workspace overflow gives NaN rows and counts once; with-replacement trees
are refused.

Measured on an MI355X (largest absolute error of a case's rows against float64 over the four routes; fp32 = the float32
restatement's; the bound is 1e-5 for every case):

    case                     err       fp32
    base                  9.4e-08    8.7e-08
    scalar_paths          1.5e-07    6.8e-08
    wide_input            2.1e-07    1.1e-07
    cora_width            4.4e-07    1.7e-07
    fp16_table            1.1e-07    1.1e-07
    no_bias               7.9e-08    6.2e-08
    long_rows             1.1e-07    1.1e-07
    isolated_roots        1.0e-07    8.7e-08
    one_root_everywhere   3.6e-08    3.6e-08
    l2_normalised         2.0e-07    1.3e-07
    wide_hidden           8.8e-08    3.2e-08
"""
import contextlib

import numpy as np
import pytest
import torch

import gcn_infer_cases as ic
import gcn_plan_cases as gc

ROUTES = [(proj, fused) for proj in (False, True) for fused in (True, False)]


@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    rowptr, col = gc.graph()[:2]
    e = HipEngine(0)
    e.load_csc(rowptr, col)
    e._gcn_case_table = None
    yield e
    e.close()


def _params(case, state):
    return ([state["conv1.lin.weight"], state["conv2.lin.weight"]],
            [state.get("conv1.bias"), state.get("conv2.bias")] if case.bias else [None, None])


@contextlib.contextmanager
def _plan_of(eng, case, state, b=None, groups=1):
    """the case's plan on a stream of its own, over the case's feature table (the engine keeps the last one loaded)"""
    from gigl_amd.engine import GcnPlan
    key = (case.dims[0], case.half)
    if eng._gcn_case_table != key:
        eng.load_features(gc.features(*key))
        eng._gcn_case_table = key
    st = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    plan = GcnPlan(eng, *_params(case, state), case.b if b is None else b, list(case.fan), groups=groups, l2_normalize=case.l2)
    try:
        with torch.cuda.stream(st):
            yield plan
        eng.synchronize()
    finally:
        plan.close()
        eng.bind_stream(torch.cuda.current_stream(eng.device))


def _dev(eng, roots):
    return torch.from_numpy(np.ascontiguousarray(roots).view(np.int32)).to(eng.device)


def _route(eng, plan, state, proj: bool, fused: bool):
    plan.set_projected_input(eng.gcn_project_features(state["conv1.lin.weight"]) if proj else None)
    plan.set_fused_root(fused)


def _check_rows(label, got, want, bound, fp32):
    got = got.detach().cpu().double()
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), label
    err = float((got - want).abs().max())
    print(f"{label}: err={err:.3e} fp32={fp32:.3e} bound={bound:.3e}")
    assert err <= bound, (label, err, bound)


def _check_graph(plan, case, name):
    """the plan's tree and union graph against the oracle's, bit for bit"""
    roots, (nbr, cnt), u = ic.batch(name)
    hb = plan.last_batch_to_host()
    for k in range(2):
        assert np.array_equal(hb["nbr"][k], nbr[k]) and np.array_equal(hb["cnt"][k], cnt[k]), (name, "tree", k)
    assert np.array_equal(hb["meta"][:5], u["meta"][:5]) and hb["meta"][8] == 0, (name, hb["meta"], u["meta"])
    nn = int(u["meta"][0])
    assert np.array_equal(hb["nodes"], u["nodes"][:nn]) and np.array_equal(hb["root_local"], u["root_local"][:case.b])
    for i in range(nn):  # (the plan's rows keep their capacity before deduplication: compare what each row holds)
        assert np.array_equal(hb["col"][hb["rowptr"][i]:hb["rowend"][i]], u["col"][u["rowptr"][i]:u["rowptr"][i + 1]]), (name, i)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ic.PLAIN_CASES)
def test_rows_match_float64_on_every_route(eng, name):
    case = ic.CASES[name]
    state = ic.state_of(case)
    want, bound, fp32 = ic.reference(name)
    roots = _dev(eng, ic.batch(name)[0])
    with _plan_of(eng, case, state) as plan:
        for proj, fused in ROUTES:
            _route(eng, plan, state, proj, fused)
            assert plan.fused_root() == (fused and ic.fused_root_by_shape(case)), (name, proj, fused)
            out = plan.run(roots)
            eng.synchronize()
            _check_rows(f"{name} projected={proj} fused={plan.fused_root()}", out, want, bound, fp32)
            again = plan.run(roots)
            eng.synchronize()
            assert torch.equal(out, again), (name, proj, fused, "two runs differ")
        _check_graph(plan, case, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["base", "scalar_paths", "wide_input"])
def test_graph_replay_is_bit_identical(eng, name):
    case = ic.CASES[name]
    state = ic.state_of(case)
    roots = _dev(eng, ic.batch(name)[0])
    other = _dev(eng, np.array(gc._roots(gc.CASES["n_valid_63"])[0].tolist() + [5], dtype=np.uint32))
    with _plan_of(eng, case, state) as plan:
        for proj, fused in ROUTES:
            _route(eng, plan, state, proj, fused)
            plan.use_graph(False)
            eager, eager_other = plan.run(roots).clone(), plan.run(other).clone()
            plan.use_graph(True)
            first = plan.run(roots).clone()  # (this call captures: it runs eagerly)
            assert torch.equal(plan.run(other), eager_other) and torch.equal(plan.run(roots), eager), (name, proj, fused)
            assert torch.equal(first, eager)
            eng.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["base", "wide_input"])
def test_groups_equal_plans_of_one_batch(eng, name):
    case = ic.CASES[name]
    state = ic.state_of(case)
    roots_h = ic.batch(name)[0]
    roots = _dev(eng, roots_h)
    got = {}
    with _plan_of(eng, case, state, b=16, groups=4) as plan:
        for proj, fused in ROUTES:
            _route(eng, plan, state, proj, fused)
            got[proj, fused] = plan.run(roots).clone()
        acc = torch.zeros(16, dtype=torch.int64, device=eng.device)
        plan.stats(roots, acc)
        eng.synchronize()
        hb = plan.last_batch_to_host()
        acc = acc.cpu().numpy()
        # (rows and edges per layer over the generic union: layer 0 the nodes of level <= 1, layer 1 the roots)
        assert acc[9] == hb["meta"][3] and acc[10] == hb["meta"][2] and acc[3] == hb["meta"][0] and acc[13] == 0
        lens = (hb["rowend"] - hb["rowptr"]).astype(np.int64)
        assert acc[5] == lens[:hb["meta"][3]].sum() and acc[6] == lens[:hb["meta"][2]].sum()
    with _plan_of(eng, case, state, b=16) as plan:
        for proj, fused in ROUTES:
            _route(eng, plan, state, proj, fused)
            single = torch.cat([plan.run(roots[g * 16:(g + 1) * 16].contiguous()).clone() for g in range(4)])
            eng.synchronize()
            assert torch.equal(single, got[proj, fused]), (name, proj, fused)


@pytest.mark.gpu
def test_new_weights_and_a_recomputed_projection(eng):
    name = "wide_input"
    case = ic.CASES[name]
    roots = _dev(eng, ic.batch(name)[0])
    with _plan_of(eng, case, ic.state_of(case)) as plan:
        for shift in (0, 1):
            state = ic.state_of(case, shift)
            want, bound, fp32 = ic.reference(name, shift)
            plan.set_weights(*_params(case, state))
            for proj in (True, False):
                _route(eng, plan, state, proj, True)
                out = plan.run(roots)
                eng.synchronize()
                _check_rows(f"{name} weights {shift} projected={proj}", out, want, bound, fp32)
    assert float((ic.reference(name, 1)[0] - ic.reference(name, 0)[0]).abs().max()) > 1e-2  # (the draws do differ)


@pytest.mark.gpu
def test_overflow_gives_nan_rows_and_counts_once(eng):
    case = ic.CASES["overflow"]
    state = ic.state_of(case)
    roots = _dev(eng, ic.batch("overflow")[0])
    with _plan_of(eng, case, state) as plan:
        for proj, fused in ROUTES:
            _route(eng, plan, state, proj, fused)
            acc = torch.zeros(1, dtype=torch.int32, device=eng.device)
            out = plan.run(roots)
            plan.overflow_add(acc)
            eng.synchronize()
            assert bool(torch.isnan(out).all()) and int(acc.item()) == 1, (proj, fused)


@pytest.mark.gpu
def test_with_replacement_trees_are_refused(eng):
    from gigl_amd._lib import MODE_REPLACE, GiglError
    case = ic.CASES["base"]
    roots = _dev(eng, ic.batch("base")[0])
    with _plan_of(eng, case, ic.state_of(case)) as plan:
        with pytest.raises(GiglError) as e:
            plan.run(roots, mode=MODE_REPLACE)
        assert e.value.code == -4  # GIGL_E_UNSUPPORTED
