"""The forward path of the GraphSAGE one-call plan (gigl_sage_plan_run), whose kernels have no entry point of their own:
linear_fused2x_kernel with fused2_images_kernel, fused2_scale_kernel and sage_fused_out_kernel<MEAN|SUM> (both layers
in one kernel, the last reduction over p rows), the eight linear_split_kernel instantiations that only
linear_tiled_strided launches (tiled A operand with and without the two-source [mean | self] operand; bf16 planes, half
split, half split with fp16 self rows; NJ 1 and 2), hs_chain_kernel, the tiled writer of gigl_gather_reduce_mixed,
gigl_gather_project_mixed (projected input) and l2_normalize_rows_kernel — every element against a float64 edge-list
formula on the plan's OWN union graph (SagePlan.last_batch_to_host), after that graph's edge multiset (global ids) has
been found equal to the CPU oracle's (oracle.sample_khop(canonical=True) + oracle.union_build): a mismatch there is a
GRAPH failure, reported as such, never a numeric one.  Cases, inputs, reference, bounds and probes live in
tests/sage_plan_cases.py (its docstring derives the bounds; it is also the child process of the knob tests).

Graph: 640 nodes built by hand — in-degrees 0, 1, 2, 3, 4, exactly the first fan-out (5), 10 and 14, a hub of 40 in-edges that
is an in-neighbour of every fourth node (its union row merges the samples of ~40 occurrences: 38 edges at fan-outs
[5, 3]), duplicate roots; a second graph whose in-degrees are all 1, 2 or 4 for the exact mean probes.  Row layouts of
the fused kernel: 4 roots / 13 rows (one partial 128-row tile), 198 roots / 492 rows (the roots end inside the second
tile), 256 roots / 561 rows (the roots end on a tile edge), three batches of 64 roots.

Inputs of the tolerance cases are drawn so that no hidden pre-activation lies within its own bound of zero (the offending
nodes' feature rows are redrawn), so the relu masks agree with the reference by construction.  Exact probes (bit for
bit): integer tables in [-8, 8], weights in {-2..2}, integer biases, under a sum and under a mean over power-of-two
degrees, on the fused path and on every path apart; the column identity (the last layer selects one hidden column per
output, all 256 columns in six set_weights calls of 48 outputs); history independence (300 distinct roots, then 5, equal
to a fresh plan); a second run equal to the first, on EVERY case; GIGL_F2_ALL_WR set — the library reads it once per
process, so in a child process of its own — gives every fused case the rows of this process, where it is unset.

BUG FOUND by `fused sum headroom`, `apart h64 sum headroom` and the cases next to them, and its fix: under a sum the
half-split scales assumed |operand| <= max fan-out x max|x| (and x fan-out again per layer in hs_chain_kernel), but a union
row merges the samples of every occurrence of its node — each sampled with its own hash key — and holds up to the node's
whole in-row: with a table of one sign next to 1.59 and fan-outs [5, 3] the hub's 38-edge row reached 60 against an assumed
7.95, its scaled fp16 plane saturated and the roots behind it came out wrong by 0.25 .. 0.47 of their own scale S (fused
0.30 / 0.36, apart 0.47, three layers 0.25).  No fan-out bounds such a row, and bounding it by the largest in-degree costs
the precision of every other row (1e-4 on R-MAT graphs), so the summed half of the operand is now MEASURED on the device
at every run (tiled_absmax_kernel) and the scale follows it.

Measured on an MI355X (worst scaled error max |got - float64| / S of the path's cases, S the element's own scale of the
last layer; next to it the same formula evaluated in float32 on the CPU, and the worst |got - float64| / bound):

    path (kernel names of tests/sage_plan_cases.py)        cases  eps       kernel   float32  worst |err| / bound
    fused, mean   linear_fused2x + sage_fused_out<MEAN>      20   1.83e-06  1.9e-07  2.0e-07  0.031
    fused, sum    linear_fused2x + sage_fused_out<SUM>        8   1.83e-06  1.8e-07  2.4e-07  0.021
    apart, two layers     ts_hs<1|2> + hs_chain              12   1.59e-06  3.2e-07  2.2e-07  0.037
    apart, two layers     ts_hs_selfhalf<1|2>, ts_hs          5   1.59e-06  2.1e-07  2.3e-07  0.027
    apart, three layers   ts_hs<1|2> + hs_chain twice         4   1.59e-06  1.8e-07  1.1e-07  0.007
    apart, three layers   ts_hs_selfhalf<1|2>, ts_hs          5   1.59e-06  2.3e-07  1.2e-07  0.006
    apart, two layers     ts_bf16<1|2>                        2   4.00e-07  2.0e-07  1.2e-07  0.151
    apart, three layers   ts_bf16<2>                          1   4.00e-07  1.9e-07  1.2e-07  0.008
    apart, two layers     tiled_bf16<2>, ts_bf16              1   4.00e-07  3.1e-07  2.1e-07  0.257
    apart, three layers   tiled_bf16<1>, ts_bf16              1   4.00e-07  1.3e-07  9.1e-08  0.076
    row-major (d % 4 != 0: pinned elsewhere)                  1   4.00e-07  2.7e-07  1.5e-07  0.115
    projected input       gather_project, ts_bf16             3   6.38e-07  2.5e-07  1.5e-07  0.119
    child GIGL_PLAN_HS_LAYERS=0                               5   1.83e-06  2.2e-07  1.6e-07  0.089
    child GIGL_GEMM_SPLIT=bf16                                5   4.00e-07  3.0e-07  1.9e-07  0.108
(eps: the largest per-layer figure of the path; the propagated terms make the whole bound 4 .. 30 x the measured error on
two layers and more on three, where each layer's error is carried on over S / |h|.  Dropping the second product's
low-plane MFMA — 1e-4 S — fails every fused case of more than four output elements at 1.8 .. 11 x its bound.)  Every exact
probe held on every case.

The file: 86 GPU tests (63 tolerance cases and 20 exact probes here, 5 + 5 cases in the two knob children, the 34 fused
cases in the GIGL_F2_ALL_WR child) and 4 CPU tests.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sage_plan_cases as sc

gpu = pytest.mark.gpu
_id = lambda c: c["label"].replace(" ", "-")


@pytest.fixture(scope="module")
def engs():
    e = sc.Engines()
    yield e
    e.close()


def _verdict(r):
    print(sc.format_case(r))
    graph = [f for f in r["fails"] if f.startswith("graph")]
    assert not graph, ("GRAPH failure (sampler / union, not the layers)", r["label"], graph)
    assert not r["fails"], (sc.format_case(r), r["fails"])


# ---- GPU: this process (no knob) ------------------------------------------------------------------------------------
_DIGESTS = {}  # label -> sha256 of the case's rows in THIS process (no knob)


def _run(engs, case):
    r = sc.run_case(engs, case)
    _DIGESTS[case["label"]] = r["digest"]
    return r


@gpu
@pytest.mark.parametrize("case", sc.default_cases(), ids=_id)
def test_plan_case_against_float64(engs, case):
    _verdict(_run(engs, case))


@gpu
@pytest.mark.parametrize("case", sc.probe_cases(), ids=_id)
def test_plan_exact_probe(engs, case):
    _verdict(_run(engs, case))


# ---- GPU: one fresh child process per knob --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode,var,value", [("hs_layers", "GIGL_PLAN_HS_LAYERS", "0"), ("bf16", "GIGL_GEMM_SPLIT", "bf16")])
def test_knob_cases_in_a_child_process(mode, var, value):
    env = dict(os.environ)
    for v in ("GIGL_PLAN_HS_LAYERS", "GIGL_GEMM_SPLIT", "GIGL_LINEAR_EXACT", "GIGL_PLAN_NO_FUSE2", "GIGL_F2_ALL_WR"):
        env.pop(v, None)
    env[var] = value
    p = subprocess.run([sys.executable, os.path.abspath(sc.__file__), mode], env=env, capture_output=True, text=True, timeout=240)
    rows = [json.loads(line[5:]) for line in p.stdout.splitlines() if line.startswith("CASE ")]
    for r in rows:
        print(sc.format_case(r))
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    assert [r["label"] for r in rows] == [c["label"] for c in sc.child_cases(mode)]
    bad = [(sc.format_case(r), r["fails"]) for r in rows if r["fails"]]
    assert not bad, bad


@gpu
def test_f2_all_wr_in_a_child_process_changes_no_bit_of_a_fused_case(engs):
    """GIGL_F2_ALL_WR=1 (every tile of the fused projection computes the W_r block, not only the tiles that hold roots) is
    read once per process: a child runs every fused case with it, this process — which must run without — has or takes
    the same cases' rows, and the two agree bit for bit"""
    assert "GIGL_F2_ALL_WR" not in os.environ, "the comparison needs this process to run with the knob unset"
    env = dict(os.environ)
    for v in ("GIGL_PLAN_HS_LAYERS", "GIGL_GEMM_SPLIT", "GIGL_LINEAR_EXACT", "GIGL_PLAN_NO_FUSE2"):
        env.pop(v, None)
    env["GIGL_F2_ALL_WR"] = "1"
    p = subprocess.run([sys.executable, os.path.abspath(sc.__file__), "f2_all_wr"], env=env, capture_output=True, text=True, timeout=240)
    rows = [json.loads(line[5:]) for line in p.stdout.splitlines() if line.startswith("CASE ")]
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    cases = sc.child_cases("f2_all_wr")
    assert [r["label"] for r in rows] == [c["label"] for c in cases] and len(cases) >= 30
    bad = [(r["label"], r["fails"]) for r in rows if r["fails"] or not r["fused"]]
    assert not bad, bad
    for r, case in zip(rows, cases):
        here = _DIGESTS.get(case["label"]) or _run(engs, case)["digest"]
        assert len(here) == 64 and r["digest"] == here, ("GIGL_F2_ALL_WR changes the rows of", case["label"])


# ---- CPU ------------------------------------------------------------------------------------------------------------
def _dispatch(case, knob=""):
    return sc.dispatch(case, sc.first_table(case), knob)


def test_every_kernel_has_a_tolerance_case_and_an_exact_probe():
    """from the parametrisation and the restated dispatch rule"""
    tol = [c for c in sc.default_cases()]
    probes = [c for c in sc.probe_cases() if c["kind"] in ("int", "colid")]
    seen_tol = set().union(*[_dispatch(c)["kernels"] for c in tol])
    seen_probe = set().union(*[_dispatch(c)["kernels"] for c in probes])
    assert len(sc.KERNELS) == 17 and set(sc.KERNELS) <= seen_tol, set(sc.KERNELS) - seen_tol
    assert set(sc.KERNELS) <= seen_probe, set(sc.KERNELS) - seen_probe
    assert {c["kind"] for c in sc.probe_cases()} == {"int", "colid", "history"}
    for kind in ("colid", "history"):  # on the fused path and on one path apart
        assert {_dispatch(c)["fused"] for c in sc.probe_cases() if c["kind"] == kind} == {True, False}
    # the children: layers >= 1 back on the bf16 planes under a half-split first layer; no half split at all
    hs = [_dispatch(c, "hs_layers") for c in sc.child_cases("hs_layers")]
    assert all(d["hs0"] and "hs_chain" not in d["kernels"] for d in hs) and any(d["fused"] for d in hs)
    assert {"ts_hs<1>", "ts_hs<2>", "ts_hs_selfhalf<2>", "ts_bf16<1>", "ts_bf16<2>"} <= set().union(*[d["kernels"] for d in hs])
    bf = [_dispatch(c, "bf16") for c in sc.child_cases("bf16")]
    assert not any(d["hs0"] or d["fused"] for d in bf)
    assert {"ts_bf16<1>", "ts_bf16<2>", "tiled_bf16<1>", "tiled_bf16<2>"} <= set().union(*[d["kernels"] for d in bf])
    # the listed shapes are all there
    fused = [c for c in sc.fused_cases()]
    assert all(_dispatch(c)["fused"] for c in fused)
    assert {c["d_in"] for c in fused} >= set(sc.F_DIN) and {c["n_out"] for c in fused} == set(sc.F_NOUT)
    assert {c["bias"] for c in fused} == {True, False} and {c["act_last"] for c in fused} == {True, False}
    assert {c["aggr"] for c in fused} == {"mean", "sum"} and {c["groups"] for c in fused} == {1, 3} and any(c["l2"] for c in fused)
    assert {c["roots"] for c in fused} >= {"partial", "inside", "edge", "groups"}
    assert {(c["tscale"], c["wscale"]) for c in fused} >= {(-20, -20), (20, 20)} and {c["tkind"] for c in fused} >= {"apart8", "edge"}
    apart = [c for c in sc.apart_cases() if not c["proj"]]
    assert not any(_dispatch(c)["fused"] for c in apart)
    assert {(c["hidden"][0], len(c["hidden"]) + 1, c["aggr"]) for c in apart} >= {(h, L, a) for h in (64, 132) for L in (2, 3)
                                                                                 for a in ("mean", "sum", "max")}
    assert sum(1 for c in apart if not _dispatch(c)["tiled"]) == 1  # (the row-major path: a single case)
    assert {c["aggr"] for c in sc.apart_cases() if c["proj"]} == {"mean", "sum"}


def test_dispatch_rule_on_hand_worked_shapes():
    def d(knob="", **kw):
        return _dispatch(sc._case("hand", **kw), knob)
    assert d()["layers"] == ["linear_fused2x", "sage_fused_out<MEAN>"] and d(aggr="sum")["layers"][1] == "sage_fused_out<SUM>"
    assert d(n_out=49)["layers"] == ["ts_hs<2>", "ts_hs<1>"] and d(no_fuse2=True)["layers"] == ["ts_hs<2>", "ts_hs<1>"]
    assert not d(aggr="max")["fused"] and not d(table="f16")["fused"] and not d(hidden=[252])["fused"] and not d(proj=True)["fused"]
    assert d(table="f16")["layers"] == ["ts_hs_selfhalf<2>", "ts_hs<1>"]
    assert d(hidden=[64], n_out=65)["layers"] == ["ts_hs<1>", "ts_hs<2>"] and d(hidden=[64], n_out=64)["layers"][1] == "ts_hs<1>"
    assert d(hidden=[64, 68], roots="small")["layers"] == ["ts_hs<1>", "ts_hs<2>", "ts_hs<1>"]
    assert d(tkind="outlier")["layers"] == ["ts_bf16<2>", "ts_bf16<1>"] and not d(tkind="outlier")["hs0"]
    assert d(tkind="outlier", table="f16", hidden=[64])["layers"] == ["tiled_bf16<1>", "ts_bf16<1>"]
    assert d(d_in=6, hidden=[64])["layers"] == ["rowmajor<1>", "rowmajor<1>"] and d(hidden=[66, 64], roots="small")["layers"][0] == "rowmajor<2>"
    assert d("hs_layers", hidden=[64])["layers"] == ["ts_hs<1>", "ts_bf16<1>"] and d("hs_layers")["fused"]
    assert d("bf16")["layers"] == ["ts_bf16<2>", "ts_bf16<1>"] and d("bf16", table="f16")["layers"] == ["tiled_bf16<2>", "ts_bf16<1>"]
    assert d(proj=True, hidden=[64])["layers"] == ["gather_project", "ts_bf16<1>"]
    # the three row layouts against the 128-row tile, and what a summed union row can hold
    lay = {k: sc.layout_of(sc._case("hand", roots=k)) for k in ("partial", "inside", "edge")}
    assert lay["partial"][1] < 128 and lay["partial"][0] < len(sc.roots_of("partial"))  # (a duplicate root)
    assert 128 < lay["inside"][0] < 256 < lay["inside"][1] and lay["inside"][0] < len(sc.roots_of("inside"))
    assert lay["edge"][0] == 256 and lay["edge"][1] > 512
    ext = sc.case_inputs(sc._case("hand", aggr="sum"))["ext"]
    longest = max(js.size for _, js in ext["rows"])
    assert 4 * max(sc.FAN2) < longest <= sc.HUB_DEG  # (a union row is NOT bounded by a fan-out: the hub's merges ~40 samples)
    deg = np.diff(sc.graph("main")[0])
    assert {0, 1, 2, 4, 5, 10, 14}.issubset(set(deg.tolist())) and deg.max() == sc.HUB_DEG and (deg > 5).sum() > 100
    assert set(np.diff(sc.graph("pow2")[0]).tolist()) == {1, 2, 4}


def test_reference_is_the_stated_formula_and_every_case_keeps_its_margins():
    from oracle import gnn_ref
    case = sc._case("ref", hidden=[20, 12], roots="small", d_in=8, n_out=5)
    inp = sc.case_inputs(case)
    ext, ws, bs = inp["ext"], inp["weights"], inp["biases"]
    x = inp["x"].double().numpy()
    src = torch.from_numpy(np.concatenate([js for _, js in ext["rows"]]))
    dst = torch.from_numpy(np.concatenate([np.full(js.size, i) for i, js in ext["rows"]]))
    sd = {}
    for l, (w, b) in enumerate(zip(ws, bs)):
        d = w.shape[1] // 2
        sd.update({"conv_layers.%d.lin_l.weight" % l: w[:, :d].double(), "conv_layers.%d.lin_l.bias" % l: b.double(),
                   "conv_layers.%d.lin_r.weight" % l: w[:, d:].double()})
    h0 = torch.from_numpy(x[ext["nid"]])
    want = gnn_ref.graphsage_forward(h0, torch.stack([src, dst]), sd, 3)[torch.from_numpy(ext["root_idx"])]
    assert np.abs(sc.forward(case, x, ext, ws, bs)["y"] - want.numpy()).max() <= 1e-12
    for aggr in ("sum", "max"):  # the torch index_add_ / scatter_reduce form
        h = h0
        for l, (w, b) in enumerate(zip(ws, bs)):
            d = w.shape[1] // 2
            if aggr == "sum":
                a = torch.zeros_like(h).index_add_(0, dst, h[src])
            else:
                a = torch.full_like(h, float("-inf")).scatter_reduce(0, dst[:, None].expand(-1, h.shape[1]), h[src], "amax")
                a[torch.isinf(a)] = 0
            h = a @ w[:, :d].double().T + b.double() + h @ w[:, d:].double().T
            h = torch.relu(h) if l < 2 else h
        c2 = dict(case, aggr=aggr, l2=(aggr == "max"))
        want = h[torch.from_numpy(ext["root_idx"])]
        want = torch.nn.functional.normalize(want, dim=1, eps=1e-12) if c2["l2"] else want
        assert np.abs(sc.forward(c2, x, ext, ws, bs)["y"] - want.numpy()).max() <= 1e-12
    # no hidden pre-activation of any tolerance case within its own bound of zero; every eps below a plane product
    for knob, cases in (("", sc.default_cases() + [c for c in sc.probe_cases() if c["kind"] == "history"]),
                        ("hs_layers", sc.child_cases("hs_layers")), ("bf16", sc.child_cases("bf16"))):
        for c in cases:
            if c["kind"] == "int":
                continue
            inp = sc.case_inputs(c, knob)
            disp = sc.dispatch(c, inp["x"], knob)
            params = sc.params_of(c, disp, inp["x"], inp["weights"], inp["biases"], inp["ext"])
            assert all(4e-7 <= p[0] < 1e-5 for p in params), c["label"]
            res = sc.forward(c, inp["x"].float().numpy().astype(np.float64), inp["ext"], inp["weights"], inp["biases"], params)
            assert not sc.margin_offenders(c, res), c["label"]
            # a missing plane product (~2^-12 S) fails every element (under the L2 normalisation a row's elements share the
            # norm's error: judged on the other cases)
            two = len(c["fan"]) == 2 and not c["l2"]  # (a third layer carries two layers' errors on, each over S / |h|)
            assert np.isfinite(res["bound"]).all() and (not two or (res["bound"] < 2.0 ** -12 * res["S"]).all()), c["label"]


def test_integer_probes_are_exact_in_every_operand_split():
    """numpy emulation of the half split (hsplit_store at the power-of-two scales the kernels derive) and of the bf16
    split of every probe tensor and of every intermediate row: zero residual, and every sum below 2^24 units"""
    p2 = sc.lc.hs_pow2_scale_np

    def exact(v, s):
        v = np.asarray(v, dtype=np.float64)
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
        b1, b2, b3 = sc.lc.split3_np(v.astype(np.float32))
        assert np.array_equal(b1.astype(np.float64) + b2 + b3, v)
        if s:
            h1, h2 = sc.lc.hsplit_np(v.astype(np.float32), s)
            assert np.isfinite(h1).all() and np.array_equal((h1 + h2) / s, v)

    for knob, cases in (("", sc.probe_cases()), ("hs_layers", sc.child_cases("hs_layers")), ("bf16", sc.child_cases("bf16"))):
        for c in cases:
            if c["kind"] not in ("int", "colid"):
                continue
            inp = sc.case_inputs(c, knob)
            disp = sc.dispatch(c, inp["x"], knob)
            x = inp["x"].float().numpy().astype(np.float64)
            calls = [(inp["weights"], inp["biases"])]
            if c["kind"] == "colid":
                calls = [(inp["weights"][:-1] + [w], inp["biases"][:-1] + [b])
                         for w, b in (sc.colid_weights(c, i) for i in range((c["hidden"][-1] + 47) // 48))]
            for ws, bs in calls:
                params = sc.params_of(c, disp, inp["x"], ws, bs, inp["ext"])
                h = x[inp["ext"]["nid"]]
                dims = sc.dims_of(c)
                unit = 1.0
                for l in range(len(dims) - 1):
                    a, _ = sc.reduce_rows(h, inp["ext"]["rows"], c["aggr"])
                    unit *= 4.0 if c["aggr"] == "mean" else 1.0
                    s_a = 2.0 ** -24 / params[l][1] if params[l][1] else 0.0
                    s_w = 2.0 ** -24 / params[l][2] if params[l][2] else 0.0
                    w = ws[l].numpy().astype(np.float64)
                    # (the fused last layer splits h and W2 only: its reduction runs over p rows in fp32)
                    split = [(h, s_a), (w, s_w)] + ([] if disp["layers"][l].startswith("sage_fused_out") else [(a, s_a)])
                    for v, s in split:
                        exact(v, 0.0 if disp["layers"][l] == "gather_project" else s)
                    if s_a:
                        assert max(np.abs(v).max() for v, s in split if s == s_a) * s_a < 2.0 ** 15.99 and p2(np.abs(w).max()) == s_w
                    b = np.zeros(dims[l + 1]) if bs[l] is None else bs[l].numpy().astype(np.float64)
                    scale = np.abs(a) @ np.abs(w[:, :dims[l]]).T + np.abs(h) @ np.abs(w[:, dims[l]:]).T + np.abs(b)
                    assert scale.max() * unit < 2.0 ** 24, (c["label"], l, scale.max() * unit)
                    pre = a @ w[:, :dims[l]].T + b + h @ w[:, dims[l]:].T
                    assert np.array_equal(pre * unit, np.round(pre * unit))
                    h = np.maximum(pre, 0) if (l < len(dims) - 2 or c["act_last"]) else pre
