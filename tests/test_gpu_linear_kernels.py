"""The dense projection kernels of csrc/agg.hip — linear_split_kernel's live instantiations, and linear_lds_kernel /
linear_mfma_kernel behind GIGL_LINEAR_EXACT — through their four public entry points (gigl_linear, gigl_linear_batched,
gigl_linear_grouped, gigl_sage_project_features), against a float64 product of the very tensors uploaded, at the shapes
where the kernels change path: the wm halves and the partial last row tile, the dword-store epilogue (n % 4 != 0), one and
two 64-column tiles with the second nearly empty, k below one MFMA step, ragged last k-chunks, the two-chunks-ahead
refill, element loads (k % 4 != 0), the XCD tile remap with whole groups and leftover workgroups, operand rows 2^-60 ..
2^60 apart, batch / group indices in grid.y, fp16 and fp32 feature tables up to the multi-chunk loop.  Cases, inputs,
reference, bounds and probes live in tests/linear_cases.py (also the child process of the two knob tests: both knobs
are read once per process).

Every element is judged on its own scale S = sum_k |a||w| + |b|:
    bf16-plane kernels (no half split)   |got - ref| <= 4e-7 S                       (the bound of test_gpu_linear_split.py)
    fp16 table + half-split weights      |got - ref| <= (4e-7 + 2^-21) S + 2^-38 max|w| sum_k |a|
                                         (the kernel comment's weight-plane error max(2^-22 |w|, 2^-39 max|w|), A exact,
                                         with a factor 2, plus the accumulation term)
    GIGL_LINEAR_EXACT kernels            the larger of 4e-7 S and 4 x the scaled error of torch.matmul in float32 on the
                                         same inputs (the factor covers the summation order); nothing comes from the kernel
and every case also runs probes whose answers are exact (selection rows, integer column sums, rows behind m_dev kept
bit for bit, rows before m_dev equal to the m_cap == m_dev run, non-finite rows isolated).  The non-finite probe runs
with act = 0: the activation is `val > 0 ? val : 0`, which turns a NaN into 0.

Measured on an MI355X (worst scaled error max |got - float64| / S of the family's cases, next to the float32 CPU
product's own):

    kernel family (tests/linear_cases.py names)        cases   kernel    float32 reference
    split<1,vec>   linear_split_kernel<1, true>             17   3.8e-07   2.1e-07
    split<2,vec>   linear_split_kernel<2, true>             43   3.5e-07   3.1e-07
    split<1,elem>  linear_split_kernel<1, false>             7   1.9e-07   2.0e-07
    split<2,elem>  linear_split_kernel<2, false>            14   3.4e-07   2.5e-07
    split_y<1>     <1, true>, batch / group in grid.y        5   2.6e-07   2.2e-07
    split_y<2>     <2, true>, batch / group in grid.y        5   3.1e-07   2.8e-07
    ahalf_hs<1>    <1, true, false, true, true>              8   3.0e-07   3.0e-07   (bound 8.8e-07 S + ...)
    ahalf_hs<2>    <2, true, false, true, true>             11   4.1e-07   4.6e-07   (bound 8.8e-07 S + ...)
    ahalf<1>       <1, true, false, true>  (child, bf16)     4   3.0e-07   3.0e-07
    ahalf<2>       <2, true, false, true>  (child, bf16)    11   4.0e-07   4.6e-07   (3.98e-07: next to the bound)
    lds<1>         linear_lds_kernel<1>    (child, exact)    5   1.9e-07   1.9e-07
    lds<2>         linear_lds_kernel<2>    (child, exact)   35   3.3e-07   2.6e-07
    mfma<1>        linear_mfma_kernel<1>   (child, exact)    2   2.0e-07   1.8e-07
    mfma<2>        linear_mfma_kernel<2>   (child, exact)   10   2.5e-07   2.0e-07
(the fp16 tables hold +-65504 next to subnormal halves: the float32 CPU product itself is at 4.6e-07 S there).  Every
exact probe held on every case.  The file: 111 GPU tests (107 cases and 2 row-count checks here, 55 + 18 cases in the two
children) and 4 CPU tests, 8.3 s in all, the two children 2.5 s and 2.3 s, every other test under 0.1 s.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import linear_cases as lc

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gigl_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


# ---- GPU: this process (no knob) ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", lc.default_cases(), ids=lambda c: c["label"].replace(" ", "-"))
def test_projection_case(eng, case):
    r = lc.run_case(eng, case)
    print(lc.format_case(r))
    assert not r["fails"], (lc.format_case(r), r["fails"])


@gpu
@pytest.mark.parametrize("k", [36, 33])
def test_rows_do_not_depend_on_the_row_count(eng, k):
    assert lc.row_independence(eng, k)


# ---- GPU: one fresh child process per knob --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode,var,value", [("exact", "GIGL_LINEAR_EXACT", "1"), ("bf16", "GIGL_GEMM_SPLIT", "bf16")])
def test_knob_cases_in_a_child_process(mode, var, value):
    env = dict(os.environ)
    env.pop("GIGL_LINEAR_EXACT", None)
    env.pop("GIGL_GEMM_SPLIT", None)
    env[var] = value
    p = subprocess.run([sys.executable, os.path.abspath(lc.__file__), mode], env=env, capture_output=True, text=True, timeout=240)
    rows = [json.loads(line[5:]) for line in p.stdout.splitlines() if line.startswith("CASE ")]
    for r in rows:
        print(lc.format_case(r))
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    want = [c["label"] for c in lc.child_cases(mode)]
    assert [r["label"] for r in rows][:len(want)] == want and len(rows) == len(want) + (2 if mode == "exact" else 0)
    bad = [(lc.format_case(r), r["fails"]) for r in rows if r["fails"]]
    assert not bad, bad


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_every_instantiation_has_a_tolerance_case_and_a_probe():
    """from the parametrisation and the restated dispatch rule: every run_case is a tolerance case plus the probes"""
    runs = {"": lc.default_cases(), "exact": lc.child_cases("exact"), "bf16": lc.child_cases("bf16")}
    seen = {k: {c["kernel"] for c in v} for k, v in runs.items()}
    assert {"split<1,vec>", "split<2,vec>", "split<1,elem>", "split<2,elem>", "ahalf_hs<1>", "ahalf_hs<2>", "split_y<1>",
            "split_y<2>"} <= seen[""]
    assert seen["exact"] == {"lds<1>", "lds<2>", "mfma<1>", "mfma<2>"}
    assert {"ahalf<1>", "ahalf<2>"} <= seen["bf16"]
    assert len(lc.INSTANTIATIONS) == 14 and set(lc.INSTANTIATIONS) <= set().union(*seen.values())
    for k, cases in runs.items():
        for kern in seen[k]:
            mine = [c for c in cases if c["kernel"] == kern]
            assert any(md >= 3 for c in mine for _, md, _ in c["spec"]), kern  # (the non-finite probe ran)
            assert any(c["tail"] for c in mine) or all(c["kind"] == "table" for c in mine), kern  # (tables have no m_dev)
    # the rule itself on hand-worked shapes
    assert lc.linear_kernel(36, 64) == "split<1,vec>" and lc.linear_kernel(36, 65) == "split<2,vec>"
    assert lc.linear_kernel(33, 64) == "split<1,elem>" and lc.linear_kernel(1, 257) == "split<2,elem>"
    assert lc.linear_kernel(36, 32, True) == "lds<1>" and lc.linear_kernel(36, 33, True) == "lds<2>"
    assert lc.linear_kernel(5, 32, True) == "mfma<1>" and lc.linear_kernel(5, 33, True) == "mfma<2>"
    assert lc.table_kernel("f16", 36, 32) == "ahalf_hs<1>" and lc.table_kernel("f16", 36, 33) == "ahalf_hs<2>"
    assert lc.table_kernel("f16", 36, 32, "bf16") == "ahalf<1>" and lc.table_kernel("f16", 36, 33, "bf16") == "ahalf<2>"
    assert lc.table_kernel("f16", 6, 33) == "split<2,elem>" and lc.table_kernel("f32", 36, 2) == "split<1,vec>"
    assert lc.table_kernel("f16", 36, 33, "exact") == "lds<2>"
    # the listed shapes are all there, none of them dropped by the de-duplication
    shapes = {s[:3] for s in lc.linear_shapes()}
    m0, k0, n0 = lc.BASE
    assert {(m, k0, n0) for m in lc.M_SWEEP} | {(m0, k0, n) for n in lc.N_SWEEP} | set(lc.REMAP) <= shapes
    assert {(m0, k, n0) for k in lc.K_VEC + lc.K_ELEM} <= shapes
    acts = {(s[3], s[4]) for s in lc.linear_shapes()}
    assert acts == {(0, True), (1, True), (0, False), (1, False)}
    t = {s[:3] for s in lc.table_shapes()}
    r0, d0, o0 = lc.T_BASE
    assert {(r0, d, o0) for d in lc.T_D} | {(r0, d0, o) for o in lc.T_NOUT} | {(r, d0, o0) for r in lc.T_ROWS} | set(lc.T_MULTI) <= t
    assert {s[3] for s in lc.table_shapes() if s[:3] == lc.T_BASE} == set(lc.T_WSCALE)


def test_remap_cases_have_whole_groups_and_leftovers():
    assert lc.remap_ids(1153, 129) == (16, 4)
    assert lc.remap_ids(1153, 64) == (8, 2)
    assert lc.remap_ids(2048, 257) == (48, 0)
    assert lc.remap_ids(*lc.BASE[::2]) == (0, 2)  # (small grids keep the plain mapping)
    assert all(lc.remap_ids(m, n)[1] > 0 for m, _, n in lc.REMAP[:2])
    assert all(lc.remap_ids(m, n)[0] > 0 for m, _, n in lc.REMAP)


def test_reference_and_bounds_are_the_stated_ones():
    g = torch.Generator().manual_seed(5)
    a, w, b = torch.randn(37, 19, generator=g), torch.randn(11, 19, generator=g), torch.randn(11, generator=g)
    want = F.linear(a.double(), w.double(), b.double())
    assert (lc.reference(a, w, b, 0) - want).abs().max().item() <= 1e-12
    assert (lc.reference(a, w, b, 1) - want.clamp(min=0)).abs().max().item() <= 1e-12
    assert (lc.reference(a.half(), w, None, 0) - F.linear(a.half().double(), w.double())).abs().max().item() <= 1e-12
    s = lc.scale_of(a, w, b)
    assert (s - F.linear(a.double().abs(), w.double().abs(), b.double().abs())).abs().max().item() <= 1e-12
    assert (lc.scale_of(a, w, None) - F.linear(a.double().abs(), w.double().abs())).abs().max().item() <= 1e-12
    bound, rel = lc.bound_of("split", s, a, w, 1.0)
    assert rel == 4e-7 and torch.equal(bound, 4e-7 * s)
    bound, rel = lc.bound_of("hs", s, a, w, 1.0)
    want = (4e-7 + 2.0 ** -21) * s + 2.0 ** -38 * w.abs().max().item() * a.double().abs().sum(1).unsqueeze(1)
    assert rel == 4e-7 + 2.0 ** -21 and (bound - want).abs().max().item() <= 1e-12 * want.max().item()
    assert lc.bound_of("exact", s, a, w, 1e-9)[1] == 4e-7 and lc.bound_of("exact", s, a, w, 3e-7)[1] == 4 * 3e-7
    # the scaled error: a known perturbation of one element, and a non-finite value
    got = want = lc.reference(a, w, b, 0)
    got = got.clone()
    got[3, 4] += 1e-3 * s[3, 4]
    assert abs(lc.scaled_err(got, want, s) - 1e-3) < 1e-9
    got[0, 0] = float("nan")
    assert lc.scaled_err(got, want, s) == float("inf")
    assert lc.scaled_err(lc.fp32_product(a, w, b, 1), lc.reference(a, w, b, 1), s) < 4e-7


def test_operand_splits_are_exact_on_every_input():
    """numpy emulation of split3 and of hsplit_store with hs_pow2_scale over every tensor the GPU cases upload: the bf16
    planes sum back to the input exactly and none is subnormal, the probes' integers sit in the first plane alone, fp16
    rows need two planes, the half-split residual is within max(2^-22 |x|, 2^-39 max|x|)"""
    tiny = float(np.finfo(np.float32).tiny)

    def planes_ok(x, first_only=False, two=False):
        x = x.float().numpy()
        b1, b2, b3 = lc.split3_np(x)
        assert np.array_equal(b1.astype(np.float64) + b2.astype(np.float64) + b3.astype(np.float64), x.astype(np.float64))
        for p in (b1, b2, b3):
            assert not ((p != 0) & (np.abs(p) < tiny)).any()
        if first_only:
            assert not b2.any() and not b3.any()
        if two:
            assert not b3.any()

    assert lc.hs_pow2_scale_np(1.0) == 2.0 ** 14 and lc.hs_pow2_scale_np(251.0) == 2.0 ** 7
    assert lc.hs_pow2_scale_np(2.0 ** -100) == 2.0 ** 60 and lc.hs_pow2_scale_np(3e38) == 2.0 ** -60
    seen = set()
    for case in lc.default_cases():  # (the children upload the same tensors: same labels' shapes, same seeds)
        key = (case["kind"] == "table", case.get("a_kind"), case.get("wscale"), case.get("shared_a"), case["k"], case["n"],
               tuple(case["spec"]))
        if key in seen:
            continue
        seen.add(key)
        inp = lc.case_inputs(case)
        half = case.get("a_kind") == "f16"
        for a in inp["a"]:
            planes_ok(a, two=half)
        for w in inp["w"]:
            planes_ok(w)
        for t in inp["sel_a"] + inp["ones_a"] + [inp["w_int"]]:
            planes_ok(t, first_only=True)
        assert float(inp["w_int"].max()) <= 251 and float(inp["w_int"].sum(1).max() + 48) < 2 ** 24
        if half and case["k"] % 4 == 0:
            for w in inp["w"] + [inp["w_int"]]:
                x = w.numpy().astype(np.float64)
                top = np.abs(x).max()
                s = lc.hs_pow2_scale_np(top)
                assert 2.0 ** 14 <= top * s < 2.0 ** 15
                h1, h2 = lc.hsplit_np(w.numpy(), s)
                resid = np.abs(x - (h1 + h2) / s)
                assert (resid <= np.maximum(2.0 ** -22 * np.abs(x), 2.0 ** -39 * top)).all()
                if w is inp["w_int"]:
                    assert not h2.any() and np.array_equal(h1 / s, x)
