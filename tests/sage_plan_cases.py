"""TEST INFRASTRUCTURE ONLY: the cases, inputs, float64 reference, per-element bounds and exact probes of
tests/test_gpu_sage_plan_layers.py, plus a plain-Python mirror of the GraphSAGE plan's dispatch rule (csrc/pipeline.hip
step_sage_reduce / step_sage_project / fused2_on / plan_refresh_half_split) and of the half-split scales the library derives on the device
(hs_scale_kernel, hs_chain_kernel, fused2_scale_kernel in csrc/agg.hip).

Run as a program (`python tests/sage_plan_cases.py hs_layers|bf16|f2_all_wr`) it is the CHILD of the knob tests:
GIGL_PLAN_HS_LAYERS, GIGL_GEMM_SPLIT and GIGL_F2_ALL_WR are read once per process, so the parent sets one of them in the
child's environment; the child runs that knob's cases once and prints one line `CASE {json}` per case (label, kernels,
err, fp32, ratio, eps, fails, digest).  Under GIGL_F2_ALL_WR the fused projection must give the very rows it gives without:
that child prints each fused case's digest, and the parent compares it with its own run of the case.

Reference.  A plain float64 formula over the very tensors uploaded, row by row over an edge list:
    h_{l+1}[i] = act( reduce_{j -> i} h_l[j] . W_l^T + b + h_l[i] . W_r^T ),   reduce = mean | sum | max (0 for no edge)
on the plan's OWN union graph (SagePlan.last_batch_to_host), every layer over every node of it, then the optional
x / max(|x|_2, 1e-12).  An fp16 table is widened exactly.

Bound, per element and carried through the layers.  With A = reduce(H), RA = reduce(|H|) (max: |A|), EH the bound of the
previous layer's rows (0 for the table) and n_i the number of edges of row i:
    RE = reduce(EH) + n_i 2^-24 RA                          (the fp32 reduction; nothing for max)
    S  = RA |W_l|^T + |H| |W_r|^T + |b|                     the element's own scale
    P  = RE |W_l|^T + EH |W_r|^T                            what the operand's error can do (relu is 1-Lipschitz)
    E  = eps (S + P) + P + fa sum_k |w_k| + fw sum_k (|a_k| + its error)
  bf16-plane kernels        eps = 4e-7 (the bound of test_gpu_linear_kernels.py), fa = fw = 0: the three planes are exact
  half split                every operand element carries max(2^-22 |x|, 2^-25 / s) with s the operand's power-of-two
                            scale (the plane below the second is a subnormal half: the kernels' "2^-39 max|x|"), taken
                            with the factor 2 of test_gpu_linear_kernels.py: eps = 4e-7 + 2^-20 + 2^-22 (both operands,
                            the dropped low x low product), fa = 2^-24 / s_a, fw = 2^-24 / s_w
  fused second product      the same with s_h from B = K max|W1| max|a| + max|b1| as fused2_scale_kernel bounds it,
                            recomputed here from the inputs, plus 2^-22 for the fp32 reduction's epilogue
  under a sum               no fan-out bounds a union row (it merges the samples of every occurrence of its node): the
                            library measures the summed half of the operand on the device; here its largest magnitude
                            comes from the float64 reference of the same rows
  projected input           eps = 4e-7 + 2^-22 (the bf16-plane projection of the table, then one fp32 reduction)
The scales s are recomputed from the inputs the way the kernels do; nothing comes from a kernel's output.  Every eps is
below 1e-5: a missing plane product costs ~2^-12 S and fails.
"""
import functools
import hashlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import linear_cases as lc  # noqa: E402  (split3_np, hsplit_np, hs_pow2_scale_np)

U = 2.0 ** -24
EPS_BF16 = 4e-7
EPS_HS = 4e-7 + 2.0 ** -20 + 2.0 ** -22
EPS_F2 = EPS_HS + 2.0 ** -22
EPS_PROJ = EPS_BF16 + 2.0 ** -22
META_LEVEL0, META_OVERFLOW = 2, 8

N_NODES = 640
HUB, HUB_DEG = 0, 40
DEGS = [0, 1, 2, 3, 5, 5, 9, 14]  # in-degree of node v by v % 8 (the first fan-out is 5), + the hub for v % 8 in (3, 6)
FAN2, FAN3 = [5, 3], [3, 2, 2]
POW2_FAN2, POW2_FAN3 = [4, 4], [4, 4, 4]

KERNELS = [
    # the fused pair of layers
    "linear_fused2x", "fused2_images", "fused2_scale", "sage_fused_out<MEAN>", "sage_fused_out<SUM>",
    # linear_split_kernel<NJ, ...> reached through linear_tiled_strided only
    "tiled_bf16<1>", "tiled_bf16<2>", "ts_bf16<1>", "ts_bf16<2>", "ts_hs<1>", "ts_hs<2>", "ts_hs_selfhalf<1>",
    "ts_hs_selfhalf<2>",
    "hs_chain", "gather_tiled", "gather_project", "l2_normalize",
]


# ---- graphs ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph(kind: str):
    """(rowptr, col, largest in-degree) of a CSC by destination.  "main": in-degrees 0, 1, 2, 3, exactly the first fan-out,
    10 and 14, and a hub of 40 in-edges that is itself an in-neighbour of every fourth node (reached from many roots at hop
    0, and at hop 1 through them).  "pow2": every in-degree is 1, 2 or 4 <= every fan-out used with it, so a union row IS
    the node's row and a mean divides by a power of two."""
    import oracle
    src, dst = [], []
    n = N_NODES
    if kind == "main":
        for v in range(1, n):
            for j in range(DEGS[v % 8]):
                src.append((v * 17 + 31 * j + 1) % n)
                dst.append(v)
            if v % 8 in (3, 6):
                src.append(HUB)
                dst.append(v)
        for j in range(HUB_DEG):
            src.append(n - HUB_DEG + j)
            dst.append(HUB)
    else:
        assert kind == "pow2", kind
        for v in range(n):
            for j in range([1, 2, 4][v % 3]):
                src.append((v * 17 + 31 * j + 1) % n)
                dst.append(v)
    rowptr, col = oracle.build_csc(n, np.array(src, np.uint32), np.array(dst, np.uint32), is_directed=True)
    return rowptr, col, int(np.diff(rowptr).max())


def roots_of(kind: str, groups: int = 1) -> np.ndarray:
    """partial: 5 roots, one twice (a single partial 128-row tile).  inside: 200 roots with duplicates (the roots end
    inside the second tile).  edge: 256 distinct roots (the roots end on a tile edge).  wide: 300 distinct roots.
    few: 5 distinct roots repeated to 300.  groups: 64 roots per batch.  small: 7 roots, one twice."""
    if kind == "partial":
        r = np.array([3, 10, 3, 17, 26], np.uint32)
    elif kind == "inside":
        r = (np.arange(200) * 3 + 2) % N_NODES
        r[7], r[150] = r[3], r[3]
    elif kind == "edge":
        r = np.arange(256) + 2
    elif kind == "wide":
        r = np.arange(300) * 2 + 1
    elif kind == "few":
        r = np.tile(np.array([6, 18, 30, 42, 54]), 60)
    elif kind == "hubroot":  # the hub is a root too: its row merges its own sample with one sample per root it is sampled for
        r = (np.arange(200) * 3 + 2) % N_NODES
        r[0] = HUB
    elif kind == "smallhub":
        r = np.array([2, 6, 10, 14, 18, 22, 3, HUB], np.uint32)
    elif kind == "small":
        r = np.array([2, 6, 10, 14, 18, 22, 3, 2], np.uint32)
    else:
        assert kind == "groups", kind
        r = (np.arange(64 * groups) * 7 + 2) % N_NODES
    return np.ascontiguousarray(r, dtype=np.uint32)


# ---- cases ----------------------------------------------------------------------------------------------------------
def _case(label, **kw):
    c = dict(label=label, kind="tol", table="f32", d_in=36, hidden=[256], n_out=47, aggr="mean", bias=True, act_last=False,
             groups=1, roots="inside", l2=False, no_fuse2=False, proj=False, tkind="normal", tscale=0, wscale=0,
             bkind="normal", graph="main", fan=None)
    c.update(kw)
    if c["fan"] is None:
        pow2 = c["graph"] == "pow2"
        c["fan"] = {1: (POW2_FAN2 if pow2 else FAN2), 2: (POW2_FAN3 if pow2 else FAN3)}[len(c["hidden"])]
    assert len(c["fan"]) == len(c["hidden"]) + 1
    return c


F_DIN = [4, 12, 16, 36, 44, 100, 128, 260]
F_NOUT = [1, 47, 48]


def fused_cases():
    out = [_case("fused d%d" % d, d_in=d) for d in F_DIN]
    out += [_case("fused out%d" % n, n_out=n, bias=(n != 1), act_last=(n == 48)) for n in F_NOUT if n != 47]
    out += [_case("fused nobias", bias=False), _case("fused act_last", act_last=True),
            _case("fused sum", aggr="sum"), _case("fused sum d100 act_last nobias", aggr="sum", d_in=100, act_last=True, bias=False),
            _case("fused groups3", groups=3, roots="groups"), _case("fused groups3 sum d12", groups=3, roots="groups", aggr="sum", d_in=12),
            _case("fused partial", roots="partial"), _case("fused partial sum d4 out1", roots="partial", aggr="sum", d_in=4, n_out=1),
            _case("fused edge", roots="edge"), _case("fused edge d100 out48", roots="edge", d_in=100, n_out=48),
            _case("fused l2", l2=True), _case("fused l2 sum out48", l2=True, aggr="sum", n_out=48),
            _case("fused 2^-20", tscale=-20, wscale=-20), _case("fused 2^20", tscale=20, wscale=20),
            _case("fused 2^20 sum", tscale=20, wscale=-20, aggr="sum"), _case("fused rows 2^-8 apart", tkind="apart8"),
            _case("fused sum headroom", aggr="sum", tkind="edge"), _case("fused sum headroom d100", aggr="sum", tkind="edge", d_in=100)]
    return out


def apart_cases():
    out = []
    for hid in (64, 132):
        for layers in (2, 3):
            for i, aggr in enumerate(("mean", "sum", "max")):
                tab = "f16" if (i + layers + (hid == 132)) % 2 else "f32"
                out.append(_case("apart h%d L%d %s %s" % (hid, layers, aggr, tab), hidden=[hid] * (layers - 1), aggr=aggr,
                                 table=tab, n_out=(47 if hid == 64 else 70), roots=("small" if layers == 3 else "inside"),
                                 act_last=(aggr == "max")))
    # both table kinds at both widths on the two-layer mean (the self-half instantiations, NJ 1 and 2)
    out += [_case("apart h%d L2 mean %s d100" % (hid, tab), hidden=[hid], table=tab, d_in=100, n_out=(33 if hid == 64 else 129))
            for hid in (64, 132) for tab in ("f32", "f16")]
    # tables that decline the half split: every layer on the bf16 planes (fp16: the first layer's operand is [mean | self])
    out += [_case("apart outlier h%d L%d %s %s" % (hid, layers, aggr, tab), hidden=[hid] * (layers - 1), table=tab, aggr=aggr,
                  tkind="outlier", n_out=(47 if hid == 64 else 70), roots=("small" if layers == 3 else "inside"))
            for hid, layers, aggr, tab in [(64, 2, "mean", "f32"), (132, 3, "sum", "f32"), (132, 2, "max", "f16"),
                                           (64, 3, "mean", "f16"), (256, 2, "mean", "f32")]]
    # the fused shape with the layers apart (read at plan creation), magnitudes, the sum's headroom, the row-major path
    out += [_case("apart h256 nofuse", no_fuse2=True), _case("apart h256 nofuse sum edge", no_fuse2=True, aggr="sum", roots="edge"),
            _case("apart h64 2^-20", hidden=[64], tscale=-20, wscale=-20), _case("apart h132 L3 2^20 f16", hidden=[132, 132],
                                                                                 table="f16", tscale=10, wscale=20, roots="small"),
            _case("apart h64 rows 2^-8 apart", hidden=[64], tkind="apart8"),
            _case("apart h64 sum headroom", hidden=[64], aggr="sum", tkind="edge"),
            # ... and the layers behind: hidden rows next to the bound hs_chain_kernel derives, summed over the hub's row
            _case("apart h64 sum headroom hidden", hidden=[64], aggr="sum", tkind="edge", bkind="edge", roots="hubroot"),
            _case("apart h132 L3 sum headroom hidden", hidden=[132, 132], aggr="sum", tkind="edge", bkind="edge", roots="smallhub",
                  fan=[5, 3, 2]),
            _case("apart h132 L3 sum headroom f16", hidden=[132, 132], aggr="sum", tkind="edge", table="f16", roots="small",
                  fan=[5, 3, 2]),
            _case("apart h64 l2 groups3", hidden=[64], l2=True, groups=3, roots="groups"),
            _case("apart rowmajor d6", hidden=[64], d_in=6)]
    out += [_case("proj h64 mean", hidden=[64], proj=True), _case("proj h256 sum", proj=True, aggr="sum", n_out=48),
            _case("proj h132 L3 mean", hidden=[132, 132], proj=True, roots="small", n_out=70)]
    return out


def _probe(label, **kw):
    kw.setdefault("tkind", "int")
    kw.setdefault("roots", "small")
    return _case(label, kind=kw.pop("kind", "int"), **kw)


def probe_cases():
    """exact probes: integer tables / weights / biases (sum on the main graph, mean where every degree is a power of
    two), the column identity, history independence; repeatability rides on every run"""
    out = [_probe("int fused sum", aggr="sum", roots="inside"), _probe("int fused mean", graph="pow2", roots="inside"),
           _probe("int fused sum groups3 nobias", aggr="sum", groups=3, roots="groups", bias=False, d_in=44, n_out=48),
           _probe("int fused mean l2 out1", graph="pow2", n_out=1, l2=True)]
    for tab in ("f32", "f16"):
        for tk in ("int", "int_outlier"):
            out.append(_probe("int apart h64 L2 sum %s %s" % (tab, tk), hidden=[64], aggr="sum", table=tab, tkind=tk))
            aggr = "mean" if tk == "int" else "max"  # (the outlier's sums leave 2^24 sixty-fourths after three means)
            out.append(_probe("int apart h68 L3 %s %s %s" % (aggr, tab, tk), hidden=[68, 68], graph="pow2", table=tab, tkind=tk,
                              n_out=70, aggr=aggr))
    out += [_probe("int apart h256 nofuse sum", no_fuse2=True, aggr="sum", roots="inside"),
            _probe("int apart h64 max l2 out1", hidden=[64], aggr="max", n_out=1, l2=True),
            _probe("int proj h64 sum", hidden=[64], proj=True, aggr="sum"),
            _probe("int proj h68 L3 mean", hidden=[68, 68], proj=True, graph="pow2", n_out=70),
            _probe("colid fused", kind="colid", aggr="sum", n_out=48, roots="inside"),
            _probe("colid apart h64", kind="colid", aggr="sum", n_out=48, hidden=[64], roots="inside"),
            _probe("history fused", kind="history", tkind="normal", roots="wide"),
            _probe("history apart h64", kind="history", tkind="normal", roots="wide", hidden=[64])]
    return out


def default_cases():
    return fused_cases() + apart_cases()


def child_cases(mode: str):
    if mode == "hs_layers":  # layers >= 1 stay on the bf16 planes, the first keeps the half split
        return [_case("child hs_layers h64 L2 mean", hidden=[64]), _case("child hs_layers h132 L3 sum f16", hidden=[132, 132],
                                                                         aggr="sum", table="f16", roots="small", n_out=70),
                _case("child hs_layers h256 nofuse", no_fuse2=True), _case("child hs_layers fused", d_in=44),
                _probe("child hs_layers int h64 sum", hidden=[64], aggr="sum")]
    if mode == "f2_all_wr":  # every case that runs the fused pair of layers: the rows must not depend on the knob
        return fused_cases() + [c for c in probe_cases() if " fused" in c["label"]]
    assert mode == "bf16", mode  # no half split anywhere: no fused layers, fp16 tables take the [mean | self] operand
    return [_case("child bf16 h256 d36"), _case("child bf16 h256 sum f16", aggr="sum", table="f16"),
            _case("child bf16 h64 L2 f16", hidden=[64], table="f16"), _case("child bf16 h132 L3 max", hidden=[132, 132],
                                                                            aggr="max", roots="small", n_out=70),
            _probe("child bf16 int h64 sum f16", hidden=[64], aggr="sum", table="f16")]


# ---- the dispatch rule, restated ------------------------------------------------------------------------------------
def dims_of(case):
    return [case["d_in"]] + list(case["hidden"]) + [case["n_out"]]


def table_takes_half_split(x: torch.Tensor) -> bool:
    """gigl_feat_half_split_scale: the largest magnitude inside [2^-46, 2^74], finite, and the mean non-zero magnitude no
    more than 2^10 below the largest"""
    a = np.abs(x.float().numpy().astype(np.float64))
    if not np.isfinite(a).all() or not a.any():
        return False
    top = float(np.float32(a.max()))
    return 2.0 ** -46 <= top <= 2.0 ** 74 and a.sum() / np.count_nonzero(a) >= a.max() * 2.0 ** -10


def dispatch(case, x: torch.Tensor, knob: str = ""):
    """{"hs0", "fused", "layers": [kernel of layer l's projection], "kernels": set of KERNELS the run launches}.
    knob: "" | "hs_layers" (GIGL_PLAN_HS_LAYERS=0) | "bf16" (GIGL_GEMM_SPLIT=bf16)"""
    dims = dims_of(case)
    hops = len(dims) - 1
    f16 = case["table"] == "f16"
    tiled = all(d % 4 == 0 and d <= 2048 for d in dims[:hops])
    hs0 = tiled and knob != "bf16" and table_takes_half_split(x)
    proj = case["proj"]
    fused = (hops == 2 and dims[1] == 256 and 1 <= dims[2] <= 48 and dims[0] % 4 == 0 and dims[0] >= 4 and not case["no_fuse2"]
             and tiled and hs0 and not proj and not f16 and case["aggr"] in ("mean", "sum"))
    layers, kern = [], set()
    for l in range(hops):
        nj = 2 if dims[l + 1] > 64 else 1
        if l == 0 and proj:
            layers.append("gather_project")
            kern.add("gather_project")
            continue
        if fused:
            layers.append("linear_fused2x" if l == 0 else "sage_fused_out<%s>" % case["aggr"].upper())
            kern |= {"linear_fused2x", "fused2_images", "fused2_scale", "sage_fused_out<%s>" % case["aggr"].upper(), "gather_tiled"}
            continue
        if not tiled:
            layers.append("rowmajor<%d>" % nj)
            continue
        kern.add("gather_tiled")
        self_half = l == 0 and hs0 and f16
        two_src = l > 0 or not f16 or self_half
        if l >= 1 and hs0 and not proj and knob != "hs_layers":
            layers.append("ts_hs<%d>" % nj)
            kern.add("hs_chain")
        elif two_src:
            hs = l == 0 and hs0
            layers.append(("ts_hs_selfhalf<%d>" if hs and self_half else "ts_hs<%d>" if hs else "ts_bf16<%d>") % nj)
        else:
            layers.append("tiled_bf16<%d>" % nj)
        kern.add(layers[-1])
    if case["l2"]:
        kern.add("l2_normalize")
    return dict(hs0=hs0, fused=fused, layers=layers, kernels=kern, tiled=tiled)


def layer_params(case, disp, x, weights, biases, amax):
    """[(eps, fa, fw)] per layer, the half-split scales recomputed the way the kernels derive them.  amax[l]: the largest
    |reduce_j h_j| of layer l from the float64 reference — under a sum the library measures that half of the operand on
    the device (gigl_tiled_absmax) instead of bounding it, since no fan-out bounds a union row"""
    dims = dims_of(case)
    p2 = lc.hs_pow2_scale_np
    f32 = lambda v: float(np.float32(v))
    wmax = [float(w.abs().max()) for w in weights]
    bmax = [0.0 if b is None else float(b.abs().max()) for b in biases]
    summed = case["aggr"] == "sum"
    tmax = float(np.float32(x.float().abs().max()))
    first = (p2(f32(max(tmax, amax[0]) if summed else tmax)), p2(wmax[0]))  # (hs_scale_kernel)
    out, prev = [], None
    for l, name in enumerate(disp["layers"]):
        if name == "gather_project":
            out.append((EPS_PROJ, 0.0, 0.0))
        elif name.startswith("ts_hs") and l == 0 or name == "linear_fused2x":
            out.append((EPS_HS, 2.0 ** -24 / first[0], 2.0 ** -24 / first[1]))
            prev = first
        elif name.startswith("sage_fused_out"):  # (fused2_scale_kernel)
            b = f32(2 * dims[0] * 2.0 ** 30 / prev[0] / prev[1] + bmax[0])
            out.append((EPS_F2, 2.0 ** -24 / (p2(b) * 0.5), 2.0 ** -24 / p2(wmax[1])))
        elif name.startswith("ts_hs"):  # (a layer >= 1: hs_chain_kernel, chained from the first layer's scales)
            b = f32(2 * dims[l - 1] * 2.0 ** 30 / prev[0] / prev[1] + bmax[l - 1])
            if summed:
                b = max(b, f32(amax[l]))
            prev = (p2(b) * 0.5, p2(wmax[l]))
            out.append((EPS_HS, 2.0 ** -24 / prev[0], 2.0 ** -24 / prev[1]))
        else:
            out.append((EPS_BF16, 0.0, 0.0))
            prev = first if l == 0 else prev
    return out


def params_of(case, disp, x, weights, biases, ext):
    amax = forward(case, x.float().numpy().astype(np.float64), ext, weights, biases)["amax"]
    return layer_params(case, disp, x, weights, biases, amax)


# ---- inputs (CPU tensors; the very ones that are uploaded) ----------------------------------------------------------
def _rng(case, salt: int):
    return np.random.default_rng([abs(hash_label(case["label"])) % (1 << 31), salt])


def hash_label(s: str) -> int:
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) % 1000000007
    return h


def draw_rows(case, rng, rows: int) -> np.ndarray:
    d, tk = case["d_in"], case["tkind"]
    if tk in ("int", "int_outlier"):
        return rng.integers(-8 if tk == "int" else -2, 9 if tk == "int" else 3, size=(rows, d)).astype(np.float32)
    if tk == "edge":  # fan x max|x| just under a power of two, every value next to the largest and of one sign
        return (1.59 * (1 - 0.1 * rng.random((rows, d)))).astype(np.float32)
    x = rng.standard_normal((rows, d)) / 4
    if tk == "outlier":
        x = x * 2.0 ** -11
    return (x * 2.0 ** case["tscale"]).astype(np.float32)


def make_table(case, rng) -> np.ndarray:
    x = draw_rows(case, rng, N_NODES)
    tk = case["tkind"]
    if tk == "apart8":
        x = x * (2.0 ** -(np.arange(N_NODES) % 9)).astype(np.float32)[:, None]
    if tk == "edge":
        x[5, 0] = 1.59
    if tk == "outlier":
        x[3, 1], x[77, 0], x[HUB, 2] = 4.0 * 2.0 ** case["tscale"], -4.0 * 2.0 ** case["tscale"], 4.0 * 2.0 ** case["tscale"]
    if tk == "int_outlier":
        x[3, 1] = 2048.0
    return x


def make_weights(case, rng):
    dims = dims_of(case)
    ws, bs = [], []
    integer = case["tkind"].startswith("int")
    for l in range(len(dims) - 1):
        if integer:
            w = rng.integers(-2, 3, size=(dims[l + 1], 2 * dims[l])).astype(np.float32)
            b = rng.integers(-3, 4, size=dims[l + 1]).astype(np.float32)
        else:
            sc = 2.0 ** case["wscale"]
            w = (rng.standard_normal((dims[l + 1], 2 * dims[l])) / math.sqrt(2 * dims[l]) * sc).astype(np.float32)
            w[0] *= 1e-3  # (a row far below the largest weight)
            b = (rng.standard_normal(dims[l + 1]) * 0.1 * 2.0 ** case["tscale"] * sc ** (l + 1)).astype(np.float32)
            if case["bkind"] == "edge" and l < len(dims) - 2:  # every hidden row next to the bound K max|w| max|a| + max|b| that
                b = (3000.0 * (1 - 0.1 * rng.random(dims[l + 1]))).astype(np.float32)  # hs_chain_kernel derives: a large bias
        ws.append(torch.from_numpy(w))
        bs.append(torch.from_numpy(b) if case["bias"] else None)
    return ws, bs


def first_table(case) -> torch.Tensor:
    """the table as first drawn (before any row is redrawn for the relu margins): what the dispatch rule looks at"""
    return to_table(case, make_table(case, _rng(case, 1)))


def to_table(case, x: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.half() if case["table"] == "f16" else t


def oracle_ext(case):
    """the union graph(s) of the case from the CPU oracle, as an extended node list: (nid [n] table row of node i,
    rows [(i, sources)], root_idx [b], keys: sorted (dst_global << 32 | src_global) of every edge, meta per group)"""
    import oracle
    rowptr, col, _ = graph(case["graph"])
    roots = roots_of(case["roots"], case["groups"])
    G = case["groups"]
    b = roots.size // G
    nid, rows, root_idx, keys, metas, off = [], [], [], [], [], 0
    for g in range(G):
        r = roots[g * b:(g + 1) * b]
        nbr, _ = oracle.sample_khop(rowptr, col, r, case["fan"], canonical=True)
        o = oracle.union_build(r, case["fan"], nbr)
        nn = int(o["meta"][0])
        nid.append(o["nodes"].astype(np.int64))
        for i in range(nn):
            js = o["col"][o["rowptr"][i]:o["rowptr"][i + 1]].astype(np.int64)
            if js.size:
                rows.append((off + i, off + js))
                keys.append((int(o["nodes"][i]) << 32) | o["nodes"][js].astype(np.int64))
        root_idx.append(off + o["root_local"].astype(np.int64))
        metas.append(o["meta"].copy())
        off += nn
    keys = np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    return dict(nid=np.concatenate(nid), rows=rows, root_idx=np.concatenate(root_idx), keys=keys, metas=metas)


def plan_ext(case, hb):
    """the same view of the plan's own union graph (SagePlan.last_batch_to_host).  Plans of up to two hops keep pure leaves
    as GLOBAL ids in the rows of the last computed level: those sources become extra nodes behind the local ones"""
    hops = len(case["fan"])
    meta = hb["meta"]
    nn = int(meta[0])
    n_rows = int(meta[META_LEVEL0 + hops - 1])  # nodes of level < hops: the rows that have in-edges
    leaf_global = hops <= 2
    n_local_rows = (int(meta[META_LEVEL0 + hops - 2]) if hops >= 2 else 0) if leaf_global else n_rows
    nodes = hb["nodes"].astype(np.int64)
    nid = np.concatenate([nodes, np.arange(N_NODES, dtype=np.int64)]) if leaf_global else nodes
    rows, keys = [], []
    for i in range(n_rows):
        js = hb["col"][hb["rowptr"][i]:hb["rowend"][i]].astype(np.int64) & 0xFFFFFFFF
        if not js.size:
            continue
        if i >= n_local_rows:
            if js.max() >= N_NODES:
                return None
            js = nn + js
        elif js.max() >= nn:
            return None
        rows.append((i, js))
        keys.append((int(nodes[i]) << 32) | nid[js])
    keys = np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    return dict(nid=nid, rows=rows, root_idx=hb["root_local"].astype(np.int64), keys=keys,
                n_roots=int(meta[META_LEVEL0]), n_rows=n_rows,
                computed=[int(meta[META_LEVEL0 + hops - 1 - l]) for l in range(hops)])


# ---- reference and bounds -------------------------------------------------------------------------------------------
def reduce_rows(h: np.ndarray, rows, aggr: str):
    """(reduce_{j -> i} h[j], edges of row i) over the edge list, one segment of it per row (rows: [(i, sources)], none
    of them empty); a row without edges reduces to 0"""
    out = np.zeros_like(h)
    cnt = np.zeros(h.shape[0])
    if not rows:
        return out, cnt
    dst = np.array([i for i, _ in rows])
    lens = np.array([js.size for _, js in rows])
    v = h[np.concatenate([js for _, js in rows])]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    out[dst] = np.maximum.reduceat(v, starts, axis=0) if aggr == "max" else np.add.reduceat(v, starts, axis=0)
    if aggr == "mean":
        out[dst] /= lens[:, None].astype(h.dtype)
    cnt[dst] = lens
    return out, cnt


def forward(case, x: np.ndarray, ext, weights, biases, params=None, dtype=np.float64):
    """the forward over every node of ext in `dtype`; with params ([(eps, fa, fw)] per layer) also the per-element
    bounds.  -> dict(y [b, n_out], pre [per layer], E [per layer], S (last layer's scale), bound [b, n_out])"""
    dims = dims_of(case)
    hops = len(dims) - 1
    aggr = case["aggr"]
    h = x[ext["nid"]].astype(dtype)
    eh = np.zeros_like(h, dtype=np.float64)
    pres, errs, amax = [], [], []
    s = None
    for l in range(hops):
        d = dims[l]
        w = weights[l].numpy().astype(dtype)
        wl, wr = w[:, :d], w[:, d:]
        b = np.zeros(dims[l + 1], dtype) if biases[l] is None else biases[l].numpy().astype(dtype)
        a, cnt = reduce_rows(h, ext["rows"], aggr)
        pre = a @ wl.T + b + h @ wr.T
        amax.append(float(np.abs(a).max()) if a.size else 0.0)
        act = l < hops - 1 or case["act_last"]
        if params is not None:
            eps, fa, fw = params[l]
            ah = np.abs(h).astype(np.float64)
            ra = np.abs(a).astype(np.float64) if aggr == "max" else reduce_rows(ah, ext["rows"], aggr)[0]
            re = reduce_rows(eh, ext["rows"], aggr)[0]
            if aggr != "max":
                re = re + cnt[:, None] * U * ra
            awl, awr = np.abs(wl).astype(np.float64), np.abs(wr).astype(np.float64)
            s = ra @ awl.T + ah @ awr.T + np.abs(b).astype(np.float64)
            p = re @ awl.T + eh @ awr.T
            floor = fa * (awl.sum(1) + awr.sum(1))[None, :] + fw * ((ra + re).sum(1) + (ah + eh).sum(1))[:, None]
            eh = eps * (s + p) + p + floor
            errs.append(eh)
        pres.append(pre)
        h = np.maximum(pre, 0) if act else pre
    r = ext["root_idx"]
    y = h[r]
    out = dict(y=y, pre=pres, E=errs, amax=amax)
    if params is not None:
        bound, sc = eh[r], s[r]
        if case["l2"]:
            ny = np.sqrt((y.astype(np.float64) ** 2).sum(1, keepdims=True))
            ne = np.sqrt((bound ** 2).sum(1, keepdims=True))
            den = np.maximum(ny - ne, 1e-300)
            bound = np.where(ny > 1e-12, (bound + np.abs(y) / np.maximum(ny, 1e-300) * ne) / den + 2.0 ** -21 * np.abs(y) / np.maximum(ny, 1e-300), np.inf)
            sc = sc / np.maximum(ny, 1e-300)
        out.update(bound=bound, S=sc)
    if case["l2"]:
        ny = np.sqrt((y ** 2).sum(1, keepdims=True))
        out["y"] = y / np.maximum(ny, dtype(1e-12))
    return out


def margin_offenders(case, res, computed=None):
    """nodes with a pre-activation within its own bound of zero, over every layer whose activation is on.  computed[l]:
    the plan computes layer l for the first computed[l] nodes only (level <= hops - 1 - l, numbered level by level); the
    rows behind them are never read (on the plan's own graph they are not even the union's: leaf sources stand there as
    bare table rows)"""
    hops = len(case["fan"])
    bad = set()
    for l in range(hops):
        if l < hops - 1 or case["act_last"]:
            n = None if computed is None else computed[l]
            bad |= set(np.nonzero((np.abs(res["pre"][l][:n]) <= res["E"][l][:n]).any(1))[0].tolist())
    return sorted(bad)


@functools.lru_cache(maxsize=8)
def _inputs(key: str, knob: str):
    case = json.loads(key)
    ext = oracle_ext(case)
    rng = _rng(case, 1)
    x = make_table(case, rng)
    ws, bs = make_weights(case, _rng(case, 2))
    redraws = 0
    if case["kind"] in ("tol", "history"):
        for _ in range(40):  # no hidden pre-activation within its own bound of zero: redraw the offending nodes' rows
            xt = to_table(case, x)
            disp = dispatch(case, xt, knob)
            res = forward(case, xt.float().numpy().astype(np.float64), ext, ws, bs, params_of(case, disp, xt, ws, bs, ext))
            bad = margin_offenders(case, res)
            if not bad:
                break
            ids = np.unique(ext["nid"][bad])
            x[ids] = draw_rows(case, rng, ids.size)
            if case["tkind"] == "apart8":
                x[ids] *= (2.0 ** -(ids % 9)).astype(np.float32)[:, None]
            redraws += ids.size
        else:
            raise AssertionError("no table without a pre-activation next to zero: " + case["label"])
    xt = to_table(case, x)
    return dict(x=xt, weights=ws, biases=bs, roots=roots_of(case["roots"], case["groups"]), ext=ext, redraws=redraws)


def case_inputs(case, knob: str = ""):
    """every tensor the case uploads, and the oracle's view of its union graph"""
    return _inputs(json.dumps(case, sort_keys=True), knob)


def colid_weights(case, call: int):
    """the last layer selects one hidden column per output: W_l picks column 48 call + c, W_r the one 7 further"""
    hid, n = case["hidden"][-1], case["n_out"]
    w = torch.zeros(n, 2 * hid)
    k = (48 * call + torch.arange(n)) % hid
    w[torch.arange(n), k] = 1
    w[torch.arange(n), hid + (k + 7) % hid] = 1
    b = ((torch.arange(n) + call) % 5 - 2).float()
    return w, b


def scaled_err(got: np.ndarray, ref: np.ndarray, s: np.ndarray) -> float:
    d = np.abs(got.astype(np.float64) - ref) / np.where(s > 0, s, 1.0)
    d = d[s > 0]
    if d.size == 0:
        return 0.0
    return float("inf") if not np.isfinite(d).all() else float(d.max())


# ---- the runs (GPU) -------------------------------------------------------------------------------------------------
class Engines:
    """one engine per table kind; the graph is loaded when it changes, the table per case"""

    def __init__(self):
        self._e = {}

    def get(self, case):
        from gigl_amd.engine import HipEngine
        k = case["table"]
        if k not in self._e:
            self._e[k] = [HipEngine(0), None]
        eng, g = self._e[k]
        if g != case["graph"]:
            rowptr, col, _ = graph(case["graph"])
            eng.load_csc(rowptr, col)
            self._e[k][1] = case["graph"]
        return eng

    def close(self):
        for eng, _ in self._e.values():
            eng.close()
        self._e = {}


def make_plan(eng, case, inp, roots=None):
    dev = eng.device
    b = (roots if roots is not None else inp["roots"]).size // case["groups"]
    ws = [w.to(dev) for w in inp["weights"]]
    bs = [None if x is None else x.to(dev) for x in inp["biases"]]
    old = os.environ.pop("GIGL_PLAN_NO_FUSE2", None)
    if case["no_fuse2"]:
        os.environ["GIGL_PLAN_NO_FUSE2"] = "1"
    try:
        plan = eng.make_sage_plan(ws, bs, b, case["fan"], case["act_last"], case["groups"], case["aggr"], case["l2"])
    finally:
        os.environ.pop("GIGL_PLAN_NO_FUSE2", None)
        if old is not None:
            os.environ["GIGL_PLAN_NO_FUSE2"] = old
    if case["proj"]:
        plan.set_projected_input(eng.project_features(ws[0]))
    return plan


def _dev_roots(eng, roots):
    return torch.from_numpy(np.ascontiguousarray(roots, np.uint32).view(np.int32)).to(eng.device)


def run_case(engs, case, knob: str = ""):
    """one case -> {label, kernels, err, fp32, ratio, eps, fails}: the graph check first, then the verdict of the case's
    kind and repeatability on every case; digest: sha256 of the first run's rows"""
    inp = case_inputs(case, knob)
    eng = engs.get(case)
    eng.load_features(inp["x"])
    disp = dispatch(case, inp["x"], knob)
    r = dict(label=case["label"], kernels=sorted(disp["kernels"]), err=0.0, fp32=0.0, ratio=0.0, eps=0.0, fails=[], digest="")
    fails = r["fails"]
    plan = make_plan(eng, case, inp)
    try:
        if plan.fused_layers() != disp["fused"] or plan.half_split() != disp["hs0"]:
            fails.append("dispatch: fused %s half split %s" % (plan.fused_layers(), plan.half_split()))
        roots = _dev_roots(eng, inp["roots"])
        out = plan.run(roots).cpu().numpy()
        r["digest"] = hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()
        hb = plan.last_batch_to_host()
        ext = plan_ext(case, hb)
        if hb["meta"][META_OVERFLOW] != 0 or ext is None or not np.array_equal(ext["keys"], inp["ext"]["keys"]):
            fails.append("graph: the plan's union is not the oracle's")
            return r
        want = layout_of(case)
        if want and (ext["n_roots"], ext["n_rows"]) != want:
            fails.append("graph: layout %s != %s" % ((ext["n_roots"], ext["n_rows"]), want))
        if not np.array_equal(plan.run(roots).cpu().numpy(), out, equal_nan=True):
            fails.append("repeatability")
        x64 = inp["x"].float().numpy().astype(np.float64)
        if case["kind"] == "tol":
            params = params_of(case, disp, inp["x"], inp["weights"], inp["biases"], ext)
            res = forward(case, x64, ext, inp["weights"], inp["biases"], params)
            f32 = forward(case, inp["x"].float().numpy(), ext, inp["weights"], inp["biases"], None, np.float32)
            r["eps"] = max(p[0] for p in params)
            r["err"], r["fp32"] = scaled_err(out, res["y"], res["S"]), scaled_err(f32["y"], res["y"], res["S"])
            r["ratio"] = scaled_err(out, res["y"], res["bound"])
            if margin_offenders(case, res, ext["computed"]):
                fails.append("inputs: a pre-activation within its bound of zero")
            if not (np.isfinite(out).all() and (np.abs(out.astype(np.float64) - res["y"]) <= res["bound"]).all()):
                fails.append("tolerance")
        elif case["kind"] == "int":
            res = forward(case, x64, ext, inp["weights"], inp["biases"])
            if not np.array_equal(out.astype(np.float64), res["y"].astype(np.float32).astype(np.float64)):
                fails.append("integer probe")
            elif not case["l2"] and not np.array_equal(res["y"], np.round(res["y"] * 64) / 64):
                fails.append("inputs: the probe's answer is no dyadic integer")
        elif case["kind"] == "colid":
            hid = case["hidden"][-1]
            for call in range((hid + 47) // 48):
                w2, b2 = colid_weights(case, call)
                ws, bs = inp["weights"][:-1] + [w2], inp["biases"][:-1] + [b2]
                plan.set_weights([w.to(eng.device) for w in ws], [None if b is None else b.to(eng.device) for b in bs])
                got = plan.run(roots).cpu().numpy()
                res = forward(case, x64, ext, ws, bs)
                if not np.array_equal(got.astype(np.float64), res["y"]):
                    fails.append("column identity, call %d: columns %s" % (call, np.nonzero((got != res["y"]).any(0))[0][:8].tolist()))
        else:
            assert case["kind"] == "history", case["kind"]
            few = roots_of("few")
            got = plan.run(_dev_roots(eng, few)).cpu().numpy()
            fresh = make_plan(eng, case, inp, few)
            try:
                if not np.array_equal(fresh.run(_dev_roots(eng, few)).cpu().numpy(), got, equal_nan=True):
                    fails.append("history independence")
            finally:
                fresh.close()
            if not np.isfinite(got).all():
                fails.append("history: non-finite rows")
    finally:
        plan.close()
    return r


def run_digest(engs, case):
    """the case's rows only -> {label, fused, digest, fails}: what a process run under a knob that must not change a bit
    reports for the comparison with run_case's digest of a process without it (the float64 verdict is that process's)"""
    inp = case_inputs(case)
    eng = engs.get(case)
    eng.load_features(inp["x"])
    plan = make_plan(eng, case, inp)
    try:
        roots = _dev_roots(eng, inp["roots"])
        out = plan.run(roots).cpu().numpy()
        r = dict(label=case["label"], fused=bool(plan.fused_layers()), fails=[],
                 digest=hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest())
        if not np.array_equal(plan.run(roots).cpu().numpy(), out, equal_nan=True):
            r["fails"].append("repeatability")
        return r
    finally:
        plan.close()


def layout_of(case):
    """(distinct roots, rows of the first layer) the layout cases rely on — None where the case does not care.  From the
    oracle; tests/test_gpu_sage_plan_layers.py checks the three layouts against the 128-row tile"""
    if case["groups"] != 1 or len(case["fan"]) != 2:
        return None
    m = case_inputs(case)["ext"]["metas"][0]
    return int(m[2]), int(m[3])


def format_case(r) -> str:
    return "%s %s err=%.3g fp32=%.3g eps=%.3g err/bound=%.3g" % (r["label"], r["kernels"], r["err"], r["fp32"], r["eps"], r["ratio"])


def main(mode: str) -> int:
    var = {"hs_layers": "GIGL_PLAN_HS_LAYERS", "bf16": "GIGL_GEMM_SPLIT", "f2_all_wr": "GIGL_F2_ALL_WR"}[mode]
    assert os.environ.get(var), "the knob is not set"
    engs = Engines()
    for case in child_cases(mode):
        print("CASE " + json.dumps(run_digest(engs, case) if mode == "f2_all_wr" else run_case(engs, case, mode)), flush=True)
    engs.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
