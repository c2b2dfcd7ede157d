"""TEST INFRASTRUCTURE ONLY: the cases, inputs, float64 reference, bounds and exact probes of
tests/test_gpu_linear_kernels.py, plus a plain-Python mirror of the projection's dispatch rule and a numpy emulation of
the operand splits (split3, hsplit_store with hs_pow2_scale in csrc/agg.hip).

Run as a program (`python tests/linear_cases.py exact|bf16`) it is the CHILD of the knob tests: GIGL_LINEAR_EXACT and
GIGL_GEMM_SPLIT are read once per process, so the parent sets one of them in the child's environment; the child runs
every case of that knob once and prints one line `CASE {json}` per case (label, kernel, err, fp32, bound, fails)."""
import json
import math
import os
import sys

import numpy as np
import torch

SENT = -123.5  # y is pre-filled with it: rows / columns the kernel must not write keep it bit for bit
INF = float("inf")

BASE = (129, 36, 68)
M_SWEEP = [1, 63, 64, 65, 127, 128, 129, 300]
N_SWEEP = [1, 3, 4, 31, 32, 33, 60, 64, 65, 68, 96, 127, 128, 129, 132, 257]
K_VEC = [4, 8, 12, 16, 20, 28, 32, 36, 48, 64, 68, 96, 100, 132, 200]
K_ELEM = [1, 2, 3, 5, 33, 65, 97, 201]
REMAP = [(1153, 4, 129), (1153, 4, 64), (2048, 4, 257)]
# element loads with one column tile / with n <= 32 (the exact kernels' switch), and a ragged last chunk at n > 128
COMBOS = [(129, 33, 33), (65, 5, 3), (300, 97, 31), (129, 201, 64), (300, 200, 132)]
TAIL_M_DEV = [0, 1, 64, 65, 128]  # and m_cap - 1

T_BASE = (129, 36, 33)  # rows, d, n_out
T_D = [4, 36, 100, 6]
T_NOUT = [1, 2, 32, 33, 47, 64, 65]
T_ROWS = [1, 129, 1000]
T_COMBOS = [(1000, 6, 65), (129, 100, 64), (1000, 4, 1), (129, 6, 1)]
T_WSCALE = [2.0 ** -40, 1.0, 2.0 ** 40]
CHUNK = 1 << 19  # rows per launch of gigl_sage_project_features
T_MULTI = [(CHUNK, 4, 1), (CHUNK, 4, 2), (CHUNK + 133, 4, 1), (CHUNK + 133, 4, 2)]

GROUP_CAPS, GROUP_MS = [700, 130, 5000, 64, 256], [651, 130, 4097, 0, 1]  # (the layout of test_gpu_hetero.py)


# ---- the dispatch rule, restated ------------------------------------------------------------------------------------
def linear_kernel(k: int, n: int, exact: bool = False) -> str:
    """which kernel gigl_linear launches: k and n alone decide (never the row count)"""
    if not exact:
        return "split<%d,%s>" % (2 if n > 64 else 1, "vec" if k % 4 == 0 else "elem")
    if k % 4 == 0:
        return "lds<%d>" % (2 if n > 32 else 1)
    return "mfma<%d>" % (2 if n > 32 else 1)


def gridy_kernel(n: int) -> str:
    """gigl_linear_batched / gigl_linear_grouped: the vector-load split kernel with the product index in grid.y"""
    return "split_y<%d>" % (2 if n > 64 else 1)


def table_kernel(dtype: str, d: int, n_out: int, knob: str = "") -> str:
    """gigl_sage_project_features: knob "" | "bf16" (GIGL_GEMM_SPLIT=bf16) | "exact" (GIGL_LINEAR_EXACT)"""
    nn = 2 * n_out
    if dtype == "f32" or d % 4 != 0 or knob == "exact":  # (fp16 rows: the widened copy first)
        return linear_kernel(d, nn, knob == "exact")
    return "%s<%d>" % ("ahalf" if knob == "bf16" else "ahalf_hs", 2 if nn > 64 else 1)


INSTANTIATIONS = ["split<1,vec>", "split<2,vec>", "split<1,elem>", "split<2,elem>", "lds<1>", "lds<2>", "mfma<1>", "mfma<2>",
                  "ahalf_hs<1>", "ahalf_hs<2>", "ahalf<1>", "ahalf<2>", "split_y<1>", "split_y<2>"]


def remap_ids(m_cap: int, n: int):
    """(workgroup ids inside whole groups of 8 row tiles x all column tiles, leftover ids) of the XCD tile remap"""
    bn = 128 if n > 64 else 64
    tiles_n = (n + bn - 1) // bn
    grid = ((m_cap + 127) // 128) * tiles_n
    span = 8 * tiles_n
    full = grid // span * span
    return full, grid - full


# ---- cases ----------------------------------------------------------------------------------------------------------
def linear_shapes():
    """[(m, k, n, act, bias)]: one axis at a time around BASE, then the combinations; act / bias cycle over the list"""
    m0, k0, n0 = BASE
    shapes = [(m, k0, n0) for m in M_SWEEP] + [(m0, k0, n) for n in N_SWEEP] + [(m0, k, n0) for k in K_VEC + K_ELEM]
    shapes += REMAP + COMBOS
    seen, out = set(), []
    for s in shapes:
        if s not in seen:
            seen.add(s)
            out.append(s + (len(out) % 2, (len(out) // 2) % 2 == 0))
    return out


def linear_cases(exact: bool = False):
    return [dict(kind="linear", label="linear m%d k%d n%d act%d bias%d" % (m, k, n, act, bias), kernel=linear_kernel(k, n, exact),
                 fam="exact" if exact else "split", spec=[(m, m, bias)], k=k, n=n, act=act, tail=True)
            for m, k, n, act, bias in linear_shapes()]


def batched_cases():
    out = []
    for i, (batch, n, shared) in enumerate([(1, 33, False), (2, 33, True), (5, 33, False), (1, 70, True), (2, 70, False),
                                            (5, 70, True)]):
        out.append(dict(kind="batched", label="batched b%d n%d %s" % (batch, n, "sharedA" if shared else "ownA"),
                        kernel=gridy_kernel(n), fam="split", spec=[(129, 129, i % 2 == 0)] * batch, k=36, n=n, act=i % 2,
                        tail=True, shared_a=shared))
    return out


def grouped_cases():
    return [dict(kind="grouped", label="grouped k%d n%d" % (k, n), kernel=gridy_kernel(n), fam="split",
                 spec=[(c, m, i != 1) for i, (c, m) in enumerate(zip(GROUP_CAPS, GROUP_MS))], k=k, n=n, act=1, tail=False)
            for k in (36, 100) for n in (33, 129)]


def table_shapes():
    r0, d0, o0 = T_BASE
    shapes = [(r0, d, o0) for d in T_D] + [(r0, d0, o) for o in T_NOUT] + [(r, d0, o0) for r in T_ROWS] + T_COMBOS
    seen, out = set(), []
    for s in shapes:
        if s not in seen:
            seen.add(s)
            out.append(s + (T_WSCALE[len(out) % 3],))
    out += [T_BASE + (s,) for s in T_WSCALE if T_BASE + (s,) not in out]  # the base shape at every weight scale
    return out + [s + (1.0,) for s in T_MULTI]


def table_cases(knob: str = "", dtypes=("f16", "f32")):
    out = []
    for rows, d, n_out, ws in table_shapes():
        for dt in dtypes:
            if (rows, d, n_out) in T_MULTI and knob:
                continue  # (the chunk loop does not depend on the knob)
            kern = table_kernel(dt, d, n_out, knob)
            fam = "hs" if kern.startswith("ahalf_hs") else ("exact" if knob == "exact" else "split")
            out.append(dict(kind="table", label="table %s rows%d d%d out%d w2^%d" % (dt, rows, d, n_out, round(math.log2(ws))),
                            kernel=kern, fam=fam, spec=[(rows, rows, False)], k=d, n=2 * n_out, act=0, tail=False, a_kind=dt,
                            wscale=ws))
    return out


def default_cases():
    return linear_cases() + batched_cases() + grouped_cases() + table_cases()


def child_cases(mode: str):
    if mode == "exact":
        return linear_cases(exact=True)
    assert mode == "bf16", mode
    return table_cases("bf16", dtypes=("f16",))


# ---- inputs (CPU tensors; the very ones that are uploaded) ----------------------------------------------------------
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum(int(v) * p for v, p in zip(key, (1000003, 10007, 101, 7, 3))) + 12345)
    return g


def tol_a(cap: int, k: int, kind: str = "f32", seed: int = 0) -> torch.Tensor:
    g = _gen(cap, k, seed, 1)
    a = torch.randn(cap, k, generator=g)
    if kind == "f32":  # rows of very different scale, exact powers of two
        e = torch.tensor([0.0, 30.0, 60.0, -60.0, -30.0])[torch.arange(cap) % 5]  # (row 0 at the bias's scale: m = 1)
        return a * torch.pow(torch.tensor(2.0), e).unsqueeze(1)
    a = (a * 8).half()  # an fp16 table with zeros, subnormal halves and the largest finite halves
    flat = a.view(-1)
    flat[0::7] = 0
    flat[3::11] = torch.tensor(5 * 2.0 ** -24).half()
    flat[4::22] = torch.tensor(-1023 * 2.0 ** -24).half()
    flat[5::13] = 65504.0
    flat[6::26] = -65504.0
    return a


def tol_w(n: int, k: int, wscale: float = 1.0, seed: int = 0) -> torch.Tensor:
    w = torch.randn(n, k, generator=_gen(n, k, seed, 2)) / math.sqrt(k)
    w[0] *= 1e-4
    return w * wscale


def tol_b(n: int, wscale: float = 1.0, seed: int = 0) -> torch.Tensor:
    return torch.randn(n, generator=_gen(n, seed, 3)) * wscale


def sel_index(m: int, k: int) -> torch.Tensor:
    return (7 * torch.arange(m) + 3) % k


def sel_a(m: int, k: int, dtype=torch.float32) -> torch.Tensor:
    a = torch.zeros(m, k, dtype=dtype)
    a[torch.arange(m), sel_index(m, k)] = 1
    return a


def w_int(n: int, k: int) -> torch.Tensor:
    j, c = torch.arange(n).unsqueeze(1), torch.arange(k).unsqueeze(0)
    return (1 + ((37 * j + 11 * c) % 251)).float()


def b_int(n: int) -> torch.Tensor:
    return ((13 * torch.arange(n)) % 97 - 48).float()


def case_inputs(case):
    """every tensor the case uploads: {"a": [...], "w": [...], "b": [...], "sel_a", "ones_a", "w_int", "b_int"}"""
    k, n = case["k"], case["n"]
    kind, ws = case.get("a_kind", "f32"), case.get("wscale", 1.0)
    dt = torch.float16 if kind == "f16" else torch.float32
    a_s, w_s, b_s = [], [], []
    for i, (cap, _, bias) in enumerate(case["spec"]):
        a_s.append(a_s[0] if (case.get("shared_a") and i) else tol_a(cap, k, kind, i))
        w_s.append(tol_w(n, k, ws, i))
        b_s.append(tol_b(n, ws, i) if bias else None)
    return dict(a=a_s, w=w_s, b=b_s, sel_a=[sel_a(cap, k, dt) for cap, _, _ in case["spec"]],
                ones_a=[torch.ones(cap, k, dtype=dt) for cap, _, _ in case["spec"]], w_int=w_int(n, k), b_int=b_int(n))


# ---- reference and bounds -------------------------------------------------------------------------------------------
def reference(a, w, b, act):
    """float64 on the CPU; fp16 rows are widened exactly"""
    ref = a.double() @ w.double().T
    if b is not None:
        ref = ref + b.double()
    return ref.clamp(min=0) if act else ref


def scale_of(a, w, b):
    """S = sum_k |a||w| + |b|, per element"""
    s = a.double().abs() @ w.double().abs().T
    return s + b.double().abs() if b is not None else s


def fp32_product(a, w, b, act):
    y = torch.matmul(a.float(), w.float().T)
    if b is not None:
        y = y + b.float()
    return y.clamp(min=0) if act else y


def scaled_err(got, ref, s) -> float:
    """max |got - ref| / S over the elements with S > 0 (inf when got holds a non-finite value there)"""
    d = (got.double() - ref).abs() / s
    d = d[s > 0]
    if d.numel() == 0:
        return 0.0
    return INF if not bool(torch.isfinite(d).all()) else d.max().item()


def bound_of(fam: str, s, a, w, fp32_err: float):
    """(per-element bound, its relative figure).  split: 4e-7 S.  hs: the documented weight-plane model with a factor
    2 plus the accumulation term.  exact: the larger of 4e-7 S and 4 x the float32 CPU product's scaled error."""
    if fam == "split":
        return 4e-7 * s, 4e-7
    if fam == "hs":
        rel = 4e-7 + 2.0 ** -21
        return rel * s + 2.0 ** -38 * w.double().abs().max() * a.double().abs().sum(1, keepdim=True), rel
    assert fam == "exact", fam
    rel = max(4e-7, 4 * fp32_err)
    return rel * s, rel


# ---- numpy emulation of the operand splits --------------------------------------------------------------------------
_HI = np.uint32(0xFFFF0000)


def split3_np(x):
    """the three bf16 planes of csrc/agg.hip's split3, as float32 arrays"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        b1 = (x.view(np.uint32) & _HI).view(np.float32)
        r1 = (x - b1).astype(np.float32)
        b2 = (r1.view(np.uint32) & _HI).view(np.float32)
        r2 = (r1 - b2).astype(np.float32)
        b3 = (r2.view(np.uint32) & _HI).view(np.float32)
    return b1, b2, b3


def hs_pow2_scale_np(m: float) -> float:
    bits = int(np.float32(m).view(np.uint32))
    e = ((bits >> 23) & 0xFF) - 127
    if ((bits >> 23) & 0xFF) == 0:
        e = -126
    return 2.0 ** max(-60, min(60, 14 - e))


def hsplit_np(x, s: float):
    """(h1, h2) fp16 planes of hsplit_store at scale s, as float64 arrays of the SCALED values"""
    xs = (np.asarray(x, dtype=np.float32) * np.float32(s)).astype(np.float32)
    h1 = xs.astype(np.float16)
    h2 = (xs - h1.astype(np.float32)).astype(np.float32).astype(np.float16)
    return h1.astype(np.float64), h2.astype(np.float64)


# ---- the products (GPU) ---------------------------------------------------------------------------------------------
def _i32(dev, v):
    return torch.tensor([int(v)], dtype=torch.int32, device=dev)


def make_prod(eng, kind: str, shared_a: bool = False):
    """prod(problems, act) -> ([y on the CPU per problem], [failure notes]); a problem is (a [cap, k], w [n, k], b | None, m_dev)"""
    dev = eng.device
    up = lambda t: None if t is None else t.to(dev)

    def linear(probs, act):
        (a, w, b, md), = probs
        y = torch.full((a.shape[0], w.shape[0]), SENT, device=dev)
        eng.linear(up(a), up(w), up(b), _i32(dev, md), int(a.shape[0]), act, out=y)
        return [y.cpu()], []

    def batched(probs, act):
        import ctypes as C
        batch, (cap, k), n = len(probs), probs[0][0].shape, probs[0][1].shape[0]
        md = probs[0][3]
        assert all(p[3] == md and (p[2] is None) == (probs[0][2] is None) for p in probs)
        a = up(probs[0][0] if shared_a else torch.stack([p[0] for p in probs]))
        w = up(torch.stack([p[1] for p in probs]))
        b = up(None if probs[0][2] is None else torch.stack([p[2] for p in probs]))
        ldy = n * batch + 3
        y = torch.full((cap, ldy), SENT, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        rc = eng._lib.gigl_linear_batched(eng._ctx, p(a), p(w), p(b), p(_i32(dev, md)), cap, k, n, act, batch,
                                          0 if shared_a else cap * k, n * k, ldy, p(y))
        assert rc == 0, rc
        y = y.cpu()
        notes = [] if bool((y[:, n * batch:] == SENT).all()) else ["columns past n*batch written"]
        return [y[:, i * n:(i + 1) * n].contiguous() for i in range(batch)], notes

    def grouped(probs, act):
        groups = [(up(a), up(w), up(b), _i32(dev, md), torch.full((a.shape[0], w.shape[0]), SENT, device=dev))
                  for a, w, b, md in probs]
        eng.linear_grouped(groups, int(probs[0][0].shape[1]), int(probs[0][1].shape[0]), act=act)
        return [g[4].cpu() for g in groups], []

    def table(probs, act):
        (a, w, b, md), = probs
        assert b is None and act == 0 and md == a.shape[0]
        n_out = w.shape[0] // 2
        eng.load_features(a)
        return [eng.project_features(torch.cat([w[:n_out], w[n_out:]], dim=1)).cpu()], []

    return dict(linear=linear, batched=batched, grouped=grouped, table=table)[kind]


def _sent(y) -> bool:
    return bool((y == SENT).all())


def run_case(eng, case):
    """tolerance case + the exact probes of one case -> {label, kernel, err, fp32, bound, fails}"""
    prod = make_prod(eng, case["kind"], case.get("shared_a", False))
    inp, spec, act, fam = case_inputs(case), case["spec"], case["act"], case["fam"]
    k, n = case["k"], case["n"]
    fails, err, f32 = [], 0.0, 0.0
    G = range(len(spec))
    mds = [md for _, md, _ in spec]

    def call(a_s, w_s, b_s, act_, mds_=None):
        ys, notes = prod([(a_s[i], w_s[i], b_s[i], (mds_ or mds)[i]) for i in G], act_)
        fails.extend(notes)
        return ys

    # tolerance against float64, every element on its own scale
    ys = call(inp["a"], inp["w"], inp["b"], act)
    refs, bounds = [], []
    rel = 0.0
    for i in G:
        a, w, b, md = inp["a"][i][:mds[i]], inp["w"][i], inp["b"][i], mds[i]
        ref, s = reference(a, w, b, act), scale_of(a, w, b)
        e32 = scaled_err(fp32_product(a, w, b, act), ref, s)
        bound, rel = bound_of(fam, s, a, w, e32)
        refs.append((reference(a, w, b, 0), s))
        bounds.append(bound)
        f32 = max(f32, e32)
        err = max(err, scaled_err(ys[i][:md], ref, s))
        if not bool(((ys[i][:md].double() - ref).abs() <= bound).all()):
            fails.append("tolerance[%d]" % i)
        if not _sent(ys[i][md:]):
            fails.append("tolerance rows past m_dev[%d]" % i)

    # selection probe: y[i] = W[:, sel(i)] exactly, bias off
    wi, bi = inp["w_int"], inp["b_int"]
    ys = call(inp["sel_a"], [wi] * len(spec), [None] * len(spec), act)
    for i in G:
        md = mds[i]
        if not (torch.equal(ys[i][:md], wi[:, sel_index(md, k)].T.contiguous()) and _sent(ys[i][md:])):
            fails.append("selection[%d]" % i)

    # column-sum probe: exact integers, integer bias
    ys = call(inp["ones_a"], [wi] * len(spec), [bi if bias else None for _, _, bias in spec], act)
    for i in G:
        md, row = mds[i], wi.sum(1) + (bi if spec[i][2] else 0)
        if act:
            row = row.clamp(min=0)
        if not (torch.equal(ys[i][:md], row.expand(md, n).contiguous()) and _sent(ys[i][md:])):
            fails.append("column sum[%d]" % i)

    # non-finite isolation (act 0: the activation's compare turns a NaN into 0)
    if any(md >= 3 for md in mds):
        a_s, hit = [], []
        for i in G:
            md = mds[i]
            a = inp["a"][i].clone()
            r1, r2 = md // 3, (2 * md) // 3
            if md >= 3:
                a[r1, (5 * r1) % k] = INF
                a[r2, (3 * r2) % k] = float("nan")
            a_s.append(a)
            hit.append((r1, r2))
        if case.get("shared_a"):
            a_s = [a_s[0]] * len(spec)
        ys = call(a_s, inp["w"], inp["b"], 0)
        for i in G:
            md = mds[i]
            if md < 3:
                continue
            keep = torch.ones(md, dtype=torch.bool)
            keep[list(hit[i])] = False
            ok = bool(((ys[i][:md].double() - refs[i][0]).abs() <= bounds[i])[keep].all())
            if not (ok and not bool(torch.isfinite(ys[i][list(hit[i])]).any())):
                fails.append("non-finite isolation[%d]" % i)

    # tail rows: m_dev < m_cap, NaN rows behind m_dev, the sentinel kept, the rows before equal to the m_cap == m_dev run
    if case["tail"]:
        cap = spec[0][0]
        for md in sorted({v for v in TAIL_M_DEV + [cap - 1] if 0 <= v < cap}):
            a_s = []
            for i in G:
                a = inp["a"][i].clone()
                a[md:] = float("nan")
                a_s.append(a)
            if case.get("shared_a"):
                a_s = [a_s[0]] * len(spec)
            ys = call(a_s, inp["w"], inp["b"], act, [md] * len(spec))
            base = call([a[:md].contiguous() for a in a_s], inp["w"], inp["b"], act, [md] * len(spec)) if md else None
            for i in G:
                if not (_sent(ys[i][md:]) and (md == 0 or torch.equal(ys[i][:md], base[i]))):
                    fails.append("tail rows m_dev=%d[%d]" % (md, i))
    return dict(label=case["label"], kernel=case["kernel"], err=err, fp32=f32, bound=rel, fails=fails)


def row_independence(eng, k: int, n: int = 129):
    """the first 100 rows at m_cap = 100 and inside m_cap = 1153 (another grid, another tile mapping): bit-identical"""
    prod = make_prod(eng, "linear")
    a, w, b = tol_a(1153, k), tol_w(n, k), tol_b(n)
    (small,), _ = prod([(a[:100].contiguous(), w, b, 100)], 1)
    (large,), _ = prod([(a, w, b, 1153)], 1)
    return torch.equal(small, large[:100])


def format_case(r) -> str:
    return "%s [%s] err=%.3g fp32=%.3g bound=%.3g" % (r["label"], r["kernel"], r["err"], r["fp32"], r["bound"])


def main(mode: str) -> int:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    assert os.environ.get({"exact": "GIGL_LINEAR_EXACT", "bf16": "GIGL_GEMM_SPLIT"}[mode]), "the knob is not set"
    from gigl_amd.engine import HipEngine
    eng = HipEngine(0)
    for case in child_cases(mode):
        print("CASE " + json.dumps(run_case(eng, case)), flush=True)
    if mode == "exact":
        for k in (36, 33):
            print("CASE " + json.dumps(dict(label="row independence k%d" % k, kernel=linear_kernel(k, 129, True), err=0.0, fp32=0.0,
                                            bound=0.0, fails=[] if row_independence(eng, k) else ["row independence"])), flush=True)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
