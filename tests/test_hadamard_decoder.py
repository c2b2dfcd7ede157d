"""The fused hadamard_MLP decoder with one hidden layer (csrc/hadamard.hip) against the reference's literal formula (python/gigl/
src/common/models/layers/decoder.py:64-70: q.unsqueeze(1) * c through Linear -> ReLU -> Linear [-> ReLU], summed over the last
axis) in fp64 on the CPU through torch autograd, the backward under a random [Q, C] weight on the scores.  Tiles: 64 pair rows
(one query, 64 candidates), 64-column blocks of h, K chunks of 32; D or ld no multiple of 4 takes the scalar loader.  Bars: scores
within 1e-5 max(1, max|want|), each gradient within 1e-4 of that tensor's max|grad64|; on the hard inputs the larger of that and
twice the error of the same formula in torch fp32 on the CPU.

Measured on an MI355X: scores within 2.6e-7 of max(1, max|want|); gradients within 7.5e-6 of max|grad64| over the shape grid and
the hard inputs (the largest: db1 at a shape where its terms nearly cancel; typically 1e-7 to 3e-7)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["scores", "dq", "dc", "dw0", "db0", "dw1", "db1"]
GRID = [(nq, nc, d, h) for nq, nc in [(1, 1), (1, 65), (65, 1), (63, 64), (64, 65), (129, 70)]
        for d, h in [(4, 2), (30, 31), (33, 65), (128, 64)]] + [(65, 66, 512, 130), (65, 66, 36, 512), (65, 66, 5, 1)]
# b0, b1, plain_last: cycled over the grid, every combination of (b0, b1) and every value of plain_last with h <= 64 and h > 64
FLAGS = [(True, True, False), (False, True, True), (True, False, True), (False, False, False), (True, True, True)]


def formula(q, c, w0, b0, w1, b1, plain_last, wgt):
    """-> [scores, dq, dc, dw0, db0, dw1, db1] (None for an absent bias) in the dtype of the inputs, on their device"""
    ts = [None if t is None else t.detach().clone().requires_grad_(True) for t in (q, c, w0, b0, w1, b1)]
    q, c, w0, b0, w1, b1 = ts
    x = torch.relu(torch.nn.functional.linear(q.unsqueeze(1) * c, w0, b0))
    x = torch.nn.functional.linear(x, w1, b1)
    scores = (x if plain_last else torch.relu(x)).sum(-1)
    (scores * wgt).sum().backward()
    return [scores.detach()] + [None if t is None else t.grad for t in ts]


def inputs(nq, nc, d, h, b0, b1, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    return [r(nq, d), r(nc, d), r(h, d) / d ** 0.5, 0.1 * r(h) if b0 else None, r(1, h) / h ** 0.5, 0.1 * r(1) if b1 else None]


def fused(ts, plain_last, wgt, wide=False):
    from gigl_amd.engine import default_engine
    from gigl_amd.link_prediction import hadamard_mlp_scores
    ts = [None if t is None else t.to(DEV) for t in ts]
    if wide:  # q, c as column slices of wider matrices: ld = d + 5, d + 6 (33 + 5 = 38: no multiple of 4)
        ts[:2] = [torch.cat((t, torch.ones(t.shape[0], 5 + k, device=DEV)), dim=1)[:, :t.shape[1]] for k, t in enumerate(ts[:2])]
    ts = [None if t is None else t.detach().requires_grad_(True) for t in ts]
    scores = hadamard_mlp_scores(*ts, plain_last, default_engine(torch.device(DEV)))
    (scores * wgt.to(DEV)).sum().backward()
    return [scores.detach().cpu()] + [None if t is None else t.grad.cpu() for t in ts]


def check(ts, plain_last, hard=False, wide=False):
    wgt = torch.randn(ts[0].shape[0], ts[1].shape[0], generator=torch.Generator().manual_seed(1))
    got = fused(ts, plain_last, wgt, wide)
    want = formula(*[None if t is None else t.double() for t in ts], plain_last, wgt.double())
    fp32 = formula(*ts, plain_last, wgt) if hard else want
    for k, (name, g, w, f) in enumerate(zip(NAMES, got, want, fp32)):
        assert (g is None) == (w is None), name
        if w is None:
            continue
        assert g.shape == w.shape and torch.isfinite(g).all(), name
        scale = max(1.0, float(w.abs().max())) if k == 0 else float(w.abs().max())
        err, bar = float((g.double() - w).abs().max()), (1e-5 if k == 0 else 1e-4) * scale
        if hard:
            bar = max(bar, 2 * float((f.double() - w).abs().max()))
        print(f"{name}: err {err:.3e} = {err / scale if scale else 0.0:.3e} of the scale, bar {bar:.3e}")
        assert err <= bar, (name, err, bar)
    return got, want


@pytest.mark.parametrize("k", range(len(GRID)), ids=lambda k: "x".join(map(str, GRID[k])))
def test_shape_grid(k):
    nq, nc, d, h = GRID[k]
    b0, b1, plain_last = FLAGS[k % len(FLAGS)]
    check(inputs(nq, nc, d, h, b0, b1, seed=k), plain_last)


@pytest.mark.parametrize("kind", ["zero_query", "duplicate", "scaled", "wide", "clamped"])
def test_hard_inputs(kind):
    ts = inputs(65, 66, 33, 65, kind != "zero_query", True, seed=7)
    if kind == "zero_query":
        ts[0][5] = 0
    elif kind == "duplicate":
        ts[1][64] = ts[1][3]
    elif kind == "scaled":
        ts[0][::3] *= 1e4
    elif kind == "clamped":  # -b1 between the two middle values of the bias-free scores: half of them clamp to 0, none sits at 0
        mid = formula(*ts[:5], None, True, torch.zeros(65, 66))[0].flatten().sort().values[65 * 33 - 1:65 * 33 + 1]
        ts[5] = -mid.mean().reshape(1)
    got, want = check(ts, kind != "clamped", hard=True, wide=kind == "wide")
    if kind == "zero_query":  # pre = 0 on the whole row: nothing flows through it
        assert not got[1][5].any() and not want[1][5].any()
    if kind == "clamped":
        assert 0.3 < float((want[0] == 0).double().mean()) < 0.7


def test_backward_is_deterministic():
    ts, wgt = inputs(129, 70, 33, 65, True, True, seed=3), torch.randn(129, 70, generator=torch.Generator().manual_seed(1))
    a, b = fused(ts, False, wgt), fused(ts, False, wgt)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_module_route():
    """[33, 65, 1] takes the fused route — the functional entry's bits; [32, 16, 8, 1] keeps the composed one"""
    from gigl_amd.engine import default_engine
    from gigl_amd.link_prediction import DecoderType, LinkPredictionDecoder
    wgt = torch.randn(65, 66, generator=torch.Generator().manual_seed(1))
    for channels, bias in [([33, 65, 1], [True, False]), ([32, 16, 8, 1], True)]:
        torch.manual_seed(len(channels))
        dec = LinkPredictionDecoder(DecoderType.hadamard_MLP, channels, bias=bias).to(DEV)
        dec.engine = default_engine(torch.device(DEV))
        q, c = (torch.randn(n, channels[0]).to(DEV).requires_grad_(True) for n in (65, 66))
        scores = dec(q, c)
        (scores * wgt.to(DEV)).sum().backward()
        prm = dict(dec.named_parameters())
        assert sorted(prm) == sorted(f"mlp_decoder.lins.{i}.{n}" for i in range(len(channels) - 1)
                                     for n in (["weight", "bias"] if bias is True or bias[i] else ["weight"]))
        got = [scores.detach().cpu(), q.grad.cpu(), c.grad.cpu()] + [p.grad.cpu() for p in prm.values()]
        if len(channels) == 3:
            lins = dec.mlp_decoder.lins
            ts = [q, c, lins[0].weight, lins[0].bias, lins[1].weight, lins[1].bias]
            want = [t for t in fused([t if t is None else t.detach().cpu() for t in ts], False, wgt) if t is not None]
            assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
        else:  # the composed route against the fp64 formula of its three layers
            ts = [t.detach().cpu().double().requires_grad_(True) for t in (q, c, *prm.values())]
            x = ts[0].unsqueeze(1) * ts[1]
            for i in range(3):
                x = torch.relu(torch.nn.functional.linear(x, ts[2 + 2 * i], ts[3 + 2 * i]))
            want = x.sum(-1)
            (want * wgt.double()).sum().backward()
            for k, (g, w) in enumerate(zip(got, [want.detach()] + [t.grad for t in ts])):
                scale = max(1.0, float(w.abs().max())) if k == 0 else float(w.abs().max())
                assert float((g.double() - w).abs().max()) <= (1e-5 if k == 0 else 1e-4) * scale, k


def test_empty_sides():
    from gigl_amd.engine import default_engine
    from gigl_amd.link_prediction import hadamard_mlp_scores
    ts = [t.to(DEV).requires_grad_(True) for t in inputs(0, 7, 8, 4, True, True)]
    scores = hadamard_mlp_scores(*ts, False, default_engine(torch.device(DEV)))
    scores.sum().backward()
    assert scores.shape == (0, 7) and all(t.grad.shape == t.shape and not t.grad.any() for t in ts)
