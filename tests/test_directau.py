"""DirectAU: the fused uniformity / alignment losses (csrc/pairwise.hip) and the task against fp64 formulas of the
reference (python/gigl/src/common/models/layers/loss.py:591-626, task.py:656-696).  Row tile of the MFMA kernels: 64.
Bars: loss within 1e-5 absolute, gradient within 1e-4 of max|grad64|.

Measured on an MI355X: every case stays below 3.7e-7 (loss) and 3.7e-5 (gradient: 65 x 512 at t = 2; 2.7e-5 below that
width).  The hardest of the narrow ones are the d = 1 shapes: the
normalised rows are +1 or -1, two clusters of exact duplicates, so r_i x_i and sum_j w_ij x_j are both ~ the cluster size
while the gradient is ~ exp(-8) of that (csrc/pairwise.hip, pair_fix3, is what keeps that difference)."""
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"


def rows(n, d, seed, kind="plain"):
    g = torch.Generator().manual_seed(seed)
    if kind == "collapsed":
        x = torch.nn.functional.normalize(torch.randn(1, d, generator=g), dim=1) + 1e-3 * torch.randn(n, d, generator=g)
    elif kind == "dup":
        x = torch.randn((n + 1) // 2, d, generator=g).repeat_interleave(2, dim=0)[:n]
    else:
        x = torch.randn(n, d, generator=g)
    x = torch.nn.functional.normalize(x, dim=1)
    if kind == "view":  # rows of a wider matrix: ld > d
        return torch.cat((x, torch.randn(n, 7, generator=g)), dim=1).to(DEV)[:, :d]
    return x.to(DEV)


def u64(x, t):
    return torch.pdist(x.double().cpu()).pow(2).mul(-t).exp().mean().log()


def a64(u, p, alpha):
    return (u.double().cpu() - p.double().cpu()).norm(p=2, dim=1).pow(alpha).mean()


def check(loss_fn, ref_fn, u, p):
    """loss_fn(u, p) on the device against ref_fn(u, p) in fp64, value and both gradients"""
    u, p = u.detach().requires_grad_(True), p.detach().requires_grad_(True)
    got = loss_fn(u, p)
    got.backward()
    u_ref, p_ref = u.detach().double().cpu().requires_grad_(True), p.detach().double().cpu().requires_grad_(True)
    want = ref_fn(u_ref, p_ref)
    want.backward()
    errs = [abs(float(got) - float(want))]
    assert errs[0] <= 1e-5, (float(got), float(want))
    for mine, ref in ((u.grad, u_ref.grad), (p.grad, p_ref.grad)):
        errs.append(float((mine.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300))
        assert float((mine.double().cpu() - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), errs
    print("max errors (loss abs, grad rel to max): %.3g %.3g" % (errs[0], max(errs[1:])))


NS, DS = (2, 3, 63, 64, 65, 129, 257), (1, 4, 16, 30, 36, 260)
SHAPES = list(dict.fromkeys([(n, d) for n in NS for d in (16, 30)] + [(n, d) for n in (65, 129) for d in DS]))
# the backward's 128-column chunk with its second 64-column group and its last 32-column block partly filled (vectorised
# loads and not), and the widest rows the kernels serve (four full chunks)
SHAPES += [(65, 100), (65, 97), (65, 512)]


@gpu
@pytest.mark.parametrize("t", [2.0, 0.5])
@pytest.mark.parametrize("n,d", SHAPES)
def test_uniformity_against_fp64(n, d, t):
    from gigl_amd.link_prediction import UniformityLoss
    check(UniformityLoss(temperature=t), lambda u, p: (u64(u, t) + u64(p, t)) / 2, rows(n, d, 1), rows(n, d, 2))


@gpu
@pytest.mark.parametrize("kind", ["view", "dup", "collapsed"])
def test_uniformity_hard_inputs(kind):
    from gigl_amd.link_prediction import UniformityLoss
    check(UniformityLoss(temperature=2.0), lambda u, p: (u64(u, 2.0) + u64(p, 2.0)) / 2, rows(129, 16, 3, kind),
          rows(129, 16, 4, kind))


@gpu
@pytest.mark.parametrize("alpha", [2.0, 1.0])
@pytest.mark.parametrize("n,d", [(1, 1), (1, 30), (65, 1), (65, 30)])
def test_alignment_against_fp64(n, d, alpha):
    from gigl_amd.link_prediction import AligmentLoss
    u, p = rows(n, d, 5), rows(n, d, 6)
    p[n // 2] = u[n // 2]  # a pair at distance 0: zero gradient, not NaN
    check(AligmentLoss(alpha=alpha), lambda a, b: a64(a, b, alpha), u, p)


@gpu
def test_directau_forward():
    from gigl_amd.nablp_spec import BatchEmbeddings, DirectAU, NodeAnchorBasedLinkPredictionTaskInputs

    def task_loss(u, p):
        emb = BatchEmbeddings(query_embeddings=u, repeated_query_embeddings={0: u}, pos_embeddings={0: p},
                              hard_neg_embeddings={}, random_neg_embeddings={})
        ti = NodeAnchorBasedLinkPredictionTaskInputs(main_batch=None, random_neg_batch=None, batch_embeddings=emb)
        loss, count = DirectAU(gamma=0.5, alpha=2.0, temperature=2.0)(ti, None, False, torch.device(DEV))
        assert count == 1
        return loss

    check(task_loss, lambda u, p: a64(u, p, 2.0) + 0.5 * (u64(u, 2.0) + u64(p, 2.0)) / 2, rows(70, 16, 7), rows(70, 16, 8))


def test_spec_wiring():
    from gigl_amd.nablp_spec import DirectAU, HipNodeAnchorLinkPredictionSpec
    for extra, want_t in (({}, 2.0), ({"directau_temperature": "1.0"}, 1.0)):
        spec = HipNodeAnchorLinkPredictionSpec(task_path="gigl_amd.nablp_spec.DirectAU", gamma="0.5", softmax_temp="0.07",
                                               **extra)
        (task,) = spec.tasks._task_to_fn_map.values()
        assert type(task) is DirectAU and task.gamma == 0.5
        assert task.uniformity_loss.temperature == want_t and task.alignment_loss.alpha == 2.0
        assert spec._train_plan_task_kwargs() is None


@gpu
def test_reproducible():
    from gigl_amd.link_prediction import UniformityLoss
    out = []
    for _ in range(2):
        u, p = rows(257, 36, 9).requires_grad_(True), rows(257, 36, 10).requires_grad_(True)
        loss = UniformityLoss()(u, p)
        loss.backward()
        out.append((loss.detach().cpu(), u.grad.cpu(), p.grad.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*out))


@gpu
def test_width_out_of_range_is_an_error():
    from gigl_amd.link_prediction import UniformityLoss
    with pytest.raises(RuntimeError, match="d=513"):
        UniformityLoss()(rows(4, 513, 11), rows(4, 513, 12))
