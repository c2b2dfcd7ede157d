"""Link-prediction head: inner-product decoder (HIP GEMM) and the retrieval loss.

Mirror of (paths relative to the reference root):
  DecoderType, LinkPredictionDecoder   python/gigl/src/common/models/layers/decoder.py:10-70
      inner_product: scores = torch.mm(q, c.T)   (:64-66)  -> gigl_linear(q, c) (same NT GEMM, exact fp32 MFMA)
      hadamard_MLP: scores = MLP(q.unsqueeze(1) * c).sum(-1)  (:67-69, PyG MLP, un-vendored: "parity unpinned")
          -> one hidden layer ([D, h, 1], relu, D and h <= 512): csrc/hadamard.hip, scores and gradients fused, no per-pair
             tensor; other depths: the first layer of all pairs as one projection by query-scaled weights, the rest on
             gigl_linear
  LinkPredictionGNN                    python/gigl/src/common/models/pyg/link_prediction.py:33-60
  RetrievalLoss                        python/gigl/src/common/models/layers/loss.py:177-360
      calculate_batch_retrieval_loss :209-277, _mask_by_query_ids :279-305, _mask_by_candidate_ids :307-331
  AligmentLoss, UniformityLoss         python/gigl/src/common/models/layers/loss.py:591-626  (csrc/pairwise.hip)
  GRACELoss                            python/gigl/src/common/models/layers/loss.py:362-416  (csrc/contrast.hip)
  WhiteningDecorrelationLoss, GBTLoss  python/gigl/src/common/models/layers/loss.py:444-534  (csrc/correlate.hip)
  BGRLLoss, TBGRLLoss                  python/gigl/src/common/models/layers/loss.py:537-588  (csrc/bootstrap.hip)
  FeatureReconstructionLoss            python/gigl/src/common/models/layers/loss.py:419-441  (csrc/reconstruct.hip)
The loss is one fused device pass over the score matrix (csrc/loss.hip: temperature, sampling-probability correction,
both masks, log-softmax and the summed cross-entropy, plus its backward), pinned by the reference's known-answer tests
(tests/test_link_prediction.py restates loss_test.py:61-166 and decoder_test.py:44-62).
"""
from __future__ import annotations

from enum import Enum
from typing import List, Optional

import torch
import torch.nn as nn
from .engine import dev_i32


class DecoderType(Enum):
    hadamard_MLP = "hadamard_MLP"
    inner_product = "inner_product"

    @classmethod
    def get_all_criteria(cls) -> List[str]:
        return [m.name for m in cls]


class _InnerProductFn(torch.autograd.Function):
    """scores[Q, C] = q[Q, D] @ c[C, D]^T on the fp32 MFMA GEMM; backward = two more GEMMs"""

    @staticmethod
    def forward(ctx, q, c, eng):
        q, c = q.contiguous(), c.contiguous()
        m = dev_i32(q.device, q.shape[0])
        ctx.eng = eng
        ctx.save_for_backward(q, c)
        return eng.linear(q, c, None, m, int(q.shape[0]), 0)

    @staticmethod
    def backward(ctx, ds):
        q, c = ctx.saved_tensors
        eng = ctx.eng
        ds = ds.contiguous()
        mq = dev_i32(q.device, q.shape[0])
        mc = dev_i32(q.device, c.shape[0])
        dq = eng.linear(ds, c.t().contiguous(), None, mq, int(q.shape[0]), 0)               # [Q,C]@[C,D]
        dc = eng.linear(ds.t().contiguous(), q.t().contiguous(), None, mc, int(c.shape[0]), 0)  # [C,Q]@[Q,D]
        return dq, dc, None


class LinkPredictionDecoder(nn.Module):
    def __init__(self, decoder_type: DecoderType = DecoderType.inner_product,
                 decoder_channel_list: Optional[List[int]] = None, **mlp_kwargs):
        super().__init__()
        self.decoder_type = decoder_type  # AttributeError on a non-enum, like the reference (`.value` below)
        self.decoder_channel_list = decoder_channel_list
        if self.decoder_type.value == "hadamard_MLP" and not isinstance(decoder_channel_list, list):
            raise ValueError("The decoder channel list must be provided when using 'hadamard_MLP' decoder, however "
                             f"you provided {decoder_channel_list}")
        if isinstance(decoder_channel_list, list) and len(decoder_channel_list) <= 1:
            raise ValueError("The decoder channel list must have length at least 2, however you provided a list of "
                             f"length {len(decoder_channel_list)}")
        if isinstance(decoder_channel_list, list) and decoder_channel_list[-1] != 1:
            raise ValueError("The last element in decoder channel list must be equal to 1, however you provided "
                             f"{decoder_channel_list[-1]}")
        if self.decoder_type.value == "hadamard_MLP":
            self.mlp_decoder = _DecoderMLP(decoder_channel_list, **mlp_kwargs)
        self.engine = None

    def forward(self, query_embeddings: torch.Tensor, candidate_embeddings: torch.Tensor) -> torch.Tensor:
        if self.engine is None:
            raise RuntimeError("LinkPredictionDecoder needs a HipEngine (decoder.engine = eng); no CPU fallback")
        if self.decoder_type.value == "hadamard_MLP":
            return self.mlp_decoder.pair_scores(query_embeddings, candidate_embeddings, self.engine)
        return _InnerProductFn.apply(query_embeddings, candidate_embeddings, self.engine)


class _DecoderMLP(nn.Module):
    """the hadamard_MLP decoder's MLP with PyG MLP's parameter layout (`lins.{i}`; decoder.py:52-60 passes act,
    act_first, bias, plain_last, norm) evaluated on every (query, candidate) pair WITHOUT materialising the
    [Q*C, D] matrix of elementwise products: lin_0(q * c) = (W_0 * q) c, so the first layer of all pairs is ONE
    projection of the candidates by the [Q*h_1, D] matrix of query-scaled weights; the remaining layers run on the
    resulting [C*Q, h_1] rows.  score = sum over the last layer's (single) output."""

    def __init__(self, channel_list: List[int], act=torch.relu, act_first: bool = False, bias=False,
                 plain_last: bool = False, norm=None):
        super().__init__()
        if norm is not None:
            raise NotImplementedError("hadamard_MLP with a normalisation layer is not built")
        if isinstance(act, str):
            if act != "relu":
                raise NotImplementedError(f"hadamard_MLP activation {act!r} is not built (relu)")
            act = torch.relu
        n = len(channel_list) - 1
        biases = list(bias) if isinstance(bias, (list, tuple)) else [bool(bias)] * n
        if len(biases) != n:
            raise ValueError(f"Number of bias values provided ({len(biases)}) does not match the number of layers ({n})")
        self.lins = nn.ModuleList([nn.Linear(channel_list[i], channel_list[i + 1], bias=biases[i]) for i in range(n)])
        self.act, self.act_first, self.plain_last = act, bool(act_first), plain_last

    def pair_scores(self, q: torch.Tensor, c: torch.Tensor, eng) -> torch.Tensor:
        from .models_hetero import _linear
        if (len(self.lins) == 2 and self.act is torch.relu and not self.act_first and q.dim() == c.dim() == 2
                and max(self.lins[0].weight.shape) <= HADAMARD_MAX_WIDTH):  # [D, h, 1]: the fused kernels
            return hadamard_mlp_scores(q, c, self.lins[0].weight, self.lins[0].bias, self.lins[1].weight, self.lins[1].bias,
                                       self.plain_last, eng)
        nq, nc = int(q.shape[0]), int(c.shape[0])
        n = len(self.lins)
        w0 = self.lins[0].weight                                     # [h1, D]
        h1 = int(w0.shape[0])
        scaled = (q.unsqueeze(1) * w0.unsqueeze(0)).reshape(nq * h1, -1)  # row (q, j) = W_0[j] * q
        x = _linear(eng, c, scaled, None).view(nc * nq, h1)            # row (c, q) = lin_0(q * c) before the bias
        if self.lins[0].bias is not None:
            x = x + self.lins[0].bias
        for i in range(n):
            if i > 0:
                x = _linear(eng, x, self.lins[i].weight, self.lins[i].bias)
            if self.act is not None and not (self.plain_last and i == n - 1):
                x = self.act(x)
        return x.view(nc, nq, -1).sum(dim=-1).t().contiguous()


HADAMARD_MAX_WIDTH = 512  # csrc/hadamard.hip serves 1 <= D, h <= 512


class _FusedHadamardMLP(torch.autograd.Function):
    """the hadamard_MLP decoder with one hidden layer, all Q x C pairs (csrc/hadamard.hip: the first layer on the matrix cores
    with q * c formed on the way into LDS; bias, ReLU and lins.1 folded from the accumulators); backward = two launches that
    rebuild the hidden tile — nothing but the inputs is saved — and fixed-order folds of their partial sums."""

    @staticmethod
    def forward(ctx, q, c, w0, b0, w1, b1, plain_last, eng):
        ctx.eng, ctx.plain_last = eng, bool(plain_last)
        ctx.save_for_backward(q, c, w0, b0, w1, b1)
        return eng.hadamard_mlp_scores(q, c, w0, b0, w1, b1, plain_last)

    @staticmethod
    def backward(ctx, ds):
        q, c, w0, b0, w1, b1 = ctx.saved_tensors
        dq, dc, dw0, db0, dw1, db1 = ctx.eng.hadamard_mlp_scores_backward(q, c, w0, b0, w1, b1, ctx.plain_last,
                                                                          ds.to(torch.float32))
        return dq, dc, dw0, db0, dw1.view(w1.shape), None if db1 is None else db1.view(b1.shape), None, None


def hadamard_mlp_scores(q, c, w0, b0, w1, b1, plain_last: bool, engine):
    """scores [Q, C] = relu(relu((q[:, None] * c) @ w0.T + b0) @ w1.T + b1).sum(-1) — without the outer relu when plain_last —
    of the hadamard_MLP decoder with decoder_channel_list [D, h, 1]: w0 [h, D], b0 [h] | None, w1 [1, h], b1 [1] | None; D, h
    <= 512.  Differentiable in all six tensors; device fp32 tensors."""
    if w0.dim() != 2 or max(w0.shape) > HADAMARD_MAX_WIDTH or w1.numel() != w0.shape[0]:
        raise ValueError(f"hadamard_mlp_scores serves [D, h, 1] with D, h <= {HADAMARD_MAX_WIDTH}: w0 {tuple(w0.shape)}, w1 "
                         f"{tuple(w1.shape)}")
    return _FusedHadamardMLP.apply(q, c, w0, b0, w1, b1, bool(plain_last), engine)


class LinkPredictionGNN(nn.Module):
    """encoder + decoder pair (link_prediction.py:33-60): forward = encoder embeddings, decode = scores"""

    def __init__(self, encoder: nn.Module, decoder: LinkPredictionDecoder):
        super().__init__()
        self._encoder = encoder
        self._decoder = decoder

    def forward(self, data, *args, **kwargs) -> torch.Tensor:
        return self._encoder(data, *args, **kwargs)

    def decode(self, query_embeddings: torch.Tensor, candidate_embeddings: torch.Tensor) -> torch.Tensor:
        return self._decoder(query_embeddings, candidate_embeddings)

    @property
    def encoder(self) -> nn.Module:
        return self._encoder

    @property
    def decoder(self) -> LinkPredictionDecoder:
        return self._decoder


def _ids_on(t: Optional[torch.Tensor], dev, n: int, what: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = t.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    if t.numel() != n:
        raise ValueError(f"{what}: expected {n} ids, got {t.numel()}")
    return t


class _FusedRetrievalLoss(torch.autograd.Function):
    """scores -> summed softmax cross-entropy against the diagonal, with the temperature, the sampling-probability
    correction and both masks applied inside the kernel (csrc/loss.hip); backward = one more pass over the scores"""

    @staticmethod
    def forward(ctx, scores, eng, temperature, cand_prob, query_ids, cand_ids):
        scores = scores.contiguous()
        loss, lse, _ = eng.retrieval_loss(scores, temperature, cand_prob, query_ids, cand_ids)
        ctx.eng, ctx.temperature = eng, temperature
        ctx.save_for_backward(scores, lse, cand_prob, query_ids, cand_ids)
        return loss

    @staticmethod
    def backward(ctx, g):
        scores, lse, cand_prob, query_ids, cand_ids = ctx.saved_tensors
        d = ctx.eng.retrieval_loss_backward(scores, ctx.temperature, cand_prob, query_ids, cand_ids, lse,
                                            g.to(torch.float32).contiguous())
        return d, None, None, None, None, None


class _MaskedLogits(torch.autograd.Function):
    """the masked logits themselves (for a caller-supplied loss module): the masks add constants, so the gradient is
    the incoming one over the temperature"""

    @staticmethod
    def forward(ctx, scores, eng, temperature, cand_prob, query_ids, cand_ids):
        _, _, masked = eng.retrieval_loss(scores.contiguous(), temperature, cand_prob, query_ids, cand_ids,
                                          want_masked=True)
        ctx.temperature = temperature
        return masked

    @staticmethod
    def backward(ctx, g):
        return (g / ctx.temperature if ctx.temperature is not None else g), None, None, None, None, None


class RetrievalLoss(nn.Module):
    """Same constructor and `calculate_batch_retrieval_loss` signature as the reference's RetrievalLoss
    (python/gigl/src/common/models/layers/loss.py:177-277); the body is ONE fused device pass (gigl_retrieval_loss)
    instead of the mask tensors + CrossEntropyLoss.  A caller-supplied `loss` module receives the masked logits and
    eye(Q, C) targets, as in the reference.  Device tensors only: there is no CPU path."""

    def __init__(self, loss: Optional[nn.Module] = None, temperature: Optional[float] = None,
                 remove_accidental_hits: bool = False):
        super().__init__()
        if temperature is not None and temperature < 1e-12:
            raise ValueError("The temperature is expected to be greater than 1e-12, however you provided "
                             f"{temperature}")
        self._loss = loss  # None: summed cross-entropy, computed inside the kernel
        self._temperature = temperature
        self._remove_accidental_hits = remove_accidental_hits

    def calculate_batch_retrieval_loss(self, scores: torch.Tensor,
                                       candidate_sampling_probability: Optional[torch.Tensor] = None,
                                       query_ids: Optional[torch.Tensor] = None,
                                       candidate_ids: Optional[torch.Tensor] = None,
                                       device: torch.device = torch.device("cpu")) -> torch.Tensor:
        from .engine import default_engine
        if self._remove_accidental_hits and candidate_ids is None:
            raise ValueError("When accidental hit removal is enabled, candidate ids must be supplied.")
        if not scores.is_cuda:
            raise RuntimeError("RetrievalLoss runs on the HIP device only (scores is a CPU tensor); no CPU fallback")
        q, c = int(scores.shape[0]), int(scores.shape[1])
        if q > c:
            raise AssertionError("Number of queries should be less than or equal to number of candidates in a batch")
        dev = scores.device
        eng = default_engine(dev)
        scores = scores.to(torch.float32)
        prob = None
        if candidate_sampling_probability is not None:
            prob = candidate_sampling_probability.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            if prob.numel() != c:  # (the reference's `scores - log(prob)` would fail to broadcast)
                raise ValueError(f"candidate_sampling_probability has {prob.numel()} entries for {c} candidates")
        qid = _ids_on(query_ids, dev, q, "query_ids")
        cid = _ids_on(candidate_ids, dev, c, "candidate_ids") if self._remove_accidental_hits else None
        if self._loss is None:
            return _FusedRetrievalLoss.apply(scores, eng, self._temperature, prob, qid, cid)
        masked = _MaskedLogits.apply(scores, eng, self._temperature, prob, qid, cid)
        return self._loss(masked, target=torch.eye(q, c, device=dev))


class _FusedUniformity(torch.autograd.Function):
    """rows -> log of the mean pairwise Gaussian potential (csrc/pairwise.hip: centring, the Gram tiles on the matrix cores,
    exp and the reduction in one pass); backward = a second sweep that recomputes the weights, no n x n tensor either way"""

    @staticmethod
    def forward(ctx, x, eng, temperature):
        loss, xc, sq, pair_sum = eng.uniformity_loss(x, temperature)
        ctx.eng, ctx.temperature = eng, temperature
        ctx.save_for_backward(xc, sq, pair_sum)
        return loss

    @staticmethod
    def backward(ctx, g):
        xc, sq, pair_sum = ctx.saved_tensors
        dx = ctx.eng.uniformity_loss_backward(xc, sq, ctx.temperature, pair_sum, g.to(torch.float32).contiguous())
        return dx, None, None


class _FusedAlignment(torch.autograd.Function):
    """mean_i |u_i - p_i|^alpha over the rows (csrc/pairwise.hip)"""

    @staticmethod
    def forward(ctx, u, p, eng, alpha):
        loss, norm = eng.alignment_loss(u, p, alpha)
        ctx.eng, ctx.alpha = eng, alpha
        ctx.save_for_backward(u, p, norm)
        return loss

    @staticmethod
    def backward(ctx, g):
        u, p, norm = ctx.saved_tensors
        du, dp = ctx.eng.alignment_loss_backward(u, p, ctx.alpha, norm, g.to(torch.float32).contiguous())
        return du, dp, None, None


def _device_rows(t: torch.Tensor, who: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{who} runs on the HIP device only (got a CPU tensor); no CPU fallback")
    if t.dim() != 2:
        raise ValueError(f"{who}: expected [n, d] embeddings, got shape {tuple(t.shape)}")
    return t.to(torch.float32)


class AligmentLoss(nn.Module):
    """The reference's AligmentLoss (python/gigl/src/common/models/layers/loss.py:591-606; its spelling): the mean of
    |user_i - item_i|^alpha over the positive pairs, one fused device pass (gigl_alignment_loss).  Device tensors only."""

    def __init__(self, alpha: Optional[float] = 2.0):
        super().__init__()
        self.alpha = alpha

    def forward(self, user_embeddings: torch.Tensor, item_embeddings: torch.Tensor) -> torch.Tensor:
        from .engine import default_engine
        u, p = _device_rows(user_embeddings, "AligmentLoss"), _device_rows(item_embeddings, "AligmentLoss")
        if u.shape != p.shape:
            raise ValueError(f"AligmentLoss: {tuple(u.shape)} user rows against {tuple(p.shape)} item rows")
        return _FusedAlignment.apply(u, p, default_engine(u.device), float(self.alpha))


class UniformityLoss(nn.Module):
    """The reference's UniformityLoss (loss.py:609-626): (U(user) + U(item)) / 2 with U(x) = log mean_{i<j}
    exp(-temperature |x_i - x_j|^2), each side one fused MFMA pass (gigl_uniformity_loss) instead of pdist -> pow -> mul ->
    exp -> mean -> log.  Device tensors only."""

    def __init__(self, temperature: float = 2.0):
        super().__init__()
        self.temperature = temperature

    def forward(self, user_embeddings: torch.Tensor, item_embeddings: torch.Tensor) -> torch.Tensor:
        from .engine import default_engine
        u, p = _device_rows(user_embeddings, "UniformityLoss"), _device_rows(item_embeddings, "UniformityLoss")
        eng, t = default_engine(u.device), float(self.temperature)
        return (_FusedUniformity.apply(u, eng, t) + _FusedUniformity.apply(p, eng, t)) / 2


class _FusedGrace(torch.autograd.Function):
    """two views' rows -> the GRACE contrastive loss (csrc/contrast.hip: normalisation, the three cosine Gram matrices on the
    matrix cores, a running-maximum log-sum-exp per row); backward = a second sweep that recomputes the softmax weights and
    multiplies them into the rows, no n x n tensor either way"""

    @staticmethod
    def forward(ctx, h1, h2, eng, temperature):
        loss, a, b, norm, lse = eng.grace_loss(h1, h2, temperature)
        ctx.eng, ctx.temperature = eng, temperature
        ctx.save_for_backward(a, b, norm, lse)
        return loss

    @staticmethod
    def backward(ctx, g):
        a, b, norm, lse = ctx.saved_tensors
        dh1, dh2 = ctx.eng.grace_loss_backward(a, b, norm, lse, ctx.temperature, g.to(torch.float32).contiguous())
        return dh1, dh2, None, None


class GRACELoss(nn.Module):
    """The reference's GRACELoss (loss.py:362-416): the mean over rows of -log(e^{sim12_ii / T} / (sum_{j != i} e^{sim11_ij / T}
    + sum_j e^{sim12_ij / T})), averaged with its mirror image, sim = cosine similarity — evaluated in log space by one fused
    MFMA pass (gigl_grace_loss) instead of four n x n exp matrices, so it is finite at the reference task's default T = 0.001
    where the literal form is inf - inf.  forward -> (loss, 1).  Device tensors only."""

    def __init__(self, temperature: Optional[float] = None):
        super().__init__()
        if temperature is None:  # (the reference would fail dividing by it)
            raise ValueError("GRACELoss needs a temperature")
        self.temperature = float(temperature)

    def forward(self, h1: torch.Tensor, h2: torch.Tensor, device: Optional[torch.device] = None):
        from .engine import default_engine
        h1, h2 = _device_rows(h1, "GRACELoss"), _device_rows(h2, "GRACELoss")
        if h1.shape != h2.shape:
            raise ValueError(f"GRACELoss: {tuple(h1.shape)} rows of view 1 against {tuple(h2.shape)} of view 2")
        return _FusedGrace.apply(h1, h2, default_engine(h1.device), self.temperature), 1


class _FusedCorrelation(torch.autograd.Function):
    """two views' rows -> GBTLoss (lambd None) or WhiteningDecorrelationLoss (csrc/correlate.hip: column statistics in fp64, the
    d x d correlation as a split-K MFMA product, loss and dL/dC from the folded tiles); backward = one Gram-shaped product per
    view with the standardisation's gradient in its epilogue"""

    @staticmethod
    def forward(ctx, h1, h2, eng, lambd):
        loss, saved, _ = eng.gbt_loss(h1, h2) if lambd is None else eng.whitening_loss(h1, h2, lambd)
        ctx.eng, ctx.n, ctx.gbt = eng, int(h1.shape[0]), lambd is None
        ctx.save_for_backward(*saved)
        return loss

    @staticmethod
    def backward(ctx, g):
        back = ctx.eng.gbt_loss_backward if ctx.gbt else ctx.eng.whitening_loss_backward
        dh1, dh2 = back(ctx.saved_tensors, ctx.n, g.to(torch.float32).contiguous())
        return dh1, dh2, None, None


def _two_views(h1: torch.Tensor, h2: torch.Tensor, who: str):
    h1, h2 = _device_rows(h1, who), _device_rows(h2, who)
    if h1.shape != h2.shape:
        raise ValueError(f"{who}: {tuple(h1.shape)} rows of view 1 against {tuple(h2.shape)} of view 2")
    return h1, h2


class GBTLoss(nn.Module):
    """The reference's GBTLoss (loss.py:491-534), graph Barlow Twins: with both views' columns standardised (mean, unbiased
    std + 1e-15) and C = z_a^T z_b / n, sum_a (1 - C_aa)^2 + (1 / d) sum_{a != b} C_ab^2 — one fused pass (gigl_gbt_loss).
    forward -> (loss, 1).  A constant column gets z = 0 as in the reference and a zero gradient where the reference's autograd
    gives NaN.  Device tensors only; n >= 2, d <= 512."""

    def forward(self, z_a: torch.Tensor, z_b: torch.Tensor, device: Optional[torch.device] = None):
        from .engine import default_engine
        z_a, z_b = _two_views(z_a, z_b, "GBTLoss")
        return _FusedCorrelation.apply(z_a, z_b, default_engine(z_a.device), None), 1


class WhiteningDecorrelationLoss(nn.Module):
    """The reference's WhiteningDecorrelationLoss (loss.py:444-488), CCA-SSG: with z_k the standardised views and c_k = z_k^T z_k
    / N, |z1 - z2|_F / N + lambd (|I - c1|_F + |I - c2|_F) — one fused pass (gigl_whitening_loss), fp32 (the reference's loss is
    fp64 because its identity matrix is).  forward -> (loss, 1); N must be the row count.  A constant column, where the
    reference's loss is NaN, enters as z = 0 and receives a zero gradient.  Device tensors only; n >= 2, d <= 512."""

    def __init__(self, lambd: float = 1e-3):
        super().__init__()
        self.lambd = float(lambd)

    def forward(self, h1: torch.Tensor, h2: torch.Tensor, N: int, device: Optional[torch.device] = None):
        from .engine import default_engine
        h1, h2 = _two_views(h1, h2, "WhiteningDecorrelationLoss")
        if int(N) != h1.shape[0]:
            raise ValueError(f"WhiteningDecorrelationLoss: N={N} is not the number of rows ({h1.shape[0]})")
        return _FusedCorrelation.apply(h1, h2, default_engine(h1.device), self.lambd), 1


class _FusedBootstrapHead(torch.autograd.Function):
    """the two views' online rows, the targets and the predictor head's parameters -> the BGRL (neg_y None) or TBGRL loss
    (csrc/bootstrap.hip: Linear -> ReLU -> Linear on the matrix cores with the hidden tile kept in LDS, the cosine terms folded
    from the second product's accumulators); backward = one launch for the row side (dQ, dH, dE) and two weight-gradient
    calls.  w1 None: enc1, enc2 are already projected (the loss modules)."""

    @staticmethod
    def forward(ctx, enc1, enc2, y1, y2, neg_y, w1, b1, w2, b2, eng, neg_lambda):
        head = None if w1 is None else (w1, b1, w2, b2)
        loss, (q, stat, hidden, rows, head) = eng.bootstrap_loss(enc1, enc2, y1, y2, neg_y, head, neg_lambda)
        ctx.eng, ctx.neg_lambda, ctx.tbgrl, ctx.head = eng, neg_lambda, neg_y is not None, head is not None
        ctx.save_for_backward(q, stat, *rows[:4], *(rows[4:] if ctx.tbgrl else ()), *((hidden, *head) if ctx.head else ()))
        return loss

    @staticmethod
    def backward(ctx, g):
        q, stat, *rest = ctx.saved_tensors
        rows = rest[:4] + ([rest[4]] if ctx.tbgrl else [None])
        tail = rest[5 if ctx.tbgrl else 4:]
        hidden, head = (tail[0], tuple(tail[1:])) if ctx.head else (None, None)
        de1, de2, dhead = ctx.eng.bootstrap_loss_backward((q, stat, hidden, rows, head), ctx.neg_lambda,
                                                          g.to(torch.float32).contiguous())
        return (de1, de2, None, None, None, *(dhead or (None,) * 4), None, None)


def _bootstrap_rows(who: str, *rows):
    rows = [_device_rows(t.detach() if k >= 2 else t, who) for k, t in enumerate(rows)]
    if any(t.shape != rows[0].shape for t in rows):
        raise ValueError(f"{who}: rows of different shapes {[tuple(t.shape) for t in rows]}")
    return rows


class BGRLLoss(nn.Module):
    """The reference's BGRLLoss (loss.py:537-556): 2 - mean cos(q1, y2) - mean cos(q2, y1) over already-projected rows, the
    targets constants — the row sums and their gradient by the bootstrap kernels without the head's products (gigl_bootstrap_
    loss, w1 NULL).  forward -> (loss, 1).  Device tensors only; the tasks go through _FusedBootstrapHead, head included."""

    def forward(self, q1: torch.Tensor, q2: torch.Tensor, y1: torch.Tensor, y2: torch.Tensor):
        from .engine import default_engine
        q1, q2, y1, y2 = _bootstrap_rows("BGRLLoss", q1, q2, y1, y2)
        return _FusedBootstrapHead.apply(q1, q2, y1, y2, None, None, None, None, None, default_engine(q1.device), 0.0), 1


class TBGRLLoss(nn.Module):
    """The reference's TBGRLLoss (loss.py:559-588): neg_lambda (mean cos(q1, neg_y) + mean cos(q2, neg_y)) - (1 - neg_lambda)
    (mean cos(q1, y2) + mean cos(q2, y1)), as BGRLLoss.  forward -> (loss, 1)."""

    def __init__(self, neg_lambda: float = 0.12):
        super().__init__()
        self.neg_lambda = float(neg_lambda)

    def forward(self, q1: torch.Tensor, q2: torch.Tensor, y1: torch.Tensor, y2: torch.Tensor, neg_y: torch.Tensor):
        from .engine import default_engine
        q1, q2, y1, y2, neg_y = _bootstrap_rows("TBGRLLoss", q1, q2, y1, y2, neg_y)
        return _FusedBootstrapHead.apply(q1, q2, y1, y2, neg_y, None, None, None, None, default_engine(q1.device),
                                         self.neg_lambda), 1


def bootstrap_head_loss(enc1, enc2, y1, y2, neg_y, head: nn.Sequential, neg_lambda: float):
    """the tasks' entry: head = Sequential(Linear(out, hid), ReLU, Linear(hid, out)) -> the loss tensor"""
    from .engine import default_engine
    who = "TBGRL" if neg_y is not None else "BGRL"
    rows = _bootstrap_rows(who, enc1, enc2, y1, y2, *(() if neg_y is None else (neg_y,)))
    return _FusedBootstrapHead.apply(*rows[:4], rows[4] if neg_y is not None else None, head[0].weight, head[0].bias,
                                     head[2].weight, head[2].bias, default_engine(rows[0].device), float(neg_lambda))


class _FusedFeatureReconstruction(torch.autograd.Function):
    """the encoder's rows of all nodes, the unmasked features, the roots and the decoder's parameters -> the scaled-cosine-error
    loss of the reconstructed root rows (csrc/reconstruct.hip: the root rows' neighbour sums, both Linears on the matrix cores
    with the intermediate kept in LDS, the row sums folded from the second product's accumulators); backward = one launch for
    the row side, a gather that writes every row of dE once, and two weight-gradient calls.  Gradients to enc, w_ed, w_rel,
    b_rel; none to x.  w_ed None: enc holds the predictions and x the targets, row for row (the loss module)."""

    @staticmethod
    def forward(ctx, enc, x, w_ed, w_rel, b_rel, eng, alpha, graph, roots):
        decoder = None if w_ed is None else (w_ed, w_rel, b_rel)
        loss, saved = eng.feature_reconstruction_loss(enc, x, alpha, graph, roots, decoder)
        ctx.eng = eng
        ctx.keys = [k for k, v in saved.items() if torch.is_tensor(v)]
        ctx.rest = {k: v for k, v in saved.items() if not torch.is_tensor(v)}
        ctx.save_for_backward(*(saved[k] for k in ctx.keys))
        return loss

    @staticmethod
    def backward(ctx, g):
        saved = dict(zip(ctx.keys, ctx.saved_tensors), **ctx.rest)
        d_rows, d_dec = ctx.eng.feature_reconstruction_loss_backward(saved, g.to(torch.float32).contiguous())
        return (d_rows, None, *(d_dec or (None,) * 3), None, None, None, None)


class FeatureReconstructionLoss(nn.Module):
    """The reference's FeatureReconstructionLoss (loss.py:419-441; GraphMAE's scaled cosine error): mean_i (1 - <x_i / |x_i|,
    y_i / |y_i|>)^alpha over already-decoded rows, the targets constants — the row sums, the fold and their gradient by the
    reconstruction kernels without the gather and the products (gigl_feature_reconstruction_loss, w_ed NULL).  forward -> (loss,
    1).  Device tensors only; the task goes through feature_reconstruction_loss, decoder included."""

    def __init__(self, alpha: float = 3.0):
        super().__init__()
        self.alpha = float(alpha)

    def forward(self, x_target: torch.Tensor, x_pred: torch.Tensor):
        from .engine import default_engine
        x_target, x_pred = _device_rows(x_target.detach(), "FeatureReconstructionLoss"), _device_rows(x_pred, "FeatureReconstructionLoss")
        if x_target.shape != x_pred.shape:
            raise ValueError(f"FeatureReconstructionLoss: rows of different shapes {tuple(x_target.shape)}, {tuple(x_pred.shape)}")
        return _FusedFeatureReconstruction.apply(x_pred, x_target, None, None, None, default_engine(x_pred.device), self.alpha, None,
                                                 None), 1


def feature_reconstruction_loss(enc, x, graph, roots, w_ed, w_rel, b_rel, alpha: float):
    """the task's entry: enc [N, out] the encoder's rows over `graph`, x [N, in] the unmasked features, roots [B] -> the loss"""
    from .engine import default_engine
    enc, x = _device_rows(enc, "FeatureReconstruction"), _device_rows(x.detach(), "FeatureReconstruction")
    return _FusedFeatureReconstruction.apply(enc, x, w_ed, w_rel, b_rel, default_engine(enc.device), float(alpha), graph, roots)
