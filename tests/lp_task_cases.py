"""What the Margin / Softmax plan tests share (tests/test_gpu_lp_task_plan.py): the 390-node graph of
tests/test_gpu_lp_hard_negatives.py, batches built on the HOST (so that the CPU restatement can be run over the very same
batches without a GPU), the tasks' loss in torch over root embeddings, and the CPU restatement of a training run.

main roots: b x T ids, T = 1 + P + H, anchor-major (anchor, positive slots, hard-negative slots; an empty slot repeats the
anchor); counts: [2 b] = positives per anchor, then hard negatives per anchor — what HipEngine.nablp_main_roots writes.  The
positives are the sampler's (counter 3 over the out-edges, here the same undirected graph: oracle.sample_khop reproduces
them, tests/test_gpu_parity.py::test_positives_counter_three), the hard negatives are drawn here."""
import numpy as np
import torch

import oracle
from oracle import gnn_ref

N, N_ISOLATED, FAN = 390, 5, [10, 5]
MARGIN, SOFTMAX_T = 0.3, 0.1


def graph_and_features():
    """the graph of test_gpu_lp_hard_negatives._engine (four permutations' edges, both directions, the last five nodes
    without an edge) and its features"""
    rng = np.random.default_rng(8)
    m = N - N_ISOLATED
    s = np.tile(np.arange(m), 4).astype(np.uint32)
    d = np.concatenate([rng.permutation(m) for _ in range(4)]).astype(np.uint32)
    rowptr, col = oracle.build_csc(N, s, d, is_directed=False)
    assert int(np.diff(rowptr).max()) <= FAN[0]
    x = (np.random.default_rng(0).standard_normal((N, 100)) / 4).astype(np.float32)
    return rowptr, col, x


def host_batches(rowptr, col, b, P, H, n_rn, steps, seed):
    """-> [(main roots uint32 [b T], counts int32 [2 b] ([b] when H == 0), random negatives uint32 [n_rn])] holding, asserted:
    hard-negative counts of 0, fewer than H and H, an anchor WITHOUT a positive (an isolated node) that has hard negatives,
    an anchor with fewer than P positives when P >= 2"""
    rng = np.random.default_rng(seed)
    T = 1 + P + H
    out, seen = [], set()
    for step in range(steps):
        anchors = rng.permutation(N - N_ISOLATED)[:b].astype(np.uint32)
        if step == 1:
            anchors[0] = N - 1
        nbr, cnt = oracle.sample_khop(rowptr, col, anchors, [P], first_counter=3, canonical=True)
        pos, kp = nbr[0].reshape(b, P), cnt[0].astype(np.int32)
        roots = np.repeat(anchors.reshape(b, 1), T, axis=1)
        kn = np.zeros(b, dtype=np.int32)
        for i in range(b):
            roots[i, 1:1 + kp[i]] = pos[i, :kp[i]]
            if H:
                kn[i] = [H, H // 2, 0, H][(i + step) % 4]
                roots[i, 1 + P:1 + P + kn[i]] = rng.permutation(N)[:kn[i]]
                seen.add("no hard" if kn[i] == 0 else "all hard" if kn[i] == H else "fewer hard")
            if kp[i] == 0 and (kn[i] > 0 or H == 0):
                seen.add("anchor without a positive")
            if kp[i] < P:
                seen.add("fewer positives")
        counts = np.concatenate([kp, kn]) if H else kp
        out.append((roots.reshape(-1).copy(), counts.astype(np.int32), rng.permutation(N)[:n_rn].astype(np.uint32)))
    want = {"anchor without a positive", "fewer positives"}
    if H:
        want |= {"no hard", "all hard"} | ({"fewer hard"} if H >= 2 else set())
    assert want <= seen, (want, seen)
    return out


def task_loss_torch(emb_main, emb_rn, counts, b, P, H, kind, param, weight):
    """the task over the roots' embeddings (emb_main [b T, d] anchor-major, emb_rn [n_rn, d]), in torch, for autograd:
    per (anchor, positive) the negatives are the anchor's own hard negatives and every random negative.
    Margin (MarginLoss, reduction sum / pairs): relu(m - pos + neg); Softmax: cross-entropy of the positive against its
    negatives at temperature T / positives.  -> (weight x loss, [m - pos + neg of every pair] for Margin | None)"""
    T, dev = 1 + P + H, emb_main.device
    counts = torch.as_tensor(counts).to(dev).to(torch.int64)
    kp = counts[:b]
    kn = counts[b:] if H else torch.zeros(b, dtype=torch.int64, device=dev)
    e = emb_main.view(b, T, -1)
    anchor = e[:, 0]
    pos = (anchor.unsqueeze(1) * e[:, 1:1 + P]).sum(-1)                                            # [b, P]
    neg = torch.cat([(anchor.unsqueeze(1) * e[:, 1 + P:]).sum(-1), anchor @ emb_rn.T], dim=1)      # [b, H + n_rn]
    ok_p = torch.arange(P, device=dev).view(1, P) < kp.view(-1, 1)
    ok_n = torch.cat([torch.arange(H, device=dev).view(1, H) < kn.view(-1, 1),
                      torch.ones((b, emb_rn.shape[0]), dtype=torch.bool, device=dev)], dim=1)
    pair = ok_p.unsqueeze(2) & ok_n.unsqueeze(1)                                                    # [b, P, H + n_rn]
    if kind == "Margin":
        h = param - pos.unsqueeze(2) + neg.unsqueeze(1)
        loss = (torch.relu(h) * pair).sum() / max(int(pair.sum()), 1)
        return weight * loss, h.detach()[pair]
    z = torch.cat([pos.unsqueeze(2), neg.unsqueeze(1).expand(b, P, -1)], dim=2) / param
    keep = torch.cat([torch.ones((b, P, 1), dtype=torch.bool, device=dev), pair], dim=2)
    lse = torch.logsumexp(z.masked_fill(~keep, float("-inf")), dim=2)
    loss = ((lse - pos / param) * ok_p).sum() / max(int(ok_p.sum()), 1)
    return weight * loss, None


def cpu_margin_kink(dims, b, P, H, n_rn, steps, batch_seed, model_seed, weight=1.0, lr=5e-3, weight_decay=1e-6, gat_heads=0):
    """the CPU restatement of `steps` Margin training steps of the GraphSAGE plan (oracle sample -> union -> gnn_ref fp32
    forward -> normalise -> the loss above -> autograd -> Adam) — gat_heads > 0: of the GAT plan (two gnn_ref.gat_conv layers,
    not normalised) — -> (pairs, smallest |m - pos + neg| over every pair of every step): how the plan test's seeds were chosen"""
    from gigl_amd.models import GraphSAGE
    from gigl_amd.models_attn import GAT
    rowptr, col, x = graph_and_features()
    batches = host_batches(rowptr, col, b, P, H, n_rn, steps, batch_seed)
    torch.manual_seed(model_seed)
    if gat_heads:
        model = GAT(*dims, num_layers=2, heads=gat_heads, should_l2_normalize_embedding_layer_output=False)
    else:
        model = GraphSAGE(*dims, num_layers=2, should_l2_normalize_embedding_layer_output=True)
    params = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(list(params.values()), lr=lr, weight_decay=weight_decay, foreach=False)
    pairs, closest = 0, float("inf")
    for roots, counts, rn in batches:
        embs = []
        for r in (roots, rn):
            nbr, _ = oracle.sample_khop(rowptr, col, r, FAN, canonical=True)
            u = oracle.union_build(r, FAN, nbr)
            ei = gnn_ref.union_edge_index(u["rowptr"], u["col"])
            out = torch.from_numpy(x[u["nodes"].astype(np.int64)])
            if gat_heads:
                for l, hd in enumerate((gat_heads, 1)):
                    q = f"conv_layers.{l}."
                    out = gnn_ref.gat_conv(out, ei, params[q + "lin.weight"], params[q + "att_src"], params[q + "att_dst"],
                                           params[q + "bias"], hd)
                    if l == 0:
                        out = torch.relu(out)
            else:
                out = torch.nn.functional.normalize(gnn_ref.graphsage_forward(out, ei, params, 2), p=2, dim=1)
            embs.append(out[torch.from_numpy(u["root_local"].astype(np.int64))])
        loss, h = task_loss_torch(embs[0], embs[1], counts, b, P, H, "Margin", MARGIN, weight)
        pairs += int(h.numel())
        closest = min(closest, float(h.abs().min()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    return pairs, closest
