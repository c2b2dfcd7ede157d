"""The host side of link-prediction plans in a world of ranks, without a GPU: the train_plan trainer argument, and the rank
striding of the ROOT batches a plan is fed (ResidentGraph.nablp_root_batches / random_negative_root_batches) — a rank's plan
route must see the anchors and the random negatives its autograd route (nablp_batches / random_negative_batches) sees, in
the same number on every rank, or the ranks of a data-parallel job would step a different number of times."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch


def test_train_plan_argument_is_checked(monkeypatch):
    """an unknown value raises, as eval_plan's does; "off" and a job off the in-HBM route keep the autograd loop"""
    from gigl_amd.nablp_spec import HipNodeAnchorLinkPredictionSpec
    for bad in ("sometimes", "yes", "1", ""):
        with pytest.raises(ValueError):
            HipNodeAnchorLinkPredictionSpec(train_plan=bad)._library_plan(None)
    no_hbm = lambda self, cfg: None
    monkeypatch.setattr(HipNodeAnchorLinkPredictionSpec, "_hbm_split", no_hbm)
    for ok in ("auto", "on", "off", "OFF", "Auto"):
        assert HipNodeAnchorLinkPredictionSpec(train_plan=ok)._library_plan(None) is None
    assert HipNodeAnchorLinkPredictionSpec()._library_plan(None) is None


class _FakeEngine:
    """sample_positives of an engine: positive j of anchor a is 1000 * (j + 1) + a, anchors divisible by 3 have one fewer"""

    def sample_positives(self, anchors, P, sampling_seed=42):
        a = anchors.to(torch.int64).view(-1, 1)
        pos = (1000 * (torch.arange(P).view(1, P) + 1) + a).to(torch.int32)
        cnt = torch.where(a.view(-1) % 3 == 0, P - 1, P).to(torch.int32)
        return pos.reshape(-1), cnt


def _resident(rank, world, n_nodes=23):
    from gigl_amd.hbm import ResidentGraph
    res = object.__new__(ResidentGraph)
    res.rank, res.world, res.device, res.seed = rank, world, torch.device("cpu"), 42
    res.engine = _FakeEngine()
    res.node_ids, res._order_prefixes = np.arange(n_nodes, dtype=np.int64), []
    res.train_graph = lambda roots, pad_to=None: (SimpleNamespace(roots=roots.clone()), None)
    return res


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n_ids,batch", [(23, 4), (24, 4), (3, 4), (17, 1)])
def test_a_ranks_root_batches_are_the_spans_of_its_graph_batches(world, n_ids, batch):
    """anchors: the root batches of rank r hold the anchors, positives and counts of nablp_batches' batches of rank r, as many
    on every rank (a short rank wraps around); together the ranks cover every anchor"""
    P = 2
    ids = (np.arange(n_ids, dtype=np.int64) * 5 + 1) % 97
    n_pos = np.full(n_ids, P, dtype=np.int64)
    counts, covered = [], set()
    for rank in range(world):
        res = _resident(rank, world)
        graph_side = list(res.nablp_batches(ids, n_pos, batch, P))
        root_side = list(res.nablp_root_batches(ids, n_pos, batch, P))
        assert len(graph_side) == len(root_side)
        for g, (roots, cnt, chunk) in zip(graph_side, root_side):
            assert np.array_equal(g.anchor_ids, chunk)
            assert torch.equal(g.graph.roots, roots) and cnt.dtype == torch.int32
            assert roots.numel() == chunk.size * (1 + P) and torch.equal(roots.view(-1, 1 + P)[:, 0].long(), torch.from_numpy(chunk))
            covered.update(chunk.tolist())
        counts.append(len(root_side))
    n_batches = -(-n_ids // batch)
    assert counts == [-(-n_batches // world)] * world
    assert covered == set(ids.tolist())


@pytest.mark.parametrize("world", [1, 2, 3])
def test_a_ranks_random_negative_roots_are_its_random_negative_batches(world):
    """random negatives: the looping root stream of rank r is the root_ids of random_negative_batches' stream of rank r —
    over more than one pass, the short last chunk of a pass included"""
    from itertools import islice
    n_nodes, batch = 23, 4
    n_chunks = -(-n_nodes // batch)
    take = 2 * -(-n_chunks // world) + 1
    seen = set()
    for rank in range(world):
        res = _resident(rank, world, n_nodes)
        graph_side = [b.root_ids for b in islice(res.random_negative_batches(batch), take)]
        root_side = [r.numpy().view(np.uint32).astype(np.int64) for r in islice(res.random_negative_root_batches(batch), take)]
        assert len(graph_side) == len(root_side) == take
        for g, r in zip(graph_side, root_side):
            assert np.array_equal(g, r)
        seen.update(int(v) for r in root_side for v in r)
    assert seen == set(range(n_nodes))
