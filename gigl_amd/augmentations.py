"""Graph augmentations for the two-view self-supervised tasks, over nn.GraphData.

Mirror of python/gigl/src/common/models/pyg/graph/augmentations.py:6-57 (drop_feature, get_augmented_graph): every edge is
kept with probability 1 - edge_drop_ratio (PyG dropout_edge), self loops are removed and one self loop per node is added,
and whole feature columns are zeroed with probability feat_drop_ratio; graph_perm (TBGRL's negative view) first shuffles the
rows of x and redraws every edge's ends.  Plain torch ops on whatever device the graph is
on: O(E + n D) per view, not the hot path.  `generator` makes the draws reproducible (the reference uses the global one).
"""
from __future__ import annotations

from typing import Optional

import torch

from .nn import GraphData


def _uniform(size: int, device, generator: Optional[torch.Generator]) -> torch.Tensor:
    # (drawn on the generator's device, the CPU unless told otherwise: the same seed gives the same view on any device)
    gen_dev = generator.device if generator is not None else device
    return torch.rand(size, dtype=torch.float32, device=gen_dev, generator=generator).to(device)


def drop_feature(x: torch.Tensor, drop_prob: float, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """augmentations.py:6-21: zero every column of x with probability drop_prob"""
    if drop_prob == 0:
        return x
    if drop_prob < 0 or drop_prob > 1:
        raise ValueError(f"Invalid probability provided for Feat Drop, got {drop_prob}")
    keep = _uniform(x.size(1), x.device, generator) >= drop_prob
    return x * keep.to(x.dtype)


def get_augmented_graph(graph: GraphData, edge_drop_ratio: float = 0.3, feat_drop_ratio: float = 0.3,
                        graph_perm: bool = False, generator: Optional[torch.Generator] = None) -> GraphData:
    """augmentations.py:24-57 -> a new GraphData (with its CSR when the graph is on the device); `graph` is left as it is"""
    if edge_drop_ratio < 0 or edge_drop_ratio > 1:
        raise ValueError(f"Invalid probability provided for Edge Drop, got {edge_drop_ratio}")
    if feat_drop_ratio < 0 or feat_drop_ratio > 1:
        raise ValueError(f"Invalid probability provided for Feat Drop, got {feat_drop_ratio}")
    if graph.edge_attr is not None:
        # (the reference masks edge_attr by the dropped edges and then rewrites the self loops of edge_index alone: the two
        # end up with different lengths)
        raise NotImplementedError("get_augmented_graph over a graph with edge_attr is not built")
    x, ei = graph.features(), graph.edge_index
    n, dev = int(x.shape[0]), x.device
    if graph_perm:
        # augmentations.py:44-47: the rows of x shuffled, every edge end redrawn below num_nodes - 1 (drawn on the generator's
        # device, as _uniform)
        gen_dev = generator.device if generator is not None else dev
        x = x[torch.randperm(n, device=gen_dev, generator=generator).to(dev)]
        ei = torch.randint(0, max(n - 1, 1), tuple(ei.shape), dtype=ei.dtype, device=gen_dev, generator=generator).to(dev)
    keep = ei[0] != ei[1]
    if edge_drop_ratio > 0:
        keep = keep & (_uniform(int(ei.shape[1]), dev, generator) >= edge_drop_ratio)
    loops = torch.arange(n, dtype=ei.dtype, device=dev)
    out = GraphData(x=drop_feature(x, feat_drop_ratio, generator),
                    edge_index=torch.cat((ei[:, keep], torch.stack((loops, loops))), dim=1))
    if dev.type == "cuda":
        out._build_csr()
    return out
