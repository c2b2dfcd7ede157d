"""TEST INFRASTRUCTURE ONLY: CPU restatement of the keyed SamplingOp methods (TopK / RandomWeighted) of the typed DAG
sampler, the results contract of gigl_expand_frontier_keyed (include/gigl_hip.h):
  TopK            key[i] = w[i]
  RandomWeighted  key[i] = fl32(w[i] * u[i]), u[i] = ((xxh64_int32((i + 1) + K + seed*counter) >> 40) + 1) * 2^-24
the f largest keys (IEEE order, -0 == +0, NaN below every number, ties to the lower position), returned ascending by id.
The hash is the CPU oracle's exported xxh64 (through ctypes); everything else is numpy float32."""
from collections import deque

import numpy as np

from oracle.oracle import xxh64_int32

MASK = 0xFFFFFFFF
INVALID = 0xFFFFFFFF


def random_weighted_u(n: int, ksum: int, hash_add: int) -> np.ndarray:
    """u[0..n) of one row: position i hashes wrap32((i + 1) + K + seed*counter)"""
    base = (int(ksum) + int(hash_add)) & MASK
    h = np.array([xxh64_int32((base + i + 1) & MASK) for i in range(n)], dtype=np.uint64)
    return ((h >> np.uint64(40)) + np.uint64(1)).astype(np.float32) * np.float32(2.0 ** -24)


def row_keys(w, method: str, ksum: int = 0, hash_add: int = 0) -> np.ndarray:
    w = np.asarray(w, dtype=np.float32)
    if method == "top_k":
        return w
    assert method == "random_weighted", method
    return (w * random_weighted_u(w.size, ksum, hash_add)).astype(np.float32)


def pick(row, w, f: int, method: str, ksum: int = 0, hash_add: int = 0) -> np.ndarray:
    """the taken neighbours of one row (ascending ids); n <= f: the whole row, no key read"""
    row = np.asarray(row, dtype=np.uint32)
    if row.size <= f:
        return row.copy()
    key = row_keys(w, method, ksum, hash_add)
    nan = np.isnan(key)
    neg = np.where(nan, np.float32(0), -key)  # (-0 and +0 compare equal: the position decides)
    order = np.lexsort((np.arange(row.size), neg, nan))  # numbers first, larger key first, lower position first
    return np.sort(row[np.sort(order[:f])])


def expand(rowptr, col, key_col, nodes, ksums, f: int, hash_add: int, method: str):
    """gigl_expand_frontier_keyed on host arrays -> (nbr [m*f] uint32, cnt [m] int32)"""
    m = len(nodes)
    nbr = np.full(m * f, INVALID, dtype=np.uint32)
    cnt = np.zeros(m, dtype=np.int32)
    n_rows = len(rowptr) - 1
    for i, (v, k) in enumerate(zip(np.asarray(nodes, dtype=np.uint32).tolist(), np.asarray(ksums, dtype=np.uint32).tolist())):
        if v == INVALID or v >= n_rows:
            continue
        s, e = int(rowptr[v]), int(rowptr[v + 1])
        got = pick(col[s:e], key_col[s:e], f, method, k, hash_add)
        nbr[i * f:i * f + got.size] = got
        cnt[i] = got.size
    return nbr, cnt


def csr_with_weights(n: int, rows, cols, w):
    """CSR over distinct (row, col) pairs, ascending columns; the weight of a pair = its FIRST input row's"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    w = np.asarray(w, dtype=np.float32)
    key = rows * (1 << 32) + cols
    uniq, first = np.unique(key, return_index=True)  # (np.unique returns the first occurrence)
    r = (uniq >> 32).astype(np.int64)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, r + 1, 1)
    return np.cumsum(rowptr), (uniq & MASK).astype(np.uint32), w[first]


def neighbour_weights(edges, columns):
    """edges {et: (src, dst)}, columns {et: {name: fp32 [n_edges]}} ->
    {(et, direction, name): {node: (sorted distinct neighbours, their weights)}} (first input row wins)"""
    out = {}
    for et, cols in columns.items():
        src, dst = (np.asarray(a, dtype=np.int64) for a in edges[et])
        n = int(max(src.max(initial=0), dst.max(initial=0))) + 1
        for direction, rows, other in (("INCOMING", dst, src), ("OUTGOING", src, dst)):
            for name, w in cols.items():
                rp, cl, ww = csr_with_weights(n, rows, other, w)
                out[(et, direction, name)] = {v: (cl[rp[v]:rp[v + 1]], ww[rp[v]:rp[v + 1]])
                                              for v in range(n) if rp[v + 1] > rp[v]}
    return out


def sample_for_root(root, ops, nbrs, weights, node_types, condensed_edge_types, root_type, sampling_seed=42):
    """oracle/dag_sampler.sample_for_root's traversal with the op's own pick: the hash permutation for a uniform op,
    the keyed rule above for top_k / random_weighted -> (edge set, node set)"""
    from oracle.oracle import hash_permutation
    by_name = {op.op_name: op for op in ops}
    children = {op.op_name: [] for op in ops}
    for op in ops:
        for p in op.input_op_names:
            if p in by_name:
                children[p].append(op.op_name)
    parents = {op.op_name: [p for p in op.input_op_names if p in by_name] for op in ops}
    queue = deque(op.op_name for op in ops if not op.input_op_names)
    results = {}
    while queue:
        name = queue.popleft()
        op = by_name[name]
        if name in results:
            continue
        if not parents[name]:
            frontier = [root]
        else:
            if not all(p in results for p in parents[name]):
                continue
            frontier = sorted({v for p in parents[name] for v, _ in results[p][1]})
        if not frontier:
            continue
        outgoing = op.sampling_direction == "OUTGOING"
        direction = "OUTGOING" if outgoing else "INCOMING"
        cet = condensed_edge_types[op.edge_type]
        got_type = node_types[op.edge_type.dst_node_type if outgoing else op.edge_type.src_node_type]
        counter = 1 + [o.op_name for o in ops].index(name)
        method = getattr(op, "sampling_method", "random_uniform")
        e_set, n_set = set(), set()
        for v in frontier:
            if method == "random_uniform":
                row = nbrs[(op.edge_type, direction)].get(v)
                if row is None:
                    continue
                taken = hash_permutation(row, (root + v) & MASK, sampling_seed=sampling_seed,
                                         counter=counter)[: op.num_nodes_to_sample]
            else:
                rw = weights[(op.edge_type, direction, op.edge_feat_name)].get(v)
                if rw is None:
                    continue
                taken = pick(rw[0], rw[1], op.num_nodes_to_sample, method, (root + v) & MASK,
                             (sampling_seed * counter) & MASK)
            for u in taken.tolist():
                e_set.add((v, u, cet) if outgoing else (u, v, cet))
                n_set.add((u, got_type))
        results[name] = (e_set, n_set)
        queue.extend(children[name])
    edges, nodes = set(), {(root, node_types[root_type])}
    for e_set, n_set in results.values():
        edges |= e_set
        nodes |= n_set
    return edges, nodes
