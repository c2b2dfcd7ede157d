"""TopK / RandomWeighted SamplingOps on the device (gigl_expand_frontier_keyed, csrc/keyed.hip) against the CPU
restatement of the rule (tests/keyed_rule.py): the bare expansion bit for bit over rows from empty to ~20k edges, the
typed DAG sampler per root and as device-encoded records, the one-call typed plan, and the sampler job end to end."""
import os
import shutil

import numpy as np
import pytest
import torch

import keyed_rule
from oracle import dag_sampler
from gigl_amd import wire
from gigl_amd.graphdb_sampler import (INCOMING, OUTGOING, RANDOM_WEIGHTED, TOP_K, EdgeType,
                                      HipGraphDBSampler, SamplingOp, SamplingOpDAG, _wrap)

pytestmark = pytest.mark.gpu

X = EdgeType("a", "x", "a")
INVALID = keyed_rule.INVALID


@pytest.fixture(scope="module")
def hubs():
    """one node type, one edge type: five hubs (in- and out-degree up to ~20k), a power-law bulk, repeated (src, dst)
    rows with different weights; weights = small integers (exact ties), signed zeros, negatives, a few NaN"""
    rng = np.random.default_rng(11)
    n = 30000
    src, dst = [], []
    for hub, deg in zip(range(5), (20000, 9000, 3000, 1500, 700)):
        others = rng.choice(np.arange(5, n), size=deg, replace=False)
        src += [others, np.full(deg, hub)]
        dst += [np.full(deg, hub), others]
    k = 60000
    src.append(rng.zipf(1.5, k) % n)
    dst.append(rng.integers(0, n, k))
    src, dst = np.concatenate(src).astype(np.uint32), np.concatenate(dst).astype(np.uint32)
    dup = rng.choice(src.size, 5000, replace=False)  # repeated rows: the first one's weight counts
    src, dst = np.concatenate([src, src[dup]]), np.concatenate([dst, dst[dup]])
    w = rng.integers(-3, 4, src.size).astype(np.float32)
    w[rng.random(src.size) < 0.1] = -0.0
    w[rng.random(src.size) < 0.01] = np.nan
    w[-5000:] = 100.0  # (would win every row if the repeats' weight were used)
    s = HipGraphDBSampler({"a": 0}, {"a": n}, {X: (src, dst)}, {X: 0}, edge_key_columns={X: {"w": w}})
    yield s, n, src, dst, w
    s.close()


def _frontier(rng, n):
    m = 3000
    nodes = rng.integers(0, n, m).astype(np.uint32)
    nodes[rng.choice(m, 40, replace=False)] = np.repeat(np.arange(5), 8)  # every hub, repeated
    nodes[rng.choice(m, 200, replace=False)] = INVALID
    nodes[:3] = [n + 5, INVALID, 0]  # (an id past the graph's rows: an empty slot)
    ksums = rng.integers(0, 2**32, m, dtype=np.uint64).astype(np.uint32)
    return nodes, ksums


def test_expand_frontier_keyed_matches_the_restatement(hubs):
    s, n, src, dst, w = hubs
    eng = s.engine
    rng = np.random.default_rng(5)
    nodes, ksums = _frontier(rng, n)
    nodes_d = torch.from_numpy(nodes.view(np.int32)).to(eng.device)
    ksums_d = torch.from_numpy(ksums.view(np.int32)).to(eng.device)
    from gigl_amd._lib import SAMPLE_RANDOM_WEIGHTED, SAMPLE_TOPK
    for direction in (INCOMING, OUTGOING):
        rows, cols = (dst, src) if direction == INCOMING else (src, dst)
        rowptr, col, kw = keyed_rule.csr_with_weights(n, rows, cols, w)
        key_col = s.key_column(X, direction, "w")
        assert np.array_equal(key_col.cpu().numpy().view(np.uint32), kw.view(np.uint32))  # first row wins, col order
        assert int(np.diff(rowptr).max()) >= 20000
        for method, code in (("top_k", SAMPLE_TOPK), ("random_weighted", SAMPLE_RANDOM_WEIGHTED)):
            for f in (1, 7, 64, 65, 257, 1024):
                hash_add = 42 * (1 + f % 5)
                nbr, cnt = eng.expand_frontier_keyed(nodes_d, ksums_d, f, hash_add, code, key_col,
                                                     s._key(X, direction))
                want_nbr, want_cnt = keyed_rule.expand(rowptr, col, kw, nodes, ksums, f, hash_add, method)
                got_nbr = nbr.cpu().numpy().view(np.uint32)
                assert np.array_equal(cnt.cpu().numpy(), want_cnt), (direction, method, f)
                bad = np.flatnonzero((got_nbr != want_nbr).reshape(-1, f).any(axis=1))
                assert bad.size == 0, (direction, method, f, bad[:5], nodes[bad[:5]])
    # fanouts outside [1, GIGL_MAX_FANOUT] are unsupported, as for the uniform rule
    from gigl_amd._lib import GiglError
    with pytest.raises(GiglError):
        eng.expand_frontier_keyed(nodes_d, ksums_d, 1025, 42, SAMPLE_TOPK, s.key_column(X, INCOMING, "w"), s._key(X, INCOMING))


def test_uniform_ops_unchanged_beside_keyed_columns(hubs):
    """a sampler with keyed columns loaded samples uniform ops exactly like one without"""
    s, n, src, dst, w = hubs
    plain = HipGraphDBSampler({"a": 0}, {"a": n}, {X: (src, dst)}, {X: 0})
    try:
        s.key_column(X, OUTGOING, "w")
        ops = [SamplingOp("u1", X, 10, [], INCOMING), SamplingOp("k", X, 5, ["u1"], INCOMING, TOP_K, "w"),
               SamplingOp("u2", X, 7, ["u1"], OUTGOING)]
        roots = torch.from_numpy(np.random.default_rng(3).integers(0, n, 300).astype(np.int32))
        dag = SamplingOpDAG.from_ops(ops)
        r_keyed = s.run_dag(roots, dag)
        # (the same op positions — an op's counter is 1 + its position — with the keyed op made uniform)
        r_plain = plain.run_dag(roots, SamplingOpDAG.from_ops([ops[0], SamplingOp("k", X, 5, ["u1"], INCOMING), ops[2]]))
        for name in ("u1", "u2"):
            assert torch.equal(r_keyed[name].nbr.cpu(), r_plain[name].nbr.cpu()), name
            assert torch.equal(r_keyed[name].cnt.cpu(), r_plain[name].cnt.cpu()), name
    finally:
        plain.close()


def _reference_fixture(golden_dir):
    from gigl_amd.ingest import COL_F32, COL_I64, read_columns
    base = os.path.join(golden_dir, "ref_assets/subgraph_sampler/heterogeneous/node_anchor_based_link_prediction")

    def table(rel, cols):
        data, _ = read_columns([os.path.join(base, rel, "data.tfrecord")], cols)
        return data
    nodes = {"author": table("node_features_dir/user/features", [("node_id", COL_I64, 1), ("f0", COL_F32, 1), ("f1", COL_F32, 1)]),
             "paper": table("node_features_dir/story/features", [("node_id", COL_I64, 1), ("f0", COL_F32, 1), ("f1", COL_F32, 1)])}
    a2p, p2a = EdgeType("author", "author_to_paper", "paper"), EdgeType("paper", "paper_to_author", "author")
    ecols = [("src", COL_I64, 1), ("dst", COL_I64, 1), ("f0", COL_F32, 1), ("f1", COL_F32, 1)]
    et_tables = {a2p: table("edge_features_dir/user-to-story/main_edges/features", ecols),
                 p2a: table("edge_features_dir/story-to-user/main_edges/features", ecols)}
    n = {t: int(d["node_id"].max()) + 1 for t, d in nodes.items()}
    feats = {}
    for t, d in nodes.items():
        x = np.zeros((n[t], 2), np.float32)
        x[d["node_id"][:, 0]] = np.concatenate([d["f0"], d["f1"]], axis=1)
        feats[t] = x
    edges = {et: (d["src"][:, 0].astype(np.uint32), d["dst"][:, 0].astype(np.uint32)) for et, d in et_tables.items()}
    efeats = {et: np.concatenate([d["f0"], d["f1"]], axis=1) for et, d in et_tables.items()}
    cols = {et: {"f0": efeats[et][:, 0].copy(), "f1": efeats[et][:, 1].copy()} for et in edges}
    return a2p, p2a, n, feats, edges, efeats, cols


def _mixed_plans(a2p, p2a):
    return {"paper": [SamplingOp("u", a2p, 3, [], INCOMING),
                      SamplingOp("t", a2p, 1, ["u"], OUTGOING, TOP_K, "f0"),
                      SamplingOp("w", p2a, 1, ["t"], OUTGOING, RANDOM_WEIGHTED, "f1")],
            "author": [SamplingOp("t", p2a, 2, [], INCOMING, TOP_K, "f0"),
                       SamplingOp("w", a2p, 1, ["t"], INCOMING, RANDOM_WEIGHTED, "f1"),
                       SamplingOp("u", a2p, 2, [], OUTGOING)]}


def test_reference_fixture_mixed_dag(golden_dir):
    """the reference's heterogeneous fixture, a DAG mixing uniform, topK(f0) and randomWeighted(f1) ops: run_dag per
    root == the restatement; the device-encoded typed records == the host assembly, byte for byte; the one-call typed
    plan == the staged path (batch graphs and every op's results)"""
    a2p, p2a, n, feats, edges, efeats, cols = _reference_fixture(golden_dir)
    types, cet = {"author": 0, "paper": 1}, {a2p: 0, p2a: 1}
    s = HipGraphDBSampler(types, n, edges, cet, feats, edge_features=efeats, edge_key_columns=cols)
    try:
        nbrs = dag_sampler.neighbour_lists(edges)
        weights = keyed_rule.neighbour_weights(edges, cols)
        for root_type, ops in _mixed_plans(a2p, p2a).items():
            dag = SamplingOpDAG.from_ops(ops)
            roots = np.arange(n[root_type])
            msgs = s.getKHopSubgraphForRootNodes(roots, root_type, dag)
            for r, m in zip(roots, msgs):
                want_e, want_n = keyed_rule.sample_for_root(int(r), ops, nbrs, weights, types, cet, root_type)
                assert {(e.src_node_id, e.dst_node_id, e.condensed_edge_type) for e in m.neighborhood.edges} == want_e
                assert {(x.node_id, x.condensed_node_type) for x in m.neighborhood.nodes} == want_n
            dev = s.encode_records(roots, root_type, dag, tfrecord_frame=False)
            assert [m.SerializeToString() for m in msgs] == dev
            # the one-call plan: batch graphs and op results equal to the staged path
            g0, ri0, u0 = s.batch_graph(roots, root_type, dag)
            g1, ri1, u1 = s.batch_graph_plan(roots, root_type, dag, b_max=64)
            torch.cuda.synchronize()
            assert set(u0) == set(u1) and all(torch.equal(u0[t], u1[t]) for t in u0)
            assert all(torch.equal(g0.edge_index_dict[k], g1.edge_index_dict[k]) for k in g0.edge_index_dict)
            assert torch.equal(ri0, ri1)
            res = s.run_dag(torch.from_numpy(roots.astype(np.int32)), dag)
            pl = s.typed_plan(root_type, dag, 64)
            for i, name in enumerate(pl["order"]):
                r = res[name]
                b, w_, f = r.nbr.shape
                assert int(pl["out"].op_width[i]) == w_
                got = _wrap(pl["out"].op_nbr[i], b * w_ * f, torch.int32, s.engine.device)
                assert torch.equal(got.cpu(), r.nbr.reshape(-1).cpu()), (root_type, name)
                got_c = _wrap(pl["out"].op_cnt[i], b * w_, torch.int32, s.engine.device)
                assert torch.equal(got_c.cpu(), r.cnt.reshape(-1).cpu()), (root_type, name)
        # (some keyed rows are longer than their op's fanout: the keys decide)
        assert any(row.size > 2 for d in weights.values() for row, _ in d.values())
    finally:
        s.close()


def test_keyed_ops_on_a_dblp_shaped_graph():
    """rows long enough to select from (a Zipf author side): per-root sets == the restatement, the one-call plan (and
    a clone of it) == the staged path"""
    rng = np.random.default_rng(21)
    n = {"author": 3000, "paper": 5000}
    k = 40000
    a = (rng.zipf(1.6, k) % n["author"]).astype(np.uint32)
    p = rng.integers(0, n["paper"], k).astype(np.uint32)
    a2p, p2a = EdgeType("author", "author_to_paper", "paper"), EdgeType("paper", "paper_to_author", "author")
    edges = {a2p: (a, p), p2a: (p, a)}
    cols = {et: {"f0": rng.integers(0, 5, k).astype(np.float32), "f1": rng.random(k).astype(np.float32)} for et in edges}
    types, cet = {"author": 0, "paper": 1}, {a2p: 0, p2a: 1}
    feats = {t: rng.standard_normal((n[t], 4)).astype(np.float32) for t in n}
    s = HipGraphDBSampler(types, n, edges, cet, feats, edge_key_columns=cols)
    try:
        nbrs = dag_sampler.neighbour_lists(edges)
        weights = keyed_rule.neighbour_weights(edges, cols)
        ops = [SamplingOp("t", a2p, 70, [], INCOMING, TOP_K, "f0"),
               SamplingOp("w", a2p, 5, ["t"], OUTGOING, RANDOM_WEIGHTED, "f1"),
               SamplingOp("u", p2a, 3, ["w"], OUTGOING)]
        dag = SamplingOpDAG.from_ops(ops)
        roots = rng.choice(n["paper"], 200, replace=False)
        msgs = s.getKHopSubgraphForRootNodes(roots, "paper", dag)
        for r, m in zip(roots, msgs):
            want_e, want_n = keyed_rule.sample_for_root(int(r), ops, nbrs, weights, types, cet, "paper")
            assert {(e.src_node_id, e.dst_node_id, e.condensed_edge_type) for e in m.neighborhood.edges} == want_e
        g0, ri0, u0 = s.batch_graph(roots, "paper", dag)
        g1, ri1, u1 = s.batch_graph_plan(roots, "paper", dag, b_max=256)
        torch.cuda.synchronize()
        assert all(torch.equal(u0[t], u1[t]) for t in u0)
        assert all(torch.equal(g0.edge_index_dict[k], g1.edge_index_dict[k]) for k in g0.edge_index_dict)
        import ctypes as C
        from gigl_amd import _lib
        eng = s.engine
        pl = s.typed_plan("paper", dag, 256)
        clone = C.c_void_p()
        _lib.check(eng._lib.gigl_typed_plan_clone(pl["plan"], eng._ctx, C.byref(clone)), eng._ctx)
        try:
            out = _lib.GiglTypedPlanOut()
            _lib.check(eng._lib.gigl_typed_plan_buffers(clone, C.byref(out)), eng._ctx)
            rt = torch.from_numpy(roots.astype(np.int32)).to(eng.device)
            _lib.check(eng._lib.gigl_typed_plan_run(clone, C.c_void_p(rt.data_ptr()), len(roots)), eng._ctx)
            res = s.run_dag(rt, dag)
            torch.cuda.synchronize()
            for i, name in enumerate(pl["order"]):
                b, w_, f = res[name].nbr.shape
                got = _wrap(out.op_nbr[i], b * w_ * f, torch.int32, eng.device)
                assert torch.equal(got.cpu(), res[name].nbr.reshape(-1).cpu()), name
        finally:
            eng._lib.gigl_typed_plan_destroy(clone)
    finally:
        s.close()


@pytest.fixture(scope="module")
def workdir(golden_dir, tmp_path_factory):
    base = tmp_path_factory.mktemp("gigl_keyed")
    shutil.copytree(os.path.join(golden_dir, "configs"), base / "configs")
    shutil.copytree(os.path.join(golden_dir, "ref_assets"), base / "ref_assets")
    return str(base)


def test_subgraph_sampler_job_with_top_k(workdir):
    """SubgraphSampler.run on the reference's heterogeneous config with a strategy whose ops are topK: every frontier
    node's sampled edges in the written TFRecords are its top-f by the feature (ties to the lower id)"""
    import yaml
    from gigl_amd.config import GbmlConfigPbWrapper, tfrecord_files
    from gigl_amd.subgraph_sampler import SubgraphSampler, load_preprocessed_typed_graph
    doc = yaml.safe_load(open(os.path.join(workdir, "configs/hetero_nablp_frozen_gbml_config.yaml")))
    a2p = {"srcNodeType": "author", "relation": "author_to_paper", "dstNodeType": "paper"}
    p2a = {"srcNodeType": "paper", "relation": "paper_to_author", "dstNodeType": "author"}
    doc["datasetConfig"]["subgraphSamplerConfig"]["subgraphSamplingStrategy"] = {"messagePassingPaths": {"paths": [
        {"rootNodeType": "paper", "samplingOps": [
            {"opName": "k", "edgeType": a2p, "topK": {"numNodesToSample": 1, "edgeFeatName": "f0"}}]},
        {"rootNodeType": "author", "samplingOps": [
            {"opName": "k", "edgeType": p2a, "topK": {"numNodesToSample": 1, "edgeFeatName": "f1"}}]}]}}
    out = doc["sharedConfig"]["flattenedGraphMetadata"]["nodeAnchorBasedLinkPredictionOutput"]
    for key, v in out.items():
        if isinstance(v, str):
            out[key] = v.replace("hetero_nablp", "hetero_topk")
        else:
            for t in v:
                v[t] = v[t].replace("hetero_nablp", "hetero_topk")
    uri = "configs/hetero_topk_gbml_config.yaml"
    yaml.safe_dump(doc, open(os.path.join(workdir, uri), "w"))
    SubgraphSampler().run("job", uri, None, uri_base=workdir)
    cfg = GbmlConfigPbWrapper.from_uri(uri, uri_base=workdir)
    node_types, num, ids, feats, edges, cet, efeats = load_preprocessed_typed_graph(cfg)
    name_of = {"author": ("paper_to_author", 1), "paper": ("author_to_paper", 0)}  # (the op's edge type, feature column)
    checked = 0
    for t in ("author", "paper"):
        rel, fcol = name_of[t]
        et = [e for e in cet if e.relation == rel][0]
        src, dst = edges[et]
        rp, cl, ww = keyed_rule.csr_with_weights(max(num.values()), dst, src, efeats[et][:, fcol])  # INCOMING rows
        recs = [wire.RootedNodeNeighborhood.FromString(r) for f in tfrecord_files(cfg.random_negative_tfrecord_uri_prefixes[t])
                for r in wire.read_tfrecords(f)]
        assert sorted(m.root_node.node_id for m in recs) == ids[t].tolist()
        for m in recs:
            v = m.root_node.node_id
            row, w = cl[rp[v]:rp[v + 1]], ww[rp[v]:rp[v + 1]]
            got = sorted(e.src_node_id for e in m.neighborhood.edges if e.dst_node_id == v and e.condensed_edge_type == cet[et])
            want = keyed_rule.pick(row, w, 1, "top_k").tolist()
            assert got == want, (t, v)
            if row.size > 1:
                k_ = np.where(np.isnan(w), -np.inf, w)
                assert got == [int(row[np.argmax(k_)])]  # the largest weight, the lowest id among equals
                checked += 1
    assert checked > 0
