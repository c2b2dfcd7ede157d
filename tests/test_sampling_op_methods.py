"""The keyed SamplingOp methods (TopK / RandomWeighted, subgraph_sampling_strategy.proto:7-58) on the host: config
parsing into SamplingOp, the per-op validation of sampling_op.py:46-84, and the CPU restatement of the selection rule
(tests/keyed_rule.py) on hand-worked rows."""
import json
import os

import numpy as np
import pytest
import yaml

from keyed_rule import MASK, pick, random_weighted_u, row_keys
from gigl_amd.config import GbmlConfigPbWrapper
from gigl_amd.graphdb_sampler import (INCOMING, OUTGOING, RANDOM_UNIFORM, RANDOM_WEIGHTED, TOP_K, EdgeType, SamplingOp,
                                      SubgraphSamplingValidationError, validate_sampling_op_dags)

A2P = EdgeType("author", "author_to_paper", "paper")
P2A = EdgeType("paper", "paper_to_author", "author")
A2P_D = {"srcNodeType": "author", "relation": "author_to_paper", "dstNodeType": "paper"}
P2A_D = {"srcNodeType": "paper", "relation": "paper_to_author", "dstNodeType": "author"}


def _cfg(golden_dir, ops_paper, ops_author=None):
    doc = yaml.safe_load(open(os.path.join(golden_dir, "configs", "hetero_nablp_frozen_gbml_config.yaml")))
    paths = [{"rootNodeType": "paper", "samplingOps": ops_paper}]
    if ops_author is not None:
        paths.append({"rootNodeType": "author", "samplingOps": ops_author})
    doc["datasetConfig"]["subgraphSamplerConfig"]["subgraphSamplingStrategy"] = {"messagePassingPaths": {"paths": paths}}
    cfg = GbmlConfigPbWrapper(doc)
    cfg.uri_base = golden_dir
    return cfg


def _dags(cfg):
    from gigl_amd.subgraph_sampler import sampling_op_dags
    return sampling_op_dags(cfg, ["paper", "author"])


# ---- SamplingOp and config parsing -------------------------------------------------------------------------------
def test_sampling_op_defaults_keep_positional_construction():
    op = SamplingOp("a", A2P, 3, [], OUTGOING)
    assert op.sampling_method == RANDOM_UNIFORM and op.edge_feat_name is None and not op.keyed
    k = SamplingOp("k", A2P, 3, [], INCOMING, TOP_K, "f0")
    assert k.keyed and k.edge_feat_name == "f0"


def test_config_parses_all_three_methods(golden_dir):
    cfg = _cfg(golden_dir, [
        {"opName": "u", "edgeType": A2P_D, "randomUniform": {"numNodesToSample": 3}},
        {"opName": "t", "edgeType": A2P_D, "inputOpNames": ["u"], "samplingDirection": "OUTGOING",
         "topK": {"numNodesToSample": 2, "edgeFeatName": "f0"}},
        {"opName": "w", "edgeType": P2A_D, "inputOpNames": ["t"], "samplingDirection": "OUTGOING",
         "randomWeighted": {"numNodesToSample": 4, "edgeFeatName": "f1"}}])
    dag = _dags(cfg)["paper"]
    ops = {n: dag.nodes[n].sampling_op for n in dag.op_order}
    assert (ops["u"].sampling_method, ops["u"].num_nodes_to_sample, ops["u"].edge_feat_name) == (RANDOM_UNIFORM, 3, None)
    assert (ops["t"].sampling_method, ops["t"].num_nodes_to_sample, ops["t"].edge_feat_name) == (TOP_K, 2, "f0")
    assert (ops["w"].sampling_method, ops["w"].num_nodes_to_sample, ops["w"].edge_feat_name) == (RANDOM_WEIGHTED, 4, "f1")
    assert ops["t"].sampling_direction == OUTGOING and ops["t"].input_op_names == ["u"]


def test_edge_key_columns_cut_the_named_feature(golden_dir):
    from gigl_amd.subgraph_sampler import edge_key_columns, load_preprocessed_typed_graph, typed_edge_feature_layout
    cfg = _cfg(golden_dir, [{"opName": "t", "edgeType": A2P_D, "topK": {"numNodesToSample": 2, "edgeFeatName": "f1"}}])
    layout = typed_edge_feature_layout(cfg)
    assert layout[A2P] == [("f0", 1), ("f1", 1)]
    _, _, _, _, edges, _, efeats = load_preprocessed_typed_graph(cfg)
    cols = edge_key_columns(cfg, _dags(cfg), efeats)
    assert list(cols) == [A2P] and list(cols[A2P]) == ["f1"]
    np.testing.assert_array_equal(cols[A2P]["f1"], efeats[A2P][:, 1])
    assert cols[A2P]["f1"].shape == (edges[A2P][0].size,)


# ---- validation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op, error_type", [
    ({"opName": "z", "edgeType": A2P_D, "randomUniform": {"numNodesToSample": 0}}, "INVALID_NUM_NODES_TO_SAMPLE"),
    ({"opName": "z", "edgeType": A2P_D, "topK": {"numNodesToSample": -1, "edgeFeatName": "f0"}}, "INVALID_NUM_NODES_TO_SAMPLE"),
    ({"opName": "z", "edgeType": A2P_D, "topK": {"numNodesToSample": 2}}, "EMPTY_EDGE_FEAT_NAME"),
    ({"opName": "z", "edgeType": A2P_D, "randomWeighted": {"numNodesToSample": 2, "edgeFeatName": ""}}, "EMPTY_EDGE_FEAT_NAME"),
    ({"opName": "z", "edgeType": A2P_D, "topK": {"numNodesToSample": 2, "edgeFeatName": "weight"}},
     "EDGE_FEAT_NAME_NOT_IN_EDGE_FEATURES"),
    ({"opName": "z", "edgeType": A2P_D, "userDefined": {"pathToUdf": "x.y"}}, "UNSUPPORTED_SAMPLING_METHOD"),
])
def test_config_validation_errors(golden_dir, op, error_type):
    with pytest.raises(SubgraphSamplingValidationError) as e:
        _dags(_cfg(golden_dir, [op]))
    assert e.value.error_type == error_type


def test_validation_of_keyed_ops_against_feature_keys():
    nts, ets = ["author", "paper"], [A2P, P2A]
    keys = {A2P: {"f0": 1, "emb": 4}, P2A: {"f0": 1}}
    ok = {"paper": [SamplingOp("t", A2P, 2, [], INCOMING, TOP_K, "f0")]}
    validate_sampling_op_dags(ok, nts, ets, edge_feature_keys=keys)
    validate_sampling_op_dags(ok, nts, ets)  # (no feature keys given: only the name's presence is checked)
    cases = [(SamplingOp("t", A2P, 2, [], INCOMING, TOP_K, "emb"), "EDGE_FEAT_NOT_SCALAR"),
             (SamplingOp("t", A2P, 2, [], INCOMING, RANDOM_WEIGHTED, "nope"), "EDGE_FEAT_NAME_NOT_IN_EDGE_FEATURES"),
             (SamplingOp("t", A2P, 2, [], INCOMING, RANDOM_WEIGHTED, None), "EMPTY_EDGE_FEAT_NAME"),
             (SamplingOp("t", A2P, 0, [], INCOMING), "INVALID_NUM_NODES_TO_SAMPLE"),
             (SamplingOp("t", A2P, 2, [], INCOMING, "user_defined"), "UNSUPPORTED_SAMPLING_METHOD")]
    for op, err in cases:
        with pytest.raises(SubgraphSamplingValidationError) as e:
            validate_sampling_op_dags({"paper": [op]}, nts, ets, edge_feature_keys=keys)
        assert e.value.error_type == err, (op, err)
    # (a keyed op on an edge type without features)
    with pytest.raises(SubgraphSamplingValidationError) as e:
        validate_sampling_op_dags({"author": [SamplingOp("t", P2A, 2, [], INCOMING, TOP_K, "f0")]}, nts, ets,
                                  edge_feature_keys={A2P: {"f0": 1}})
    assert e.value.error_type == "EDGE_FEAT_NAME_NOT_IN_EDGE_FEATURES"


# ---- the selection rule on hand-worked rows --------------------------------------------------------------------------
ROW = np.array([3, 5, 8, 13, 21, 34], dtype=np.uint32)


def test_top_k_order_and_ties():
    w = np.array([1, 4, 4, 2, 4, 0], dtype=np.float32)
    # keys 4 at positions 1, 2, 4: ties go to the lower position
    assert pick(ROW, w, 1, "top_k").tolist() == [5]
    assert pick(ROW, w, 2, "top_k").tolist() == [5, 8]
    assert pick(ROW, w, 3, "top_k").tolist() == [5, 8, 21]
    assert pick(ROW, w, 4, "top_k").tolist() == [5, 8, 13, 21]  # then key 2 (13), output ascending by id


def test_nan_ranks_below_every_number_and_signed_zeros_tie():
    w = np.array([np.nan, -np.inf, -0.0, 0.0, np.nan, -1.0], dtype=np.float32)
    assert pick(ROW, w, 1, "top_k").tolist() == [8]  # -0 (position 2) == +0 (position 3): the lower position
    assert pick(ROW, w, 2, "top_k").tolist() == [8, 13]
    assert pick(ROW, w, 3, "top_k").tolist() == [8, 13, 34]  # -1
    assert pick(ROW, w, 4, "top_k").tolist() == [5, 8, 13, 34]  # -inf before either NaN
    assert pick(ROW, w, 5, "top_k").tolist() == [3, 5, 8, 13, 34]  # NaNs last, the lower position first


def test_negative_weights_and_short_rows():
    w = np.array([-5, -1, -3, -2, -4, -6], dtype=np.float32)
    assert pick(ROW, w, 2, "top_k").tolist() == [5, 13]
    # n <= f: the whole row, whatever the keys (NaN included)
    allnan = np.full(6, np.nan, dtype=np.float32)
    assert pick(ROW, allnan, 6, "top_k").tolist() == ROW.tolist()
    assert pick(ROW, allnan, 1024, "random_weighted", 7, 42).tolist() == ROW.tolist()
    assert pick(ROW[:0], allnan[:0], 3, "top_k").size == 0


def test_random_weighted_u_against_the_xxh64_golden_vectors(golden_dir):
    vec = json.load(open(os.path.join(golden_dir, "xxh64_int32.json")))["vectors"]
    seed42 = [v for v in vec if v["seed"] == 42]
    assert seed42
    for v in seed42:
        x = int(v["x"]) & MASK
        # u of position 0 of a row whose K + hash_add = x - 1
        u = random_weighted_u(1, (x - 1) & MASK, 0)[0]
        want = np.float32((int(v["h"], 16) >> 40) + 1) * np.float32(2.0 ** -24)
        assert u == want and 0 < u <= 1
    u = random_weighted_u(4096, 123456, 42 * 3)
    assert u.dtype == np.float32 and u.min() > 0 and u.max() <= 1
    assert np.all((u * np.float32(2 ** 24)) == np.round(u * np.float32(2 ** 24)))  # on the 2^-24 grid


def test_random_weighted_key_is_one_fp32_multiply():
    w = np.array([1.5, 3.0, 0.1, -2.0, 7.25, 1e-3], dtype=np.float32)
    k = row_keys(w, "random_weighted", 99, 42 * 2)
    u = random_weighted_u(6, 99, 84)
    assert k.dtype == np.float32
    np.testing.assert_array_equal(k, (w * u).astype(np.float32))
    got = pick(ROW, w, 3, "random_weighted", 99, 84)
    order = sorted(range(6), key=lambda i: (-float(k[i]), i))[:3]
    assert got.tolist() == sorted(ROW[order].tolist())
    # the weights scale the draw: zero weights never beat positive ones
    w0 = np.array([0, 0, 0, 1, 0, 2], dtype=np.float32)
    assert pick(ROW, w0, 2, "random_weighted", 5, 42).tolist() == [13, 34]
