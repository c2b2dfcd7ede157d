"""The training plans' dropout without a GPU: the mask's restatement (tests/dropout_ref.py) against the known answers of the
block function and the distribution it must have, and the host wiring — trainerArgs `dropout` / `dropout_seed` reach the
encoder and the plan, a bad p raises, a GAT encoder with dropout keeps the autograd loop."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import dropout_ref

# include/gigl_hip.h (gigl_sage_train_plan_set_dropout): the Random123 vectors
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_block_function_known_answers(counter, key, want):
    assert dropout_ref.philox4x32_10(counter, key) == want


def test_threshold_and_scale_are_the_float32_ps():
    assert dropout_ref.threshold(0.0) == 0 and dropout_ref.threshold(0.5) == 1 << 31
    # 0.1 as a float32 is 0.100000001490116...: T comes from that number, not from the double 0.1
    assert dropout_ref.threshold(0.1) == int(math.floor(float(np.float32(0.1)) * 2.0 ** 32)) == 429496736
    assert dropout_ref.threshold(float(np.nextafter(np.float32(1), np.float32(0)))) < 1 << 32
    assert dropout_ref.scale(0.5) == np.float32(2) and dropout_ref.scale(0.0) == np.float32(1)


@pytest.mark.parametrize("p,seed", [(0.1, 0), (0.5, 0), (0.9, 0), (0.5, 0x1234567890ABCDEF)])
def test_keep_fraction(p, seed):
    """n = 257 x 256 elements: the kept count lies within 6 sigma of n (1 - T / 2^32), sigma = sqrt(n p (1 - p)) elements"""
    rows, cols = 257, 256
    n = rows * cols
    keep = dropout_ref.keep_mask(seed, 3, 0, 0, rows, cols, p)
    want = n * (1.0 - dropout_ref.threshold(p) / 2.0 ** 32)
    sigma = math.sqrt(n * p * (1.0 - p))
    got = int(keep.sum())
    print(f"p={p} seed={seed:#x}: kept {got} of {n}, expected {want:.1f}, sigma {sigma:.1f}")
    assert abs(got - want) <= 6.0 * sigma


def test_p_zero_keeps_everything():
    assert dropout_ref.keep_mask(5, 1, 0, 0, 3, 6, 0.0).all()


def test_masks_differ_between_steps_encodes_layers_and_seeds():
    base = dict(seed=11, step=2, encode=0, layer=0)
    m0 = dropout_ref.keep_mask(rows=9, cols=33, p=0.5, **base)
    for change in (dict(step=3), dict(encode=1), dict(layer=1), dict(seed=12), dict(seed=11 + (1 << 32))):
        m1 = dropout_ref.keep_mask(rows=9, cols=33, p=0.5, **{**base, **change})
        differing = int((m0 != m1).sum())
        # (two independent fair masks of 297 elements agree everywhere with probability 2^-297)
        assert 297 // 4 < differing < 3 * 297 // 4, (change, differing)
    # ... and the same integers give the same mask; a narrower output is a prefix of the wider one's rows
    assert np.array_equal(m0, dropout_ref.keep_mask(rows=9, cols=33, p=0.5, **base))
    assert np.array_equal(m0[:, :6], dropout_ref.keep_mask(rows=9, cols=6, p=0.5, **base))


# ---- host wiring

def _cfg(feature_dim):
    return SimpleNamespace(is_heterogeneous=False, preprocessed_metadata=SimpleNamespace(nodes=[SimpleNamespace(feature_dim=feature_dim)]),
                           num_positive_samples=1)


def test_dropout_reaches_the_encoder():
    from gigl_amd.nablp_spec import HipNodeAnchorLinkPredictionSpec
    from gigl_amd.task_specs import HipGraphSageNodeClassificationSpec
    lp = HipNodeAnchorLinkPredictionSpec(dropout="0.5", dropout_seed="7")
    enc = lp.init_model(_cfg(8)).encoder
    assert enc.dropout.p == 0.5 and lp.dropout == 0.5 and lp.dropout_seed == 7
    assert not enc._plain and enc._plain_but_dropout
    nc = HipGraphSageNodeClassificationSpec(dropout="0.25")
    assert nc.init_model(_cfg(8)).dropout.p == 0.25 and nc._dropout == 0.25 and nc._dropout_seed == 0
    # absent: the encoder's own default, no seed
    lp0 = HipNodeAnchorLinkPredictionSpec()
    assert lp0.init_model(_cfg(8)).encoder.dropout.p == 0.0 and lp0.dropout is None and lp0.dropout_seed == 0


def test_outside_training_mode_a_dropout_model_is_plain():
    from gigl_amd.models import GraphSAGE
    m = GraphSAGE(8, 8, 8, num_layers=2, dropout=0.5)
    assert m.training and not m._plain and not m._plain_now and m._plain_but_dropout
    m.eval()
    assert not m._plain and m._plain_now
    assert not GraphSAGE(8, 8, 8, num_layers=2, dropout=0.5, batchnorm=True).eval()._plain_now


@pytest.mark.parametrize("bad", ["1.0", "-0.1", "1.5", "nan"])
def test_a_bad_p_raises(bad):
    from gigl_amd.engine import _plan_dropout
    from gigl_amd.models import GraphSAGE
    from gigl_amd.nablp_spec import HipNodeAnchorLinkPredictionSpec
    from gigl_amd.task_specs import HipGraphSageNodeClassificationSpec
    for spec in (HipNodeAnchorLinkPredictionSpec, HipGraphSageNodeClassificationSpec):
        with pytest.raises(ValueError):
            spec(dropout=bad)
    with pytest.raises(ValueError):
        _plan_dropout(GraphSAGE(8, 8, 8), float(bad), 0)


def test_the_plans_dropout_defaults_to_the_models():
    from gigl_amd.engine import _plan_dropout
    from gigl_amd.models import GraphSAGE
    m = GraphSAGE(8, 8, 8, dropout=0.5)
    assert _plan_dropout(m, None, 3) == (0.5, 3)
    assert _plan_dropout(m, 0.0, -1) == (0.0, 0xFFFFFFFFFFFFFFFF)  # (an explicit p wins; the seed is a 64-bit word)


def _lp_spec_on_a_fake_resident(monkeypatch, feat_dim, **kwargs):
    from gigl_amd._lib import MODE_SPARK_HASH
    from gigl_amd.nablp_spec import HipNodeAnchorLinkPredictionSpec
    spec = HipNodeAnchorLinkPredictionSpec(**kwargs)
    cfg = _cfg(feat_dim)
    spec.init_model(cfg)
    monkeypatch.setattr(HipNodeAnchorLinkPredictionSpec, "_hbm_split", lambda self, c: {"train": None})
    eng = SimpleNamespace(_graph=object(), _feat=object(), feat_dim=feat_dim, edge_feat_dim=0)
    spec._resident = SimpleNamespace(train_as_graph_data=False, feat_dim=feat_dim, fanouts=[10, 5], engine=eng, sharded=False,
                                     mode=MODE_SPARK_HASH, nablp_slots=lambda P: (P, 0))
    return spec, cfg


def test_a_graphsage_job_hands_dropout_and_seed_to_the_plan(monkeypatch):
    from gigl_amd import engine
    made = []

    class FakePlan:
        def __init__(self, eng, enc, *args, **kw):
            made.append((enc, kw))
    monkeypatch.setattr(engine, "NablpTrainPlan", FakePlan)
    spec, cfg = _lp_spec_on_a_fake_resident(monkeypatch, 8, dropout="0.5", dropout_seed="9")
    assert isinstance(spec._library_train_plan(cfg), FakePlan)
    (enc, kw), = made
    assert enc.dropout.p == 0.5 and kw["dropout"] == 0.5 and kw["dropout_seed"] == 9


def test_a_gat_encoder_with_dropout_does_not_get_a_plan(monkeypatch):
    from gigl_amd import engine
    refused = []
    init = engine.GatNablpTrainPlan.__init__

    def recording_init(self, *args, **kw):
        try:
            init(self, *args, **kw)
        except NotImplementedError as exc:
            refused.append((kw.get("dropout"), str(exc)))
            raise
    monkeypatch.setattr(engine.GatNablpTrainPlan, "__init__", recording_init)
    args = dict(gnn_model_class_path="gigl_amd.models_attn.GAT", hidden_dim="16", out_channels="32", num_heads="2")
    spec, cfg = _lp_spec_on_a_fake_resident(monkeypatch, 100, dropout="0.5", **args)
    assert engine.GatNablpTrainPlan.applies(spec.model.encoder, 100)  # (without dropout this encoder has a plan)
    assert spec._library_train_plan(cfg) is None
    (p, why), = refused
    assert p == 0.5 and "dropout" in why
