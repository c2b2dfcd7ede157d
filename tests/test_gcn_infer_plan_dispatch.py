"""What decides whether the stock node-classification model reaches the one-call inference plan (gigl_gcn_plan_*): the
library's symbols, TwoLayerGCN's plan interface and the shapes make_plan refuses — no GPU."""
import pytest
import torch

from gigl_amd import _lib
from gigl_amd.models_attn import TwoLayerGCN

SYMBOLS = ("gigl_gcn_plan_create", "gigl_gcn_plan_set_weights", "gigl_gcn_project_features",
           "gigl_gcn_plan_set_projected_input", "gigl_gcn_plan_set_fused_root", "gigl_gcn_plan_fused_root")


class _Engine:
    """what make_plan asks of an engine before it creates anything: the loaded table's width"""

    def __init__(self, feat_dim: int):
        self.feat_dim = feat_dim


def test_the_six_symbols_are_bound():
    assert all(s in _lib.SYMBOLS for s in SYMBOLS)


def test_the_model_has_the_plan_interface():
    for name in ("make_plan", "plan_params", "projected_input_pays"):
        assert callable(getattr(TwoLayerGCN, name, None)), name


@pytest.mark.parametrize("bias", [True, False])
def test_plan_params_are_the_pyg_named_tensors(bias):
    model = TwoLayerGCN(12, 5, hid_dim=6, bias=bias)
    sd = model.state_dict()
    (w1, w2), (b1, b2) = model.plan_params()
    assert tuple(w1.shape) == (6, 12) and tuple(w2.shape) == (5, 6)  # [out, in], as PyG keeps lin.weight
    assert torch.equal(w1, sd["conv1.lin.weight"]) and torch.equal(w2, sd["conv2.lin.weight"])
    if bias:
        assert torch.equal(b1, sd["conv1.bias"]) and torch.equal(b2, sd["conv2.bias"])
    else:
        assert b1 is None and b2 is None
    assert not w1.requires_grad and not w2.requires_grad


def test_projection_pays_for_rows_wider_than_the_hidden_layer():
    assert TwoLayerGCN(1433, 7, hid_dim=16).projected_input_pays(_Engine(1433))
    assert not TwoLayerGCN(100, 47, hid_dim=256).projected_input_pays(_Engine(100))
    assert not TwoLayerGCN(16, 7, hid_dim=16).projected_input_pays(_Engine(16))


def test_make_plan_refuses_three_hops_and_another_table_width():
    model = TwoLayerGCN(12, 5, hid_dim=6)
    with pytest.raises(NotImplementedError):
        model.make_plan(_Engine(12), 8, [5, 3, 2])
    with pytest.raises(NotImplementedError):
        model.make_plan(_Engine(12), 8, [5])
    with pytest.raises(NotImplementedError):
        model.make_plan(_Engine(10), 8, [5, 3])
