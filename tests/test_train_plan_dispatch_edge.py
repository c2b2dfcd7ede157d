"""Which edge-featured GAT encoders the trainer hands to engine.GatEdgeNablpTrainPlan (no GPU: the predicate only):
two GATConv(edge_dim) or two EdgeAttrGATConv layers whose edge_dim is the resident edge table's width, 1..64, over
everything GatNablpTrainPlan asks of the node side.  GatNablpTrainPlan.applies itself keeps refusing edge_dim models."""
import pytest

BASE = dict(in_dim=100, hid_dim=16, out_dim=32, heads=2, edge_dim=6)


@pytest.mark.parametrize("kw,feat_dim,edge_feat_dim,want", [
    (dict(BASE), 100, 6, True),                                             # GATConv(edge_dim), widths match
    (dict(BASE, conv="edge_attr_gat"), 100, 6, True),                       # EdgeAttrGATConv, shared message weight
    (dict(BASE, conv="edge_attr_gat", share_edge_att_message_weight=False), 100, 6, True),
    (dict(BASE, heads=1, edge_dim=64), 100, 64, True),
    (dict(BASE, heads=4, edge_dim=1), 100, 1, True),
    (dict(BASE, in_dim=768, hid_dim=128, out_dim=128, edge_dim=16), 768, 16, True),   # configs[4] with an edge table
    (dict(BASE), 100, 7, False),                                            # the table's width is not the model's
    (dict(BASE), 100, 0, False),                                            # no table
    (dict(BASE, edge_dim=65), 100, 65, False),                              # a lane per component: at most 64
    (dict(BASE, num_layers=3), 100, 6, False),
    (dict(BASE, heads=3), 100, 6, False),                                   # heads outside {1, 2, 4}
    (dict(BASE, in_dim=32), 32, 6, False),                                  # 2 x 16 >= 32: rows too narrow for the input side
    (dict(BASE, in_dim=24, hid_dim=16, heads=2), 24, 6, False),
    (dict(BASE), 64, 6, False),                                             # the node table is not what the model expects
    (dict(BASE, in_dim=1024, heads=4), 1024, 6, False),                     # four heads over > 768 floats: not built
    (dict(BASE, edge_dim=None), 100, 6, False),                             # no edge features: GatNablpTrainPlan's model
])
def test_gat_edge_plan_predicate(kw, feat_dim, edge_feat_dim, want):
    from gigl_amd.engine import GatEdgeNablpTrainPlan
    from gigl_amd.models_attn import GAT
    kw = dict(kw)
    model = GAT(kw.pop("in_dim"), kw.pop("hid_dim"), kw.pop("out_dim"), num_layers=kw.pop("num_layers", 2), **kw)
    assert GatEdgeNablpTrainPlan.applies(model, feat_dim, edge_feat_dim) is want


def test_mixed_conv_classes_are_refused():
    from gigl_amd.engine import GatEdgeNablpTrainPlan
    from gigl_amd.models_attn import GAT
    plain = GAT(100, 16, 32, num_layers=2, heads=2, edge_dim=6)
    attr = GAT(100, 16, 32, num_layers=2, heads=2, edge_dim=6, conv="edge_attr_gat")
    assert GatEdgeNablpTrainPlan.applies(plain, 100, 6) is True and GatEdgeNablpTrainPlan.applies(attr, 100, 6) is True
    plain.conv_layers[1] = attr.conv_layers[1]  # GATConv then EdgeAttrGATConv
    assert type(plain.conv_layers[0]) is not type(plain.conv_layers[1])
    assert GatEdgeNablpTrainPlan.applies(plain, 100, 6) is False


@pytest.mark.parametrize("conv", ["gat", "edge_attr_gat"])
def test_the_edge_free_plan_still_refuses_edge_models(conv):
    from gigl_amd.engine import GatNablpTrainPlan
    from gigl_amd.models_attn import GAT
    model = GAT(100, 16, 32, num_layers=2, heads=2, edge_dim=6, conv=conv)
    assert GatNablpTrainPlan.applies(model, 100) is False
    assert GatNablpTrainPlan.applies(GAT(100, 16, 32, num_layers=2, heads=2), 100) is True


def test_other_encoders_are_not_taken_for_the_edge_plan():
    from gigl_amd.engine import GatEdgeNablpTrainPlan
    from gigl_amd.models import GraphSAGE
    assert GatEdgeNablpTrainPlan.applies(GraphSAGE(100, 16, 8, num_layers=2), 100, 6) is False
