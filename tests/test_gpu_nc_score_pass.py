"""ResidentGraph.score_roots — a whole scoring pass of a node-classification model: every batch one call of the model's
one-call plan, the rows compared and counted on the device (gigl_nc_eval_metrics), ONE blocking host read per pass — against
ResidentGraph.encode plus torch on the host over the same batches, on the small graph of tests/gcn_plan_cases.py with the
stock TwoLayerGCN (tests/gcn_infer_cases.py) and a two-layer mean GraphSAGE (tests/sage_plan_cases.py's formula).

Counts are compared exactly.  For the GCN both sides run the same plan over the same rows.  For GraphSAGE the reference is the
staged forward, another route to the same rows within the project's 1e-5 forward bound; so every test first asserts, from
the float64 restatement alone (tests/nc_eval_cases.py), that every root's two largest logits lie at least 1e-3 apart — no
root is left out, the seeds were chosen for it — and the labels come from the float64 predictions: two roots in three are
correct by construction.  The mean loss is compared with float64 cross-entropy of encode's rows at rtol 1e-4 / atol 1e-5
for the GCN; for GraphSAGE (rows of another route, each logit within 1e-5) at atol 3e-5 + rtol 1e-4: a logit error e moves
a row's logsumexp - row[label] by at most 2 e."""
import numpy as np
import pytest
import torch

import gcn_infer_cases as ic
import gcn_plan_cases as gc
import nc_eval_cases as nc

B = 16
IDS = np.random.default_rng(0).permutation(gc.N_RMAT)[:37].astype(np.int64)  # two whole calls and one of 5 roots
GCN_CASE = ic.CASES["base"]


def _cluster_ids():
    """the 16 roots of gcn_infer_cases' overflow case — a node, its sampled children and full-fan-out nodes: their union
    outgrows a regular plan's workspace by construction of the data — then 21 ordinary roots"""
    return np.concatenate([ic.batch("overflow")[0].astype(np.int64), IDS[:21]])


class Setup:
    def __init__(self, kind: str):
        from gigl_amd.engine import HipEngine
        from gigl_amd.hbm import ResidentGraph
        from gigl_amd.models_attn import TwoLayerGCN
        self.kind = kind
        self.eng = HipEngine(0)
        rowptr, col = gc.graph()[:2]
        self.eng.load_csc(rowptr, col)
        self.eng.load_features(gc.features(24))
        self.res = ResidentGraph.from_engine(self.eng, np.arange(gc.N_NODES), [5, 3])
        if kind == "gcn":
            self.cpu = TwoLayerGCN(24, 7, hid_dim=32, is_training=False)
            self.cpu.load_state_dict(ic.state_of(GCN_CASE))
            self.second = ic.state_of(GCN_CASE, 1)
        else:
            self.cpu = nc.sage_state(7)
            self.second = nc.sage_state(5).state_dict()
        import copy
        self.model = copy.deepcopy(self.cpu).to(self.eng.device).eval()

    def rows64(self, ids):
        if self.kind == "gcn":
            return nc.gcn_rows64(GCN_CASE, self.cpu.state_dict(), ids, B)
        return nc.sage_rows64(self.cpu, ids, B)

    def load_second(self):
        self.cpu.load_state_dict(self.second)
        self.model.load_state_dict(self.second)  # (copies in place: the parameters' versions move, the plan follows)

    def encode_rows(self, ids, staged: bool) -> torch.Tensor:
        outs = []
        for hb in self.res.root_batches(ids, B, 1):
            hb.force_staged = staged
            outs.append(self.res.encode(self.model, hb).cpu())
        return torch.cat(outs)

    def close(self):
        self.res.close()
        self.eng.close()


@pytest.fixture(scope="module", params=["gcn", "sage"])
def setup(request):
    s = Setup(request.param)
    yield s
    s.close()


def _labels(s, ids):
    r64 = s.rows64(ids)
    m = nc.margins(r64)
    print(f"{s.kind}: smallest float64 top-2 margin over {len(ids)} roots {float(m.min()):.3e}")
    assert float(m.min()) >= nc.MARGIN  # EVERY root
    return r64, nc.labels_for(r64)


def _check(s, ids, want_redone=None):
    r64, labels = _labels(s, ids)
    before = s.res.overflow_redone
    got = s.res.score_roots(s.model, ids, labels, B)
    assert s.res.overflow_redone == before + got["redone"] and not s.res._unsettled  # (every deferred call was settled)
    n_calls = -(-len(ids) // B)
    # the float64 restatement alone: two in three
    correct64 = int((torch.argmax(r64, dim=1).numpy() == labels).sum())
    assert correct64 == len(ids) - len(range(0, len(ids), 3))
    rows = s.encode_rows(ids, staged=(s.kind == "sage"))  # (GraphSAGE: the staged forward)
    correct, evaluated = nc.host_counts(rows, labels)
    print(f"{s.kind}: {got} against encode + torch on the host {correct} of {evaluated}")
    assert (got["correct"], got["evaluated"]) == (correct, evaluated) == (correct64, len(ids))
    assert got["calls"] == n_calls and 0 <= got["redone"] <= n_calls
    if want_redone is not None:
        assert got["redone"] >= want_redone
    lab = torch.from_numpy(labels)
    loss = float((torch.logsumexp(rows.double(), 1) - rows.double().gather(1, lab.reshape(-1, 1)).reshape(-1)).mean())
    atol = nc.LOSS_ATOL if s.kind == "gcn" else 3e-5
    print(f"{s.kind}: mean loss {got['loss']!r} against float64 over encode's rows {loss!r}")
    assert abs(got["loss"] - loss) <= atol + nc.LOSS_RTOL * abs(loss)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("n", [32, 37, 1])
def test_pass_equals_encode_and_torch_on_the_host(setup, n):
    _check(setup, IDS[:n])


@pytest.mark.gpu
def test_no_roots(setup):
    got = setup.res.score_roots(setup.model, np.zeros(0, np.int64), np.zeros(0, np.int64), B)
    assert got == {"correct": 0, "evaluated": 0, "loss": 0.0, "calls": 0, "redone": 0}
    assert got["correct"] / max(got["evaluated"], 1) == 0.0


@pytest.mark.gpu
def test_a_call_that_overflows_is_redone(setup):
    _check(setup, _cluster_ids(), want_redone=1)


@pytest.mark.gpu
def test_one_blocking_host_read_per_pass(setup, monkeypatch):
    ids = IDS[:37]
    _, labels = _labels(setup, ids)
    first = setup.res.score_roots(setup.model, ids, labels, B)  # (the plan exists and is captured from here on)
    assert first["redone"] == 0
    reads = []
    for name in ("cpu", "item", "tolist", "__int__", "__bool__", "__float__"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    again = setup.res.score_roots(setup.model, ids, labels, B)
    monkeypatch.undo()
    assert again == first and reads == ["cpu"], reads


@pytest.mark.gpu
def test_changed_weights_are_seen_by_the_next_pass(setup):
    ids = IDS[:37]
    _, labels = _labels(setup, ids)  # the first state's labels are kept for both passes
    first = setup.res.score_roots(setup.model, ids, labels, B)
    setup.load_second()
    r64 = setup.rows64(ids)
    assert float(nc.margins(r64).min()) >= nc.MARGIN
    want = int((torch.argmax(r64, dim=1).numpy() == labels).sum())
    second = setup.res.score_roots(setup.model, ids, labels, B)
    print(f"{setup.kind}: {first['correct']} correct, then {second['correct']} (float64: {want})")
    assert want != first["correct"] and second["correct"] == want and second["evaluated"] == 37
    rows = setup.encode_rows(ids, staged=(setup.kind == "sage"))
    assert nc.host_counts(rows, labels) == (want, 37)
