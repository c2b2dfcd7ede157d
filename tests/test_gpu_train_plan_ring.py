"""The announced-batch ring of the training plans (csrc/pipeline.hip: PlanRing, gigl_run_part of csrc/step_parts.h): what a
step computes does not depend on what was announced ahead of it — one batch or two, none, a batch that is then not the
one trained on — and a change of the sampling seed forgets every announced batch (include/gigl_hip.h, the CONTRACT of an
announced batch).  Every comparison is between two runs of the same library over the same batches from the same initial
weights, one with announcements and one without.  Two runs of the SAME call sequence already differ in the last bit of a
loss (the backward sums with float atomics; measured before the ring existed), so the runs are held to the bound this
file's sibling holds the plan to against autograd (tests/test_gpu_train_plan.py): rtol 2e-6, atol 1e-6 on a loss, 2e-5 on
Adam's state."""
import numpy as np
import pytest
import torch

import oracle
from helpers import assert_adam_state, rmat_edges

N, D, HID, FAN = 1 << 10, 16, 16, [3, 2]
LOSS_BOUND = lambda loss: 1e-6 + 2e-6 * abs(loss)


@pytest.fixture(scope="module")
def setup():
    from gigl_amd.engine import HipEngine
    s, d = rmat_edges(10, 20000, seed=21)
    rowptr, col = oracle.build_csc(N, s, d, is_directed=False)
    x = (np.random.default_rng(1).standard_normal((N, D)) / 4).astype(np.float32)
    eng = HipEngine(0)
    eng.load_csc(rowptr, col)
    eng.load_features(x)
    dst = np.repeat(np.arange(N, dtype=np.uint32), np.diff(rowptr).astype(np.int64))
    eng.build_from_coo(N, dst, col.astype(np.uint32), is_directed=True, out_graph=True)  # (the positives are drawn from it)
    st = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    eng.bind_stream(st)
    yield eng, rowptr, col, st
    eng.bind_stream(torch.cuda.current_stream(eng.device))
    eng.close()


def _seed_matters(rowptr, col, roots, seeds):
    """the CPU sampler draws different trees for these roots under the two seeds, from nodes with more neighbours than fan-out"""
    roots = roots.cpu().numpy().view(np.uint32)
    roots = roots[roots != 0xFFFFFFFF]
    assert (np.diff(rowptr)[roots.astype(np.int64)] > FAN[0]).any()
    a, b = (oracle.sample_khop(rowptr, col, roots, FAN, sampling_seed=s, canonical=True)[0] for s in seeds)
    return any((u != v).any() for u, v in zip(a, b))


def _nc_model(eng, classes=4):
    from gigl_amd.models import GraphSAGE
    torch.manual_seed(5)
    return GraphSAGE(D, HID, classes, num_layers=2).to(eng.device)


def _nc_run(eng, st, init, b, steps):
    """a fresh plan over a copy of `init`; steps = [(roots, labels, kwargs of SageTrainPlan.step)] -> losses, trained
    parameters, Adam's moments"""
    import copy
    from gigl_amd.engine import SageTrainPlan
    model = copy.deepcopy(init)
    plan = SageTrainPlan(eng, model, b, FAN, lr=0.01, weight_decay=5e-4)
    torch.cuda.synchronize()  # (the plan's fused weights were laid out on torch's stream)
    with torch.cuda.stream(st):
        got = [plan.step(r, l, **kw).clone() for r, l, kw in steps]
    eng.synchronize()
    moments = plan.moments()
    eng.synchronize()
    plan.store(model)
    plan.close()
    return [float(v) for v in got], model.state_dict(), moments


@pytest.mark.gpu
def test_two_batches_ahead_changes_nothing(setup):
    """nine steps, each announcing the next batch and the one after — but one step announces neither, one announces a
    second-next batch that is not the one that comes, and one is given roots other than those announced for it — against
    the same steps with nothing announced: the same losses and the same trained state"""
    eng, rowptr, col, st = setup
    b, steps = 32, 9
    rng = np.random.default_rng(2)
    perm = rng.permutation(N).astype(np.uint32).view(np.int32)
    R = [torch.from_numpy(perm[i * b:(i + 1) * b].copy()).to(eng.device) for i in range(steps + 2)]  # (two strays)
    Y = [torch.from_numpy(rng.integers(0, 4, b)).to(eng.device) for _ in range(steps)]
    stray2, stray1 = R[steps], R[steps + 1]
    ahead = []
    for i in range(steps):
        n1 = R[i + 1] if i + 1 < steps else None
        n2 = R[i + 2] if i + 2 < steps else None
        if i == 3:
            n1 = n2 = None      # announces neither (step 4 was announced by step 2: its workspace is still held)
        if i == 5:
            n2 = stray2         # a second-next batch that step 7 is not given
        if i == 7:
            n1 = stray1         # step 8 is given other roots than announced
        ahead.append(dict(next_roots=n1, next_roots2=n2))
    model = _nc_model(eng)
    want, want_p, want_m = _nc_run(eng, st, model, b, [(R[i], Y[i], {}) for i in range(steps)])
    got, got_p, got_m = _nc_run(eng, st, model, b, [(R[i], Y[i], ahead[i]) for i in range(steps)])
    print("two ahead:", got, "nothing announced:", want, "largest difference", max(abs(g - w) for g, w in zip(got, want)))
    assert all(np.isfinite(want)) and len(set(want)) == steps
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-6)
    assert_adam_state("two batches ahead vs nothing announced", got_p, got_m, want_p, want_m, tol_m=2e-5, tol_v=2e-5, tol_p=2e-5)


def _lp_batch(eng, rng, b, P, n_rn):
    anchors = torch.from_numpy(rng.permutation(N)[:b].astype(np.uint32).view(np.int32)).to(eng.device)
    pos, cnt = eng.sample_positives(anchors, P, sampling_seed=42)
    a2 = anchors.view(-1, 1)
    grouped = torch.where(torch.arange(P, device=eng.device).view(1, P) < cnt.view(-1, 1), pos.view(-1, P), a2.expand(-1, P))
    roots = torch.cat([a2, grouped], dim=1).reshape(-1).contiguous()
    rn = torch.from_numpy(rng.permutation(N)[:n_rn].astype(np.uint32).view(np.int32)).to(eng.device)
    return roots, cnt.to(torch.int32).contiguous(), rn


def _seed_change_losses(step_of, batches, rowptr, col, roots1):
    """step 1's loss of three fresh plans over batches 0, 1: (seed 1 announcing batch 1, then seed 2), (the same, nothing
    announced), (seed 1 twice).  step_of() -> (step(batch, seed, next batch or None) -> loss, close)"""
    assert _seed_matters(rowptr, col, roots1, (1, 2))
    out = []
    for announce, seed1 in ((True, 2), (False, 2), (False, 1)):
        step, close = step_of()
        step(batches[0], 1, batches[1] if announce else None)
        out.append(step(batches[1], seed1, None))
        close()
    return out


def _assert_seed_rule(announced, plain, old_seed):
    print("step 1 under the new seed: announced", announced, "not announced", plain, "| under the old seed", old_seed)
    assert np.isfinite([announced, plain, old_seed]).all()
    assert abs(old_seed - plain) >= 100 * LOSS_BOUND(plain)  # (the test can fail: the old seed's trees give another loss)
    assert abs(announced - plain) <= LOSS_BOUND(plain)


@pytest.mark.gpu
def test_a_seed_change_forgets_the_announced_batch_node_classification(setup):
    from gigl_amd.engine import SageTrainPlan
    eng, rowptr, col, st = setup
    b = 32
    rng = np.random.default_rng(3)
    perm = rng.permutation(N).astype(np.uint32).view(np.int32)
    batches = [(torch.from_numpy(perm[i * b:(i + 1) * b].copy()).to(eng.device), torch.from_numpy(rng.integers(0, 4, b)).to(eng.device))
               for i in range(2)]
    model = _nc_model(eng)

    def step_of():
        plan = SageTrainPlan(eng, model, b, FAN, lr=0.01, weight_decay=5e-4)
        torch.cuda.synchronize()

        def step(batch, seed, nxt):
            with torch.cuda.stream(st):
                loss = plan.step(batch[0], batch[1], sampling_seed=seed, next_roots=None if nxt is None else nxt[0]).clone()
            eng.synchronize()
            return float(loss)
        return step, plan.close
    _assert_seed_rule(*_seed_change_losses(step_of, batches, rowptr, col, batches[1][0]))


@pytest.mark.gpu
def test_a_seed_change_forgets_the_announced_batch_link_prediction(setup):
    from gigl_amd.engine import NablpTrainPlan
    from gigl_amd.models import GraphSAGE
    eng, rowptr, col, st = setup
    b, P, n_rn = 16, 1, 8
    rng = np.random.default_rng(4)
    with torch.cuda.stream(st):  # (sample_positives runs on the engine's stream: torch's glue around it too)
        batches = [_lp_batch(eng, rng, b, P, n_rn) for _ in range(2)]
    eng.synchronize()
    torch.manual_seed(6)
    model = GraphSAGE(D, HID, 16, num_layers=2, should_l2_normalize_embedding_layer_output=True).to(eng.device)

    def step_of():
        plan = NablpTrainPlan(eng, model, b, P, n_rn, FAN, temperature=0.07, lr=5e-3, weight_decay=1e-6)
        torch.cuda.synchronize()

        def step(batch, seed, nxt):
            with torch.cuda.stream(st):
                loss = plan.step(*batch, sampling_seed=seed, next_roots=None if nxt is None else (nxt[0], nxt[2])).clone()
            eng.synchronize()
            return float(loss[0])
        return step, plan.close
    _assert_seed_rule(*_seed_change_losses(step_of, batches, rowptr, col, batches[1][0]))
