"""TEST INFRASTRUCTURE ONLY: inputs and the float64 restatement of tests/test_gpu_nc_eval_kernel.py and
tests/test_gpu_nc_score_pass.py — what NodeClassificationModelingTaskSpec.score computes per batch (argmax, ==, sum;
node_classification_modeling_task_spec.py:190-227) plus the cross-entropy of the rows whose label lies inside the row.

Reference.  Predictions: torch.argmax(dim=1) over the same fp32 rows (the first index among equal maxima, the first NaN of
a row that holds one).  Loss: logsumexp(row) - row[label] in FLOAT64 over the fp32 values widened exactly, summed in float64.
A label outside [0, width) is evaluated, never correct, and has no loss.  Nothing here reads a result of the code under test.
"""
import numpy as np
import torch

LOSS_RTOL, LOSS_ATOL = 1e-4, 1e-5  # the project's bar for a loss


def reference(rows: torch.Tensor, labels: torch.Tensor):
    """rows fp32 [n, width], labels int64 [n] (any device) -> (pred int64 [n] cpu, correct, evaluated, loss_sum fp64,
    loss_rows)"""
    rows, labels = rows.detach(), labels.detach()
    n, width = rows.shape
    pred = torch.argmax(rows, dim=1).cpu() if n else torch.zeros(0, dtype=torch.int64)
    lab = labels.cpu()
    inside = (lab >= 0) & (lab < width)
    r64 = rows.cpu().double()[inside]
    if r64.shape[0]:
        loss = torch.logsumexp(r64, dim=1) - r64.gather(1, lab[inside].reshape(-1, 1)).reshape(-1)
        loss_sum = float(loss.sum())
    else:
        loss_sum = 0.0
    return pred, int((pred == lab).sum()), int(n), loss_sum, int(inside.sum())


def random_rows(n: int, width: int, seed: int, scale: float = 3.0):
    """rows on a fine grid of fp32 values (a few exact ties among a row's columns at larger widths) and labels inside them"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(-4096, 4097, (n, width), generator=g).float() * (scale / 4096.0)
    labels = torch.randint(0, width, (n,), generator=g, dtype=torch.int64)
    return rows, labels


def tie_rows(width: int):
    """rows whose maximum appears twice or more — inside one lane's four columns, in two lanes' columns, on either side of the
    16-byte boundaries at columns 3/4 and 63/64 — and rows that are all equal; -> (rows, the first index of each row's maximum)"""
    pairs = [(0, 1), (1, 3), (2, 3), (3, 4), (0, 4), (4, 7), (5, 9), (3, 8), (63, 64), (62, 63), (60, 64), (64, 67), (1, 130),
             (255, 256), (3, 999)]
    rows, first = [], []
    g = torch.Generator().manual_seed(width)
    for a, b in pairs:
        if b >= width:
            continue
        for order in (0, 1):  # (the later column written first or last: the order of writing must not matter)
            r = torch.rand(width, generator=g) - 2.0
            r[b if order else a] = 1.5
            r[a if order else b] = 1.5
            rows.append(r)
            first.append(a)
    for v in (0.0, -3.25, float("-inf")):
        rows.append(torch.full((width,), v))
        first.append(0)
    return torch.stack(rows).float(), torch.tensor(first, dtype=torch.int64)


def margins(rows64: torch.Tensor) -> torch.Tensor:
    """the gap between a row's largest and second largest logit (float64 rows of width >= 2)"""
    top = torch.topk(rows64, 2, dim=1).values
    return top[:, 0] - top[:, 1]


def host_counts(rows: torch.Tensor, labels: np.ndarray):
    """score()'s counts of rows already on the host: (correct, evaluated)"""
    pred = torch.argmax(rows.cpu(), dim=1).numpy()
    return int((pred == np.asarray(labels)).sum()), int(len(labels))


# ---- a scoring pass over the small graph of tests/gcn_plan_cases.py: batches as ResidentGraph.root_batches pads them, the
# float64 rows of TwoLayerGCN (tests/gcn_infer_cases.py) and of a two-layer mean GraphSAGE (tests/sage_plan_cases.py)
SAGE_DIMS, SAGE_FAN = (24, 32, 7), (5, 3)
MARGIN = 1e-3  # 100 x the project's 1e-5 forward bound: no root's prediction hangs on the route that computed its row


def pass_batches(ids: np.ndarray, b: int):
    """[(the b roots of a call, uint32, a short last call padded with its first root; the number of real roots)]"""
    out = []
    for lo in range(0, len(ids), b):
        r = np.asarray(ids[lo:lo + b], dtype=np.uint32)
        out.append((np.concatenate([r, np.full(b - r.size, r[0], np.uint32)]), r.size))
    return out


def _unions(ids, b, fan):
    import gcn_plan_cases as gc
    rowptr, col = gc.graph()[:2]
    for roots, k in pass_batches(ids, b):
        nbr, _ = gc.oracle.sample_khop(rowptr, col, roots, list(fan), canonical=True)
        yield gc.oracle.union_build(roots, list(fan), nbr), k


def gcn_rows64(case, state, ids: np.ndarray, b: int) -> torch.Tensor:
    """float64 rows [len(ids), out] of the eval-time TwoLayerGCN, batch by batch over the oracle's union graphs"""
    import gcn_infer_cases as ic
    return torch.cat([ic.forward(case, state, u, torch.float64)[:k] for u, k in _unions(ids, b, case.fan)])


def sage_state(seed: int):
    """a two-layer mean GraphSAGE of SAGE_DIMS on the CPU, biases off zero"""
    from gigl_amd.models import GraphSAGE
    torch.manual_seed(seed)
    model = GraphSAGE(in_dim=SAGE_DIMS[0], hid_dim=SAGE_DIMS[1], out_dim=SAGE_DIMS[2], num_layers=2)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for c in model.conv_layers:
            c.lin_l.bias.copy_((torch.rand(c.lin_l.bias.shape, generator=g) - 0.5) * 0.2)
    return model.eval()


def sage_rows64(model, ids: np.ndarray, b: int) -> torch.Tensor:
    """float64 rows [len(ids), out] of `model` (CPU weights), batch by batch: tests/sage_plan_cases.py's formula over the
    oracle's union graph of every call"""
    import gcn_plan_cases as gc
    import sage_plan_cases as sp
    ws, bs = model.fused_params()
    ws, bs = [w.cpu() for w in ws], [None if v is None else v.cpu() for v in bs]
    case = sp._case("score pass", d_in=SAGE_DIMS[0], hidden=[SAGE_DIMS[1]], n_out=SAGE_DIMS[2], fan=list(SAGE_FAN))
    x64 = gc.features(SAGE_DIMS[0]).astype(np.float64)
    out = []
    for u, k in _unions(ids, b, SAGE_FAN):
        nn = int(u["meta"][0])
        rows = [(i, u["col"][u["rowptr"][i]:u["rowptr"][i + 1]].astype(np.int64)) for i in range(nn)
                if u["rowptr"][i + 1] > u["rowptr"][i]]
        ext = dict(nid=u["nodes"].astype(np.int64)[:nn], rows=rows, root_idx=u["root_local"].astype(np.int64))
        out.append(torch.from_numpy(sp.forward(case, x64, ext, ws, bs)["y"][:k]))
    return torch.cat(out)


def labels_for(rows64: torch.Tensor) -> np.ndarray:
    """labels that make two roots in three correct: the float64 prediction, moved one class on for every third root"""
    pred = torch.argmax(rows64, dim=1).numpy()
    return np.where(np.arange(pred.size) % 3 == 0, (pred + 1) % rows64.shape[1], pred).astype(np.int64)
