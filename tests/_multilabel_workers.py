"""Data, float64 reference and worker processes of tests/test_multilabel.py and tests/test_multilabel_gpu.py (spawn start method),
in the pattern of tests/_nodeclass_workers.py."""
import os
import queue
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from _nodeclass_workers import SETS, gather_rows, initial_weights  # noqa: E402

# the planted multi-label problem of the end-to-end tests
N, NNZ, COMMUNITY, GRAPH_SEED = 3000, 36000, 150, 3
LABELS, FIN, HIDDEN, NLAYERS = 6, 24, 32, 2
EPOCHS, LR, WEIGHT_SEED = 12, 0.02, 5
DROPOUT, DROPOUT_SEED = 0.5, 11
KINDS, FLIP = 8, 0.03              # communities fold to 8 kinds, each with a fixed subset of the labels; 3 % of the bits flipped


def make_dataset(dirname, n=N, nnz=NNZ, community=COMMUNITY, seed=GRAPH_SEED, labels=LABELS, fin=FIN, noise=1.5):
    """A seeded planted-community graph (pattern .mtx); every community switches on the fixed label subset of its kind, 3 % of
    the bits are flipped; features = the kind's centre + noise; a seeded 50 / 20 / 20 split with 10 % of the rows in no set,
    whose label rows hold 7 (anything goes there); part vectors for 1, 2, 3 ranks.  Returns the paths and the arrays."""
    from scipy.io import mmwrite
    from conftest import pkg
    synth = pkg("synth")
    keys = synth.sbm_undirected(n, nnz, seed, community=community).numpy()
    A = sp.coo_matrix((np.ones(keys.size, np.float32), (keys // n, keys % n)), shape=(n, n))
    comm = synth.sbm_communities(n, seed, community=community).numpy()
    rng = np.random.default_rng(seed + 200)
    kind = comm % KINDS
    subsets = (rng.random((KINDS, labels)) < 0.4).astype(np.uint8)
    subsets[0, :] = 0
    subsets[1, :] = 1                                            # a kind without labels and one with all of them
    Y = subsets[kind] ^ (rng.random((n, labels)) < FLIP).astype(np.uint8)
    centres = rng.standard_normal((KINDS, fin))
    X = (centres[kind] + noise * rng.standard_normal((n, fin))).astype(np.float32)
    u = rng.random(n)
    split = np.where(u < 0.5, 1, np.where(u < 0.7, 2, np.where(u < 0.9, 3, 0))).astype(np.uint8)
    Y[split == 0] = 7
    paths = {"A": os.path.join(dirname, "sbm.mtx"), "features": os.path.join(dirname, "features.npy"),
             "labels": os.path.join(dirname, "labels.npy"), "split": os.path.join(dirname, "split.npy")}
    mmwrite(paths["A"], A, field="pattern", symmetry="general")
    np.save(paths["features"], X)
    np.save(paths["labels"], Y)
    np.save(paths["split"], split)
    for P in (1, 2, 3):
        pv = np.random.default_rng(seed + P).integers(0, P, n)
        paths["pv%d" % P] = os.path.join(dirname, "sbm.%d.rp" % P)
        with open(paths["pv%d" % P], "w") as fh:
            fh.write(" ".join(map(str, pv.tolist())) + "\n")
    return paths, {"A": A.tocsr(), "X": X, "labels": Y, "split": split}


def bce64(x, y):
    """Element-wise binary cross entropy with logits in float64 numpy: y ? softplus(-x) : softplus(x)."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        t = np.where(y, -x, x)
        return np.where(np.isnan(x), np.nan, np.maximum(t, 0.0) + np.log1p(np.exp(-np.abs(x))))


def stats64(x, y, split):
    """The record of pgcn_masked_bce_f32 in float64 numpy: x float [n, C], y bool [n, C], split uint8 [n]."""
    elem = bce64(x, y)
    pred = np.asarray(x) > 0
    out = {"loss_sum": [0.0] * 4, "tp": [0] * 4, "fp": [0] * 4, "fn": [0] * 4,
           "rows": [int(((split == 0) | (split > 3)).sum())] + [int((split == k).sum()) for k in (1, 2, 3)]}
    for k in (1, 2, 3):
        m = split == k
        out["loss_sum"][k] = float(elem[m].sum())
        out["tp"][k], out["fp"][k], out["fn"][k] = int((pred & y)[m].sum()), int((pred & ~y)[m].sum()), int((~pred & y)[m].sum())
    return out


def _report64(logits, y, split):
    x = logits.numpy()
    st = stats64(x, y, split)
    near = np.abs(x) < 1e-4 * float(np.abs(x).max())                      # elements that may be predicted either way
    out = {"loss": {}, "tp": {}, "fp": {}, "fn": {}, "rows": {}, "near": {}, "micro_f1": {}}
    for k, name in enumerate(SETS, 1):
        r = st["rows"][k]
        out["rows"][name], out["tp"][name], out["fp"][name], out["fn"][name] = r, st["tp"][k], st["fp"][k], st["fn"][k]
        out["loss"][name] = st["loss_sum"][k] / max(r * x.shape[1], 1)
        out["near"][name] = int(near[split == k].sum())
        d = 2 * st["tp"][k] + st["fp"][k] + st["fn"][k]
        out["micro_f1"][name] = 2 * st["tp"][k] / d if d else float("nan")
    out["pred"], out["near_elems"] = x > 0, near
    return out


def float64_reference(data, widths, epochs=EPOCHS, lr=LR, dropout=0.0, dropout_seed=DROPOUT_SEED, weight_seed=WEIGHT_SEED):
    """The same model in float64, plain torch: sparse D^-1/2 (A + I) D^-1/2, the model's initial weights, ReLU on every layer but
    the last, the host statement of the dropout masks, BCEWithLogitsLoss (mean) over the train rows, Adam.  Per epoch the record
    the engine reports: without dropout of the training step's logits, with dropout of an eval forward after the update;
    "final": the record of the trained model."""
    from conftest import pkg
    D = pkg("dropout")
    n = data["A"].shape[0]
    B = (data["A"] + sp.identity(n, format="csr")).astype(np.float64)
    B.data[:] = 1.0
    dr = 1.0 / np.sqrt(np.asarray(B.sum(axis=1)).reshape(-1))
    dc = 1.0 / np.sqrt(np.asarray(B.sum(axis=0)).reshape(-1))
    Ah = (sp.diags(dr) @ B @ sp.diags(dc)).tocoo()
    At = torch.sparse_coo_tensor(np.vstack([Ah.row, Ah.col]), Ah.data, (n, n), dtype=torch.float64).coalesce()
    X = torch.from_numpy(data["X"]).double()
    split = data["split"]
    y = data["labels"] == 1                                               # (rows in no set hold 7: never looked at)
    train = torch.from_numpy(split == 1)
    ytrain = torch.from_numpy(y)[train].double()
    Ws = [w.double().requires_grad_(True) for w in initial_weights(widths, weight_seed)]
    opt = torch.optim.Adam(Ws, lr=lr)
    thr, scale = D.threshold(dropout)

    def forward(step):
        h = X
        for l, w in enumerate(Ws):
            h = torch.sparse.mm(At, h) @ w.t()
            if l < len(Ws) - 1:
                h = h.clamp_min(0)
                if step is not None and dropout > 0.0:
                    keep = D.keep_mask(dropout_seed, step, l, np.arange(n), h.shape[1], thr)
                    h = torch.where(keep, h * scale, torch.zeros((), dtype=torch.float64))
        return h

    out = []
    for epoch in range(epochs):
        logits = forward(epoch)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits[train], ytrain)
        opt.zero_grad()
        loss.backward()
        opt.step()
        with torch.no_grad():
            out.append(_report64(forward(None) if dropout > 0.0 else logits.detach(), y, split))
    with torch.no_grad():
        final = _report64(forward(None), y, split)
    return out, final


def run_worker(rank, P, port, paths, gpu, q, dropout=0.0, epochs=EPOCHS, seed=WEIGHT_SEED, composed=False):
    """PGCN.run(..., task="multilabel") on rank `rank` of `P` (gloo; the checker-backed kernels on the CPU, the real ones on the
    GPU): reports the model's history, the final eval record, the trained model's logits for the owned rows and how often the
    provider's masked_bce / masked_bce_backward ran.  `composed`: the framework composition instead of the kernels."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M = pkg("PGCN")
    calls = {"masked_bce": 0, "masked_bce_backward": 0}
    if gpu:
        M._kernel_provider = None
        HK = pkg("kernels").HipKernels
        for name in calls:
            def counted(self, *a, _f=getattr(HK, name), _n=name, **kw):
                calls[_n] += 1
                return _f(self, *a, **kw)
            setattr(HK, name, counted)
    else:
        from oracle_kernels import OracleKernels
        M._kernel_provider = OracleKernels()       # test-only checker-backed kernels: no masked_bce -> the composition
    if composed:
        M._masked_bce_kernels = lambda *a: None
    M._exchanger = None
    got = {}

    def fn(*a, **kw):
        torch.manual_seed(seed)                    # every rank draws the same initial weights
        buf = io.StringIO()
        with redirect_stdout(buf):
            model = M.run(*a, **kw)
        data = M._nodedata.load_multilabel(paths["features"], paths["labels"], paths["split"], M._engine_current.part.owned,
                                           N, device=M.device)
        model.eval()
        with torch.no_grad():
            logits = model(data.features)
        got.update(history=model.history, best=model.best, widths=model.widths, stdout=buf.getvalue(),
                   final=M.evaluate_multilabel(model, data.features, data.labels, data.split),
                   own=M._engine_current.part.owned.cpu().numpy(), logits=logits.cpu().numpy(),
                   hip=type(M._engine_current.k).__name__)

    kw = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=HIDDEN, epochs=epochs, lr=LR,
              task="multilabel")
    if dropout > 0.0:
        kw.update(dropout=dropout, dropout_seed=DROPOUT_SEED)
    M.init_process(rank, P, fn, NLAYERS, HIDDEN, paths["A"], paths["pv%d" % P], "gloo", "sym", **kw)
    got["rank"], got["calls"] = rank, calls
    q.put(got)


def spawn_run(P, paths, gpu, **kw):
    import multiprocessing as mp
    from conftest import free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=run_worker, args=(r, P, port, paths, gpu, q), kwargs=kw) for r in range(P)]
    saved = os.environ.get("HIP_VISIBLE_DEVICES")
    if gpu:
        os.environ["HIP_VISIBLE_DEVICES"] = (saved or "0").split(",")[0]      # every rank on the one GPU
    try:
        for p in procs:
            p.start()
    finally:
        if gpu:
            if saved is None:
                os.environ.pop("HIP_VISIBLE_DEVICES", None)
            else:
                os.environ["HIP_VISIBLE_DEVICES"] = saved
    # a rank that dies before it reports ends the wait at once (its peers would sit in a collective until the time limit)
    res, deadline = [], time.monotonic() + 600
    while len(res) < P:
        try:
            res.append(q.get(timeout=0.2))
        except queue.Empty:
            failed = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode not in (None, 0)]
            if failed or time.monotonic() > deadline:
                for p in procs:
                    if p.is_alive():
                        p.terminate()
                for p in procs:
                    p.join(timeout=10)
                raise AssertionError("ranks (rank, exit code) %s of %d ended without a result" % (failed or "none", P))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return sorted(res, key=lambda r: r["rank"])


def check_against_reference(res, ref, final, data, floor=1e-5):
    """The rule of tests/_nodeclass_workers.check_against_reference, per element instead of per row: per reported epoch every
    set's loss within `floor` (relative) of the float64 reference and its TP / FP / FN within the reference's near-tie elements
    of that set (|float64 logit| below 1e-4 max |logit|: the prediction x > 0 may fall either way; at most 1 % of the set's
    elements); for the trained model every element outside the near ties predicted as the reference predicts it.  Returns the
    largest relative loss error."""
    n = data["A"].shape[0]
    C = data["labels"].shape[1]
    worst = 0.0
    hist = res[0]["history"]
    assert [h["epoch"] for h in hist] == list(range(len(ref)))
    for h, want in zip(hist, ref):
        for name in SETS:
            assert h["rows"][name] == want["rows"][name] == int((data["split"] == 1 + SETS.index(name)).sum())
            assert want["near"][name] <= 0.01 * want["rows"][name] * C, (h["epoch"], name, want["near"][name])
            for c in ("tp", "fp", "fn"):
                assert abs(h[c][name] - want[c][name]) <= want["near"][name], (h["epoch"], name, c, h[c][name], want[c][name])
            e = abs(h["losses"][name] - want["loss"][name]) / max(abs(want["loss"][name]), 1e-30)
            worst = max(worst, e)
            assert e <= floor, (h["epoch"], name, h["losses"][name], want["loss"][name], e)
            d = 2 * h["tp"][name] + h["fp"][name] + h["fn"][name]
            assert h["micro_f1"][name] == (2 * h["tp"][name] / d if d else float("nan")) or (d == 0 and np.isnan(h["micro_f1"][name]))
        assert h["loss"] == h["losses"]["train"] and h["train"] == h["micro_f1"]["train"]
    pred = gather_rows(res, "logits", n) > 0
    in_set = (data["split"] != 0)[:, None]
    differ = (pred != final["pred"]) & in_set
    assert not (differ & ~final["near_elems"]).any(), int((differ & ~final["near_elems"]).sum())
    for name in SETS:
        for c in ("tp", "fp", "fn"):
            assert abs(res[0]["final"][c][name] - final[c][name]) <= final["near"][name]
        assert res[0]["final"]["rows"][name] == final["rows"][name]
    return worst
