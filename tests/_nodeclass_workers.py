"""Data, float64 reference and worker processes of tests/test_nodeclass.py and tests/test_nodeclass_gpu.py (spawn start method), in
the pattern of tests/_dropout_workers.py."""
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

SETS = ("train", "val", "test")
# the data set of the end-to-end tests
N, NNZ, COMMUNITY, GRAPH_SEED = 3000, 36000, 150, 3
CLASSES, FIN, HIDDEN, NLAYERS = 7, 24, 32, 2
EPOCHS, LR, WEIGHT_SEED = 12, 0.02, 5
DROPOUT, DROPOUT_SEED = 0.5, 11


def make_dataset(dirname, n=N, nnz=NNZ, community=COMMUNITY, seed=GRAPH_SEED, classes=CLASSES, fin=FIN, noise=1.5):
    """A seeded planted-community graph (pattern .mtx), labels = community folded to `classes`, features = a class centre +
    noise, a seeded 50 / 20 / 20 split with 10 % of the rows in no set (label -1), and part vectors for 1, 2, 3 ranks.
    Returns the paths and the arrays."""
    from scipy.io import mmwrite
    from conftest import pkg
    synth = pkg("synth")
    keys = synth.sbm_undirected(n, nnz, seed, community=community).numpy()
    A = sp.coo_matrix((np.ones(keys.size, np.float32), (keys // n, keys % n)), shape=(n, n))
    comm = synth.sbm_communities(n, seed, community=community).numpy()
    rng = np.random.default_rng(seed + 100)
    y = (comm % classes).astype(np.int64)
    centres = rng.standard_normal((classes, fin))
    X = (centres[y] + noise * rng.standard_normal((n, fin))).astype(np.float32)
    u = rng.random(n)
    split = np.where(u < 0.5, 1, np.where(u < 0.7, 2, np.where(u < 0.9, 3, 0))).astype(np.uint8)
    labels = np.where(split == 0, -1, y).astype(np.int64)
    paths = {"A": os.path.join(dirname, "sbm.mtx"), "features": os.path.join(dirname, "features.npy"),
             "labels": os.path.join(dirname, "labels.npy"), "split": os.path.join(dirname, "split.npy")}
    mmwrite(paths["A"], A, field="pattern", symmetry="general")
    np.save(paths["features"], X)
    np.save(paths["labels"], labels)
    np.save(paths["split"], split)
    for P in (1, 2, 3):
        pv = np.random.default_rng(seed + P).integers(0, P, n)
        paths["pv%d" % P] = os.path.join(dirname, "sbm.%d.rp" % P)
        with open(paths["pv%d" % P], "w") as fh:
            fh.write(" ".join(map(str, pv.tolist())) + "\n")
    return paths, {"A": A.tocsr(), "X": X, "labels": labels, "split": split}


def initial_weights(widths, seed=WEIGHT_SEED):
    """The model's own initial weights: the layers run() builds after torch.manual_seed(seed), in its order."""
    torch.manual_seed(seed)
    return [torch.nn.Linear(a, b, bias=False).weight.detach().clone() for a, b in zip(widths, widths[1:])]


def _stats64(logits, labels, split):
    out = {"loss": {}, "correct": {}, "rows": {}, "near": {}}
    top = torch.topk(logits, 2, dim=1).values
    near = (top[:, 0] - top[:, 1]) < 1e-4 * float(logits.abs().max())     # rows that may be predicted either way
    pred = logits.argmax(1)
    for k, name in enumerate(SETS, 1):
        m = torch.from_numpy(split == k)
        yk = torch.from_numpy(labels)[m]
        out["rows"][name] = int(m.sum())
        out["loss"][name] = float(torch.nn.functional.cross_entropy(logits[m], yk, reduction="sum") / max(int(m.sum()), 1))
        out["correct"][name] = int((pred[m] == yk).sum())
        out["near"][name] = int(near[m].sum())
    out["pred"], out["near_rows"] = pred.numpy(), near.numpy()
    return out


def float64_reference(data, widths, epochs=EPOCHS, lr=LR, dropout=0.0, dropout_seed=DROPOUT_SEED, weight_seed=WEIGHT_SEED):
    """The same model in float64, plain torch: sparse D^-1/2 (A + I) D^-1/2, the model's initial weights, ReLU on every layer but
    the last, the host statement of the dropout masks, mean cross entropy over the train rows, Adam.  Per epoch the record the
    engine reports: without dropout of the training step's logits, with dropout of an eval forward after the update; "final":
    the record of the trained model."""
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
    y, split = data["labels"], data["split"]
    train = torch.from_numpy(split == 1)
    ytrain = torch.from_numpy(y)[train]
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
        loss = torch.nn.functional.cross_entropy(logits[train], ytrain)
        opt.zero_grad()
        loss.backward()
        opt.step()
        with torch.no_grad():
            out.append(_stats64(forward(None) if dropout > 0.0 else logits.detach(), y, split))
    with torch.no_grad():
        final = _stats64(forward(None), y, split)
    return out, final


def run_worker(rank, P, port, paths, gpu, q, dropout=0.0, epochs=EPOCHS, seed=WEIGHT_SEED):
    """PGCN.run(...) with the data options on rank `rank` of `P` (gloo; the checker-backed kernels on the CPU, the real ones on the
    GPU): reports the model's history, the final eval record and the trained model's predictions for the owned rows."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M = pkg("PGCN")
    if gpu:
        M._kernel_provider = None
    else:
        from oracle_kernels import OracleKernels
        M._kernel_provider = OracleKernels()       # test-only checker-backed kernels: no masked_nll -> the composition
    M._exchanger = None
    got = {}

    def fn(*a, **kw):
        torch.manual_seed(seed)                    # every rank draws the same initial weights
        buf = io.StringIO()
        with redirect_stdout(buf):
            model = M.run(*a, **kw)
        data = M._nodedata.load(paths["features"], paths["labels"], paths["split"], M._engine_current.part.owned,
                                N, device=M.device)
        model.eval()
        with torch.no_grad():
            logits = model(data.features)
        got.update(history=model.history, best=model.best, widths=model.widths, stdout=buf.getvalue(),
                   final=M.evaluate(model, data.features, data.labels, data.split), own=M._engine_current.part.owned.cpu().numpy(),
                   pred=logits.argmax(1).cpu().numpy(), logits=logits.cpu().numpy(),
                   hip=type(M._engine_current.k).__name__)

    kw = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=HIDDEN, epochs=epochs, lr=LR)
    if dropout > 0.0:
        kw.update(dropout=dropout, dropout_seed=DROPOUT_SEED)
    M.init_process(rank, P, fn, NLAYERS, HIDDEN, paths["A"], paths["pv%d" % P], "gloo", "sym", **kw)
    got["rank"] = rank
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
    res = [q.get(timeout=600) for _ in range(P)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return sorted(res, key=lambda r: r["rank"])


def gather_rows(res, key, n):
    out = None
    for r in res:
        v = r[key]
        out = np.zeros((n,) + v.shape[1:], v.dtype) if out is None else out
        out[r["own"]] = v
    return out


def check_against_reference(res, ref, final, data, floor=1e-5):
    """The accuracy criterion and the loss bound of the suite: per reported epoch the train loss within `floor` (relative) of the
    float64 reference and every set's correct count within the reference's near-tie rows of that set (top-two float64 gap below
    1e-4 max |logit|; at most 1 % of the set); for the trained model every row outside the near ties predicted as the reference
    predicts it.  Returns the largest relative loss error."""
    n = data["A"].shape[0]
    worst = 0.0
    hist = res[0]["history"]
    assert [h["epoch"] for h in hist] == list(range(len(ref)))
    for h, want in zip(hist, ref):
        for name in SETS:
            assert h["rows"][name] == want["rows"][name] == int((data["split"] == 1 + SETS.index(name)).sum())
            assert want["near"][name] <= 0.01 * want["rows"][name], (h["epoch"], name, want["near"][name])
            assert abs(h["correct"][name] - want["correct"][name]) <= want["near"][name], (h["epoch"], name, h["correct"][name], want)
            e = abs(h["losses"][name] - want["loss"][name]) / max(abs(want["loss"][name]), 1e-30)
            worst = max(worst, e)
            assert e <= floor, (h["epoch"], name, h["losses"][name], want["loss"][name], e)
        assert h["loss"] == h["losses"]["train"]
    pred = gather_rows(res, "pred", n)
    differ = pred != final["pred"]
    assert not (differ & ~final["near_rows"]).any(), int((differ & ~final["near_rows"]).sum())
    for name in SETS:
        assert abs(res[0]["final"]["correct"][name] - final["correct"][name]) <= final["near"][name]
        assert res[0]["final"]["rows"][name] == final["rows"][name]
    return worst
