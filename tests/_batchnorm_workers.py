"""Definitions, data, float64 reference and worker processes of tests/test_batchnorm.py and tests/test_batchnorm_gpu.py (spawn start
method), in the pattern of tests/_nodeclass_workers.py."""
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

import _nodeclass_workers as NW  # noqa: E402

N, CLASSES, FIN, HIDDEN, NLAYERS = NW.N, NW.CLASSES, NW.FIN, 32, 3
EPOCHS, LR, WEIGHT_SEED = 8, 0.01, 5
DROPOUT, DROPOUT_SEED = 0.5, 11
MOMENTUM, EPS = 0.1, 1e-5
SETS = NW.SETS


# ---- the definition in float64 numpy ------------------------------------------------------------------------------------------------

def stats64(X):
    """(mean, biased variance clamped at 0, N) per column of X, from the sums the kernels form: sum x / N, sum x^2 / N - mean^2."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    mean = X.sum(0) / n
    var = np.maximum((X * X).sum(0) / n - mean * mean, 0.0)
    return mean, var, n


def bn64(X, gamma, beta, eps=EPS, keep=None, scale=1.0, mean=None, var=None):
    """(Y, mean, invstd) of y = keep ? max(0, gamma (x - mean) invstd + beta) * scale : 0 in float64; mean / var given: eval mode."""
    X = np.asarray(X, np.float64)
    if mean is None:
        mean, var, _ = stats64(X)
    invstd = 1.0 / np.sqrt(np.asarray(var, np.float64) + eps)
    Y = np.maximum(np.asarray(gamma, np.float64) * (X - mean) * invstd + np.asarray(beta, np.float64), 0.0)
    if keep is not None:
        Y = np.where(keep, Y * scale, 0.0)
    return Y, mean, invstd


def running64(rm, rv, mean, var, n, momentum=MOMENTUM):
    unbiased = var * n / (n - 1) if n > 1 else var
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unbiased


def bn_backward64(G, Y, X, mean, invstd, gamma, scale=1.0, n_global=None, S=None):
    """(dX, dgamma, dbeta, S1, S2) with g' = Y > 0 ? G scale : 0 and xh = (X - mean) invstd; S = (S1, S2) given: the global sums."""
    G, X = np.asarray(G, np.float64), np.asarray(X, np.float64)
    gm = np.where(np.asarray(Y) > 0, G * scale, 0.0)
    xh = (X - mean) * invstd
    S1, S2 = gm.sum(0), (gm * xh).sum(0)
    T1, T2 = (S1, S2) if S is None else S
    n = X.shape[0] if n_global is None else n_global
    dX = np.asarray(gamma, np.float64) * invstd * (gm - T1 / n - xh * T2 / n)
    return dX, S2, S1, S1, S2


# ---- the data set: the planted-community problem of the node-classification tests, features shifted and scaled per community ------------

def make_dataset(dirname):
    """NW.make_dataset renumbered so that every community is a range of vertex ids (the generator permutes them), plus: every
    community's features times 0.5 .. 2 and plus -2 .. 2, both growing with the community's index -- a rank that owns an id range
    sees other means and variances than the graph's; contiguous part vectors ``cpv<P>`` next to the random ``pv<P>``."""
    from scipy.io import mmwrite
    from conftest import pkg
    paths, data = NW.make_dataset(dirname)
    n = NW.N
    comm = pkg("synth").sbm_communities(n, NW.GRAPH_SEED, community=NW.COMMUNITY).numpy()
    order = np.argsort(comm, kind="stable")                    # new id i holds old vertex order[i]
    new_of_old = np.empty(n, np.int64)
    new_of_old[order] = np.arange(n)
    A = data["A"].tocoo()
    A = sp.coo_matrix((A.data, (new_of_old[A.row], new_of_old[A.col])), shape=(n, n))
    t = comm[order].astype(np.float64) / max(int(comm.max()), 1)
    X = (data["X"][order].astype(np.float64) * (0.5 + 1.5 * t)[:, None] + (4.0 * t - 2.0)[:, None]).astype(np.float32)
    data = {"A": A.tocsr(), "X": X, "labels": data["labels"][order], "split": data["split"][order]}
    mmwrite(paths["A"], A, field="pattern", symmetry="general")
    np.save(paths["features"], X)
    np.save(paths["labels"], data["labels"])
    np.save(paths["split"], data["split"])
    for P in (1, 2, 3):
        pv = (np.arange(n) * P) // n
        paths["cpv%d" % P] = os.path.join(dirname, "sbm.%d.cp" % P)
        with open(paths["cpv%d" % P], "w") as fh:
            fh.write(" ".join(map(str, pv.tolist())) + "\n")
    half = X[: n // 2].astype(np.float64)
    assert np.abs(half.mean(0) - X.astype(np.float64).mean(0)).max() > 0.3          # rank-local statistics differ visibly
    return paths, data


def initial_weights(widths, seed=WEIGHT_SEED):
    return NW.initial_weights(widths, seed)


def float64_reference(data, widths, epochs=EPOCHS, lr=LR, dropout=0.0, dropout_seed=DROPOUT_SEED, weight_seed=WEIGHT_SEED):
    """The model of run(norm="batch") in float64, one process, plain torch: every layer but the last is
    drop(relu(BN(A_hat H W^T))) by the definition (statistics over all n vertices, biased variance from sum x^2 / n - mean^2, running
    statistics with the unbiased one), Adam over weights, scales and shifts.  Per epoch the record the engine reports (without
    dropout: the training step's own logits; with dropout: an eval forward with the running statistics after the update).
    Returns (records, final record, [(running_mean, running_var)] per normalised layer)."""
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
    L = len(Ws)
    gammas = [torch.ones(widths[l + 1], dtype=torch.float64, requires_grad=True) for l in range(L - 1)]
    betas = [torch.zeros(widths[l + 1], dtype=torch.float64, requires_grad=True) for l in range(L - 1)]
    running = [(torch.zeros(widths[l + 1], dtype=torch.float64), torch.ones(widths[l + 1], dtype=torch.float64)) for l in range(L - 1)]
    opt = torch.optim.Adam(Ws + gammas + betas, lr=lr)
    thr, scale = D.threshold(dropout)

    def forward(step):
        h = X
        for l, w in enumerate(Ws):
            h = torch.sparse.mm(At, h) @ w.t()
            if l == L - 1:
                break
            if step is not None:
                mean = h.sum(0) / n
                var = ((h * h).sum(0) / n - mean * mean).clamp_min(0)
                with torch.no_grad():
                    rm, rv = running[l]
                    running[l] = ((1 - MOMENTUM) * rm + MOMENTUM * mean, (1 - MOMENTUM) * rv + MOMENTUM * var * n / (n - 1))
            else:
                mean, var = running[l]
            h = (gammas[l] * (h - mean) / torch.sqrt(var + EPS) + betas[l]).clamp_min(0)
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
            out.append(NW._stats64(forward(None) if dropout > 0.0 else logits.detach(), y, split))
    with torch.no_grad():
        final = NW._stats64(forward(None), y, split)
    return out, final, [(rm.numpy(), rv.numpy()) for rm, rv in running]


def run_worker(rank, P, port, paths, gpu, q, dropout=0.0, epochs=EPOCHS, seed=WEIGHT_SEED, partvec="pv", optimizer=None, norm="batch",
               nlayers=NLAYERS):
    """PGCN.run(..., norm=...) on rank `rank` of `P` over gloo (the checker-backed kernels on the CPU, the real ones on the GPU)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M = pkg("PGCN")
    if gpu == "composed":                            # a HIP device, but a provider without the batch-norm kernels: the composition
        K = pkg("kernels")

        class NoNorm(K.HipKernels):
            def __getattribute__(self, name):
                if name.startswith("bn_"):
                    raise AttributeError(name)
                return super().__getattribute__(name)

        M._kernel_provider = NoNorm(torch.device("cuda:0"))
    elif gpu:
        M._kernel_provider = None
    else:
        from oracle_kernels import OracleKernels
        M._kernel_provider = OracleKernels()
    M._exchanger = None
    got = {}

    def fn(*a, **kw):
        torch.manual_seed(seed)
        buf = io.StringIO()
        with redirect_stdout(buf):
            model = M.run(*a, **kw)
        got.update(history=model.history, best=model.best, widths=model.widths, stdout=buf.getvalue(),
                   running=[(m.running_mean.cpu().numpy(), m.running_var.cpu().numpy()) for m in model if getattr(m, "norm", None)],
                   params=[p.detach().cpu().numpy() for p in model.parameters()], hip=type(M._engine_current.k).__name__)

    kw = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=HIDDEN, epochs=epochs, lr=LR)
    if norm is not None:
        kw["norm"] = norm
    if dropout > 0.0:
        kw.update(dropout=dropout, dropout_seed=DROPOUT_SEED)
    if optimizer is not None:
        kw["optimizer"] = optimizer
    M.init_process(rank, P, fn, nlayers, HIDDEN, paths["A"], paths["%s%d" % (partvec, P)], "gloo", "sym", **kw)
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
        os.environ["HIP_VISIBLE_DEVICES"] = (saved or "0").split(",")[0]
    try:
        for p in procs:
            p.start()
    finally:
        if gpu:
            if saved is None:
                os.environ.pop("HIP_VISIBLE_DEVICES", None)
            else:
                os.environ["HIP_VISIBLE_DEVICES"] = saved
    import queue
    import time
    res, deadline = [], time.time() + 600
    while len(res) < P:                              # a rank that died answers at once, not when a time limit runs out
        try:
            res.append(q.get(timeout=0.2))
        except queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            if dead or time.time() > deadline:
                for p in procs:
                    p.kill()
                raise AssertionError("worker exit codes %r before every rank reported" % ([p.exitcode for p in procs],))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return sorted(res, key=lambda r: r["rank"])


def check_losses(res, ref, bound=1e-5):
    """Every reported epoch's loss of every set within `bound` (relative, floor 1) of the float64 loop; returns the largest error."""
    hist = res[0]["history"]
    assert [h["epoch"] for h in hist] == list(range(len(ref)))
    worst = 0.0
    for h, want in zip(hist, ref):
        for name in SETS:
            e = abs(h["losses"][name] - want["loss"][name]) / max(1.0, abs(want["loss"][name]))
            worst = max(worst, e)
            assert e <= bound, (h["epoch"], name, h["losses"][name], want["loss"][name], e)
    return worst


def check_running(res, running, bound=1e-5):
    worst = 0.0
    for r in res:                                    # every rank holds the same running statistics
        assert len(r["running"]) == len(running)
        for (rm, rv), (wm, wv) in zip(r["running"], running):
            for got, want in ((rm, wm), (rv, wv)):
                e = float((np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))).max())
                worst = max(worst, e)
                assert e <= bound, e
    return worst
