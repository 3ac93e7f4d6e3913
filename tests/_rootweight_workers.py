"""Definitions, float64 reference and worker processes of tests/test_rootweight.py and tests/test_rootweight_gpu.py (spawn start
method), in the pattern of tests/_batchnorm_workers.py whose data set and spawn helpers they share."""
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

import _batchnorm_workers as BW  # noqa: E402
import _nodeclass_workers as NW  # noqa: E402

N, CLASSES, FIN, HIDDEN, NLAYERS = BW.N, BW.CLASSES, BW.FIN, BW.HIDDEN, 3
EPOCHS, LR, WEIGHT_SEED = 8, 0.01, 5
DROPOUT, DROPOUT_SEED = 0.5, 11
MASK_STEP = 123                    # the training step whose masks the workers report
SETS = NW.SETS
WIDTHS = [FIN, HIDDEN, HIDDEN, CLASSES]

make_dataset = BW.make_dataset
check_losses = BW.check_losses


# ---- the definition in numpy ---------------------------------------------------------------------------------------------------------------

def combine32(z1, z2, b, relu, keep=None, scale=1.0):
    """The kernel's statement in fp32 numpy: t = (z1 + z2) + b, each addition rounded to fp32, an absent (None) term not added;
    relu: keep ? max(0, t) * scale : 0 (max as `t < 0 ? 0 : t`)."""
    t = np.asarray(z1, np.float32)
    if z2 is not None:
        t = (t + np.asarray(z2, np.float32)).astype(np.float32)
    if b is not None:
        t = (t + np.asarray(b, np.float32)[None, :]).astype(np.float32)
    if not relu:
        return t.copy()
    y = np.where(t < 0, np.float32(0), t).astype(np.float32)
    if keep is not None:
        y = np.where(keep, (y * np.float32(scale)).astype(np.float32), np.float32(0)).astype(np.float32)
    return y


def masked_grad32(G, Y, relu, scale=1.0):
    G = np.asarray(G, np.float32)
    if not relu:
        return G.copy()
    return np.where(np.asarray(Y) > 0, (G * np.float32(scale)).astype(np.float32), np.float32(0)).astype(np.float32)


def dbias_error_and_bound(dbias, Gm):
    """(|dbias - fp32(ref64)|, ulp32(ref64) + n 2^-52 sum |Gm|) per column, ref64 the float64 column sum of the fp32 Gm: one rounding
    of the result to fp32 plus the worst case of n double additions."""
    Gd = np.asarray(Gm, np.float64)
    n = Gd.shape[0]
    ref = Gd.sum(0)
    r32 = ref.astype(np.float32)
    ulp = np.spacing(np.abs(r32)).astype(np.float64)
    return np.abs(np.asarray(dbias, np.float64) - r32.astype(np.float64)), ulp + n * 2.0 ** -52 * np.abs(Gd).sum(0)


# ---- the float64 loop -----------------------------------------------------------------------------------------------------------------------

def initial_parameters(widths, root_weight=True, seed=WEIGHT_SEED):
    """[(W_n, W_r or None)] per layer: the model's own initial weights -- run() builds layer by layer after torch.manual_seed(seed),
    ``linear`` before ``root``; the biases start at zero."""
    torch.manual_seed(seed)
    out = []
    for a, b in zip(widths, widths[1:]):
        wn = torch.nn.Linear(a, b, bias=False).weight.detach().double().numpy().copy()
        wr = torch.nn.Linear(a, b, bias=False).weight.detach().double().numpy().copy() if root_weight else None
        out.append((wn, wr))
    return out


def float64_reference(data, widths=WIDTHS, epochs=EPOCHS, lr=LR, dropout=0.0, dropout_seed=DROPOUT_SEED, weight_seed=WEIGHT_SEED,
                      root_weight=True, bias=True):
    """run(root_weight=True, bias=True) restated in float64 numpy, one process: every layer is act(A_hat H W_n^T + H W_r^T + b) with
    ReLU and the host statement of the dropout masks on all layers but the last, the mean cross entropy over the train rows, the
    backward written out (dH = A_hat^T (Gm W_n) + Gm W_r, db = column sums of Gm), Adam with torch's defaults.  Per epoch the record the
    engine reports (without dropout: the training step's own logits; with dropout: an eval forward after the update).  Returns
    (records, best epoch = the first of the best validation accuracy)."""
    from conftest import pkg
    D = pkg("dropout")
    n = data["A"].shape[0]
    B = (data["A"] + sp.identity(n, format="csr")).astype(np.float64)
    B.data[:] = 1.0
    dr = 1.0 / np.sqrt(np.asarray(B.sum(axis=1)).reshape(-1))
    dc = 1.0 / np.sqrt(np.asarray(B.sum(axis=0)).reshape(-1))
    Ah = (sp.diags(dr) @ B @ sp.diags(dc)).tocsr()
    AhT = Ah.T.tocsr()
    X = data["X"].astype(np.float64)
    y, split = data["labels"], data["split"]
    train = split == 1
    n_train = int(train.sum())
    L = len(widths) - 1
    params = []                      # flat list of arrays, the layout [W_n, W_r, b] per layer
    for (wn, wr), fout in zip(initial_parameters(widths, root_weight, weight_seed), widths[1:]):
        params.append([wn, wr, np.zeros(fout) if bias else None])
    flat = [p for layer in params for p in layer if p is not None]
    m = [np.zeros_like(p) for p in flat]
    v = [np.zeros_like(p) for p in flat]
    thr, scale = D.threshold(dropout)
    b1, b2, eps = 0.9, 0.999, 1e-8

    def forward(step):
        h, saved = X, []
        for l, (wn, wr, b) in enumerate(params):
            ah = Ah @ h
            z = ah @ wn.T
            if wr is not None:
                z = z + h @ wr.T
            if b is not None:
                z = z + b
            keep = None
            if l < L - 1:
                out = np.maximum(z, 0.0)
                if step is not None and dropout > 0.0:
                    keep = D.keep_mask(dropout_seed, step, l, np.arange(n), z.shape[1], thr).numpy()
                    out = np.where(keep, out * scale, 0.0)
            else:
                out = z
            saved.append((h, ah, z, keep))
            h = out
        return h, saved

    def backward(logits, saved):
        zmax = logits.max(1, keepdims=True)
        p = np.exp(logits - zmax)
        p /= p.sum(1, keepdims=True)
        g = np.zeros_like(logits)
        rows = np.nonzero(train)[0]
        g[rows] = p[rows]
        g[rows, y[rows]] -= 1.0
        g /= n_train
        grads = [None] * L
        for l in range(L - 1, -1, -1):
            h, ah, z, keep = saved[l]
            wn, wr, b = params[l]
            if l < L - 1:
                g = np.where(z > 0, g, 0.0)
                if keep is not None:
                    g = np.where(keep, g * scale, 0.0)
            grads[l] = [g.T @ ah, g.T @ h if wr is not None else None, g.sum(0) if b is not None else None]
            if l > 0:
                gh = AhT @ (g @ wn)
                if wr is not None:
                    gh = gh + g @ wr
                g = gh
        return [x for layer in grads for x in layer if x is not None]

    out = []
    for epoch in range(epochs):
        logits, saved = forward(epoch)
        grads = backward(logits, saved)
        t = epoch + 1
        for p, g, mi, vi in zip(flat, grads, m, v):
            mi *= b1
            mi += (1 - b1) * g
            vi *= b2
            vi += (1 - b2) * g * g
            p -= (lr / (1 - b1 ** t)) * (mi / (np.sqrt(vi) / np.sqrt(1 - b2 ** t) + eps))
        rec_logits = forward(None)[0] if dropout > 0.0 else logits
        out.append(NW._stats64(torch.from_numpy(np.ascontiguousarray(rec_logits)), y, split))
    acc = [r["correct"]["val"] / max(r["rows"]["val"], 1) for r in out]
    return out, int(np.argmax(acc))


# ---- the workers ----------------------------------------------------------------------------------------------------------------------------

def run_worker(rank, P, port, paths, gpu, q, dropout=0.0, epochs=EPOCHS, seed=WEIGHT_SEED, partvec="pv", optimizer=None, norm=None,
               nlayers=NLAYERS, root_weight=True, bias=True, masks=False):
    """PGCN.run(..., root_weight=..., bias=...) on rank `rank` of `P` over gloo (the checker-backed kernels on the CPU, the real ones on
    the GPU; gpu == "composed": a HIP provider that lacks the combine kernels).  ``masks``: also the first hidden layer's output of the
    trained model in train mode at step MASK_STEP and in eval mode, with the rows' global ids."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M = pkg("PGCN")
    if gpu == "composed":
        K = pkg("kernels")

        class NoCombine(K.HipKernels):
            def __getattribute__(self, name):
                if name.startswith("combine_"):
                    raise AttributeError(name)
                return super().__getattribute__(name)

        M._kernel_provider = NoCombine(torch.device("cuda:0"))
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
                   names=[n for n, _ in model.named_parameters()], own=M._engine_current.part.owned.cpu().numpy(),
                   params=[p.detach().cpu().numpy() for p in model.parameters()], hip=type(M._engine_current.k).__name__)
        if masks:
            data = M._nodedata.load(paths["features"], paths["labels"], paths["split"], M._engine_current.part.owned, N, device=M.device)
            layer = model[0]
            with torch.no_grad():
                layer.state.step.fill_(MASK_STEP)
                model.train()
                got["y_train"] = layer(data.features).cpu().numpy()
                model.eval()
                got["y_eval"] = layer(data.features).cpu().numpy()

    kw = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=HIDDEN, epochs=epochs, lr=LR)
    if norm is not None:
        kw["norm"] = norm
    if dropout > 0.0:
        kw.update(dropout=dropout, dropout_seed=DROPOUT_SEED)
    if optimizer is not None:
        kw["optimizer"] = optimizer
    if root_weight:
        kw["root_weight"] = True
    if bias:
        kw["bias"] = True
    M.init_process(rank, P, fn, nlayers, HIDDEN, paths["A"], paths["%s%d" % (partvec, P)], "gloo", "sym", **kw)
    got["rank"] = rank
    q.put(got)


def spawn_run(P, paths, gpu, **kw):
    """BW.spawn_run with this file's worker."""
    saved = BW.run_worker
    BW.run_worker = run_worker
    try:
        return BW.spawn_run(P, paths, gpu, **kw)
    finally:
        BW.run_worker = saved


def gather_rows(res, key, n=N):
    return NW.gather_rows(res, key, n)
