"""Reference, measurements and worker processes of tests/test_fused_adam.py and tests/test_fused_adam_gpu.py (spawn start method), in
the pattern of tests/_nodeclass_workers.py, whose planted-community data and statistics these tests import."""
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

import _nodeclass_workers as W  # noqa: E402

LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8
WD = 5e-4
THIRD = float(np.float32(1.0 / 3.0))       # the gradient scale of three ranks as the kernel receives it (a float argument)


def adam64(p, g, m, v, t, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0, decoupled=False, grad_scale=1.0):
    """The definition in float64 numpy: update number t (1-based) of p, m, v from the gradient g; returns the new (p, m, v)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    gi = g * grad_scale
    if decoupled:
        p = p * (1.0 - lr * weight_decay)
    else:
        gi = gi + weight_decay * p
    m = m + (gi - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * gi * gi
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    return p - (lr / bc1) * m / denom, m, v


def make_case(n, steps, seed):
    """fp32 start values and one fp32 gradient per step: mixed signs, a tenth of the gradients exactly 0, a tenth 1e-30."""
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = []
    for _ in range(steps):
        g = (rng.standard_normal(n) * np.exp(rng.uniform(-6, 1, n))).astype(np.float32)
        u = rng.random(n)
        g[u < 0.1] = 0.0
        g[(u >= 0.1) & (u < 0.2)] = np.float32(1e-30) * np.sign(g[(u >= 0.1) & (u < 0.2)])
        grads.append(g)
    return p0, grads


def reference_steps(p0, grads, **hyper):
    """adam64 over the fp32 gradients from the fp32 start: float64 (p, m, v)."""
    p, m, v = p0.astype(np.float64), np.zeros(p0.size), np.zeros(p0.size)
    for t, g in enumerate(grads, 1):
        p, m, v = adam64(p, g, m, v, t, **hyper)
    return p, m, v


def torch_steps(p0, grads, device, dtype=torch.float32, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0, decoupled=False, grad_scale=1.0):
    """torch.optim.Adam / AdamW on `device` from the same start and gradients (scaled in `dtype` first): (p, m, v) as float64 numpy."""
    p = torch.from_numpy(p0.copy()).to(device=device, dtype=dtype).requires_grad_(True)      # (a copy: from_numpy shares memory)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    for g in grads:
        p.grad = torch.from_numpy(g).to(device=device, dtype=dtype) * grad_scale
        opt.step()
    st = opt.state[p]
    return tuple(t.detach().double().cpu().numpy() for t in (p, st["exp_avg"], st["exp_avg_sq"]))


def errors_and_bound(got, yard, ref):
    """(e_got, e_yardstick, bound) of one array against float64: bound = 2 e_yardstick + 2^-23 max(1, max |ref|) -- twice the error
    of torch's own fp32 optimiser on the same inputs (a different fma contraction of the same expression) plus one rounding of the
    value."""
    e_got = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())
    e_yard = float(np.abs(np.asarray(yard, dtype=np.float64) - ref).max())
    return e_got, e_yard, 2.0 * e_yard + 2.0 ** -23 * max(1.0, float(np.abs(ref).max()))


# ---- the data loop in float64 with adam64 -------------------------------------------------------------------------------------------

def float64_reference(data, widths, epochs=W.EPOCHS, lr=W.LR, weight_decay=0.0, decoupled=False, weight_seed=W.WEIGHT_SEED):
    """W.float64_reference without dropout, with the optimiser written out (adam64): per-epoch records of the training step's logits,
    the record of the trained model, and the trained float64 weights."""
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
    Ws = [w.double().requires_grad_(True) for w in W.initial_weights(widths, weight_seed)]
    ms, vs = [np.zeros(tuple(w.shape)) for w in Ws], [np.zeros(tuple(w.shape)) for w in Ws]

    def forward():
        h = X
        for l, w in enumerate(Ws):
            h = torch.sparse.mm(At, h) @ w.t()
            if l < len(Ws) - 1:
                h = h.clamp_min(0)
        return h

    out = []
    for epoch in range(epochs):
        logits = forward()
        loss = torch.nn.functional.cross_entropy(logits[train], ytrain)
        for w in Ws:
            w.grad = None
        loss.backward()
        with torch.no_grad():
            out.append(W._stats64(logits.detach(), y, split))
            for i, w in enumerate(Ws):
                p, ms[i], vs[i] = adam64(w.numpy(), w.grad.numpy(), ms[i], vs[i], epoch + 1, lr=lr, weight_decay=weight_decay,
                                         decoupled=decoupled)
                w.copy_(torch.from_numpy(p))
    with torch.no_grad():
        final = W._stats64(forward(), y, split)
    return out, final, [w.detach().numpy().copy() for w in Ws]


def run_worker(rank, P, port, paths, gpu, q, opts):
    """W.run_worker with the optimiser options of `opts` (run's keyword arguments); reports the trained weights too."""
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
        M._kernel_provider = OracleKernels()       # test-only checker-backed kernels: no adam_step -> the composition
    M._exchanger = None
    got = {}

    def fn(*a, **kw):
        torch.manual_seed(W.WEIGHT_SEED)
        buf = io.StringIO()
        with redirect_stdout(buf):
            model = M.run(*a, **kw)
        data = M._nodedata.load(paths["features"], paths["labels"], paths["split"], M._engine_current.part.owned, W.N, device=M.device)
        model.eval()
        with torch.no_grad():
            logits = model(data.features)
        got.update(history=model.history, best=model.best, widths=model.widths, stdout=buf.getvalue(),
                   final=M.evaluate(model, data.features, data.labels, data.split), own=M._engine_current.part.owned.cpu().numpy(),
                   pred=logits.argmax(1).cpu().numpy(), hip=type(M._engine_current.k).__name__,
                   weights=[m.linear.weight.detach().cpu().numpy() for m in model])

    kw = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=W.HIDDEN, epochs=W.EPOCHS, lr=W.LR)
    kw.update(opts)
    M.init_process(rank, P, fn, W.NLAYERS, W.HIDDEN, paths["A"], paths["pv%d" % P], "gloo", "sym", **kw)
    got["rank"] = rank
    q.put(got)


def spawn_run(P, paths, gpu, **opts):
    import multiprocessing as mp
    from conftest import free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=run_worker, args=(r, P, port, paths, gpu, q, opts)) for r in range(P)]
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
    # a rank that dies (an option run() does not know, a refused launch) never answers, and its peers wait for it in a
    # collective: watch the exit codes while waiting, so that such a run fails at once
    res, deadline = [], time.monotonic() + 600
    try:
        while len(res) < P:
            try:
                res.append(q.get(timeout=0.2))
            except queue.Empty:
                failed = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode not in (None, 0)]
                assert not failed, "rank(s) ended without a result, (rank, exit code): %s" % failed
                assert time.monotonic() < deadline, "no result after 600 s"
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join()
    return sorted(res, key=lambda r: r["rank"])


def weight_errors(res, yard, ref_weights):
    """(e_run, e_yardstick, bound) over all layers of a run's trained weights (rank 0: every rank holds the same) against the float64
    reference, the yardstick being the run with torch's own optimiser on the same device."""
    got = np.concatenate([w.reshape(-1) for w in res[0]["weights"]])
    yd = np.concatenate([w.reshape(-1) for w in yard[0]["weights"]])
    ref = np.concatenate([w.reshape(-1) for w in ref_weights])
    return errors_and_bound(got, yd, ref)
