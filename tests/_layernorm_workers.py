"""Definitions, inputs, error bounds, float64 reference loop and worker processes of tests/test_layernorm.py and
tests/test_layernorm_gpu.py (spawn start method), in the pattern of tests/_batchnorm_workers.py.

The bounds.  U = 2^-24 (fp32 unit round-off), D = ceil(log2(max(f, 2))) + 4 (the depth of a row sum: a thread's quad, the tree over
the row's threads, the division), A_i = mean_j |x_ij|; r, xh, t, c1, c2 are the float64 values on the same fp32 inputs.
  exh = (D + 8) |xh| + D r_i A_i              what fp32 can lose in xh, over U: the row sums behind mean and rstd, the subtraction
  bf  = U s (|gamma_j| exh + 2 |beta_j| + 2 |t|)         the forward, dropout scale s; compared only where |t| > bf / s (elsewhere
                                                          the sign of t is within rounding, and with it the ReLU and the mask bit)
  bx  = U r_i [(D + 8)(|gh| + B1 + |xh| B2) + (|c2| + |xh| B1) exh + |xh| B1 Ex] + U (D + 8) |dX|,  B1 = mean_j |gh|,
        B2 = mean_j |gh xh|, Ex_i = max_j exh
  bg  = U sum_i |g'| (exh + 2 |xh|),   bb = 2 U sum_i |g'|          the column sums are added in double: one rounding at the end
mean and rstd: 8 U D relative to the float64 values.  For the mean that is a bound on a sum RELATIVE TO THE SUM: no fp32 summation
keeps it on a row whose terms cancel.  Two cases of the device grid exceed it (n = 2049 at f = 3 and f = 4: HISTORY 22); for THOSE TWO
the bound is twice the figure of torch's own fp32 layer_norm on the same input and device (``torch_mean``, handed in for them alone:
MEAN_BY_TORCH); every other case, and every other formula, stands as written."""
import math
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

U = 2.0 ** -24
EPS = 1e-5
N, CLASSES, FIN, HIDDEN = NW.N, NW.CLASSES, NW.FIN, 32
EPOCHS, LR, WEIGHT_SEED = 8, 0.01, 5
DROPOUT, DROPOUT_SEED = 0.5, 11
MEAN_BY_TORCH = ((2049, 3), (2049, 4))      # (n, f) of the device grid whose mean is held to twice torch's figure (module docstring)
MASK_STEP = 123                    # the training step whose masks the workers report
SETS = NW.SETS


# ---- the definition in float64 numpy ------------------------------------------------------------------------------------------------

def ln64(X, gamma, beta, eps=EPS, keep=None, scale=1.0, R=None):
    """dict(Y, d, mean, rstd, xh, t) of Y = R + (keep ? max(0, gamma (x - mean_i) rstd_i + beta) * scale : 0) in float64: mean and the
    biased variance of every ROW, two passes."""
    X = np.asarray(X, np.float64)
    f = X.shape[1]
    mean = X.sum(1) / f
    e = X - mean[:, None]
    rstd = 1.0 / np.sqrt((e * e).sum(1) / f + eps)
    xh = e * rstd[:, None]
    t = np.asarray(gamma, np.float64) * xh + np.asarray(beta, np.float64)
    d = np.maximum(t, 0.0)
    if keep is not None:
        d = np.where(keep, d * scale, 0.0)
    return {"Y": d if R is None else np.asarray(R, np.float64) + d, "d": d, "mean": mean, "rstd": rstd, "xh": xh, "t": t}


def ln_backward64(G, X, mean, rstd, gamma, bits, scale=1.0):
    """dict(dX, dgamma, dbeta, gm, gh, c1, c2) with g' = bit ? G scale : 0, gh = g' gamma, xh = (X - mean) rstd."""
    G, X = np.asarray(G, np.float64), np.asarray(X, np.float64)
    f = X.shape[1]
    gm = np.where(bits, G * scale, 0.0)
    gh = gm * np.asarray(gamma, np.float64)
    xh = (X - mean[:, None]) * rstd[:, None]
    c1, c2 = gh.sum(1) / f, (gh * xh).sum(1) / f
    dX = rstd[:, None] * ((gh - c1[:, None]) - xh * c2[:, None])
    return {"dX": dX, "dgamma": (gm * xh).sum(0), "dbeta": gm.sum(0), "gm": gm, "gh": gh, "c1": c1, "c2": c2}


def depth(f):
    return int(math.ceil(math.log2(max(f, 2)))) + 4


def make_case(n, f, seed):
    """fp32 (X, gamma, beta, G, R): rows N(shift, spread^2) with a spread of 0.1 .. 3 and a shift of +-2 per row; row 0 = 1000 + N(0, 1),
    row 1 = 1e-3 N(0, 1), row 2 constant 0.75 (variance 0), row 3 with 5 % of its elements times 100, row 4 zeros -- as far as n goes."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, f)) * rng.uniform(0.1, 3.0, n)[:, None] + rng.choice([-2.0, 2.0], n)[:, None]
    if n > 0:
        X[0] = 1000.0 + rng.standard_normal(f)
    if n > 1:
        X[1] = 1e-3 * rng.standard_normal(f)
    if n > 2:
        X[2] = 0.75
    if n > 3:
        out = rng.random(f) < 0.05
        out[rng.integers(f)] = True
        X[3, out] *= 100.0
    if n > 4:
        X[4] = 0.0
    return tuple(a.astype(np.float32) for a in (X, rng.uniform(0.5, 1.5, f), rng.uniform(-0.5, 0.5, f), rng.standard_normal((n, f)),
                                                rng.standard_normal((n, f))))


def forward_bounds(X, gamma, beta, ref, scale=1.0):
    """(bf, compared, exh) of the module docstring from the float64 forward ``ref`` = ln64(...)."""
    X = np.asarray(X, np.float64)
    f = X.shape[1]
    D = depth(f)
    A = np.abs(X).mean(1) if f else np.zeros(X.shape[0])
    exh = (D + 8) * np.abs(ref["xh"]) + D * (ref["rstd"] * A)[:, None]
    bf = U * scale * (np.abs(np.asarray(gamma, np.float64)) * exh + 2 * np.abs(np.asarray(beta, np.float64)) + 2 * np.abs(ref["t"]))
    return bf, np.abs(ref["t"]) > bf / scale, exh


def backward_bounds(X, ref, back, exh):
    """(bx, bg, bb) from the float64 forward ``ref`` and backward ``back`` = ln_backward64(..., the kernel's own bits)."""
    f = X.shape[1]
    D = depth(f)
    xh, r = np.abs(ref["xh"]), ref["rstd"][:, None]
    gh, gm = np.abs(back["gh"]), np.abs(back["gm"])
    B1 = gh.mean(1, keepdims=True)
    B2 = np.abs(back["gh"] * ref["xh"]).mean(1, keepdims=True)
    Ex = exh.max(1, keepdims=True)
    bx = U * r * ((D + 8) * (gh + B1 + xh * B2) + (np.abs(back["c2"])[:, None] + xh * B1) * exh + xh * B1 * Ex) + \
        U * (D + 8) * np.abs(back["dX"])
    return bx, U * (gm * (exh + 2 * xh)).sum(0), 2 * U * gm.sum(0)


def check_case(tag, X, gamma, beta, G, got, keep=None, scale=1.0, R=None, eps=EPS, torch_mean=None):
    """Every bound of the module docstring on one case.  ``got``: dict of numpy arrays Y, mean, rstd, bits (bool [n, f]), dX, dgamma,
    dbeta -- what the code under test produced (dX .. from the gradient G through ITS OWN bits).  Every figure is printed before it
    is asserted; returns them.  ``torch_mean``: the row means of torch's fp32 layer_norm on the same input and device (module docstring)."""
    n, f = X.shape
    D = depth(f)
    ref = ln64(X, gamma, beta, eps, keep, scale, R)
    bf, cmp_, exh = forward_bounds(X, gamma, beta, ref, scale)
    fig = {"left_out": int((~cmp_).sum())}
    if R is not None:
        bf = bf + U * np.abs(ref["Y"])
    tiny = 1e-300
    fig["forward"] = float((np.abs(got["Y"].astype(np.float64) - ref["Y"]) / np.maximum(bf, tiny))[cmp_].max()) if cmp_.any() else 0.0
    want_bits = (ref["t"] > 0) if keep is None else (keep & (ref["t"] > 0))
    fig["mask_wrong"] = int((got["bits"] != want_bits)[cmp_].sum())
    fig["mean"] = float((np.abs(got["mean"].astype(np.float64) - ref["mean"]) / np.maximum(8 * U * D * np.abs(ref["mean"]), tiny)).max()) if n else 0.0
    if torch_mean is not None and n:
        fig["mean_torch"] = float((np.abs(torch_mean.astype(np.float64) - ref["mean"]) / np.maximum(8 * U * D * np.abs(ref["mean"]), tiny)).max())
    fig["rstd"] = float((np.abs(got["rstd"].astype(np.float64) - ref["rstd"]) / (8 * U * D * ref["rstd"])).max()) if n else 0.0
    back = ln_backward64(G, X, ref["mean"], ref["rstd"], gamma, got["bits"], scale)
    bx, bg, bb = backward_bounds(np.asarray(X, np.float64), ref, back, exh)
    fig["dX"] = float((np.abs(got["dX"].astype(np.float64) - back["dX"]) / np.maximum(bx, tiny)).max()) if n else 0.0
    fig["dgamma"] = float((np.abs(got["dgamma"].astype(np.float64) - back["dgamma"]) / np.maximum(bg, tiny)).max())
    fig["dbeta"] = float((np.abs(got["dbeta"].astype(np.float64) - back["dbeta"]) / np.maximum(bb, tiny)).max())
    print("%s n %d f %d: error / bound  forward %.3g  mean %.3g  rstd %.3g  dX %.3g  dgamma %.3g  dbeta %.3g;  mask bits wrong %d;  "
          "left out (sign of t within rounding) %d of %d" % (tag, n, f, fig["forward"], fig["mean"], fig["rstd"], fig["dX"], fig["dgamma"],
                                                             fig["dbeta"], fig["mask_wrong"], fig["left_out"], n * f), flush=True)
    if "mean_torch" in fig:
        print("    mean: torch's fp32 layer_norm on the same input and device, error / bound %.3g" % fig["mean_torch"], flush=True)
    assert fig["left_out"] <= max(2, 0.01 * n * f), fig
    assert fig["forward"] <= 1.0 and fig["mask_wrong"] == 0, fig
    assert fig["mean"] <= max(1.0, 2.0 * fig.get("mean_torch", 0.0)) and fig["rstd"] <= 1.0, fig
    assert fig["dX"] <= 1.0 and fig["dgamma"] <= 1.0 and fig["dbeta"] <= 1.0, fig
    return fig


# ---- the float64 loop of run(norm="node", residual=True) -----------------------------------------------------------------------------------

def make_dataset(dirname):
    return BW.make_dataset(dirname)


def float64_reference(data, widths, epochs=EPOCHS, lr=LR, dropout=0.0, dropout_seed=DROPOUT_SEED, weight_seed=WEIGHT_SEED, residual=True):
    """The model of run(norm="node", residual=...) in float64, one process: dense A_hat, torch double autograd, every layer but the last
    H' = [H +] drop(relu(LN(A_hat H W^T))) by the definition (the residual where the layer's two widths are equal), dropout.keep_mask for
    the masks, Adam written out in torch double over weights, scales and shifts.  Per epoch the record the engine reports (without
    dropout: the training step's own logits; with dropout: an eval forward after the update).  Returns (records, best epoch)."""
    from conftest import pkg
    D = pkg("dropout")
    n = data["A"].shape[0]
    B = (data["A"] + sp.identity(n, format="csr")).astype(np.float64)
    B.data[:] = 1.0
    dr = 1.0 / np.sqrt(np.asarray(B.sum(axis=1)).reshape(-1))
    dc = 1.0 / np.sqrt(np.asarray(B.sum(axis=0)).reshape(-1))
    Ad = torch.from_numpy((sp.diags(dr) @ B @ sp.diags(dc)).toarray())
    X = torch.from_numpy(data["X"]).double()
    y, split = data["labels"], data["split"]
    train = torch.from_numpy(split == 1)
    ytrain = torch.from_numpy(y)[train]
    Ws = [w.double().requires_grad_(True) for w in NW.initial_weights(widths, weight_seed)]
    L = len(Ws)
    gammas = [torch.ones(widths[l + 1], dtype=torch.float64, requires_grad=True) for l in range(L - 1)]
    betas = [torch.zeros(widths[l + 1], dtype=torch.float64, requires_grad=True) for l in range(L - 1)]
    params = Ws + gammas + betas
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    b1, b2, aeps = 0.9, 0.999, 1e-8
    thr, scale = D.threshold(dropout)

    def forward(step):
        h = X
        for l, w in enumerate(Ws):
            z = (Ad @ h) @ w.t()
            if l == L - 1:
                return z
            mean = z.sum(1, keepdim=True) / z.shape[1]
            e = z - mean
            d = (gammas[l] * (e / torch.sqrt((e * e).sum(1, keepdim=True) / z.shape[1] + EPS)) + betas[l]).clamp_min(0)
            if step is not None and dropout > 0.0:
                keep = D.keep_mask(dropout_seed, step, l, np.arange(n), d.shape[1], thr)
                d = torch.where(keep, d * scale, torch.zeros((), dtype=torch.float64))
            h = h + d if residual and widths[l] == widths[l + 1] else d

    out = []
    for epoch in range(epochs):
        logits = forward(epoch)
        loss = torch.nn.functional.cross_entropy(logits[train], ytrain)
        grads = torch.autograd.grad(loss, params)
        with torch.no_grad():
            for p, g, mi, vi in zip(params, grads, m, v):
                mi.mul_(b1).add_(g, alpha=1 - b1)
                vi.mul_(b2).addcmul_(g, g, value=1 - b2)
                p.sub_(lr * (mi / (1 - b1 ** (epoch + 1))) / (torch.sqrt(vi / (1 - b2 ** (epoch + 1))) + aeps))
            out.append(NW._stats64(forward(None) if dropout > 0.0 else logits.detach(), y, split))
    acc = [r["correct"]["val"] / max(r["rows"]["val"], 1) for r in out]
    return out, int(np.argmax(acc))


def run_worker(rank, P, port, paths, gpu, q, dropout=0.0, epochs=EPOCHS, seed=WEIGHT_SEED, partvec="pv", optimizer=None, norm="node",
               nlayers=8, residual=True, masks=False):
    """PGCN.run(..., norm=..., residual=...) on rank `rank` of `P` over gloo (the checker-backed kernels on the CPU, the real ones on the
    GPU; gpu == "composed": a HIP provider that lacks the layer-norm kernels).  ``masks``: also the first hidden layer's output of the
    trained model in train mode at step MASK_STEP and in eval mode, with the rows' global ids."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M = pkg("PGCN")
    if gpu == "composed":
        K = pkg("kernels")

        class NoLayerNorm(K.HipKernels):
            def __getattribute__(self, name):
                if name.startswith("ln_"):
                    raise AttributeError(name)
                return super().__getattribute__(name)

        M._kernel_provider = NoLayerNorm(torch.device("cuda:0"))
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
                   names=[n for n, _ in model.named_parameters()], buffers=[n for n, _ in model.named_buffers()],
                   residual=[bool(getattr(l, "residual", False)) for l in model], own=M._engine_current.part.owned.cpu().numpy(),
                   params=[p.detach().cpu().numpy() for p in model.parameters()], hip=type(M._engine_current.k).__name__)
        if masks or gpu:
            data = M._nodedata.load(paths["features"], paths["labels"], paths["split"], M._engine_current.part.owned, N, device=M.device)
            layer = model[0]
            model.train()
            y0 = layer(data.features)                   # (layer 0 has no residual: its output's node is the layer-norm node)
            got["node"], got["mask_dtype"] = type(y0.grad_fn).__name__, str(y0.grad_fn.saved_tensors[4].dtype)
            del y0
        if masks:
            with torch.no_grad():
                layer.state.step.fill_(MASK_STEP)
                model.train()
                got["y_train"] = layer(data.features).cpu().numpy()
                model.eval()
                got["y_eval"] = layer(data.features).cpu().numpy()

    kw = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=HIDDEN, epochs=epochs, lr=LR)
    if norm is not None:
        kw["norm"] = norm
    if residual:
        kw["residual"] = True
    if dropout > 0.0:
        kw.update(dropout=dropout, dropout_seed=DROPOUT_SEED)
    if optimizer is not None:
        kw["optimizer"] = optimizer
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


def check_losses(res, ref, bound=1e-5):
    """Every reported epoch's loss of every set within `bound` relative of the reference records; returns the largest error."""
    hist = res[0]["history"]
    assert [h["epoch"] for h in hist] == list(range(len(ref)))
    worst = 0.0
    for h, want in zip(hist, ref):
        for name in SETS:
            w = want["losses"][name] if "losses" in want else want["loss"][name]          # (a history entry, or a float64 record)
            e = abs(h["losses"][name] - w) / abs(w)
            worst = max(worst, e)
    print("largest relative loss error %.3g (bound %.3g)" % (worst, bound), flush=True)
    assert worst <= bound, worst
    return worst
