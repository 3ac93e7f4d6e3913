"""The float64 side of tests/test_train_control.py and tests/test_train_control_gpu.py: the schedule and the clip of optim.py written out
again in numpy doubles, F.adam64 under them, and the data loop of F.float64_reference with both -- in the pattern of
tests/_fused_adam_workers.py, whose cases, bound and worker processes these tests use."""
import math

import numpy as np
import scipy.sparse as sp
import torch

import _fused_adam_workers as F
import _nodeclass_workers as W


def lr64(t, sched):
    """lr_at of optim.py, restated: ``t`` updates already made, sched = (kind, base, W, T, lr_min, S, gamma)."""
    kind, base, Wm, T, lr_min, S, gamma = sched
    if kind == "cosine":
        u = min(max((t - Wm) / (T - Wm), 0.0), 1.0)
        s = lr_min + (base - lr_min) * 0.5 * (1.0 + math.cos(math.pi * u))
    elif kind == "step":
        s = base * gamma ** math.floor(max(t - Wm, 0) / S)
    else:
        s = base
    return s * (t + 1) / Wm if t < Wm else s


def clip64(grads, max_norm, grad_scale=1.0):
    """(sumsq, norm, coef) of the global L2 norm of the arrays ``grads`` in float64; coef = 1 without ``max_norm``."""
    sumsq = float(sum(np.sum(np.asarray(g, dtype=np.float64) ** 2) for g in grads))
    norm = math.sqrt(sumsq) * abs(grad_scale) if not math.isnan(sumsq) else float("nan")
    if not max_norm:
        return sumsq, norm, 1.0
    c = max_norm / (norm + 1e-6)
    return sumsq, norm, (c if c < 1.0 or math.isnan(c) else 1.0)


def reference_steps(p0, grads, sched, max_norm, first=0, **hyper):
    """F.reference_steps under the schedule and the clip: float64 (p, m, v) and the per-step records (sumsq, norm, coef, lr)."""
    p, m, v = p0.astype(np.float64), np.zeros(p0.size), np.zeros(p0.size)
    gs = hyper.pop("grad_scale", 1.0)
    recs = []
    for t, g in enumerate(grads, first):
        sumsq, norm, coef = clip64([g], max_norm, gs)
        lr = lr64(t, sched)
        recs.append((sumsq, norm, coef, lr))
        p, m, v = F.adam64(p, g, m, v, t + 1, lr=lr, grad_scale=gs * coef, **hyper)
    return (p, m, v), recs


def torch_steps(p0, grads, device, sched, max_norm, weight_decay=0.0, decoupled=False, grad_scale=1.0):
    """The yardstick: torch.optim.Adam / AdamW in fp32 on ``device`` with torch.nn.utils.clip_grad_norm_ and the learning rate set by
    hand before every step, on the same inputs; (p, m, v) as float64 numpy."""
    p = torch.from_numpy(p0.copy()).to(device=device).requires_grad_(True)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=sched[1], betas=F.BETAS, eps=F.EPS, weight_decay=weight_decay)
    for t, g in enumerate(grads):
        p.grad = torch.from_numpy(g).to(device=device) * grad_scale
        if max_norm:
            torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.param_groups[0]["lr"] = lr64(t, sched)
        opt.step()
    st = opt.state[p]
    return tuple(t.detach().double().cpu().numpy() for t in (p, st["exp_avg"], st["exp_avg_sq"]))


def float64_reference(data, widths, epochs=W.EPOCHS, lr=W.LR, sched=None, max_norm=None, weight_decay=0.0, decoupled=False,
                      weight_seed=W.WEIGHT_SEED):
    """F.float64_reference with the clip over all layers' gradients and the schedule: (per-epoch records, the trained model's record,
    the trained float64 weights, the per-epoch (norm, coef, lr))."""
    sched = sched or ("constant", lr, 0, 0, 0.0, 1, 1.0)
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

    out, ctl = [], []
    for epoch in range(epochs):
        logits = forward()
        loss = torch.nn.functional.cross_entropy(logits[train], ytrain)
        for w in Ws:
            w.grad = None
        loss.backward()
        with torch.no_grad():
            out.append(W._stats64(logits.detach(), y, split))
            _, norm, coef = clip64([w.grad.numpy() for w in Ws], max_norm)
            rate = lr64(epoch, sched)
            ctl.append((norm, coef, rate))
            for i, w in enumerate(Ws):
                p, ms[i], vs[i] = F.adam64(w.numpy(), w.grad.numpy(), ms[i], vs[i], epoch + 1, lr=rate, weight_decay=weight_decay,
                                           decoupled=decoupled, grad_scale=coef)
                w.copy_(torch.from_numpy(p))
    with torch.no_grad():
        final = W._stats64(forward(), y, split)
    return out, final, [w.detach().numpy().copy() for w in Ws], ctl


def reported(epochs, eval_every, first=0):
    """The epochs a run of ``epochs`` epochs from ``first`` reports."""
    return [e for e in range(first, first + epochs) if e % eval_every == 0 or e == first + epochs - 1]


def stop_epoch(vals, epochs_reported, patience):
    """The epoch at which ``patience`` stops a run whose reported epochs have the validation scores ``vals`` (None: it runs out)."""
    best, stale = None, 0
    for e, v in zip(epochs_reported, vals):
        if best is None or v > best:
            best, stale = v, 0
        else:
            stale += 1
        if stale >= patience:
            return e
    return None
