"""Shared by tests/test_gat_norm.py and tests/test_gat_norm_gpu.py: seeded operands of the normalising GAT tail, its definition in numpy
float64, one runner for the kernels and the composed twins, and a dense GAT model with the tail's options in any torch dtype."""
import math

import numpy as np
import torch
import torch.nn.functional as F

SEED, LAYER, EPS, P = 77, 1, 1e-5, 0.6
WHAT = ("Y", "mean", "rstd", "dX", "dbias", "dgamma", "dbeta")


def inputs(n, K, d, mean, seed):
    """fp32 operands; the global ids are spread and end at 2^31 - 1."""
    rng = np.random.default_rng(seed)
    fout = d if mean else K * d
    x = {"X": rng.standard_normal((n, K * d)), "bias": rng.standard_normal(fout), "gamma": 1 + 0.5 * rng.standard_normal(fout),
         "beta": 0.5 * rng.standard_normal(fout), "R": rng.standard_normal((n, fout)), "G": rng.standard_normal((n, fout))}
    x = {k: v.astype(np.float32) for k, v in x.items()}
    x["ids"] = np.arange(n, dtype=np.int64) * 3 + 1
    x["ids"][-1] = 2 ** 31 - 1
    return x


def shadow64(x, K, d, mean, bias, R, act, keep, scale):
    """The seven results of the definitions in include/pgcn_hip.h, in numpy float64."""
    X, G, ga, be = (x[k].astype(np.float64) for k in ("X", "G", "gamma", "beta"))
    n = X.shape[0]
    t = X.reshape(n, K, d).sum(1) * float(np.float32(1.0) / np.float32(K)) if mean else X
    if bias:
        t = t + x["bias"].astype(np.float64)
    f = t.shape[1]
    mu = t.sum(1) / f
    e = t - mu[:, None]
    rstd = 1.0 / np.sqrt((e * e).sum(1) / f + float(np.float32(EPS)))
    xh = e * rstd[:, None]
    u = ga * xh + be
    a = np.where(u > 0, u, np.expm1(u)) if act else u
    Y = np.where(keep, a * scale, 0.0) + (x["R"].astype(np.float64) if R else 0.0)
    g = np.where(keep, (G * scale) * (np.where(u <= 0, np.exp(u), 1.0) if act else 1.0), 0.0)
    gh = g * ga
    dT = rstd[:, None] * ((gh - gh.sum(1, keepdims=True) / f) - xh * ((gh * xh).sum(1, keepdims=True) / f))
    dX = np.tile(dT * float(np.float32(1.0) / np.float32(K)), (1, K)) if mean else dT
    return dict(zip(WHAT, (Y, mu, rstd, dX, dT.sum(0), (g * xh).sum(0), g.sum(0))))


def padded(t, pad, shift):
    """``t`` as a window of a NaN buffer with ``pad`` more columns, its base ``shift`` floats off a 16-byte boundary."""
    n, w = t.shape
    buf = torch.full((n * (w + pad) + 4,), float("nan"), device=t.device)[shift:shift + n * (w + pad)].view(n, w + pad)
    buf[:, :w] = t
    return buf[:, :w]


def run(M, D, x, K, d, mean, bias, R, act, drop, dev, k=None, pad=0, shift=0):
    """The seven results on ``dev``: the kernels of ``k`` (every matrix a window of a wider, shifted NaN buffer when ``pad`` or ``shift``
    is set), or the composed twins where it is None."""
    t = {key: torch.from_numpy(v).to(dev) for key, v in x.items()}
    if pad or shift:
        t.update({key: padded(t[key], pad, shift) for key in ("X", "R", "G")})
    b, r = (t["bias"] if bias else None), (t["R"] if R else None)
    thr, scale = D.threshold(P) if drop else (0, 1.0)
    state = D.DropoutState(SEED, dev) if drop else None
    v = (K, d, mean, b, t["gamma"], t["beta"])
    if k is not None:
        kw = dict(row_ids=t["ids"], seed=SEED, step=state.step, layer=LAYER, thr=thr) if drop else {}
        out = [padded(torch.zeros_like(a), pad, shift) if pad or shift else None for a in (t["G"], t["X"])]
        Y, mu, rstd = k.gat_tail_ln_forward(t["X"], *v, EPS, act, r, out=out[0], **kw)
        back = k.gat_tail_ln_backward(t["G"], t["X"], *v, mu, rstd, act, out=out[1], **kw)
    else:
        kw = dict(row_ids=t["ids"], state=state, layer=LAYER, thr=thr, scale=scale)
        Y, mu, rstd = M.gat_tail_ln_composed(t["X"], *v, EPS, act, r, **kw)
        back = M.gat_tail_ln_backward_composed(t["G"], t["X"], *v, mu, rstd, act, **kw)
    return dict(zip(WHAT, (Y, mu, rstd) + tuple(back)))


def dense_model(edge, H, params, cfg, dtype):
    """(output, {name: grad of sum(out cos(out))}) of a stack of GAT layers on the whole graph from dense operations in ``dtype``:
    ``edge`` bool [n, n] in the rows' own order, ``params`` the state of an nn.Sequential of PGAT layers, ``cfg`` per layer
    {K, concat, elu, residual, attention, keep (bool mask or None), scale}; bias and the norm are applied where the state has them."""
    p = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    h, n = H.detach().cpu().to(dtype), H.shape[0]
    for l, c in enumerate(cfg):
        g = lambda name: p.get("%d.%s" % (l, name))
        K = c["K"]
        d = g("linear.weight").shape[0] // K
        Z = (h @ g("linear.weight").t()).view(n, K, d)
        if c.get("attention") == "dot":
            q, kk = (h @ g("linear_q.weight").t()).view(n, K, d), (h @ g("linear_k.weight").t()).view(n, K, d)
            e = torch.einsum("ikd,jkd->kij", q, kk) / math.sqrt(d)
        else:
            a = g("attention")
            s1, s2 = torch.einsum("nkd,dk->nk", Z, a[:d]), torch.einsum("nkd,dk->nk", Z, a[d:])
            e = F.leaky_relu(s1.t().unsqueeze(2) + s2.t().unsqueeze(1), 0.2)
        alpha = torch.softmax(torch.where(edge.unsqueeze(0), e, torch.full((), -float("inf"), dtype=dtype)), 2)
        out = torch.einsum("kij,jkd->ikd", alpha, Z)
        t = out.reshape(n, K * d) if c["concat"] else out.mean(1)
        if g("bias") is not None:
            t = t + g("bias")
        if g("ln_weight") is not None:
            t = F.layer_norm(t, t.shape[1:], g("ln_weight"), g("ln_bias"), EPS)
        if c["elu"]:
            t = F.elu(t)
        if c.get("keep") is not None:
            t = torch.where(c["keep"], t * c["scale"], torch.zeros((), dtype=dtype))
        h = h + t if c["residual"] else t
    names = list(p)
    return h.detach(), dict(zip(names, torch.autograd.grad((h * torch.cos(h.detach())).sum(), [p[k] for k in names])))


def hold_model(case, model, out, edge, H, cfg):
    """``out`` and every parameter's gradient of ``model`` (after sum(out cos(out)).backward()) against ``dense_model`` in float64,
    the same model in fp32 as the fixture."""
    from conftest import held_to_fixture
    state = {k: v for k, v in model.state_dict().items()}
    (o64, g64), (o32, g32) = (dense_model(edge, H, state, cfg, dt) for dt in (torch.float64, torch.float32))
    held_to_fixture(case, "out", out.detach().cpu().numpy(), o32.numpy(), o64.numpy())
    for name, prm in model.named_parameters():
        e = held_to_fixture(case, "d " + name, prm.grad.cpu().numpy(), g32[name].numpy(), g64[name].numpy())
        print("%s d %s: model %.3g, fp32 dense twin %.3g from float64" % (case, name, *e))
