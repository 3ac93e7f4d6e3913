"""The definition of the softmax aggregation in float64 numpy, its error bounds, the double model and the worker processes of
tests/test_aggsoftmax.py and tests/test_aggsoftmax_gpu.py (spawn start method), in the pattern of tests/_aggmax_workers.py.

Definition (csrc/pgcn_aggsoftmax.hip), per feature column c over cand(i) = the stored columns of row i, x_j = H[j, c], beta >= 0:
    LSE[i, c] = log sum_j exp(beta x_j)          OUT[i, c] = sum_j exp(beta x_j - LSE[i, c]) x_j          empty: (0.0, -inf)
    dH[j, c]  = sum_{i : j in cand(i)} G[i, c] exp(beta x_j - LSE[i, c]) (1 + beta (x_j - OUT[i, c]))

Bounds (derived, not measured), k = |cand(i)|, range = max - min and amax = max |.| of the candidates:
    |OUT - OUT64| <= (k + 32 + 2 beta range) 2^-23 amax        |LSE - LSE64| <= (k + 32 + 2 beta range) 2^-23 max(1, |LSE64|)
k additions at 2^-24 each, an exp argument error of beta range 2^-24, a constant for exp, log, the division and up to three merges.
Backward, with the fp32 OUT / LSE handed to both sides and |G| <= 1, cnt terms per element, S = sum |G| p (1 + beta |x_j - OUT_i|):
    |D - D64| <= (cnt + 16 + 4 (beta amax + max |LSE|)) 2^-23 S + cnt 2^-120 (1 + 2 beta amax)
(the last term: the floor for terms that underflow fp32)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _aggmax_workers as AW  # noqa: E402
import _gradgrid_workers as GG  # noqa: E402

N = AW.N
FIN, CLASSES, HIDDEN, EPOCHS = AW.FIN, AW.CLASSES, AW.HIDDEN, 2
DROPOUT, DROPOUT_SEED, WEIGHT_SEED = AW.DROPOUT, AW.DROPOUT_SEED, 5
ENGINE_WIDTHS = (24, 32)
ENGINE_BETAS = (0.0, 1.0, 8.0)
MODEL_BETAS = (0.0, 1.0, 4.0)
SOFTMAX_METHODS = ("aggsoftmax", "aggsoftmax_backward")
make_dataset, bits, sym_pattern, rows = AW.make_dataset, AW.bits, AW.sym_pattern, AW.rows


# ---- the definition ---------------------------------------------------------------------------------------------------------------

def oracle_softmax(rowptr, col, H, beta):
    """dict(OUT, LSE: float64 [n, f]; k: int [n]; range, amax: float64 [n, f]) by the definition; an empty row (0, -inf)."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n, f = rowptr.shape[0] - 1, H.shape[1]
    H64 = H.astype(np.float64)
    OUT, LSE = np.zeros((n, f)), np.full((n, f), -np.inf)
    rng, amax = np.zeros((n, f)), np.zeros((n, f))
    for i in range(n):
        c = col[rowptr[i]:rowptr[i + 1]]
        if c.size:
            X = H64[c]
            z = beta * X
            top = z.max(axis=0)
            e = np.exp(z - top)
            s = e.sum(axis=0)
            OUT[i], LSE[i] = (e * X).sum(axis=0) / s, top + np.log(s)
            rng[i], amax[i] = X.max(axis=0) - X.min(axis=0), np.abs(X).max(axis=0)
    return dict(OUT=OUT, LSE=LSE, k=np.diff(rowptr), range=rng, amax=amax)


def forward_bounds(o, beta):
    """(bound on |OUT - OUT64|, bound on |LSE - LSE64|) per element; rows without entries: 0 (they are compared exactly)."""
    coef = (o["k"][:, None] + 32 + 2 * beta * o["range"]) * 2.0 ** -23
    lse = np.where(np.isfinite(o["LSE"]), o["LSE"], 0.0)
    return coef * o["amax"], np.where(o["k"][:, None] > 0, coef * np.maximum(1.0, np.abs(lse)), 0.0)


def assert_forward(OUT, LSE, o, beta, at, extra=0.0):
    """OUT / LSE (fp32) against the oracle `o` within the forward bound (+ ``extra`` on OUT); empty rows exactly (0.0f, -inf)."""
    assert OUT.dtype == np.float32 and LSE.dtype == np.float32, at
    assert not np.isnan(OUT).any() and not np.isnan(LSE).any(), (at, "NaN")
    empty = o["k"] == 0
    assert (OUT[empty] == 0).all() and (LSE[empty] == -np.inf).all(), (at, "empty rows")
    bo, bl = forward_bounds(o, beta)
    eo = np.abs(OUT.astype(np.float64) - o["OUT"])
    el = np.abs(np.where(empty[:, None], 0.0, LSE.astype(np.float64) - np.where(empty[:, None], 0.0, o["LSE"])))
    assert (eo <= bo + extra).all(), (at, "OUT", float((eo - bo - extra).max()), float((eo / np.maximum(bo + extra, 1e-300)).max()))
    assert (el <= bl).all(), (at, "LSE", float((el - bl).max()))
    return float((eo[bo > 0] / bo[bo > 0]).max()) if (bo > 0).any() else 0.0


def oracle_softmax_backward(rowptr, col, X, G, OUT, LSE, beta, n_out):
    """(D float64 [n_out, f], cnt int [n_out, f], S float64 [n_out, f]) over the FORWARD pattern (rowptr, col: row i holds its
    candidates j): X [n_out, f] the candidates' rows, G / OUT / LSE [n, f] as the kernel gets them (fp32 values, taken to float64)."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n, f = rowptr.shape[0] - 1, G.shape[1]
    ri = np.repeat(np.arange(n), np.diff(rowptr))
    D, S, cnt = np.zeros((n_out, f)), np.zeros((n_out, f)), np.zeros((n_out, f), np.int64)
    X64, G64, O64, L64 = (a.astype(np.float64) for a in (X, G, OUT, LSE))
    for c0 in range(0, f, 64):                                  # (nnz x 64 temporaries)
        c1 = min(f, c0 + 64)
        x = X64[col, c0:c1]
        p = np.exp(beta * x - L64[ri, c0:c1])
        t = G64[ri, c0:c1] * p
        np.add.at(D[:, c0:c1], col, t * (1 + beta * (x - O64[ri, c0:c1])))
        np.add.at(S[:, c0:c1], col, np.abs(t) * (1 + beta * np.abs(x - O64[ri, c0:c1])))
    cnt += np.bincount(col, minlength=n_out)[:, None]
    return D, cnt, S


def backward_bound(cnt, S, beta, amax, lmax):
    return (cnt + 16 + 4 * (beta * amax + lmax)) * 2.0 ** -23 * S + cnt * 2.0 ** -120 * (1 + 2 * beta * amax)


def assert_backward(D, rowptr, col, X, G, OUT, LSE, beta, at):
    D64, cnt, S = oracle_softmax_backward(rowptr, col, X, G, OUT, LSE, beta, X.shape[0])
    lmax = float(np.abs(LSE[np.isfinite(LSE)]).max()) if np.isfinite(LSE).any() else 0.0
    bound = backward_bound(cnt, S, beta, float(np.abs(X).max()), lmax)
    assert D.dtype == np.float32 and not np.isnan(D).any(), at
    err = np.abs(D.astype(np.float64) - D64)
    assert (err <= bound).all(), (at, "D", float((err - bound).max()), float((err / np.maximum(bound, 1e-300)).max()))
    return cnt


def merge(o1, l1, o2, l2):
    """The merge rule in numpy (any float type): two groups (OUT, LSE) as one; -inf: absent."""
    L = np.maximum(l1, l2)
    none = np.isneginf(L)
    Ls = np.where(none, 0, L)
    e1, e2 = np.exp(l1 - Ls), np.exp(l2 - Ls)
    t = np.where(none, 1, e1 + e2)
    return np.where(none, 0, (o1 * e1 + o2 * e2) / t), np.where(none, -np.inf, Ls + np.log(t))


def families(rng, n, f):
    """uniform in [-1, 1]; relu: half exact zeros; equal: every candidate equal; wide: uniform x 20 (beta range up to 320 at beta 8)."""
    u = rng.random((n, f), dtype=np.float32) * 2 - 1
    return {"uniform": u, "relu": np.maximum(rng.random((n, f), dtype=np.float32) * 2 - 1, 0).astype(np.float32),
            "equal": np.repeat(rng.random((1, f), dtype=np.float32) - 0.5, n, 0), "wide": (u * 20).astype(np.float32)}


# ---- providers --------------------------------------------------------------------------------------------------------------------

def _provider(M, gpu):
    """gpu false: the checker-backed provider (no softmax kernels: the composed route); true: the real one; "composed": the real one
    with the softmax kernels hidden."""
    from conftest import pkg
    if gpu == "composed":
        K = pkg("kernels")

        class NoSoftmax(K.HipKernels):
            def __getattribute__(self, name):
                if name in SOFTMAX_METHODS:
                    raise AttributeError(name)
                return super().__getattribute__(name)

        M._kernel_provider = NoSoftmax(torch.device("cuda:0"))
    elif gpu:
        M._kernel_provider = None
    else:
        from oracle_kernels import OracleKernels
        M._kernel_provider = OracleKernels()
    M._exchanger = None


# ---- engine level -----------------------------------------------------------------------------------------------------------------

def seeded_operands(f, kind):
    rng = np.random.default_rng([13, f, kind == "relu"])
    Hg = rng.random((N, f), dtype=np.float32) * 2 - 1
    if kind == "relu":
        Hg = np.maximum(Hg, 0).astype(np.float32)
    return Hg, rng.random((N, f), dtype=np.float32) * 2 - 1


def engine_worker(rank, P, port, paths, gpu, q, partvec="pv"):
    """forward_softmax / backward_softmax of rank `rank` of `P` over gloo on seeded global operands: per width, family and beta."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M = pkg("PGCN")
    _provider(M, gpu)
    got = {"rank": rank, "cases": []}

    def fn(r, size, nlayers, nfeatures, path_A, path_partvec, backend, **_):
        M.myrank, M.world_size = r, size
        M.device = torch.device("cuda:0") if gpu else torch.device("cpu")
        if gpu:
            torch.cuda.set_device(M.device)
        A = M._ingest.mmread(path_A)
        pv = M._partition.read_partvec(path_partvec)
        with redirect_stdout(io.StringIO()):
            M.compute_communication_maps(A, pv, r, size, "sym")
            eng = M.get_partitiont_of_adjacency_matrix(A, pv, r, "sym")
        own = eng.part.owned.cpu().numpy()
        got.update(own=own, lazy_before=eng._max is None, hip=type(eng.k).__name__)
        for f in ENGINE_WIDTHS:
            for kind in ("uniform", "relu"):
                Hg, Gg = seeded_operands(f, kind)
                H, G = torch.from_numpy(Hg[own]).to(M.device), torch.from_numpy(Gg[own]).to(M.device)
                for beta in ENGINE_BETAS:
                    OUT, LSE, halo = eng.forward_softmax(H, beta)
                    dH = eng.backward_softmax(G, H, halo, OUT, LSE, beta)
                    got["cases"].append(dict(f=f, kind=kind, beta=beta, OUT=OUT.cpu().numpy(), LSE=LSE.cpu().numpy(), dH=dH.cpu().numpy(),
                                             halo=None if halo is None else tuple(halo.shape)))
        m = eng._max
        got.update(composed=m.composed, halo_nnz=[int(a.nnz) for a in m.halo], halo_T_nnz=[int(a.nnz) for a in m.halo_T])

    M.init_process(rank, P, fn, 3, HIDDEN, paths["A"], paths["%s%d" % (partvec, P)], "gloo", "sym")
    q.put(got)


def spawn_engine(P, paths, gpu, **kw):
    return AW._spawn(engine_worker, P, paths, gpu, **kw)


def check_engine(res, data, P):
    """OUT / LSE / dH gathered over the ranks against the float64 oracle on the GLOBAL pattern, within the bounds (k, cnt, S from the
    global pattern); the halo rows are a tensor of their own at P > 1 and None at P = 1."""
    rowptr, col = sym_pattern(data["A"])
    assert all(r["lazy_before"] for r in res)
    if P > 1:
        assert all(sum(r["halo_nnz"]) > 0 and sum(r["halo_T_nnz"]) > 0 for r in res), "the halo structures hold no entries"
    worst = 0.0
    for k in range(len(res[0]["cases"])):
        c0 = res[0]["cases"][k]
        f, kind, beta = c0["f"], c0["kind"], c0["beta"]
        assert all((r["cases"][k]["halo"] is None) == (P == 1) for r in res)
        Hg, Gg = seeded_operands(f, kind)
        OUT, LSE, dH = (rows(res, lambda r, key=key: r["cases"][k][key]) for key in ("OUT", "LSE", "dH"))
        o = oracle_softmax(rowptr, col, Hg, beta)
        worst = max(worst, assert_forward(OUT, LSE, o, beta, (P, f, kind, beta)))
        assert_backward(dH, rowptr, col, Hg, Gg, OUT, LSE, beta, (P, f, kind, beta))
    return worst


# ---- model level ------------------------------------------------------------------------------------------------------------------

def config(norm="none", root=False, bias=False, residual=False, dropout=0.0, beta=1.0, nlayers=3):
    return dict(GG.config(norm, root, bias, residual, dropout, HIDDEN), beta=float(beta), nlayers=int(nlayers))


def tag(c):
    return "%s-b%g-l%d" % (GG.tag(c), c["beta"], c["nlayers"])


def model_configs():
    """plain; dropout; norm="node" + residual; root_weight + bias -- x beta in {0, 1, 4} x {2, 3} layers."""
    kinds = (dict(), dict(dropout=DROPOUT), dict(norm="node", residual=True), dict(root=True, bias=True))
    return [config(beta=b, nlayers=L, **k) for k in kinds for b in MODEL_BETAS for L in (2, 3)]


def rank_subset():
    return [config(beta=1.0, nlayers=3), config(dropout=DROPOUT, beta=4.0, nlayers=2), config(norm="node", residual=True, beta=0.0, nlayers=3),
            config(root=True, bias=True, beta=1.0, nlayers=2)]


def widths_of(c):
    return [FIN] + [c["hidden"]] * (c["nlayers"] - 1) + [CLASSES]


def softmax_aggregate(h, row, col, n, beta):
    """The definition with framework operations on the GLOBAL pattern (every row holds itself: none is empty), differentiable."""
    X = h[col]
    z = beta * X
    top = torch.full((n, h.shape[1]), float("-inf"), dtype=h.dtype).scatter_reduce(0, row.unsqueeze(1).expand(-1, h.shape[1]), z.detach(),
                                                                                   "amax", include_self=True)
    E = torch.exp(z - top[row])
    s = torch.zeros((n, h.shape[1]), dtype=h.dtype).index_add(0, row, E)
    return torch.zeros((n, h.shape[1]), dtype=h.dtype).index_add(0, row, E * X) / s


def model_softmax(data, widths, params, opts, step, dtype=torch.float64):
    """(loss, logits, {name: grad}) of GG.model64's model with the aggregation of every layer replaced by ``softmax_aggregate`` over
    the pattern of A + I.  Training mode."""
    from conftest import pkg
    D = pkg("dropout")
    n = data["A"].shape[0]
    rowptr, col = sym_pattern(data["A"])
    row = torch.from_numpy(np.repeat(np.arange(n), np.diff(rowptr)))
    col = torch.from_numpy(col)
    h = torch.from_numpy(data["X"]).to(dtype)
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    L = len(widths) - 1
    thr, scale = D.threshold(opts["dropout"])
    for l in range(L):
        z = softmax_aggregate(h, row, col, n, opts["beta"]) @ p["%d.linear.weight" % l].t()
        if opts["root"]:
            z = z + h @ p["%d.root.weight" % l].t()
        if l == L - 1:
            logits = z + p["%d.bias" % l] if opts["bias"] else z
            break
        f = z.shape[1]
        if opts["norm"] == "node":
            t = F.layer_norm(z, (f,), p["%d.ln_weight" % l], p["%d.ln_bias" % l], GG.EPS)
        else:
            t = z + p["%d.bias" % l] if opts["bias"] else z
        d = torch.relu(t)
        if opts["dropout"] > 0.0:
            keep = D.keep_mask(DROPOUT_SEED, step, l, np.arange(n), f, thr)
            d = torch.where(keep, d * scale, torch.zeros((), dtype=dtype))
        h = h + d if opts["residual"] and widths[l] == widths[l + 1] else d
    train = torch.from_numpy(data["split"] == 1)
    loss = F.cross_entropy(logits[train], torch.from_numpy(data["labels"])[train])
    names = list(p)
    grads = dict(zip(names, (g.detach() for g in torch.autograd.grad(loss, [p[k] for k in names]))))
    return loss.detach(), logits.detach(), grads


def model_worker(rank, P, port, paths, gpu, q, jobs=()):
    """AW.model_worker's protocol for run(epochs=2, lr=0.0, optimizer="torch", normalize="sym", softmax_beta=B): per job the parameters
    written into the model, the gradients before each optimiser step, this rank's loss and logits of each training step."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M = pkg("PGCN")
    _provider(M, gpu)
    cur = {}
    init = M.initiliaze_parameters

    def initialise(model):
        init(model)
        with torch.no_grad():
            for name, prm in model.named_parameters():
                prm.copy_(torch.from_numpy(cur["job"]["params"][name]))
        cur["model"] = model
        cur["names"] = [name for name, _ in model.named_parameters()]
        cur["kinds"] = sorted({type(m._aggregate).__name__ + ":" + getattr(m._aggregate, "__name__", "") for m in model})
        model.register_forward_hook(lambda m, a, out: cur["logits"].append(out.detach().cpu().numpy()) if m.training else None)

    adam_step = torch.optim.Adam.step

    def step(self, *a, **kw):
        cur["grads"].append({name: prm.grad.detach().cpu().numpy().copy() for name, prm in cur["model"].named_parameters()})
        return adam_step(self, *a, **kw)

    masked_loss = M.masked_loss

    def with_loss(*a, **kw):
        out = masked_loss(*a, **kw)
        cur["loss"].append(float(out[0].detach().double().cpu()))
        return out

    M.initiliaze_parameters = initialise
    torch.optim.Adam.step = step
    M.masked_loss = with_loss
    results = []

    def fn(r, size, nlayers, nfeatures, path_A, path_partvec, backend, **_):
        for job in jobs:
            c = job["config"]
            cur.update(job=job, grads=[], logits=[], loss=[])
            torch.manual_seed(job["seed"])
            kw = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=c["hidden"], epochs=EPOCHS, lr=0.0,
                      optimizer="torch", softmax_beta=c["beta"])
            if c["norm"] != "none":
                kw["norm"] = c["norm"]
            for name, opt in (("root", "root_weight"), ("bias", "bias"), ("residual", "residual")):
                if c[name]:
                    kw[opt] = True
            if c["dropout"] > 0.0:
                kw.update(dropout=c["dropout"], dropout_seed=DROPOUT_SEED)
            with redirect_stdout(io.StringIO()):
                M.run(r, size, c["nlayers"], c["hidden"], path_A, path_partvec, "gloo", normalize="sym", **kw)
            eng = M._engine_current
            results.append(dict(tag=tag(c), names=cur["names"], grads=cur["grads"], logits=cur["logits"], loss=cur["loss"],
                                own=eng.part.owned.cpu().numpy(), composed=eng._max.composed, hip=type(eng.k).__name__,
                                kinds=cur["kinds"]))

    M.init_process(rank, P, fn, 3, HIDDEN, paths["A"], paths["pv%d" % P], "gloo", "sym")
    q.put({"rank": rank, "results": results})


def spawn_model(P, paths, gpu, jobs):
    return [r["results"] for r in AW._spawn(model_worker, P, paths, gpu, jobs=jobs)]


def make_jobs(configs, seed=WEIGHT_SEED):
    jobs = []
    for c in configs:
        params = GG.initial_params(widths_of(c), c, seed)
        jobs.append({"config": c, "seed": seed, "params": {k: v.numpy() for k, v in params.items()}, "torch_params": params})
    return jobs


def strip(jobs):
    return [{k: v for k, v in j.items() if k != "torch_params"} for j in jobs]


def check_models(data, configs, jobs, res, case):
    """Per configuration and step: logits, loss and every reduced parameter gradient against the float64 model through
    conftest.held_to_fixture, the twin being the same model in fp32 (max(1e-5, 2 err_twin)); step 1's logits are step 0's without dropout."""
    from conftest import held_to_fixture
    P = len(res)
    held = 0
    for j, c in enumerate(configs):
        ranks = [r[j] for r in res]
        widths = widths_of(c)
        where = "aggsoftmax%s/%s/P%d" % (case, tag(c), P)
        for r in ranks:
            assert r["tag"] == tag(c) and sorted(r["names"]) == sorted(GG.parameter_names(widths, c)), where
            assert len(r["grads"]) == len(r["logits"]) == len(r["loss"]) == EPOCHS, where
        logits = [rows(ranks, lambda r, s=s: r["logits"][s]) for s in range(EPOCHS)]
        if c["dropout"] > 0.0:
            assert not np.array_equal(logits[0], logits[1]), where
        else:
            assert bits(logits[0]).tobytes() == bits(logits[1]).tobytes(), where + ": lr = 0 and no dropout, yet the steps' logits differ"
        for s in range(EPOCHS):
            opts = dict(c, task="single")
            l64, z64, g64 = model_softmax(data, widths, jobs[j]["torch_params"], opts, s, torch.float64)
            l32, z32, g32 = model_softmax(data, widths, jobs[j]["torch_params"], opts, s, torch.float32)
            at = "%s/step%d" % (where, s)
            held_to_fixture(at, "loss", np.array([sum(r["loss"][s] for r in ranks)]), l32.numpy().reshape(1), l64.numpy().reshape(1))
            held_to_fixture(at, "logits", logits[s], z32.numpy(), z64.numpy())
            held += 2
            for i, r in enumerate(ranks):
                for name in g64:
                    held_to_fixture(at + "/rank%d" % i, "grad " + name.split(".", 1)[1], r["grads"][s][name], g32[name].numpy(),
                                    g64[name].numpy())
                    held += 1
    return held


def check_hidden_against_kernels(data, configs, jobs, real, hidden, case):
    """The composed route (kernels hidden) held to the float64 model with the KERNEL route as the fixture: logits and every parameter
    gradient within conftest.held_to_fixture's bar, max(1e-5, 2 x the kernel route's own error)."""
    from conftest import held_to_fixture
    held = 0
    for j, c in enumerate(configs):
        a, b = real[0][j], hidden[0][j]
        widths = widths_of(c)
        for s in range(EPOCHS):
            _, z64, g64 = model_softmax(data, widths, jobs[j]["torch_params"], dict(c, task="single"), s, torch.float64)
            at = "aggsoftmax%s/%s/step%d" % (case, tag(c), s)
            held_to_fixture(at, "logits", rows([b], lambda r: r["logits"][s]), rows([a], lambda r: r["logits"][s]), z64.numpy())
            for name in g64:
                held_to_fixture(at, "grad " + name.split(".", 1)[1], b["grads"][s][name], a["grads"][s][name], g64[name].numpy())
                held += 1
    return held
