"""The definition of the PNA aggregators in float64 numpy (a direct two-pass transcription), their error bounds, the double model
and the worker processes of tests/test_aggpna.py and tests/test_aggpna_gpu.py, in the pattern of tests/_aggsoftmax_workers.py.

Definition (csrc/pgcn_aggpna.hip), per feature c over cand(i) = the stored columns of row i, d = |cand(i)|, x_j = H[j, c]:
    MEAN = sum x / d     MAX / MIN with the smallest global id among the extremes     VAR = sum (x - MEAN)^2 / d     STD = sqrt(VAR + 1e-5)
    d = 0: all 0, args -1.     Q = dSTD / (d STD), P = dMEAN / d - Q MEAN:
    dH[j] = sum_{i : j in cand(i)} (P[i] + (AMAX[i] == j ? dMAX[i] : 0) + (AMIN[i] == j ? dMIN[i] : 0)) + H[j] sum_i Q[i]

Bounds (derived from the arithmetic the header prescribes, u = 2^-24, written with 2^-23 = 2 u), amax = max |x|, spread = max |x - MEAN|:
    MEAN: the shifted terms |x - K| <= 2 spread are summed in d additions (error <= d u per unit of sum |x - K| <= 2 d spread, divided by
          d again), and every merge of two pieces rounds a mean of size <= amax once; a row has at most 9 + d / 32 pieces (8 slices, cuts
          of at least half a chunk of 64, one accumulated call):        |dMEAN| <= 2^-23 ((2 d + 16) spread + (10 + d / 32) amax)
    VAR:  s2 and s1^2 / d are sums of d terms <= (2 spread)^2 each with relative error (d + O(1)) u, divided by d; a merge adds
          dl^2 n_a n_b / n with dl = m_b - m_a carrying the rounding 2 u amax of the two stored means, |dl| <= 2 spread, and the weights
          n_a n_b / (n d) of all merges of a row sum to <= 1:             |dVAR| <= 2^-23 ((d + 32) 8 spread^2 + 8 spread amax)
    STD:  sqrt(VAR + eps) moves by <= |dVAR| / (2 STD) to first order; dVAR may be negative and as large as VAR itself, where the exact
          difference |e| / (sqrt(a) + sqrt(a - |e|)) reaches |e| / sqrt(a): 2 x the first-order term bounds both; plus three roundings:
                                                                           |dSTD| <= 2 |dVAR| / (2 STD) + 2^-22 STD
    dH:   cnt terms, each a few rounded products, summed in cnt additions; T = sum of the MAGNITUDES of everything added (|dMEAN| / d,
          |Q MEAN|, the selected |dMAX|, |dMIN|, |H Q|) -- Q MEAN and H Q cancel by design, the bound does not pretend they do not:
                                                                           |ddH| <= 2^-23 (cnt + 16) T"""
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
import _aggsoftmax_workers as SW  # noqa: E402
import _gradgrid_workers as GG  # noqa: E402

N, HIDDEN, EPS = AW.N, AW.HIDDEN, 1e-5
PNA_METHODS = ("aggpna", "aggpna_finish", "aggpna_backward", "pna_scale", "pna_scale_backward")
ENGINE_WIDTHS = (24, 32)
make_dataset, bits, sym_pattern, rows = AW.make_dataset, AW.bits, AW.sym_pattern, AW.rows


NROWS, NCOLS, CHUNK = 1100, 1200, 64
EMPTY = (5, 13, 400, NROWS - 1)


def host_csr(M):
    from conftest import pkg
    M = M.tocsr()
    M.sort_indices()
    return pkg("partition").HostCSR(M.shape[0], M.shape[1], torch.from_numpy(M.indptr.astype(np.int64)),
                                    torch.from_numpy(M.indices.astype(np.int32)), torch.ones(M.nnz))


def make_pattern(fmax):
    """tests/test_aggsoftmax_gpu.py's pattern: 1 100 x 1 200, rows of 0 (one between two cut rows), 1, 64, 65, 130 and 1 000 entries, two
    hub columns of 1 000 rows; its column-disjoint halves, the transpose, global ids, every family's operand and oracle, a gradient."""
    import scipy.sparse as sp
    rng = np.random.default_rng(42)
    lens = rng.integers(2, 40, NROWS)
    lens[list(EMPTY)] = 0
    lens[6], lens[10], lens[11], lens[12], lens[14], lens[15] = 1, 64, 65, 1000, 1000, 130
    hubs = rng.permutation(np.setdiff1d(np.arange(NROWS), [5, 6, 10, 11, 13, 400, NROWS - 1]))[:1000]
    rws, cls = [], []
    for i in range(NROWS):
        c = rng.choice(np.setdiff1d(np.arange(NCOLS), [3, 7]) if lens[i] < 1000 else NCOLS, lens[i], replace=False)
        rws.append(np.full(c.size, i)), cls.append(c)
    rws, cls = np.concatenate(rws + [hubs, hubs]), np.concatenate(cls + [np.full(1000, 3), np.full(1000, 7)])
    M = sp.coo_matrix((np.ones(rws.size), (rws, cls)), shape=(NROWS, NCOLS)).tocsr()
    M.sum_duplicates()
    M.sort_indices()
    got = np.diff(M.indptr)
    assert (got[list(EMPTY)] == 0).all() and got[6] == 1 and {64, 65}.issubset(set(got.tolist())) and got.max() >= 1000
    coo = M.tocoo()
    lo, hi = (sp.coo_matrix((coo.data[k], (coo.row[k], coo.col[k])), shape=M.shape).tocsr() for k in (coo.col < NCOLS // 2, coo.col >= NCOLS // 2))
    gid = rng.permutation(NCOLS) + 5000
    c = dict(M=M, MT=M.T.tocsr(), halves=(lo, hi), gid=gid, rowptr=M.indptr.astype(np.int64), col=M.indices.astype(np.int64),
             H=families(rng, NCOLS, fmax), dS=rng.random((NROWS, 4, fmax), dtype=np.float32) * 2 - 1)
    c["want"] = {fam: oracle_pna(c["rowptr"], c["col"], gid, H) for fam, H in c["H"].items()}
    return c


def families(rng, n, f):
    """uniform in [-1, 1]; relu: half exact zeros (ties); equal: every row of H equal; offset: 1000 + uniform / 100."""
    fam = SW.families(rng, n, f)
    return {"uniform": fam["uniform"], "relu": fam["relu"], "equal": fam["equal"],
            "offset": (1000 + fam["uniform"].astype(np.float64) * 1e-2).astype(np.float32)}


def oracle_pna(rowptr, col, gid, H):
    """dict of float64 [n, f] MEAN, MAX, MIN, STD, VAR, amax, spread; int AMAX, AMIN [n, f]; d [n] -- two passes per row."""
    rowptr, col, gid = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(gid, np.int64)
    n, f = rowptr.shape[0] - 1, H.shape[1]
    H64 = H.astype(np.float64)
    o = {k: np.zeros((n, f)) for k in ("MEAN", "MAX", "MIN", "STD", "VAR", "amax", "spread")}
    o["AMAX"], o["AMIN"] = np.full((n, f), -1, np.int64), np.full((n, f), -1, np.int64)
    for i in range(n):
        c = col[rowptr[i]:rowptr[i + 1]]
        if c.size:
            c = c[np.argsort(gid[c], kind="stable")]                    # ascending global id: argmax / argmin take the first of equals
            X = H64[c]
            m = X.mean(axis=0)
            o["MEAN"][i], o["VAR"][i] = m, ((X - m) ** 2).mean(axis=0)
            o["MAX"][i], o["MIN"][i] = X.max(axis=0), X.min(axis=0)
            o["AMAX"][i], o["AMIN"][i] = gid[c][X.argmax(axis=0)], gid[c][X.argmin(axis=0)]
            o["STD"][i] = np.sqrt(o["VAR"][i] + EPS)
            o["amax"][i], o["spread"][i] = np.abs(X).max(axis=0), np.abs(X - m).max(axis=0)
    o["d"] = np.diff(rowptr)
    return o


def forward_bounds(o):
    d = o["d"][:, None].astype(np.float64)
    bm = 2.0 ** -23 * ((2 * d + 16) * o["spread"] + (10 + d / 32) * o["amax"])
    bv = 2.0 ** -23 * ((d + 32) * 8 * o["spread"] ** 2 + 8 * o["spread"] * o["amax"])
    bs = np.where(d > 0, bv / np.maximum(o["STD"], 1e-300) + 2.0 ** -22 * o["STD"], 0.0)
    return np.where(d > 0, bm, 0.0), bs


def assert_forward(S, AMAX, AMIN, o, at, order_free=True):
    """S = [MEAN | MAX | MIN | STD] (fp32) against the oracle: MAX, MIN, AMAX, AMIN exactly (the winner's own fp32 value), MEAN and STD
    within their bounds; rows without entries are all 0 / -1.  Returns the largest error / bound."""
    f = AMAX.shape[1]
    assert S.dtype == np.float32 and S.shape[1] == 4 * f and not np.isnan(S).any(), at
    mean, mx, mn, sd = (S[:, k * f:(k + 1) * f] for k in range(4))
    empty = o["d"] == 0
    assert (S[empty] == 0).all() and (AMAX[empty] == -1).all() and (AMIN[empty] == -1).all(), (at, "empty rows")
    if order_free:
        assert np.array_equal(AMAX, o["AMAX"]) and np.array_equal(AMIN, o["AMIN"]), (at, "args")
        assert np.array_equal(mx.astype(np.float64), o["MAX"]) and np.array_equal(mn.astype(np.float64), o["MIN"]), (at, "extremes")
    bm, bs = forward_bounds(o)
    em, es = np.abs(mean - o["MEAN"]), np.abs(sd - o["STD"])
    print(at, "MEAN err/bound %.3g  STD err/bound %.3g" % (float((em / np.maximum(bm, 1e-300)).max()), float((es / np.maximum(bs, 1e-300)).max())))
    assert (em <= bm).all(), (at, "MEAN", float((em / np.maximum(bm, 1e-300)).max()))
    assert (es <= bs).all(), (at, "STD", float((es / np.maximum(bs, 1e-300)).max()))
    return max(float((em / np.maximum(bm, 1e-300)).max()), float((es / np.maximum(bs, 1e-300)).max()))


def cut(o, f):
    return {k: (v if k == "d" else v[:, :f]) for k, v in o.items()}


def fp32_state(o):
    """(S, AMAX, AMIN) as the forward hands them to the backward: the oracle's values rounded to fp32 / int32."""
    return (np.concatenate([o["MEAN"], o["MAX"], o["MIN"], o["STD"]], 1).astype(np.float32), o["AMAX"].astype(np.int32),
            o["AMIN"].astype(np.int32))


def assert_backward(D, rowptr, col, gid, X, dS, S, AMAX, AMIN, at):
    """D [ncols, f] against the definition in float64 over the FORWARD pattern, from the fp32 S / dS both sides get, within the bound."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n, f = rowptr.shape[0] - 1, X.shape[1]
    d = np.diff(rowptr).astype(np.float64)[:, None]
    S64, g = S.astype(np.float64), dS.astype(np.float64)
    has = d > 0
    Q = np.where(has, g[:, 3 * f:] / np.where(has, d * S64[:, 3 * f:], 1.0), 0.0)
    Pm = np.where(has, g[:, :f] / np.maximum(d, 1), 0.0)
    ri = np.repeat(np.arange(n), np.diff(rowptr))
    gj = np.asarray(gid, np.int64)[col][:, None]
    x = X.astype(np.float64)[col]
    smax, smin = np.where(AMAX[ri] == gj, g[ri, f:2 * f], 0.0), np.where(AMIN[ri] == gj, g[ri, 2 * f:3 * f], 0.0)
    want, T = np.zeros((X.shape[0], f)), np.zeros((X.shape[0], f))
    np.add.at(want, col, Pm[ri] - Q[ri] * S64[ri, :f] + smax + smin + x * Q[ri])
    np.add.at(T, col, np.abs(Pm[ri]) + np.abs(Q[ri] * S64[ri, :f]) + np.abs(smax) + np.abs(smin) + np.abs(x * Q[ri]))
    cnt = np.bincount(col, minlength=X.shape[0])[:, None]
    bound = 2.0 ** -23 * (cnt + 16) * T
    assert D.dtype == np.float32 and not np.isnan(D).any(), at
    err = np.abs(D - want)
    print(at, "dH err/bound %.3g" % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (at, "dH", float((err / np.maximum(bound, 1e-300)).max()))
    return cnt


def scalers(deg, delta):
    lg = np.log(np.maximum(deg, 1).astype(np.float64) + 1.0)
    return (lg / delta).astype(np.float32), (delta / lg).astype(np.float32)


# ---- providers and workers --------------------------------------------------------------------------------------------------------

def _provider(M, gpu):
    """gpu false: the checker-backed provider (no PNA kernels: the composed route); true: the real one; "composed": the real one with
    the PNA kernels hidden."""
    from conftest import pkg
    if gpu == "composed":
        K = pkg("kernels")

        class NoPna(K.HipKernels):
            def __getattribute__(self, name):
                if name in PNA_METHODS:
                    raise AttributeError(name)
                return super().__getattribute__(name)

        M._kernel_provider = NoPna(torch.device("cuda:0"))
        M._exchanger = None
    else:
        AW._provider(M, gpu)


def _engine(M, gpu, r, size, path_A, path_partvec):
    import io
    from contextlib import redirect_stdout
    M.myrank, M.world_size = r, size
    M.device = torch.device("cuda:0") if gpu else torch.device("cpu")
    if gpu:
        torch.cuda.set_device(M.device)
    A = M._ingest.mmread(path_A)
    pv = M._partition.read_partvec(path_partvec)
    with redirect_stdout(io.StringIO()):
        M.compute_communication_maps(A, pv, r, size, "sym")
        return M.get_partitiont_of_adjacency_matrix(A, pv, r, "sym")


def engine_worker(rank, P, port, paths, gpu, q, partvec="pv"):
    """forward_pna / backward_pna of rank `rank` of `P` over gloo on seeded global operands, the degrees, delta and the scalers."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    from conftest import pkg
    M = pkg("PGCN")
    _provider(M, gpu)
    got = {"rank": rank, "cases": []}

    def fn(r, size, nlayers, nfeatures, path_A, path_partvec, backend, **_):
        eng = _engine(M, gpu, r, size, path_A, path_partvec)
        own = eng.part.owned.cpu().numpy()
        dg = eng.pna_degrees()
        got.update(own=own, hip=type(eng.k).__name__, composed=eng._max.composed, delta=dg.delta, deg=dg.deg.cpu().numpy(),
                   a=dg.a.cpu().numpy(), b=dg.b.cpu().numpy())
        for f in ENGINE_WIDTHS:
            for kind in ("uniform", "relu"):
                Hg, _ = SW.seeded_operands(f, kind)
                Gg = np.random.default_rng([17, f]).random((N, 4 * f), dtype=np.float32) * 2 - 1
                H, G = torch.from_numpy(Hg[own]).to(M.device), torch.from_numpy(Gg[own]).to(M.device)
                S, AMAX, AMIN, halo = eng.forward_pna(H)
                dH = eng.backward_pna(G, H, halo, S, AMAX, AMIN)
                got["cases"].append(dict(f=f, kind=kind, S=S.cpu().numpy(), AMAX=AMAX.cpu().numpy(), AMIN=AMIN.cpu().numpy(),
                                         dH=dH.cpu().numpy(), halo=None if halo is None else tuple(halo.shape)))

    M.init_process(rank, P, fn, 3, HIDDEN, paths["A"], paths["%s%d" % (partvec, P)], "gloo", "sym")
    q.put(got)


def check_engine(res, data, P):
    """S / AMAX / AMIN / dH gathered over the ranks against the oracle on the GLOBAL pattern; delta, the degrees and the scalers against
    the formula.  Returns (delta, a, b) in global row order: the same bits under any P and part vector."""
    rowptr, col = sym_pattern(data["A"])
    gid = np.arange(N)
    deg = np.diff(rowptr)
    hist = np.bincount(deg)
    delta = float(np.cumsum(hist * np.log(np.arange(hist.size) + 1.0))[-1] / N)
    assert all(r["delta"] == delta for r in res), ([r["delta"] for r in res], delta)
    assert np.array_equal(rows(res, lambda r: r["deg"][:, None])[:, 0], deg)
    a, b = scalers(deg, delta)
    ga, gb = rows(res, lambda r: r["a"][:, None])[:, 0], rows(res, lambda r: r["b"][:, None])[:, 0]
    assert np.array_equal(bits(ga), bits(a)) and np.array_equal(bits(gb), bits(b))
    for k, c0 in enumerate(res[0]["cases"]):
        f, kind = c0["f"], c0["kind"]
        assert all((r["cases"][k]["halo"] is None) == (P == 1) for r in res)
        Hg, _ = SW.seeded_operands(f, kind)
        Gg = np.random.default_rng([17, f]).random((N, 4 * f), dtype=np.float32) * 2 - 1
        S, AMAX, AMIN, dH = (rows(res, lambda r, key=key: r["cases"][k][key]) for key in ("S", "AMAX", "AMIN", "dH"))
        assert_forward(S, AMAX, AMIN, oracle_pna(rowptr, col, gid, Hg), (P, f, kind))
        assert_backward(dH, rowptr, col, gid, Hg, Gg, S, AMAX, AMIN, (P, f, kind))
    return delta, ga, gb


# ---- model level ------------------------------------------------------------------------------------------------------------------

def pna_aggregate(h, row, col, n, deg):
    """[MEAN | MAX | MIN | STD] with framework operations on the GLOBAL pattern (every row holds itself), differentiable."""
    X = h[col]
    idx = row.unsqueeze(1).expand(-1, h.shape[1])
    d = deg.to(h.dtype).unsqueeze(1)
    mean = torch.zeros((n, h.shape[1]), dtype=h.dtype).index_add(0, row, X) / d
    var = torch.zeros((n, h.shape[1]), dtype=h.dtype).index_add(0, row, (X - mean[row]) ** 2) / d
    mx = torch.full_like(mean, float("-inf")).scatter_reduce(0, idx, X, "amax", include_self=True)
    mn = torch.full_like(mean, float("inf")).scatter_reduce(0, idx, X, "amin", include_self=True)
    return torch.cat([mean, mx, mn, torch.sqrt(var + EPS)], 1)


def model_pna(data, params, opts, nlayers, dtype=torch.float64):
    """(loss, logits, {name: grad}) of the model ``run(aggr="pna")`` builds, in PyG's formulation: the 12 fin wide operand
    [S | a S | b S] times the layer's weight.  No dropout; ``opts``: root, norm ("none" | "node"), bias, residual."""
    n = data["A"].shape[0]
    rowptr, col = sym_pattern(data["A"])
    deg = torch.from_numpy(np.diff(rowptr))
    row, col = torch.from_numpy(np.repeat(np.arange(n), np.diff(rowptr))), torch.from_numpy(col)
    lg = torch.log(deg.clamp(min=1).to(torch.float64) + 1.0)
    delta = lg.mean()                                                   # (every vertex of the sym pattern holds itself: d >= 1)
    a, b = (lg / delta).to(dtype).unsqueeze(1), (delta / lg).to(dtype).unsqueeze(1)
    h = torch.from_numpy(data["X"]).to(dtype)
    p = {k: torch.from_numpy(v).to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    for l in range(nlayers):
        S = pna_aggregate(h, row, col, n, deg)
        z = torch.cat([S, a * S, b * S], 1) @ p["%d.linear.weight" % l].t()
        if opts["root"]:
            z = z + h @ p["%d.root.weight" % l].t()
        if opts.get("bias") and (opts["norm"] == "none" or l == nlayers - 1):
            z = z + p["%d.bias" % l]
        if l == nlayers - 1:
            logits = z
            break
        if opts["norm"] == "node":
            z = F.layer_norm(z, (z.shape[1],), p["%d.ln_weight" % l], p["%d.ln_bias" % l], 1e-5)
        h = h + torch.relu(z) if opts.get("residual") and h.shape[1] == z.shape[1] else torch.relu(z)
    train = torch.from_numpy(data["split"] == 1)
    loss = F.cross_entropy(logits[train], torch.from_numpy(data["labels"])[train])
    names = list(p)
    grads = dict(zip(names, (g.detach() for g in torch.autograd.grad(loss, [p[k] for k in names]))))
    return loss.detach(), logits.detach(), grads


# the last one is the command line's --aggr pna --root-weight --bias --norm node --residual at three layers; it also goes through
# --save, --load and --predict (``round_trip``)
MODEL_CONFIGS = (dict(root=False, norm="none"), dict(root=True, norm="none", bias=True, residual=True, nlayers=3),
                 dict(root=True, norm="node", bias=True, residual=True, nlayers=3, round_trip=True))


def model_worker(rank, P, port, paths, gpu, q, configs=MODEL_CONFIGS, nlayers=2, scratch=None):
    """run(epochs=1, lr=0.0, optimizer="torch", normalize="sym", aggr="pna") per configuration: the parameters the model starts from,
    the gradients before the optimiser step, this rank's training logits."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M = pkg("PGCN")
    _provider(M, gpu)
    cur = {}
    adam_step = torch.optim.Adam.step

    def step(self, *a, **kw):
        cur["grads"] = {name: prm.grad.detach().cpu().numpy().copy() for name, prm in cur["model"].named_parameters()}
        return adam_step(self, *a, **kw)

    init = M.initiliaze_parameters

    def initialise(model):
        init(model)
        cur["model"] = model
        cur["params"] = {name: prm.detach().cpu().numpy().copy() for name, prm in model.named_parameters()}
        model.register_forward_hook(lambda m, a, out: cur.__setitem__("logits", out.detach().cpu().numpy()) if m.training else None)

    torch.optim.Adam.step = step
    M.initiliaze_parameters = initialise
    results = []

    def fn(r, size, nl, nfeatures, path_A, path_partvec, backend, **_):
        for c in configs:
            torch.manual_seed(5)
            kw = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=HIDDEN, epochs=1, lr=0.0,
                      optimizer="torch", aggr="pna", **({"root_weight": True} if c["root"] else {}),
                      **({"norm": c["norm"]} if c["norm"] != "none" else {}), **{k: True for k in ("bias", "residual") if c.get(k)})
            L = c.get("nlayers", nlayers)
            ck = os.path.join(scratch, "pna.%d.pt" % size) if c.get("round_trip") and scratch else None
            out = io.StringIO()
            with redirect_stdout(out):
                model = M.run(r, size, L, HIDDEN, path_A, path_partvec, "gloo", normalize="sym", **kw, **({"save": ck} if ck else {}))
            eng = M._engine_current
            res = dict(params=cur["params"], grads=cur["grads"], logits=cur["logits"], own=eng.part.owned.cpu().numpy(),
                       composed=eng._max.composed, hip=type(eng.k).__name__,
                       losses=[ln for ln in out.getvalue().splitlines() if "loss" in ln.lower()])
            if ck:          # --load --epochs 0 --predict --proba: the model rebuilt from the record, its 12 fin wide weights loaded
                with redirect_stdout(io.StringIO()):
                    again = M.run(r, size, L, HIDDEN, path_A, path_partvec, "gloo", normalize="sym",
                                  **dict(kw, epochs=0, load=ck, predict=ck + ".out", proba=True))
                res["reloaded"] = all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(model.state_dict().values(), again.state_dict().values()))
                res["eval"] = GG.eval_logits(M, again, paths)
                res["prob"] = np.load(ck + ".out.prob.npy") if r == 0 else None
            results.append(res)

    M.init_process(rank, P, fn, 3, HIDDEN, paths["A"], paths["pv%d" % P], "gloo", "sym")
    q.put({"rank": rank, "results": results})


def check_models(data, res, configs=MODEL_CONFIGS, nlayers=2):
    """Logits and every reduced parameter gradient against the float64 model through conftest.held_to_fixture, the twin being the same
    model in fp32."""
    from conftest import held_to_fixture
    held = 0
    for j, c in enumerate(configs):
        ranks = [r["results"][j] for r in res]
        params = ranks[0]["params"]
        assert all(all(np.array_equal(r["params"][k], params[k]) for k in params) for r in ranks), "the ranks start from different weights"
        assert params["0.linear.weight"].shape[1] == 12 * data["X"].shape[1]
        L = c.get("nlayers", nlayers)
        _, z64, g64 = model_pna(data, params, c, L, torch.float64)
        _, z32, g32 = model_pna(data, params, c, L, torch.float32)
        if "eval" in ranks[0]:         # the reloaded model: the saved state bit for bit, its logits and the written probabilities
            assert all(r["reloaded"] for r in ranks), "the loaded state differs from the saved one"
            z = rows(ranks, lambda r: r["eval"])
            held_to_fixture("aggpna/reloaded/P%d" % len(res), "logits", z, z32.numpy(), z64.numpy())
            want = torch.softmax(torch.from_numpy(z), 1).numpy()
            assert ranks[0]["prob"].shape == want.shape and np.abs(ranks[0]["prob"] - want).max() <= 1e-6
        at = "aggpna/%s/P%d" % (c, len(res))
        held_to_fixture(at, "logits", rows(ranks, lambda r: r["logits"]), z32.numpy(), z64.numpy())
        for i, r in enumerate(ranks):
            for name in g64:
                held_to_fixture(at + "/rank%d" % i, "grad " + name, r["grads"][name], g32[name].numpy(), g64[name].numpy())
                held += 1
    return held


def degenerate_group(dataset, dirname, name, gpu):
    """The engine and the model under tests/_degenerate_workers.py's part vector ``name``: the engine's answers against the oracle (a
    rank without rows answers with 0-row tensors), the first and the last model configuration against the double model."""
    import _degenerate_workers as DG
    paths, data = dataset
    P, who = DG.VECTORS[name]
    pv = DG.with_vector(paths, name, data, dirname, "pna")
    res = AW._spawn(engine_worker, P, pv, gpu)
    DG.check_vector(name, [r["own"] for r in res], data)
    assert all(r["composed"] == (not gpu) for r in res)
    if name in ("E2", "E3"):
        assert all(c["S"].shape[0] == 0 and c["dH"].shape[0] == 0 for c in res[who]["cases"])
    check_engine(res, data, P)
    configs = (MODEL_CONFIGS[0], {k: v for k, v in MODEL_CONFIGS[-1].items() if k != "round_trip"})
    assert check_models(data, AW._spawn(model_worker, P, pv, gpu, configs=configs), configs) > 0
