"""The definition of the max aggregation in numpy, the double model under a recorded selection and the worker processes of
tests/test_aggmax.py and tests/test_aggmax_gpu.py (spawn start method), in the pattern of tests/_gradgrid_workers.py.

Definition (csrc/pgcn_aggmax.hip): OUT[i, c] = max over the stored columns j of row i of H[j, c]; ARG[i, c] = the smallest GLOBAL id
among the j that attain it (fp32 ==: -0.0 ties with +0.0; OUT takes that j's bits); a row without entries gives (0.0, -1);
dH[j, c] = sum of G[i, c] over the i with ARG[i, c] == j."""
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _batchnorm_workers as BW  # noqa: E402
import _gradgrid_workers as GG  # noqa: E402
import _nodeclass_workers as NW  # noqa: E402

N, NNZ, COMMUNITY = GG.N, GG.NNZ, GG.COMMUNITY
FIN, CLASSES, HIDDEN, NLAYERS, EPOCHS = GG.FIN, GG.CLASSES, GG.HIDDEN, 3, 2
DROPOUT, DROPOUT_SEED, WEIGHT_SEED = GG.DROPOUT, GG.DROPOUT_SEED, 5
ENGINE_WIDTHS = (24, 32)
MAX_METHODS = ("prepare_max", "aggmax", "aggmax_backward")


# ---- the definition ---------------------------------------------------------------------------------------------------------------

def oracle_max(rowptr, col, gid, H):
    """(OUT fp32, ARG int32) by the definition: per row the candidates sorted by global id, np.argmax along them (the FIRST maximum;
    -0.0 == 0.0), an empty row (0, -1).  ``gid``: global id of every column of the structure."""
    rowptr, col, gid = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(gid, np.int64)
    n, f = rowptr.shape[0] - 1, H.shape[1]
    OUT, ARG = np.zeros((n, f), np.float32), np.full((n, f), -1, np.int32)
    for i in range(n):
        c = col[rowptr[i]:rowptr[i + 1]]
        if c.size:
            c = c[np.argsort(gid[c], kind="stable")]
            X = H[c]
            k = np.argmax(X, axis=0)
            OUT[i] = X[k, np.arange(f)]
            ARG[i] = gid[c][k]
    return OUT, ARG


def rule_max(rowptr, col, gid, H, order=None):
    """The same by the update rule, candidates taken in storage order (or permuted by ``order`` inside every row): a candidate (v, g)
    replaces (cur, a) when a < 0 or v > cur or (v == cur and g < a)."""
    n, f = rowptr.shape[0] - 1, H.shape[1]
    OUT, ARG = np.zeros((n, f), np.float32), np.full((n, f), -1, np.int32)
    for i in range(n):
        c = np.asarray(col[rowptr[i]:rowptr[i + 1]], np.int64)
        if order is not None:
            c = c[order(c.size)]
        for j in c:
            v, g = H[j], np.int32(gid[j])
            take = (ARG[i] < 0) | (v > OUT[i]) | ((v == OUT[i]) & (g < ARG[i]))
            OUT[i] = np.where(take, v, OUT[i])
            ARG[i] = np.where(take, g, ARG[i])
    return OUT, ARG


def oracle_max_backward(ARG, G, n_out):
    """(D float64 [n_out, f], sum of |terms| per element, number of terms per element): dH[j, c] = sum of G[i, c] over ARG[i, c] == j,
    ARG holding ids in 0 .. n_out - 1 or -1."""
    f = G.shape[1]
    D, S, K = np.zeros((n_out, f)), np.zeros((n_out, f)), np.zeros((n_out, f), np.int64)
    i, c = np.nonzero(ARG >= 0)
    j = ARG[i, c].astype(np.int64)
    np.add.at(D, (j, c), G[i, c].astype(np.float64))
    np.add.at(S, (j, c), np.abs(G[i, c].astype(np.float64)))
    np.add.at(K, (j, c), 1)
    return D, S, K


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def sym_pattern(A):
    """CSR (rowptr, col) of the pattern of A + I: what normalize="sym" aggregates over."""
    n = A.shape[0]
    B = (sp.csr_matrix(A) + sp.identity(n, format="csr")).tocsr()
    B.sort_indices()
    return B.indptr.astype(np.int64), B.indices.astype(np.int64)


def tie_features(n, f, seed):
    """Integers in -2 .. 2 with both signs of zero: exact ties everywhere (what ReLU outputs look like), decided by the global id."""
    rng = np.random.default_rng(seed)
    H = rng.integers(-2, 3, (n, f)).astype(np.float32)
    H[(H == 0) & (rng.random((n, f)) < 0.5)] = np.float32(-0.0)
    return H


# ---- data -------------------------------------------------------------------------------------------------------------------------

def make_dataset(dirname):
    """The planted problem of the gradient grid (n = 1100) with contiguous part vectors ``cpv<P>`` beside the random ``pv<P>``."""
    paths, data = NW.make_dataset(dirname, n=N, nnz=NNZ, community=COMMUNITY, classes=CLASSES, fin=FIN)
    for P in (1, 2, 3):
        paths["cpv%d" % P] = os.path.join(dirname, "sbm.%d.cp" % P)
        with open(paths["cpv%d" % P], "w") as fh:
            fh.write(" ".join(map(str, ((np.arange(N) * P) // N).tolist())) + "\n")
    return paths, data


def _provider(M, gpu):
    """gpu false: the checker-backed provider (no max kernels: the composed route); true: the real one; "composed": the real one with
    the max kernels hidden."""
    from conftest import pkg
    if gpu == "composed":
        K = pkg("kernels")

        class NoMax(K.HipKernels):
            def __getattribute__(self, name):
                if name in MAX_METHODS:
                    raise AttributeError(name)
                return super().__getattribute__(name)

        M._kernel_provider = NoMax(torch.device("cuda:0"))
    elif gpu:
        M._kernel_provider = None
    else:
        from oracle_kernels import OracleKernels
        M._kernel_provider = OracleKernels()
    M._exchanger = None


# ---- engine level -----------------------------------------------------------------------------------------------------------------

def engine_worker(rank, P, port, paths, gpu, q, partvec="pv"):
    """forward_max / backward_max of rank `rank` of `P` over gloo on seeded global operands, per width of ENGINE_WIDTHS: tie-rich
    integers and uniform floats forward, integer G backward; the exchange counters next to those of one sum aggregation."""
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
            for kind in ("ties", "uniform"):
                Hg, Gg = seeded_operands(f, kind)
                before = dict(eng.stats)
                OUT, ARG = eng.forward_max(torch.from_numpy(Hg[own]).to(M.device))
                mid = dict(eng.stats)
                dH = eng.backward_max(torch.from_numpy(Gg[own]).to(M.device), ARG)
                after = dict(eng.stats)
                eng.forward(torch.from_numpy(Hg[own]).to(M.device))
                summed = dict(eng.stats)
                got["cases"].append(dict(f=f, kind=kind, OUT=OUT.cpu().numpy(), ARG=ARG.cpu().numpy(), dH=dH.cpu().numpy(),
                                         fwd={k: mid[k] - before[k] for k in mid}, bwd={k: after[k] - mid[k] for k in mid},
                                         sum_fwd={k: summed[k] - after[k] for k in mid}))
        m = eng._max
        got.update(composed=m.composed, halo_nnz=[int(a.nnz) for a in m.halo], halo_T_nnz=[int(a.nnz) for a in m.halo_T])

    M.init_process(rank, P, fn, NLAYERS, HIDDEN, paths["A"], paths["%s%d" % (partvec, P)], "gloo", "sym")
    q.put(got)


def _spawn(worker, P, paths, gpu, **kw):
    saved = BW.run_worker
    BW.run_worker = worker
    try:
        return BW.spawn_run(P, paths, gpu, **kw)
    finally:
        BW.run_worker = saved


def spawn_engine(P, paths, gpu, **kw):
    return _spawn(engine_worker, P, paths, gpu, **kw)


def seeded_operands(f, kind):
    """The global operands ``engine_worker`` draws for one case."""
    rng = np.random.default_rng([7, f, kind == "ties"])
    Hg = tie_features(N, f, 11 + f) if kind == "ties" else (rng.random((N, f), dtype=np.float32) * 2 - 1)
    Gg = rng.integers(-8, 9, (N, f)).astype(np.float32)
    return Hg, Gg


def rows(res, pick):
    out = None
    for r in res:
        v = pick(r)
        out = np.zeros((N,) + v.shape[1:], v.dtype) if out is None else out
        out[r["own"]] = v
    return out


def check_engine(res, data, P):
    """Every assertion of the engine level on the answers of one worker group: OUT / ARG bit for bit the oracle's on the global graph,
    the backward exact on integer gradients, halo structures that hold entries, the exchange volume of one sum aggregation."""
    rowptr, col = sym_pattern(data["A"])
    gid = np.arange(N)
    assert all(r["lazy_before"] for r in res)
    if P > 1:
        assert all(sum(r["halo_nnz"]) > 0 and sum(r["halo_T_nnz"]) > 0 for r in res), "the halo structures hold no entries"
    for k in range(len(res[0]["cases"])):
        c0 = res[0]["cases"][k]
        Hg, Gg = seeded_operands(c0["f"], c0["kind"])
        want_out, want_arg = oracle_max(rowptr, col, gid, Hg)
        OUT, ARG, dH = (rows(res, lambda r, key=key: r["cases"][k][key]) for key in ("OUT", "ARG", "dH"))
        assert ARG.dtype == np.int32 and np.array_equal(ARG, want_arg), (P, c0["f"], c0["kind"], int((ARG != want_arg).sum()))
        assert np.array_equal(bits(OUT), bits(want_out)), (P, c0["f"], c0["kind"])
        D64, _, _ = oracle_max_backward(want_arg, Gg, N)
        assert np.array_equal(dH.astype(np.float64), D64), (P, c0["f"], c0["kind"])          # integer G: every partial sum is exact
        for r in res:
            c = r["cases"][k]
            assert c["fwd"] == c["sum_fwd"], (c["fwd"], c["sum_fwd"])                         # the exchange volume of one sum aggregation
            assert c["bwd"]["send_volume"] == c["fwd"]["recv_volume"] and c["bwd"]["recv_volume"] == c["fwd"]["send_volume"]


# ---- model level ------------------------------------------------------------------------------------------------------------------

def config(norm="none", root=False, bias=False, dropout=0.0):
    return GG.config(norm, root, bias, False, dropout, HIDDEN)


def model_configs():
    """{norm none, node} x {root_weight + bias on, off} x {dropout 0, 0.5}, plus batch norm once."""
    out = [config(norm, rb, rb, d) for norm in ("none", "node") for rb in (0, 1) for d in (0.0, DROPOUT)]
    return out + [config("batch", 1, 0, DROPOUT)]


def rank_subset():
    return [config("none", 0, 0, 0.0), config("none", 1, 1, DROPOUT), config("node", 1, 1, 0.0), config("node", 0, 0, DROPOUT)]


def widths_of(c):
    return [FIN] + [c["hidden"]] * (NLAYERS - 1) + [CLASSES]


def model_sel(data, widths, params, opts, step, args, dtype=torch.float64):
    """(loss, logits, {name: grad}) of GG.model64's model with the aggregation of layer l replaced by the gather H[args[l][i, c], c]
    (0 where -1): the exact linearisation of the max aggregation at the recorded selection ``args`` (global ids, [n, width of the
    layer's input]).  Training mode; batch statistics of the step itself."""
    from conftest import pkg
    D = pkg("dropout")
    n = data["A"].shape[0]
    h = torch.from_numpy(data["X"]).to(dtype)
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    L = len(widths) - 1
    thr, scale = D.threshold(opts["dropout"])
    for l in range(L):
        a = torch.from_numpy(args[l].astype(np.int64))
        agg = torch.where(a >= 0, torch.gather(h, 0, a.clamp(min=0)), torch.zeros((), dtype=dtype))
        z = agg @ p["%d.linear.weight" % l].t()
        if opts["root"]:
            z = z + h @ p["%d.root.weight" % l].t()
        if l == L - 1:
            logits = z + p["%d.bias" % l] if opts["bias"] else z
            break
        f = z.shape[1]
        if opts["norm"] == "batch":
            t = F.batch_norm(z, None, None, p["%d.bn_weight" % l], p["%d.bn_bias" % l], True, GG.MOMENTUM, GG.EPS)
        elif opts["norm"] == "node":
            t = F.layer_norm(z, (f,), p["%d.ln_weight" % l], p["%d.ln_bias" % l], GG.EPS)
        else:
            t = z + p["%d.bias" % l] if opts["bias"] else z
        h = torch.relu(t)
        if opts["dropout"] > 0.0:
            keep = D.keep_mask(DROPOUT_SEED, step, l, np.arange(n), f, thr)
            h = torch.where(keep, h * scale, torch.zeros((), dtype=dtype))
    train = torch.from_numpy(data["split"] == 1)
    loss = F.cross_entropy(logits[train], torch.from_numpy(data["labels"])[train])
    names = list(p)
    grads = dict(zip(names, (g.detach() for g in torch.autograd.grad(loss, [p[k] for k in names]))))
    return loss.detach(), logits.detach(), grads


def model_worker(rank, P, port, paths, gpu, q, jobs=()):
    """GG.run_worker's protocol for run(epochs=2, lr=0.0, optimizer="torch", normalize="sym", nlayers=3, aggr="max"): per job the
    parameters written into the model, the gradients before each optimiser step, this rank's loss and logits of each step -- and per
    call of forward_max made in training mode its input, OUT, ARG."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M = pkg("PGCN")
    E = pkg("engine")
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

    forward_max = E.AggregationEngine.forward_max

    def recorded(self, H):
        OUT, ARG = forward_max(self, H)
        if cur["model"].training:
            cur["calls"].append((H.detach().cpu().numpy().copy(), OUT.cpu().numpy().copy(), ARG.cpu().numpy().copy()))
        return OUT, ARG

    M.initiliaze_parameters = initialise
    torch.optim.Adam.step = step
    M.masked_loss = with_loss
    E.AggregationEngine.forward_max = recorded
    results = []

    def fn(r, size, nlayers, nfeatures, path_A, path_partvec, backend, **_):
        for job in jobs:
            c = job["config"]
            cur.update(job=job, grads=[], logits=[], loss=[], calls=[])
            torch.manual_seed(job["seed"])
            kw = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=c["hidden"], epochs=EPOCHS, lr=0.0,
                      optimizer="torch", aggr="max")
            if c["norm"] != "none":
                kw["norm"] = c["norm"]
            for name, opt in (("root", "root_weight"), ("bias", "bias")):
                if c[name]:
                    kw[opt] = True
            if c["dropout"] > 0.0:
                kw.update(dropout=c["dropout"], dropout_seed=DROPOUT_SEED)
            with redirect_stdout(io.StringIO()):
                M.run(r, size, NLAYERS, c["hidden"], path_A, path_partvec, "gloo", normalize="sym", **kw)
            eng = M._engine_current
            results.append(dict(tag=GG.tag(c), names=cur["names"], grads=cur["grads"], logits=cur["logits"], loss=cur["loss"], calls=cur["calls"],
                                own=eng.part.owned.cpu().numpy(), composed=eng._max.composed, hip=type(eng.k).__name__))

    M.init_process(rank, P, fn, NLAYERS, HIDDEN, paths["A"], paths["pv%d" % P], "gloo", "sym")
    q.put({"rank": rank, "results": results})


def spawn_model(P, paths, gpu, jobs):
    return [r["results"] for r in _spawn(model_worker, P, paths, gpu, jobs=jobs)]


def make_jobs(configs, seed=WEIGHT_SEED):
    jobs = []
    for c in configs:
        params = GG.initial_params(widths_of(c), c, seed)
        jobs.append({"config": c, "seed": seed, "params": {k: v.numpy() for k, v in params.items()}, "torch_params": params})
    return jobs


def check_models(data, configs, jobs, res, case):
    """Per configuration: (1) every recorded selection is the oracle's on the run's OWN fp32 input, bit for bit, rows gathered over the
    ranks; (2) logits, loss and every reduced parameter gradient agree with the double model under that selection through
    conftest.held_to_fixture (model / fp32 twin / double: max(1e-5, 2 err_twin)); step 1's logits are step 0's without dropout."""
    from conftest import held_to_fixture
    P = len(res)
    rowptr, col = sym_pattern(data["A"])
    gid = np.arange(N)
    held = 0
    for j, c in enumerate(configs):
        ranks = [r[j] for r in res]
        widths = widths_of(c)
        where = "aggmax%s/%s/P%d" % (case, GG.tag(c), P)
        for r in ranks:
            assert r["tag"] == GG.tag(c) and sorted(r["names"]) == sorted(GG.parameter_names(widths, c)), where
            assert len(r["calls"]) == NLAYERS * EPOCHS and len(r["grads"]) == len(r["logits"]) == len(r["loss"]) == EPOCHS, where
        logits = [rows(ranks, lambda r, s=s: r["logits"][s]) for s in range(EPOCHS)]
        if c["dropout"] > 0.0:
            assert not np.array_equal(logits[0], logits[1]), where
        else:
            assert bits(logits[0]).tobytes() == bits(logits[1]).tobytes(), where + ": lr = 0 and no dropout, yet the steps' logits differ"
        for s in range(EPOCHS):
            args = []
            for l in range(NLAYERS):
                k = s * NLAYERS + l
                Hg, OUT, ARG = (rows(ranks, lambda r, i=i: r["calls"][k][i]) for i in range(3))
                want_out, want_arg = oracle_max(rowptr, col, gid, Hg)
                assert np.array_equal(ARG, want_arg), (where, s, l, "ARG", int((ARG != want_arg).sum()))
                assert np.array_equal(bits(OUT), bits(want_out)), (where, s, l, "OUT")
                args.append(ARG)
            opts = dict(c, task="single")
            l64, z64, g64 = model_sel(data, widths, jobs[j]["torch_params"], opts, s, args, torch.float64)
            l32, z32, g32 = model_sel(data, widths, jobs[j]["torch_params"], opts, s, args, torch.float32)
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
