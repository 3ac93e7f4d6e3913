"""The definition of the personalised-PageRank propagation in numpy and in float64, the whole model with it in torch double, and the
worker processes of tests/test_propagate.py and tests/test_propagate_gpu.py (spawn start method), in the pattern of
tests/_aggmax_workers.py and tests/_gradgrid_workers.py.

Definition (csrc/pgcn_propagate.hip, engine.AggregationEngine.propagate): a = float32(alpha), b = 1.0f - a;
Z^0 = H, Z^{k+1} = fl(fl(b S) + fl(a H)) with S = A Z^k, output Z^K.  The adjoint: G^K = dOut, G^{k-1} = b A^T G^k,
dH = a sum_{k=1..K} G^k + G^0, accumulated as D <- fl(D + fl(a G^k)) and closed by fl(D + fl(b T)) at the last step.

Bound.  TOL is the 1e-5 of tests/test_hip_gpu.py, the relative error (conftest.rel_err) allowed to ONE aggregation.  K steps are held to
(K + 1) TOL against the float64 recursion: every step adds one aggregation's error and two roundings, and the map (1 - alpha) A does
not expand an error when ||A||_2 <= 1 -- true of D^-1/2 (P + I) D^-1/2 of a symmetric pattern, which is what every matrix here is (the
tests assert the symmetry).  Two partitioned runs are compared with each other at twice that."""
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

import _aggmax_workers as AW  # noqa: E402
import _batchnorm_workers as BW  # noqa: E402
import _gradgrid_workers as GG  # noqa: E402
import _gat_tail_workers as TW  # noqa: E402

TOL = 1e-5
N = GG.N                                       # the planted problem of the gradient grid (n = 1100)
FIN, CLASSES, HIDDEN, NLAYERS, EPOCHS = GG.FIN, GG.CLASSES, GG.HIDDEN, 3, 2
DROPOUT, DROPOUT_SEED = GG.DROPOUT, GG.DROPOUT_SEED
KARATE_CASES = [(K, alpha, C) for K in (1, 3, 10) for alpha in (0.0, 0.1, 0.5) for C in (1, 7, 16)]
PATTERN_N, PATTERN_CHUNK = 1100, 64
PATTERN_CASES = [(K, alpha, C) for K in (1, 2, 10) for alpha in (0.0, 0.1, 0.5) for C in (3, 7, 41, 128)]
PPR_METHODS = ("ppr_step", "ppr_step_backward")


# ---- the definition ---------------------------------------------------------------------------------------------------------------

def coefficients(alpha):
    """(a, b) as numpy float32 scalars: a = float32(alpha), b = 1.0f - a."""
    a = np.float32(alpha)
    return a, np.float32(1.0) - a


def step_np(S, H, alpha):
    """fl(fl(b S) + fl(a H)) in numpy fp32: every operation of numpy rounds on its own."""
    a, b = coefficients(alpha)
    S, H = np.asarray(S, np.float32), np.asarray(H, np.float32)
    return (b * S) + (a * H)


def step_backward_np(G, T, D, alpha, last):
    """(Gout, Dout) of one adjoint step in numpy fp32 (Gout None at the last step)."""
    a, b = coefficients(alpha)
    G, T = np.asarray(G, np.float32), np.asarray(T, np.float32)
    acc = a * G
    if D is not None:
        acc = np.asarray(D, np.float32) + acc
    bt = b * T
    if last:
        return None, acc + bt
    return bt, acc


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def propagate64(Ad, H, K, alpha):
    """Z^K of the recursion in float64 on the dense matrix, with the coefficients the kernels use."""
    a, b = (float(x) for x in coefficients(alpha))
    H = np.asarray(H, np.float64)
    Z = H
    for _ in range(K):
        Z = b * (Ad @ Z) + a * H
    return Z


def propagate_backward64(Ad, G, K, alpha):
    """dH = a sum_{k=1..K} G^k + G^0 in float64."""
    a, b = (float(x) for x in coefficients(alpha))
    G = np.asarray(G, np.float64)
    D = np.zeros_like(G)
    for _ in range(K):
        D = D + a * G
        G = b * (Ad.T @ G)
    return D + G


def sym_normalised(P):
    """D^-1/2 (P + I) D^-1/2 of the pattern of the sparse matrix ``P`` as a dense float64 array (what normalize="sym" trains on)."""
    n = P.shape[0]
    B = (sp.csr_matrix(P) + sp.identity(n, format="csr")).astype(np.float64).tocsr()
    B.data[:] = 1.0
    d = 1.0 / np.sqrt(np.asarray(B.sum(axis=1)).reshape(-1))
    return (sp.diags(d) @ B @ sp.diags(d)).toarray()


def seeded_operands(n, K, alpha, C):
    """The global H and G of one case."""
    rng = np.random.default_rng([17, K, int(round(alpha * 100)), C])
    return rng.random((n, C), dtype=np.float32) * 2 - 1, rng.random((n, C), dtype=np.float32) * 2 - 1


# ---- the kernel-level pattern of the GPU tests: stored values, rows of 0 / 1 / 64 / 65 / 1 000 entries -----------------------------

def make_pattern(dirname):
    """A symmetric 1 100-vertex matrix D^-1/2 (P + I') D^-1/2 written WITH its fp32 values (the engine loads it as stored, no
    normalisation on the fly): I' leaves out the loop of two isolated vertices, whose rows and columns are empty -- a zero block, the
    norm stays <= 1.  Stored row lengths: 0 (vertices 12 and 400), 1 (vertex 6: its loop alone), 64 (vertex 20), 65 (vertex 21) and
    1 000 (vertices 11 and 13: with a chunk of 64 both are cut into 16 tasks, the empty row 12 between them).  Part vectors for 1 and
    2 ranks (random).  Returns (paths, the dense float64 matrix of the STORED fp32 values)."""
    from scipy.io import mmwrite
    n = PATTERN_N
    rng = np.random.default_rng(64)
    special = [6, 11, 12, 13, 20, 21, 400]
    ordinary = np.setdiff1d(np.arange(n), special)
    r = rng.choice(ordinary, 2600)
    c = rng.choice(ordinary, 2600)
    rows, cols = [r], [c]
    for v, deg in ((11, 999), (13, 999), (20, 63), (21, 64)):
        nb = rng.choice(ordinary, deg, replace=False)
        rows.append(np.full(deg, v)), cols.append(nb)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    loops = np.setdiff1d(np.arange(n), [12, 400])
    Pm = sp.coo_matrix((np.ones(2 * rows.size + loops.size), (np.concatenate([rows, cols, loops]), np.concatenate([cols, rows, loops]))),
                       shape=(n, n)).tocsr()
    Pm.sum_duplicates()
    Pm.data[:] = 1.0
    deg = np.asarray(Pm.sum(axis=1)).reshape(-1)
    d = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1.0)), 0.0)
    M = (sp.diags(d) @ Pm @ sp.diags(d)).tocsr()
    M.data = M.data.astype(np.float32).astype(np.float64)            # the values as the file and the engine hold them
    lens = np.diff(M.indptr)
    assert lens[12] == lens[400] == 0 and lens[6] == 1 and lens[20] == 64 and lens[21] == 65 and lens[11] == lens[13] == 1000
    os.makedirs(dirname, exist_ok=True)
    paths = {"A": os.path.join(dirname, "pattern.mtx")}
    mmwrite(paths["A"], M.tocoo(), field="real", symmetry="general", precision=9)
    for P in (1, 2):
        pv = np.random.default_rng(5 + P).integers(0, P, n)
        paths["pv%d" % P] = os.path.join(dirname, "pattern.%d.rp" % P)
        with open(paths["pv%d" % P], "w") as fh:
            fh.write(" ".join(map(str, pv.tolist())) + "\n")
    return paths, M.toarray()


# ---- engine level -----------------------------------------------------------------------------------------------------------------

def _provider(M, gpu, chunk=None):
    """gpu false: the checker-backed provider on the CPU (no step kernels: the composed route); true: the real one (``chunk``: the
    planner's chunk); "composed": the real one with the step kernels hidden."""
    from conftest import pkg
    if gpu:
        K = pkg("kernels")
        cls = K.HipKernels
        if gpu == "composed":
            class NoPpr(K.HipKernels):
                def __getattribute__(self, name):
                    if name in PPR_METHODS:
                        raise AttributeError(name)
                    return super().__getattribute__(name)
            cls = NoPpr
        M._kernel_provider = cls(torch.device("cuda:0"), **({"chunk": chunk} if chunk else {}))
    else:
        from oracle_kernels import OracleKernels
        M._kernel_provider = OracleKernels()
    M._exchanger = None


def engine_worker(rank, P, port, paths, gpu, q, cases=(), normalize=None, pv=None, chunk=None, no_composed=False):
    """propagate / propagate_backward of rank `rank` of `P` over gloo on the seeded global operands of every case (K, alpha, C).
    ``no_composed``: the composed step functions raise -- a run that still answers ran the kernels."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M, E = pkg("PGCN"), pkg("engine")
    _provider(M, gpu, chunk)
    if no_composed:
        def refuse(*a, **k):
            raise AssertionError("the composed route ran")
        E.ppr_step_composed = E.ppr_step_backward_composed = refuse
    got = {"rank": rank, "cases": []}

    def fn(r, size, nlayers, nfeatures, path_A, path_partvec, backend, *rest, **_):
        M.myrank, M.world_size = r, size
        M.device = torch.device("cuda:0") if gpu else torch.device("cpu")
        if gpu:
            torch.cuda.set_device(M.device)
        A = M._ingest.mmread(path_A)
        partvec = M._partition.read_partvec(path_partvec)
        with redirect_stdout(io.StringIO()):
            M.compute_communication_maps(A, partvec, r, size, normalize)
            eng = M.get_partitiont_of_adjacency_matrix(A, partvec, r, normalize)
        own = eng.part.owned.cpu().numpy()
        n = A.shape[0]
        held = set(vars(eng))
        got.update(own=own, hip=type(eng.k).__name__, nslots=int(getattr(eng.A_loc, "nslots", 0) or 0))
        for K, alpha, C in cases:
            Hg, Gg = seeded_operands(n, K, alpha, C)
            before = dict(eng.stats)
            Z = eng.propagate(torch.from_numpy(Hg[own]).to(M.device), K, alpha)
            mid = dict(eng.stats)
            D = eng.propagate_backward(torch.from_numpy(Gg[own]).to(M.device), K, alpha)
            after = dict(eng.stats)
            eng.forward(torch.from_numpy(Hg[own]).to(M.device))
            one = dict(eng.stats)
            got["cases"].append(dict(K=K, alpha=alpha, C=C, Z=Z.cpu().numpy(), D=D.cpu().numpy(),
                                     fwd={k: mid[k] - before[k] for k in mid}, bwd={k: after[k] - mid[k] for k in mid},
                                     one={k: one[k] - after[k] for k in mid}))
        got["new_attributes"] = sorted(set(vars(eng)) - held)
        got["slabs"] = sorted(eng._buf)

    M.init_process(rank, P, fn, NLAYERS, HIDDEN, paths["A"], paths[pv or "pv%d" % P], "gloo", normalize)
    q.put(got)


def spawn_engine(P, paths, gpu, **kw):
    return TW.spawn(engine_worker, P, paths, gpu, **kw)


def rows(res, pick, n):
    out = None
    for r in res:
        v = pick(r)
        out = np.zeros((n,) + v.shape[1:], v.dtype) if out is None else out
        out[r["own"]] = v
    return out


def check_engine(res, Ad, cases, label=""):
    """Every case of one worker group against the float64 recursion on the dense matrix ``Ad`` within (K + 1) TOL, the adjoint
    identity within the same bound relative to the product of the norms, the exchange volume of K aggregations, nothing kept on the
    engine.  Prints every measured figure.  Returns {case: (Z, D)} gathered over the ranks."""
    from conftest import rel_err
    n = Ad.shape[0]
    assert np.array_equal(Ad, Ad.T), "the test matrix is not symmetric"
    out = {}
    assert len(res[0]["cases"]) == len(cases)
    for i, (K, alpha, C) in enumerate(cases):
        Hg, Gg = seeded_operands(n, K, alpha, C)
        Z, D = rows(res, lambda r: r["cases"][i]["Z"], n), rows(res, lambda r: r["cases"][i]["D"], n)
        assert Z.dtype == D.dtype == np.float32 and Z.shape == D.shape == (n, C)
        ez, ed = rel_err(Z, propagate64(Ad, Hg, K, alpha)), rel_err(D, propagate_backward64(Ad, Gg, K, alpha))
        lhs, rhs = float((Z.astype(np.float64) * Gg).sum()), float((Hg.astype(np.float64) * D).sum())
        ea = abs(lhs - rhs) / (np.linalg.norm(Hg.astype(np.float64)) * np.linalg.norm(Gg.astype(np.float64)))
        bound = (K + 1) * TOL
        print("%s P=%d K=%d alpha=%g C=%d: forward %.3g backward %.3g adjoint %.3g (bound %.3g)" % (label, len(res), K, alpha, C, ez, ed, ea,
                                                                                                    bound), flush=True)
        assert ez <= bound and ed <= bound and ea <= bound, (label, K, alpha, C, ez, ed, ea, bound)
        for r in res:
            c = r["cases"][i]
            assert c["fwd"] == {k: K * v for k, v in c["one"].items()}, (c["fwd"], c["one"])         # K exchanges of one aggregation each
            assert c["bwd"]["send_volume"] == c["fwd"]["recv_volume"] and c["bwd"]["recv_volume"] == c["fwd"]["send_volume"]
        out[(K, alpha, C)] = (Z, D)
    for r in res:
        assert r["new_attributes"] == [], r["new_attributes"]
    return out


def check_same(a, b, cases, label=""):
    """Two partitioned runs of the same cases agree with each other at twice the bound."""
    from conftest import rel_err
    for K, alpha, C in cases:
        for x, y, what in zip(a[(K, alpha, C)], b[(K, alpha, C)], ("forward", "backward")):
            e = rel_err(x, y)
            print("%s K=%d alpha=%g C=%d %s: %.3g between the runs" % (label, K, alpha, C, what, e), flush=True)
            assert e <= 2 * (K + 1) * TOL, (label, K, alpha, C, what, e)


# ---- model level ------------------------------------------------------------------------------------------------------------------

def make_dataset(dirname):
    """The planted problem of the gradient grid (n = 1100)."""
    return AW.make_dataset(dirname)


def config(dense, bias=False, dropout=0.0, K=10, alpha=0.1):
    c = GG.config("none", False, bias, False, dropout, HIDDEN)
    c.update(dense=bool(dense), K=int(K), alpha=float(alpha))
    return c


def model_configs():
    """Dense layers + propagate (APPNP), and GCN layers + bias + dropout + propagate."""
    return [config(True, K=10, alpha=0.1), config(False, bias=True, dropout=DROPOUT, K=3, alpha=0.1)]


def tag(c):
    return "%s%s-K%d" % (GG.tag(c), "+dense" if c["dense"] else "", c["K"])


def widths_of(c):
    return [FIN] + [c["hidden"]] * (NLAYERS - 1) + [CLASSES]


def model64(data, widths, params, c, step, dtype=torch.float64, trace=None):
    """(loss, logits after the propagation, {name: grad}) of run(normalize="sym", propagate=K, ppr_alpha=alpha[, dense_layers]) on the
    whole graph in training mode: stock operations, torch's own autograd.  ``trace`` receives every ReLU input."""
    from conftest import pkg
    D = pkg("dropout")
    n = data["A"].shape[0]
    Ad = GG.dense_adjacency(data).to(dtype)
    h = torch.from_numpy(data["X"]).to(dtype)
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    L = len(widths) - 1
    thr, scale = D.threshold(c["dropout"])
    for l in range(L):
        z = (h if c["dense"] else Ad @ h) @ p["%d.linear.weight" % l].t()
        if c["bias"]:
            z = z + p["%d.bias" % l]
        if l == L - 1:
            break
        if trace is not None:
            trace.append(z.detach())
        h = torch.relu(z)
        if c["dropout"] > 0.0:
            keep = D.keep_mask(DROPOUT_SEED, step, l, np.arange(n), z.shape[1], thr)
            h = torch.where(keep, h * scale, torch.zeros((), dtype=dtype))
    a, b = (float(x) for x in coefficients(c["alpha"]))
    logits = z
    for _ in range(c["K"]):
        logits = b * (Ad @ logits) + a * z
    train = torch.from_numpy(data["split"] == 1)
    loss = F.cross_entropy(logits[train], torch.from_numpy(data["labels"])[train])
    names = list(p)
    grads = dict(zip(names, (g.detach() for g in torch.autograd.grad(loss, [p[k] for k in names]))))
    return loss.detach(), logits.detach(), grads


_refs = {}


def reference(data, c):
    """{"seed", "params", "steps": [{"m64", "twin"}]} under the seed rule of the gradient grid: the smallest weight seed in GG.SEEDS for
    which no ReLU input of the double run lies within GG.DOUBT times the twin's largest error of that layer (from the reference alone).
    None of the two configurations is without such a seed; the rule is asserted."""
    key = tag(c)
    if key not in _refs:
        widths = widths_of(c)
        for seed in GG.SEEDS:
            params = GG.initial_params(widths, c, seed)
            steps, count = [], 0
            for s in range(EPOCHS):
                rec, traces = {}, {}
                for name, dt in (("m64", torch.float64), ("twin", torch.float32)):
                    traces[name] = []
                    loss, logits, grads = model64(data, widths, params, c, s, dt, traces[name])
                    rec[name] = {"loss": loss, "logits": logits, "grads": grads}
                for t64, t32 in zip(traces["m64"], traces["twin"]):
                    count += int((t64.abs() <= GG.DOUBT * float((t32.double() - t64).abs().max())).sum())
                steps.append(rec)
            if count == 0:
                _refs[key] = {"seed": seed, "params": params, "steps": steps, "widths": widths}
                break
        assert key in _refs, "%s: every weight seed leaves a doubtful ReLU input" % key
    return _refs[key]


def model_worker(rank, P, port, paths, gpu, q, jobs=()):
    """GG.run_worker's protocol for run(epochs=2, lr=0.0, optimizer="torch", normalize="sym", nlayers=3, propagate=..., ...): per job
    the parameters written into the model, the gradients before each optimiser step, this rank's loss and (propagated) logits."""
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
        cur["modules"] = [type(m).__name__ for m in model]
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

    def fn(r, size, nlayers, nfeatures, path_A, path_partvec, backend, *rest, **_):
        for job in jobs:
            c = job["config"]
            cur.update(job=job, grads=[], logits=[], loss=[])
            torch.manual_seed(job["seed"])
            kw = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=c["hidden"], epochs=EPOCHS, lr=0.0,
                      optimizer="torch", propagate=c["K"], ppr_alpha=c["alpha"])
            if c["dense"]:
                kw["dense_layers"] = True
            if c["bias"]:
                kw["bias"] = True
            if c["dropout"] > 0.0:
                kw.update(dropout=c["dropout"], dropout_seed=DROPOUT_SEED)
            with redirect_stdout(io.StringIO()):
                M.run(r, size, NLAYERS, c["hidden"], path_A, path_partvec, "gloo", normalize="sym", **kw)
            eng = M._engine_current
            results.append(dict(tag=tag(c), names=cur["names"], modules=cur["modules"], grads=cur["grads"], logits=cur["logits"],
                                loss=cur["loss"], own=eng.part.owned.cpu().numpy(), hip=type(eng.k).__name__,
                                stats=dict(eng.stats)))

    M.init_process(rank, P, fn, NLAYERS, HIDDEN, paths["A"], paths["pv%d" % P], "gloo", "sym")
    q.put({"rank": rank, "results": results})


def spawn_model(P, paths, gpu, configs, data):
    jobs = [{"config": c, "seed": reference(data, c)["seed"], "params": {k: v.numpy() for k, v in reference(data, c)["params"].items()}}
            for c in configs]
    return [r["results"] for r in TW.spawn(model_worker, P, paths, gpu, jobs=jobs)]


def check_models(data, configs, res, case=""):
    """Loss, logits and every reduced parameter gradient of both steps against the double model through conftest.held_to_fixture
    (model / fp32 twin / double: max(1e-5, twice the twin's error)).  Returns how many tensors were held."""
    from conftest import held_to_fixture
    P, held = len(res), 0
    for j, c in enumerate(configs):
        ref = reference(data, c)
        ranks = [r[j] for r in res]
        where = "propagate%s/%s/P%d" % (case, tag(c), P)
        for r in ranks:
            assert r["tag"] == tag(c) and r["modules"] == ["PGCN"] * NLAYERS + ["Propagate"], (where, r["modules"])
            assert sorted(r["names"]) == sorted(GG.parameter_names(ref["widths"], c)), (where, r["names"])
            assert len(r["grads"]) == len(r["logits"]) == len(r["loss"]) == EPOCHS, where
        for s, rec in enumerate(ref["steps"]):
            m64, twin = rec["m64"], rec["twin"]
            at = "%s/step%d" % (where, s)
            held_to_fixture(at, "loss", np.array([sum(r["loss"][s] for r in ranks)]), twin["loss"].numpy().reshape(1),
                            m64["loss"].numpy().reshape(1))
            held_to_fixture(at, "logits", rows(ranks, lambda r, s=s: r["logits"][s], N), twin["logits"].numpy(), m64["logits"].numpy())
            held += 2
            for i, r in enumerate(ranks):
                for name in ref["params"]:
                    held_to_fixture(at + "/rank%d" % i, "grad " + name.split(".", 1)[1], r["grads"][s][name], twin["grads"][name].numpy(),
                                    m64["grads"][name].numpy())
                    held += 1
    return held


# ---- the Cora-shaped golden graph with planted labels (the whole-model runs on the GPU) --------------------------------------------

def make_cora(dirname):
    """The pattern of tests/golden/cora.A.mtx (the file holds normalised values; the runs normalise the pattern on the fly) with its
    part vectors for 1 and 2 ranks, seven planted classes (ranges of vertex ids), features = a class centre + noise, a 50 / 20 / 20
    split with the rest in no set."""
    from conftest import gpath, read_partvec
    from scipy.io import mmread, mmwrite
    n = len(read_partvec(gpath("cora.A.mtx.1.rp")))
    A = sp.coo_matrix(mmread(gpath("cora.A.mtx")))
    assert A.shape == (n, n)
    pattern = os.path.join(dirname, "cora.pattern.mtx")
    mmwrite(pattern, sp.coo_matrix((np.ones(A.nnz, np.float32), (A.row, A.col)), shape=A.shape), field="pattern", symmetry="general")
    rng = np.random.default_rng(2708)
    y = (np.arange(n) * CLASSES // n).astype(np.int64)
    X = (rng.standard_normal((CLASSES, FIN))[y] + 1.5 * rng.standard_normal((n, FIN))).astype(np.float32)
    u = rng.random(n)
    split = np.where(u < 0.5, 1, np.where(u < 0.7, 2, np.where(u < 0.9, 3, 0))).astype(np.uint8)
    paths = {"A": pattern, "pv1": gpath("cora.A.mtx.1.rp"), "pv2": gpath("cora.A.mtx.2.rp")}
    for name, arr in (("features", X), ("labels", np.where(split == 0, -1, y).astype(np.int64)), ("split", split)):
        paths[name] = os.path.join(dirname, name + ".npy")
        np.save(paths[name], arr)
    return paths


def cpu_run_worker(rank, P, port, paths, gpu, q, **kw):
    """PW.run_worker on the CPU with the checker-backed provider -- the composed route -- also where a device is visible: run()
    takes the device when torch reports one, so this (fresh) process reports none."""
    torch.cuda.is_available = lambda: False
    import _predict_workers as PW
    return PW.run_worker(rank, P, port, paths, False, q, **kw)


def spawn_cpu_jobs(P, paths, jobs):
    return [r["jobs"] for r in TW.spawn(cpu_run_worker, P, paths, False, launcher="PGCN", jobs=jobs)]
