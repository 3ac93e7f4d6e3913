"""DropEdge in numpy and torch double, and the worker processes of tests/test_dropedge.py and tests/test_dropedge_gpu.py (spawn start
method), in the pattern of tests/_aggmax_workers.py.

Definition (csrc/pgcn_dropedge.h, include/pgcn_hip.h): the stored entry (i, j) of the pattern of A + I survives step t when
gi == gj or u(seed, t, min(gi, gj), max(gi, gj)) >= thr (global ids); with M the kept entries, r / c its row / column counts and
s = fl32(count^-1/2):  Y = s_r * (M (s_c * H)),  dH = s_c * (M^T (s_r * G)).  Only ``dropout.edge_keep`` (the integer host
statement of the mask) is taken from the package."""
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
import _gradgrid_workers as GG  # noqa: E402
import _nodeclass_workers as NW  # noqa: E402

P_DROP, SEED = 0.5, 11
ENGINE_WIDTHS = (1, 24)
STEPS = (0, 3)
NLAYERS, HIDDEN, EPOCHS = 3, GG.HIDDEN, 2
DROP_METHODS = ("dropedge_sum", "dropedge_count", "dropedge_scales", "row_scale")
U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def scales(count):
    """fl32(1 / sqrt(double count)), 1 where the count is 0: partition.degree_scales stated in numpy."""
    d = np.asarray(count, np.float64)
    return np.where(d > 0, 1.0 / np.sqrt(np.maximum(d, 1.0)), 1.0).astype(np.float32)


def kept_pattern(A, seed, step, thr, gid=None):
    """The kept entries of the pattern of A + I as a 0 / 1 CSR matrix (float64), rows and columns in the numbering of A, ``gid`` their
    global ids (None: the index)."""
    from conftest import pkg
    D = pkg("dropout")
    n = A.shape[0]
    B = (sp.csr_matrix(A) + sp.identity(n, format="csr")).tocoo()
    g = np.arange(n) if gid is None else np.asarray(gid)
    keep = D.edge_keep(seed, step, g[B.row], g[B.col], thr)
    return sp.csr_matrix((np.ones(int(keep.sum())), (B.row[keep], B.col[keep])), shape=(n, n))


def oracle(M, H=None, G=None):
    """{r, c, s_r, s_c} of a kept pattern M (any 0 / 1 sparse matrix) and, in float64 from the fp32 scales, Y and dH with their
    bounds (kept count + the two scalings) * 2^-24 * sum |terms| per element -- the bound of tests/test_aggmax_gpu.py."""
    M = sp.csr_matrix(M).astype(np.float64)
    r, c = np.asarray(M.sum(axis=1)).reshape(-1).astype(np.int64), np.asarray(M.sum(axis=0)).reshape(-1).astype(np.int64)
    s_r, s_c = scales(r), scales(c)
    out = dict(r=r, c=c, s_r=s_r, s_c=s_c)
    if H is not None:
        Hs = s_c.astype(np.float64)[:, None] * H.astype(np.float64)
        out["Y"] = s_r.astype(np.float64)[:, None] * (M @ Hs)
        out["Y_bound"] = (r + 2)[:, None] * U * (s_r.astype(np.float64)[:, None] * (M @ np.abs(Hs)))
    if G is not None:
        Gs = s_r.astype(np.float64)[:, None] * G.astype(np.float64)
        out["dH"] = s_c.astype(np.float64)[:, None] * (M.T @ Gs)
        out["dH_bound"] = (c + 2)[:, None] * U * (s_c.astype(np.float64)[:, None] * (M.T @ np.abs(Gs)))
    return out


# ---- data -------------------------------------------------------------------------------------------------------------------------

def graph_paths(dirname, name, mtx):
    """{"A", "pv<P>", "cpv<P>"} of the PATTERN of a golden matrix (cora.A.mtx holds normalised values; the runs normalise the pattern
    on the fly) with seeded random and contiguous part vectors for 1, 2 and 3 ranks."""
    from scipy.io import mmread, mmwrite
    from conftest import gpath
    A = sp.coo_matrix(mmread(gpath(mtx)))
    A = sp.coo_matrix((np.ones(A.nnz, np.float32), (A.row, A.col)), shape=A.shape)
    n = A.shape[0]
    paths = {"A": os.path.join(dirname, name + ".pattern.mtx"), "n": n}
    mmwrite(paths["A"], A, field="pattern", symmetry="general")
    A = A.tocsr()
    for P in (1, 2, 3):
        for key, pv in (("pv", np.random.default_rng(100 + P).integers(0, P, n)), ("cpv", (np.arange(n) * P) // n)):
            paths["%s%d" % (key, P)] = os.path.join(dirname, "%s.%d.%s" % (name, P, key))
            with open(paths["%s%d" % (key, P)], "w") as fh:
                fh.write(" ".join(map(str, pv.tolist())) + "\n")
    return paths, {"A": A}


def make_dataset(dirname):
    """The planted problem of the gradient grid (n = 1100) with contiguous part vectors ``cpv<P>`` beside the random ``pv<P>``."""
    paths, data = NW.make_dataset(dirname, n=GG.N, nnz=GG.NNZ, community=GG.COMMUNITY, classes=GG.CLASSES, fin=GG.FIN)
    for P in (1, 2, 3):
        paths["cpv%d" % P] = os.path.join(dirname, "sbm.%d.cp" % P)
        with open(paths["cpv%d" % P], "w") as fh:
            fh.write(" ".join(map(str, ((np.arange(GG.N) * P) // GG.N).tolist())) + "\n")
    paths["n"] = GG.N
    return paths, data


def _provider(M, gpu):
    """gpu false: the checker-backed provider (no drop kernels: the composed route); true: the real one; "composed": the real one with
    the drop kernels hidden."""
    from conftest import pkg
    if gpu == "composed":
        K = pkg("kernels")

        class NoDrop(K.HipKernels):
            def __getattribute__(self, name):
                if name in DROP_METHODS:
                    raise AttributeError(name)
                return super().__getattribute__(name)

        M._kernel_provider = NoDrop(torch.device("cuda:0"))
    elif gpu:
        M._kernel_provider = None
    else:
        from oracle_kernels import OracleKernels
        M._kernel_provider = OracleKernels()
    M._exchanger = None


def seeded_operands(n, f):
    rng = np.random.default_rng([5, n, f])
    return rng.random((n, f), dtype=np.float32) * 2 - 1, rng.random((n, f), dtype=np.float32) * 2 - 1


# ---- engine level -----------------------------------------------------------------------------------------------------------------

def engine_worker(rank, P, port, paths, gpu, q, partvec="pv"):
    """forward_drop / backward_drop of rank `rank` of `P` over gloo on seeded global operands: per step of STEPS (written into the
    state's device tensor, the tick bumped) the counts, the scale bits and, per width, Y and dH."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M = pkg("PGCN")
    D = pkg("dropout")
    _provider(M, gpu)
    got = {"rank": rank, "cases": []}
    n = paths["n"]

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
        state = D.DropoutState(SEED, M.device)
        ctx = D.EdgeDrop(P_DROP, state)
        eng.backward(eng.forward(torch.zeros((own.size, 3), device=M.device)))
        got.update(own=own, lazy_before=eng._drop is None, hip=type(eng.k).__name__)
        for step in STEPS:
            state.step.fill_(step)
            state.tick += 1
            for f in ENGINE_WIDTHS:
                Hg, Gg = seeded_operands(n, f)
                Y = eng.forward_drop(torch.from_numpy(Hg[own]).to(M.device), ctx)
                dH = eng.backward_drop(torch.from_numpy(Gg[own]).to(M.device), ctx)
                d = ctx.cache
                got["cases"].append(dict(step=step, f=f, Y=Y.cpu().numpy(), dH=dH.cpu().numpy(), r=d.r.cpu().numpy(), c=d.c.cpu().numpy(),
                                         s_r=d.s_r.cpu().numpy(), s_c=d.s_c.cpu().numpy()))
        got.update(composed=eng._drop.composed, halo_nnz=[int(a.nnz) for a in eng._drop.halo])

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


def rows(res, pick, n):
    out = None
    for r in res:
        v = pick(r)
        out = np.zeros((n,) + v.shape[1:], v.dtype) if out is None else out
        out[r["own"]] = v
    return out


def check_engine(res, data, P, n, want_bits=None):
    """Every assertion of the engine level on one worker group: counts exact and scale bits those of the definition (by global id:
    the same under any part vector), Y and dH within the bound of the float64 oracle, the adjoint identity in float64.  Returns
    {(step, f): (r, c, s_r bits, s_c bits)} by global id; ``want_bits``: such a record of another run, which must be reproduced."""
    assert all(r["lazy_before"] for r in res)
    if P > 1:
        assert all(sum(r["halo_nnz"]) > 0 for r in res), "the halo structures hold no entries"
    thr = int(np.floor(P_DROP * 2.0 ** 32 + 0.5))
    seen = {}
    for k in range(len(res[0]["cases"])):
        c0 = res[0]["cases"][k]
        step, f = c0["step"], c0["f"]
        Hg, Gg = seeded_operands(n, f)
        want = oracle(kept_pattern(data["A"], SEED, step, thr), Hg, Gg)
        got = {key: rows(res, lambda r, key=key: r["cases"][k][key], n) for key in ("Y", "dH", "r", "c", "s_r", "s_c")}
        at = (P, step, f)
        assert got["r"].dtype == np.int32 and np.array_equal(got["r"], want["r"]) and np.array_equal(got["c"], want["c"]), at
        assert np.array_equal(bits(got["s_r"]), bits(want["s_r"])) and np.array_equal(bits(got["s_c"]), bits(want["s_c"])), at
        assert want["r"].min() >= 1 and want["r"].sum() < (sp.csr_matrix(data["A"]) + sp.identity(n)).nnz, at     # self loops stay, edges go
        for key in ("Y", "dH"):
            err = np.abs(got[key].astype(np.float64) - want[key])
            assert (err <= want[key + "_bound"]).all(), at + (key, float((err - want[key + "_bound"]).max()))
        # <Y(H), G> = <H, dH(G)>: both sides in float64 from the fp32 results, within the two bounds summed against the other operand
        lhs, rhs = (got["Y"].astype(np.float64) * Gg).sum(), (Hg * got["dH"].astype(np.float64)).sum()
        slack = (want["Y_bound"] * np.abs(Gg)).sum() + (want["dH_bound"] * np.abs(Hg)).sum()
        assert abs(lhs - rhs) <= slack, at + (lhs, rhs, slack)
        seen[(step, f)] = (got["r"], got["c"], bits(got["s_r"]), bits(got["s_c"]))
        if want_bits is not None:
            assert all(np.array_equal(a, b) for a, b in zip(seen[(step, f)], want_bits[(step, f)])), at
    a, b = seen[(STEPS[0], ENGINE_WIDTHS[0])], seen[(STEPS[1], ENGINE_WIDTHS[0])]
    assert not np.array_equal(a[0], b[0]), "two steps drew the same mask"
    return seen


# ---- model level ------------------------------------------------------------------------------------------------------------------

def config(norm="none", root=False, bias=False, dropout=0.0):
    return GG.config(norm, root, bias, False, dropout, HIDDEN)


def model_configs():
    return [config(), config(dropout=GG.DROPOUT), config("node", 1, 1, GG.DROPOUT), config("batch", 1, 0, 0.0)]


def rank_subset():
    return [config(), config("node", 1, 1, GG.DROPOUT)]


def widths_of(c):
    return [GG.FIN] + [c["hidden"]] * (NLAYERS - 1) + [GG.CLASSES]


def dropped_adjacency(data, step):
    """D_r^-1/2 M D_c^-1/2 of the kept pattern of ``step`` as a dense double tensor, with the scales of the definition (fp32 values)."""
    thr = int(np.floor(P_DROP * 2.0 ** 32 + 0.5))
    M = kept_pattern(data["A"], GG.DROPOUT_SEED, step, thr)
    o = oracle(M)
    return torch.from_numpy((sp.diags(o["s_r"].astype(np.float64)) @ M @ sp.diags(o["s_c"].astype(np.float64))).toarray())


def model64_drop(data, widths, params, opts, step, dtype, buffers=None, trace=None):
    """GG.model64 in training mode with the adjacency of ``step``'s kept pattern: its table of dense adjacencies is keyed by the
    matrix object, so a copy of the pattern stands for the step and carries the dropped matrix."""
    key = data["A"].copy()
    GG._adj[id(key)] = (key, dropped_adjacency(data, step))
    try:
        return GG.model64(dict(data, A=key), widths, params, opts, step, True, dtype, buffers, trace)
    finally:
        del GG._adj[id(key)]


def reference(data, c, seed):
    widths = widths_of(c)
    params = GG.initial_params(widths, c, seed)
    opts = dict(c, task="single")
    out = {"params": params, "widths": widths, "steps": [], "seed": seed}
    bufs = {torch.float64: None, torch.float32: None}
    for step in range(EPOCHS):
        rec = {}
        for key, rkey, dt in (("m64", "relu64", torch.float64), ("twin", "relu32", torch.float32)):
            tr = []
            loss, logits, grads, b = model64_drop(data, widths, params, opts, step, dt, bufs[dt], tr)
            bufs[dt] = b
            rec[key], rec[rkey] = {"loss": loss, "logits": logits, "grads": grads}, tr
        out["steps"].append(rec)
    out["eval"] = {}
    for key, dt in (("m64", torch.float64), ("twin", torch.float32)):       # eval mode: the undropped matrix
        out["eval"][key] = {"logits": GG.model64(data, widths, params, opts, EPOCHS, False, dt, bufs[dt])[1]}
    return out


def make_jobs(data, configs):
    """GG's seed rule on this reference: the smallest weight seed in 0 .. 15 without a doubtful ReLU input at either step."""
    jobs, refs = [], {}
    for c in configs:
        for seed in GG.SEEDS:
            ref = reference(data, c, seed)
            if GG.doubtful(ref) == 0:
                break
        else:
            raise AssertionError("no weight seed without a doubtful ReLU input for %s" % GG.tag(c))
        refs[GG.tag(c)] = ref
        jobs.append({"config": c, "seed": seed, "params": {k: v.numpy() for k, v in ref["params"].items()}})
    return jobs, refs


def model_worker(rank, P, port, paths, gpu, q, jobs=(), drop_edge=P_DROP):
    """GG.run_worker's protocol for run(epochs=2, lr=0.0, optimizer="torch", normalize="sym", nlayers=3, drop_edge=...)."""
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
        model.register_forward_hook(lambda m, a, out: cur["logits"].append(out.detach().cpu().numpy()) if m.training else None)

    adam_step = torch.optim.Adam.step

    def step(self, *a, **kw):
        cur["grads"].append({name: prm.grad.detach().cpu().numpy().copy() for name, prm in cur["model"].named_parameters()})
        eng = M._engine_current
        d = cur["model"][0].drop_edge.cache if hasattr(cur["model"][0], "drop_edge") else None
        if d is not None:
            cur["counts"].append((d.r.cpu().numpy().copy(), d.c.cpu().numpy().copy(), d.s_r.cpu().numpy().copy(), d.s_c.cpu().numpy().copy()))
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
            cur.update(job=job, grads=[], logits=[], loss=[], counts=[])
            torch.manual_seed(job["seed"])
            kw = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=c["hidden"], epochs=EPOCHS, lr=0.0,
                      optimizer="torch", dropout_seed=GG.DROPOUT_SEED)
            if drop_edge is not None:
                kw["drop_edge"] = drop_edge
            if c["norm"] != "none":
                kw["norm"] = c["norm"]
            for name, opt in (("root", "root_weight"), ("bias", "bias")):
                if c[name]:
                    kw[opt] = True
            if c["dropout"] > 0.0:
                kw.update(dropout=c["dropout"])
            with redirect_stdout(io.StringIO()):
                model = M.run(r, size, NLAYERS, c["hidden"], path_A, path_partvec, "gloo", normalize="sym", **kw)
            eng = M._engine_current
            data = M._nodedata.load(paths["features"], paths["labels"], paths["split"], eng.part.owned, GG.N, device=M.device)
            model.eval()
            with torch.no_grad():
                ev = model(data.features).cpu().numpy()
            results.append(dict(tag=GG.tag(c), grads=cur["grads"], logits=cur["logits"], loss=cur["loss"], counts=cur["counts"], eval_logits=ev,
                                own=eng.part.owned.cpu().numpy(), composed=None if eng._drop is None else eng._drop.composed,
                                hip=type(eng.k).__name__))

    M.init_process(rank, P, fn, NLAYERS, HIDDEN, paths["A"], paths["pv%d" % P], "gloo", "sym")
    q.put({"rank": rank, "results": results})


def spawn_model(P, paths, gpu, jobs, **kw):
    return [r["results"] for r in _spawn(model_worker, P, paths, gpu, jobs=jobs, **kw)]


def check_models(configs, refs, res, case):
    """Per configuration: loss, logits and every reduced parameter gradient of both steps against the double model under the same
    mask, and the eval logits against the undropped double model, through conftest.held_to_fixture (max(1e-5, 2 err_twin): the
    gradient grid's bar); the two steps' logits differ (another mask).  Returns the tensors held."""
    from conftest import held_to_fixture
    P = len(res)
    held = 0
    for j, c in enumerate(configs):
        ranks = [r[j] for r in res]
        ref = refs[GG.tag(c)]
        where = "dropedge%s/%s/P%d" % (case, GG.tag(c), P)
        for r in ranks:
            assert r["tag"] == GG.tag(c) and len(r["grads"]) == len(r["logits"]) == len(r["loss"]) == EPOCHS, where
        logits = [rows(ranks, lambda r, s=s: r["logits"][s], GG.N) for s in range(EPOCHS)]
        assert not np.array_equal(logits[0], logits[1]), where + ": the second step drew the first step's mask"
        for s, rec in enumerate(ref["steps"]):
            m64, twin = rec["m64"], rec["twin"]
            at = "%s/step%d" % (where, s)
            held_to_fixture(at, "loss", np.array([sum(r["loss"][s] for r in ranks)]), twin["loss"].numpy().reshape(1), m64["loss"].numpy().reshape(1))
            held_to_fixture(at, "logits", logits[s], twin["logits"].numpy(), m64["logits"].numpy())
            held += 2
            for i, r in enumerate(ranks):
                for name in ref["params"]:
                    held_to_fixture(at + "/rank%d" % i, "grad " + name.split(".", 1)[1], r["grads"][s][name], twin["grads"][name].numpy(),
                                    m64["grads"][name].numpy())
                    held += 1
        ev = rows(ranks, lambda r: r["eval_logits"], GG.N)
        held_to_fixture(where, "eval logits", ev, ref["eval"]["twin"]["logits"].numpy(), ref["eval"]["m64"]["logits"].numpy())
        held += 1
    return held
