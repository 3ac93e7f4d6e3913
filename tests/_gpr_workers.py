"""The definition of the generalised-PageRank propagation with learned hop weights (GPR-GNN) in numpy fp32 and in float64, the whole
model with it in torch double, and the worker processes of tests/test_gpr.py and tests/test_gpr_gpu.py (spawn start method), in the
pattern of tests/_propagate_workers.py, whose helpers these reuse.

Definition (csrc/pgcn_gpr.hip, engine.AggregationEngine.gpr / gpr_backward), g = gamma as fp32, every operation rounded on its own:
forward  OUT^0 = fl(g_0 H), S^k = A S^{k-1} (S^0 = H), OUT^k = fl(OUT^{k-1} + fl(g_k S^k));
backward T^0 = G, T^k = A^T T^{k-1}, D^0 = fl(g_0 G), D^k = fl(D^{k-1} + fl(g_k T^k)), dH = D^K,
         dgamma_k = fl32(sum_{i,c} (double)T^k[i,c] (double)H[i,c]) over a rank's rows; the ranks' values are partial sums.

Bounds.  TOL is the 1e-5 of tests/_propagate_workers.py, the relative error (conftest.rel_err) allowed to ONE aggregation.  With
sum |g_k| <= 1 and ||A||_2 <= 1 (asserted: D^-1/2 (P + I) D^-1/2 of a symmetric pattern) OUT and dH are held to (K + 1) TOL against
float64: hop k carries k aggregations' errors and two roundings and enters with weight |g_k|, and the weights sum to at most 1 -- the
argument of _propagate_workers.py.  dgamma_k is a dot product of T^k, which carries k aggregations' errors, with H, plus one fp32
rounding: |err| <= (k + 1) TOL ||T64^k||_F ||H||_F (Cauchy-Schwarz).  Two partitioned runs are compared at twice the bounds."""
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

import _gradgrid_workers as GG  # noqa: E402
import _gat_tail_workers as TW  # noqa: E402
import _propagate_workers as W  # noqa: E402

TOL = W.TOL
N, FIN, CLASSES, HIDDEN, NLAYERS, EPOCHS = W.N, W.FIN, W.CLASSES, W.HIDDEN, W.NLAYERS, W.EPOCHS
DROPOUT, DROPOUT_SEED = W.DROPOUT, W.DROPOUT_SEED
KARATE_CASES = [(K, C) for K in (1, 3, 10) for C in (1, 7, 16)]
PATTERN_CASES = [(K, C) for K in (1, 2, 10) for C in (3, 7, 41, 128)]
PATTERN_CHUNK = W.PATTERN_CHUNK
GPR_METHODS = ("gpr_step", "gpr_step_backward", "gpr_dot_finish", "gpr_workspace")
GAMMA = "%d.gamma" % NLAYERS                   # the parameter's name in the model of run(nlayers=NLAYERS, gpr=K)
bits, rows, make_pattern, make_dataset, make_cora, sym_normalised = W.bits, W.rows, W.make_pattern, W.make_dataset, W.make_cora, W.sym_normalised


# ---- the definition ---------------------------------------------------------------------------------------------------------------

def step_np(X, Yin, g):
    """fl(Yin + fl(g X)) in numpy fp32 (Yin None: fl(g X)): every operation of numpy rounds on its own."""
    gx = np.float32(g) * np.asarray(X, np.float32)
    return gx if Yin is None else np.asarray(Yin, np.float32) + gx


def ppr_gamma(K, alpha):
    """The "ppr" initialisation: Python doubles, rounded to fp32 once."""
    return np.array([alpha * (1.0 - alpha) ** k for k in range(K)] + [(1.0 - alpha) ** K], np.float64).astype(np.float32)


def gpr64(Ad, H, gamma):
    """sum_k gamma_k A^k H in float64 on the dense matrix."""
    Z = np.asarray(H, np.float64)
    out = float(gamma[0]) * Z
    for k in range(1, len(gamma)):
        Z = Ad @ Z
        out = out + float(gamma[k]) * Z
    return out


def gpr_backward64(Ad, G, H, gamma):
    """(dH, dgamma, [||T^k||_F]) in float64."""
    T, H = np.asarray(G, np.float64), np.asarray(H, np.float64)
    D, dg, norms = float(gamma[0]) * T, [float((T * H).sum())], [float(np.linalg.norm(T))]
    for k in range(1, len(gamma)):
        T = Ad.T @ T
        D = D + float(gamma[k]) * T
        dg.append(float((T * H).sum()))
        norms.append(float(np.linalg.norm(T)))
    return D, np.array(dg), norms


def seeded_case(n, K, C):
    """The global H and G of one case and its gamma: both signs, scaled to sum |gamma_k| = 1 (in double, then rounded; the fp32 sum is
    asserted to stay within 1 + 2^-20)."""
    rng = np.random.default_rng([23, K, C])
    H, G = rng.random((n, C), dtype=np.float32) * 2 - 1, rng.random((n, C), dtype=np.float32) * 2 - 1
    g = rng.uniform(0.2, 1.0, K + 1) * np.where(np.arange(K + 1) % 2 == 1, -1.0, 1.0)
    g = (g / np.abs(g).sum()).astype(np.float32)
    assert (g < 0).any() and (g > 0).any() and float(np.abs(g.astype(np.float64)).sum()) <= 1.0 + 2.0 ** -20
    return H, G, g


def dot_bound(ref, t, h):
    """The kernel-level bound of one dgamma against np.dot in float64 on the same fp32 operands: one fp32 rounding plus the bound of a
    double sum of n f exact products."""
    t, h = np.asarray(t, np.float64).reshape(-1), np.asarray(h, np.float64).reshape(-1)
    return 2.0 ** -23 * abs(ref) + t.size * 2.0 ** -52 * float(np.abs(t * h).sum())


# ---- engine level -----------------------------------------------------------------------------------------------------------------

def _provider(M, gpu, chunk=None):
    """W._provider with the gpr kernels hidden for gpu == "composed"."""
    from conftest import pkg
    if gpu == "composed":
        K = pkg("kernels")

        class NoGpr(K.HipKernels):
            def __getattribute__(self, name):
                if name in GPR_METHODS:
                    raise AttributeError(name)
                return super().__getattribute__(name)
        M._kernel_provider = NoGpr(torch.device("cuda:0"), **({"chunk": chunk} if chunk else {}))
        M._exchanger = None
    else:
        W._provider(M, gpu, chunk)


def engine_worker(rank, P, port, paths, gpu, q, cases=(), normalize=None, pv=None, chunk=None, no_composed=False):
    """gpr / gpr_backward of rank `rank` of `P` over gloo on the seeded global operands of every case (K, C), with and without dH.
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
        E.gpr_step_composed = E.gpr_step_backward_composed = refuse
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
        for K, C in cases:
            Hg, Gg, g = seeded_case(n, K, C)
            H, G, gamma = (torch.from_numpy(x).to(M.device) for x in (Hg[own], Gg[own], g))
            before = dict(eng.stats)
            OUT = eng.gpr(H, gamma)
            mid = dict(eng.stats)
            D, dg = eng.gpr_backward(G, H, gamma, True)
            after = dict(eng.stats)
            none, dg2 = eng.gpr_backward(G, H, gamma, False)
            assert none is None and torch.equal(dg, dg2) and dg.dtype is torch.float32 and tuple(dg.shape) == (K + 1,)
            mark = dict(eng.stats)
            eng.forward(H)
            one = dict(eng.stats)
            got["cases"].append(dict(K=K, C=C, OUT=OUT.cpu().numpy(), D=D.cpu().numpy(), dg=dg.cpu().numpy(),
                                     fwd={k: mid[k] - before[k] for k in mid}, bwd={k: after[k] - mid[k] for k in mid},
                                     one={k: one[k] - mark[k] for k in mid}))
        got["new_attributes"] = sorted(set(vars(eng)) - held)

    M.init_process(rank, P, fn, NLAYERS, HIDDEN, paths["A"], paths[pv or "pv%d" % P], "gloo", normalize)
    q.put(got)


def spawn_engine(P, paths, gpu, **kw):
    return TW.spawn(engine_worker, P, paths, gpu, **kw)


def check_engine(res, Ad, cases, label=""):
    """Every case of one worker group against float64 on the dense matrix ``Ad``: OUT and dH within (K + 1) TOL, every dgamma_k (the
    ranks' summed) within (k + 1) TOL ||T64^k||_F ||H||_F, the exchange volume of K aggregations, nothing kept on the engine.  Prints
    every measured figure.  Returns {case: (OUT, D, dgamma)} gathered over the ranks."""
    from conftest import rel_err
    n = Ad.shape[0]
    assert np.array_equal(Ad, Ad.T) and np.linalg.norm(Ad, 2) <= 1.0 + 1e-6, "the test matrix is not symmetric with norm <= 1"
    out = {}
    assert len(res[0]["cases"]) == len(cases)
    for i, (K, C) in enumerate(cases):
        Hg, Gg, g = seeded_case(n, K, C)
        OUT, D = rows(res, lambda r: r["cases"][i]["OUT"], n), rows(res, lambda r: r["cases"][i]["D"], n)
        dg = np.sum([r["cases"][i]["dg"].astype(np.float64) for r in res], axis=0)
        assert OUT.dtype == D.dtype == np.float32 and OUT.shape == D.shape == (n, C) and dg.shape == (K + 1,)
        D64, dg64, norms = gpr_backward64(Ad, Gg, Hg, g)
        eo, ed = rel_err(OUT, gpr64(Ad, Hg, g)), rel_err(D, D64)
        bound = (K + 1) * TOL
        hn = float(np.linalg.norm(Hg.astype(np.float64)))
        edg = [abs(dg[k] - dg64[k]) / (norms[k] * hn) for k in range(K + 1)]
        print("%s P=%d K=%d C=%d: forward %.3g backward %.3g (bound %.3g) dgamma/(k+1) %.3g (bound %.3g)"
              % (label, len(res), K, C, eo, ed, bound, max(e / (k + 1) for k, e in enumerate(edg)), TOL), flush=True)
        assert eo <= bound and ed <= bound, (label, K, C, eo, ed, bound)
        for k in range(K + 1):
            assert edg[k] <= (k + 1) * TOL, (label, K, C, k, edg[k])
        for r in res:
            c = r["cases"][i]
            assert c["fwd"] == {k: K * v for k, v in c["one"].items()}, (c["fwd"], c["one"])         # K exchanges of one aggregation each
            assert c["bwd"]["send_volume"] == c["fwd"]["recv_volume"] and c["bwd"]["recv_volume"] == c["fwd"]["send_volume"]
        out[(K, C)] = (OUT, D, dg)
    for r in res:
        assert r["new_attributes"] == [], r["new_attributes"]
    return out


def check_same(a, b, Ad, cases, label=""):
    """Two partitioned runs of the same cases agree with each other at twice the bounds."""
    from conftest import rel_err
    n = Ad.shape[0]
    for K, C in cases:
        for x, y, what in zip(a[(K, C)][:2], b[(K, C)][:2], ("forward", "backward")):
            e = rel_err(x, y)
            print("%s K=%d C=%d %s: %.3g between the runs" % (label, K, C, what, e), flush=True)
            assert e <= 2 * (K + 1) * TOL, (label, K, C, what, e)
        Hg, Gg, g = seeded_case(n, K, C)
        norms = gpr_backward64(Ad, Gg, Hg, g)[2]
        hn = float(np.linalg.norm(Hg.astype(np.float64)))
        for k in range(K + 1):
            assert abs(a[(K, C)][2][k] - b[(K, C)][2][k]) <= 2 * (k + 1) * TOL * norms[k] * hn, (label, K, C, k)


# ---- model level ------------------------------------------------------------------------------------------------------------------

def config(dense, bias=False, dropout=0.0, K=10, alpha=0.1):
    return W.config(dense, bias, dropout, K, alpha)


def model_configs():
    """Dense layers + gpr=10, and GCN layers + bias + dropout + gpr=3."""
    return [config(True, K=10), config(False, bias=True, dropout=DROPOUT, K=3)]


def tag(c):
    return "gpr-" + W.tag(c)


def initial_params(widths, c, seed):
    """GG.initial_params and gamma: the "ppr" initialisation with every other weight's sign turned, so that both signs are trained."""
    p = GG.initial_params(widths, c, seed)
    p[GAMMA] = torch.from_numpy(ppr_gamma(c["K"], c["alpha"]) * np.where(np.arange(c["K"] + 1) % 2 == 1, -1, 1).astype(np.float32))
    return p


def model64(data, widths, params, c, step, dtype=torch.float64, trace=None):
    """(loss, logits after the propagation, {name: grad}) of run(normalize="sym", gpr=K[, dense_layers]) on the whole graph in training
    mode: stock operations, torch's own autograd, gamma's gradient included.  ``trace`` receives every ReLU input."""
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
    g = p[GAMMA]
    s, logits = z, g[0] * z
    for k in range(1, c["K"] + 1):
        s = Ad @ s
        logits = logits + g[k] * s
    train = torch.from_numpy(data["split"] == 1)
    loss = F.cross_entropy(logits[train], torch.from_numpy(data["labels"])[train])
    names = list(p)
    grads = dict(zip(names, (x.detach() for x in torch.autograd.grad(loss, [p[k] for k in names]))))
    return loss.detach(), logits.detach(), grads


_refs = {}


def reference(data, c):
    """W.reference for the gpr model: the seed rule of the gradient grid (no doubtful ReLU input), asserted."""
    key = tag(c)
    if key not in _refs:
        widths = W.widths_of(c)
        for seed in GG.SEEDS:
            params = initial_params(widths, c, seed)
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
    """W.model_worker's protocol for run(epochs=2, lr=0.0, optimizer="torch", normalize="sym", nlayers=3, gpr=K, ...)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M = pkg("PGCN")
    W._provider(M, gpu)
    cur = {}
    init = M.initiliaze_parameters

    def initialise(model):
        cur["drawn"] = model[-1].gamma.detach().cpu().numpy().copy()
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
                      optimizer="torch", gpr=c["K"], gpr_alpha=c["alpha"])
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
                                loss=cur["loss"], own=eng.part.owned.cpu().numpy(), hip=type(eng.k).__name__, drawn=cur["drawn"],
                                stats=dict(eng.stats)))

    M.init_process(rank, P, fn, NLAYERS, HIDDEN, paths["A"], paths["pv%d" % P], "gloo", "sym")
    q.put({"rank": rank, "results": results})


def spawn_model(P, paths, gpu, configs, data):
    jobs = [{"config": c, "seed": reference(data, c)["seed"], "params": {k: v.numpy() for k, v in reference(data, c)["params"].items()}}
            for c in configs]
    return [r["results"] for r in TW.spawn(model_worker, P, paths, gpu, jobs=jobs)]


def check_models(data, configs, res, case=""):
    """Loss, logits and every reduced parameter gradient -- gamma's included -- of both steps against the double model through
    conftest.held_to_fixture (model / fp32 twin / double).  Returns how many tensors were held."""
    from conftest import held_to_fixture
    P, held = len(res), 0
    for j, c in enumerate(configs):
        ref = reference(data, c)
        ranks = [r[j] for r in res]
        where = "gpr%s/%s/P%d" % (case, tag(c), P)
        for r in ranks:
            assert r["tag"] == tag(c) and r["modules"] == ["PGCN"] * NLAYERS + ["Gpr"], (where, r["modules"])
            assert sorted(r["names"]) == sorted(GG.parameter_names(ref["widths"], c) + [GAMMA]), (where, r["names"])
            assert len(r["grads"]) == len(r["logits"]) == len(r["loss"]) == EPOCHS, where
            assert np.array_equal(bits(r["drawn"]), bits(ppr_gamma(c["K"], c["alpha"]))), where       # what the module drew itself
        for s, rec in enumerate(ref["steps"]):
            m64, twin = rec["m64"], rec["twin"]
            at = "%s/step%d" % (where, s)
            held_to_fixture(at, "loss", np.array([sum(r["loss"][s] for r in ranks)]), twin["loss"].numpy().reshape(1),
                            m64["loss"].numpy().reshape(1))
            held_to_fixture(at, "logits", rows(ranks, lambda r, s=s: r["logits"][s], N), twin["logits"].numpy(), m64["logits"].numpy())
            held += 2
            for i, r in enumerate(ranks):
                assert GAMMA in ref["params"]
                for name in ref["params"]:
                    held_to_fixture(at + "/rank%d" % i, "grad " + name.split(".", 1)[1], r["grads"][s][name], twin["grads"][name].numpy(),
                                    m64["grads"][name].numpy())
                    held += 1
    return held


def train64(data, c, params, steps, lr):
    """{name: float64 array} after ``steps`` steps of torch's Adam in double on the gradients of ``model64`` (no dropout)."""
    assert c["dropout"] == 0.0
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam(list(p.values()), lr=lr)
    for s in range(steps):
        grads = model64(data, W.widths_of(c), {k: v.detach() for k, v in p.items()}, c, s)[2]
        for k, v in p.items():
            v.grad = grads[k].clone()
        opt.step()
    return {k: v.detach().numpy() for k, v in p.items()}


def spawn_cpu_jobs(P, paths, jobs):
    return W.spawn_cpu_jobs(P, paths, jobs)
