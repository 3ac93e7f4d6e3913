"""Definitions, float64 reference and worker processes of tests/test_gat_tail.py and tests/test_gat_tail_gpu.py (spawn start method),
in the pattern of tests/_rootweight_workers.py and tests/_gradgrid_workers.py whose data sets and spawn helpers they share.

``tail32`` / ``tail_backward32`` are the statement of csrc/pgcn_gat_tail.hip in fp32 numpy, one rounding per operation in the kernel's
order.  Where ELU takes its negative branch the statement uses float64 expm1 rounded to fp32: the device's expm1f may differ from that
by its accuracy class, so ``tail32`` also returns the mask of the elements where no expm1 is involved (bit-equality is asked there).

``model64`` is a dense GAT classifier of standard mode in torch double with torch's own autograd (LeakyReLU 0.2, softmax over the
stored entries, ELU, head mean, bias, the keep masks of dropout.keep_mask); the same function in float32 is the TWIN, and
conftest.held_to_fixture holds the model to max(1e-5, twice the twin's distance from the double run)."""
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

import _batchnorm_workers as BW  # noqa: E402
import _gradgrid_workers as GW  # noqa: E402
import _nodeclass_workers as NW  # noqa: E402
from _rootweight_workers import dbias_error_and_bound  # noqa: E402,F401

DROPOUT, DROPOUT_SEED = 0.5, 11
SLOPE = 0.2
SETS = NW.SETS
f32 = np.float32


# ---- the definition in numpy ---------------------------------------------------------------------------------------------------------------

def tail32(X, heads, d, mean, bias, act, keep=None, scale=1.0):
    """(Y, exact): the forward in fp32 numpy.  r = the heads added in index order, then * (1.0f / heads) (not for one head), or X;
    t = r + bias (None: absent); act: t > 0 ? t : fp32(expm1(double(t))); keep (None: no dropout): keep ? a * scale : 0.
    ``exact``: the elements whose value involves no expm1."""
    X = np.asarray(X, f32)
    r = X
    if mean:
        r = X[:, :d]
        for k in range(1, heads):
            r = (r + X[:, k * d:(k + 1) * d]).astype(f32)
        if heads > 1:
            r = (r * (f32(1.0) / f32(heads))).astype(f32)
    t = (r + np.asarray(bias, f32)[None, :]).astype(f32) if bias is not None else r
    exact = np.ones(t.shape, bool)
    a = t
    if act:
        exact = t > 0
        with np.errstate(over="ignore", invalid="ignore"):
            a = np.where(exact, t, np.expm1(t.astype(np.float64)).astype(f32)).astype(f32)
    if keep is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            a = np.where(keep, (a * f32(scale)).astype(f32), f32(0)).astype(f32)
        exact = exact | ~keep
    return a.copy(), exact


def tail_backward32(G, Y, heads, d, mean, act, keep=None, scale=1.0):
    """(dX, Gm) in fp32 numpy: deriv = Y > 0 ? 1 : Y * (1.0f / scale) + 1.0f (act), Gm = keep ? (G * scale) * deriv : 0, dX = Gm
    (* (1.0f / heads) with mean, not for one head) for every head."""
    G = np.asarray(G, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        gm = (G * f32(scale)).astype(f32) if keep is not None else G
        if act:
            Y = np.asarray(Y, f32)
            e = (Y * (f32(1.0) / f32(scale))).astype(f32) if keep is not None else Y
            gm = np.where(Y > 0, gm, (gm * (e + f32(1.0)).astype(f32)).astype(f32)).astype(f32)
        if keep is not None:
            gm = np.where(keep, gm, f32(0)).astype(f32)
        dX = gm
        if mean:
            dX = np.tile((gm * (f32(1.0) / f32(heads))).astype(f32) if heads > 1 else gm, (1, heads))
    return dX.copy(), gm.copy()


def ulps(got, want):
    """|got - want| in units of want's fp32 spacing (0 where both are equal, non-finite pairs included)."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore", over="ignore"):
        dist = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    return np.where(same, 0.0, dist)


# ---- the model in torch double --------------------------------------------------------------------------------------------------------------

def options(K=2, hidden=8, Ko=1, bias=False, elu=True, dropout=0.0, task="single", nlayers=2):
    return {"K": int(K), "hidden": int(hidden), "Ko": int(Ko), "bias": bool(bias), "elu": bool(elu), "dropout": float(dropout),
            "task": task, "nlayers": int(nlayers)}


def tag(o):
    return "K%dh%dKo%d%s%s%s-%s" % (o["K"], o["hidden"], o["Ko"], "+bias" if o["bias"] else "", "+elu" if o["elu"] else "",
                                    "+drop" if o["dropout"] > 0 else "", o["task"])


def classes_of(data, o):
    return int(data["labels"].shape[1]) if o["task"] == "multilabel" else int(data["labels"].max()) + 1


def layer_shapes(data, o):
    """[(fin, projected width, heads, output width)] per layer."""
    C, L = classes_of(data, o), o["nlayers"]
    fin = data["X"].shape[1]
    out = [(fin if l == 0 else o["hidden"], o["hidden"], o["K"], o["hidden"]) for l in range(L - 1)]
    return out + [(fin if L == 1 else o["hidden"], o["Ko"] * C, o["Ko"], C)]


def initial_params(data, o, seed):
    """{name: fp32 tensor} in the model's parameter order: seeded values, the biases away from zero so that a pass that ignored
    them shows."""
    rng = np.random.default_rng(1000 + seed)
    p = {}
    for l, (fin, width, K, fout) in enumerate(layer_shapes(data, o)):
        p["%d.linear.weight" % l] = torch.from_numpy((rng.standard_normal((width, fin)) * 0.3).astype(f32))
        p["%d.attention" % l] = torch.from_numpy((rng.standard_normal((2 * width // K, K)) * 0.3).astype(f32))
        if o["bias"]:
            p["%d.bias" % l] = torch.from_numpy((rng.standard_normal(fout) * 0.3).astype(f32))
    return p


def model64(data, params, o, step, training=True, dtype=torch.float64):
    """(loss, logits, {name: grad}) on the whole graph, one process."""
    from conftest import pkg
    D = pkg("dropout")
    A = data["A"]
    n = A.shape[0]
    edge = torch.from_numpy(A.toarray() != 0)
    h = torch.from_numpy(data["X"]).to(dtype)
    p = {k: v.detach().to(dtype).clone().requires_grad_(training) for k, v in params.items()}
    thr, scale = D.threshold(o["dropout"])
    shapes = layer_shapes(data, o)
    for l, (fin, width, K, fout) in enumerate(shapes):
        last = l == len(shapes) - 1
        d = width // K
        Z = (h @ p["%d.linear.weight" % l].t()).view(n, K, d)
        a = p["%d.attention" % l]
        s1 = torch.einsum("nkd,dk->nk", Z, a[:d])
        s2 = torch.einsum("nkd,dk->nk", Z, a[d:])
        e = F.leaky_relu(s1.t().unsqueeze(2) + s2.t().unsqueeze(1), SLOPE)                  # K x n x n: e[k, i, j] = s1[i] + s2[j]
        e = torch.where(edge.unsqueeze(0), e, torch.full((), -float("inf"), dtype=dtype))
        alpha = torch.softmax(e, 2)
        alpha = torch.where(edge.unsqueeze(0), alpha, torch.zeros((), dtype=dtype))        # (a row without entries: zeros, not NaN)
        out = torch.einsum("kij,jkd->ikd", alpha, Z)
        t = out.mean(1) if last else out.reshape(n, width)
        if o["bias"]:
            t = t + p["%d.bias" % l]
        if last:
            logits = t
            break
        if o["elu"]:
            t = F.elu(t)
        if training and o["dropout"] > 0.0:
            keep = D.keep_mask(o.get("dropout_seed", DROPOUT_SEED), step, l, np.arange(n), fout, thr)
            t = torch.where(keep, t * scale, torch.zeros((), dtype=dtype))
        h = t
    train = torch.from_numpy(data["split"] == 1)
    if o["task"] == "multilabel":
        y = torch.from_numpy(data["labels"] == 1)[train].to(dtype)
        loss = F.binary_cross_entropy_with_logits(logits[train], y, reduction="sum") / (int(train.sum()) * logits.shape[1])
    else:
        loss = F.cross_entropy(logits[train], torch.from_numpy(data["labels"])[train])
    grads = {}
    if training:
        names = list(p)
        grads = dict(zip(names, (g.detach() for g in torch.autograd.grad(loss, [p[k] for k in names]))))
    return loss.detach(), logits.detach(), grads


def accuracy(logits, data):
    """{set: (mean loss, accuracy)} of single-label logits, in double."""
    lg = logits.double()
    y, split = torch.from_numpy(data["labels"]), data["split"]
    out = {}
    for code, name in ((1, "train"), (2, "val"), (3, "test")):
        m = torch.from_numpy(split == code)
        out[name] = (float(F.cross_entropy(lg[m], y[m])), float((lg[m].argmax(1) == y[m]).double().mean()))
    return out


def reference(data, o, seed, epochs, lr):
    """The training run in double and as the fp32 twin: {"params", "m64" / "twin": {"steps": [{loss, logits, grads}], "eval":
    [logits after each update], "final": logits after the last}}; Adam with torch's defaults (lr = 0: the parameters stay)."""
    params = initial_params(data, o, seed)
    out = {"params": params, "seed": seed}
    for key, dt in (("m64", torch.float64), ("twin", torch.float32)):
        cur = {k: v.to(dt).clone() for k, v in params.items()}
        opt = torch.optim.Adam(list(cur.values()), lr=lr) if lr > 0 else None
        steps, evals = [], []
        for step in range(epochs):
            loss, logits, grads = model64(data, cur, o, step, True, dt)
            steps.append({"loss": loss, "logits": logits, "grads": grads})
            if opt is not None:
                for k, v in cur.items():
                    v.grad = grads[k].clone()
                opt.step()
            evals.append(model64(data, cur, o, epochs, False, dt)[1])
        out[key] = {"steps": steps, "eval": evals}
    return out


# ---- the workers ----------------------------------------------------------------------------------------------------------------------------

def _module(gpu):
    from conftest import pkg
    M = pkg("PGAT")
    if gpu:
        M._kernel_provider = None
    else:
        from oracle_kernels import OracleKernels
        M._kernel_provider = OracleKernels()
    M._exchanger = None
    M.mode = "standard"
    return M


def grad_worker(rank, P, port, paths, gpu, q, jobs=(), n=None, steps=2):
    """Rank `rank` of `P` over gloo: per job {"opts", "params"} the model of PGAT.build_classifier -- built layer by layer here, since
    run() always asks for ELU -- with the job's parameters, ``steps`` training passes at fixed parameters (the dropout step advances
    in between): this rank's loss, its rows of the logits, every parameter's gradient after the ranks' sum; then the eval logits."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from conftest import pkg, read_partvec
    from scipy.io import mmread
    M = _module(gpu)
    D = pkg("dropout")
    dist.init_process_group("gloo", rank=rank, world_size=P)
    M.myrank, M.world_size = rank, P
    M.device = torch.device("cuda:0") if gpu else torch.device("cpu")
    if gpu:
        torch.cuda.set_device(0)
    A = mmread(paths["A"])
    part = read_partvec(paths["pv%d" % P])
    M.send_map, M.recv_map = M.compute_communication_maps(A, part, rank, P)
    eng = M.get_partitiont_of_adjacency_matrix(A, part, rank)
    own = eng.part.owned.cpu().numpy()
    results = []
    for job in jobs:
        o = job["opts"]
        multilabel = o["task"] == "multilabel"
        load = M._nodedata.load_multilabel if multilabel else M._nodedata.load
        data = load(paths[o["task"]]["features"], paths[o["task"]]["labels"], paths[o["task"]]["split"], eng.part.owned, n, device=M.device)
        state = D.DropoutState(DROPOUT_SEED, M.device) if o["dropout"] > 0 else None
        widths = [data.fin] + [o["hidden"]] * (o["nlayers"] - 1)
        layers = [M.PGAT(eng, widths[l], o["hidden"], heads=o["K"], bias=o["bias"], activation="elu" if o["elu"] else None,
                         dropout=o["dropout"], layer=l, state=state) for l in range(o["nlayers"] - 1)]
        layers.append(M.PGAT(eng, widths[-1], o["Ko"] * data.classes, heads=o["Ko"], concat=False, bias=o["bias"]))
        model = torch.nn.Sequential(*layers).to(M.device)
        names = [k for k, _ in model.named_parameters()]
        assert sorted(names) == sorted(job["params"]), (names, list(job["params"]))
        with torch.no_grad():
            for k, prm in model.named_parameters():
                prm.copy_(torch.from_numpy(job["params"][k]))
        rec = {"tag": tag(o), "own": own, "loss": [], "logits": [], "grads": [], "hip": type(eng.k).__name__}
        for s in range(steps):
            model.train()
            model.zero_grad()
            logits = model(data.features)
            loss, _ = (M.masked_bce_loss if multilabel else M.masked_loss)(logits, data.labels, data.split, data.counts[1])
            loss.backward()
            M.sum_gradients(model)
            rec["loss"].append(float(loss.detach().double().cpu()))
            rec["logits"].append(logits.detach().cpu().numpy())
            rec["grads"].append({k: prm.grad.detach().cpu().numpy().copy() for k, prm in model.named_parameters()})
            if state is not None:
                state.advance()
        model.eval()
        with torch.no_grad():
            rec["eval_logits"] = model(data.features).cpu().numpy()
        results.append(rec)
    if gpu:
        torch.cuda.synchronize()
    q.put({"rank": rank, "results": results})
    dist.barrier()
    dist.destroy_process_group()


def run_worker(rank, P, port, paths, gpu, q, opts=None, params=None, epochs=3, lr=0.01, optimizer=None):
    """PGAT.run(features=..., ...) on rank `rank` of `P` over gloo with the job's parameters written in after initialisation
    (``params`` None: the run keeps what it drew; ``drawn`` reports that either way): the
    history, stdout, this rank's loss / logits / reduced gradients of every step and the eval logits after the run."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    M = _module(gpu)
    M.heads = opts["K"]
    cur = {"grads": [], "logits": [], "loss": []}
    init = M.initiliaze_parameters

    def initialise(model):
        init(model)
        cur["drawn"] = {k: prm.detach().cpu().numpy().copy() for k, prm in model.named_parameters()}
        if params is not None:
            with torch.no_grad():
                for k, prm in model.named_parameters():
                    prm.copy_(torch.from_numpy(params[k]))
        cur["model"] = model
        model.register_forward_hook(lambda m, a, out: cur["logits"].append(out.detach().cpu().numpy()) if m.training else None)

    adam_step = torch.optim.Adam.step

    def step(self, *a, **kw):
        cur["grads"].append({k: prm.grad.detach().cpu().numpy().copy() for k, prm in cur["model"].named_parameters()})
        return adam_step(self, *a, **kw)

    def with_loss(f):
        def g(*a, **kw):
            out = f(*a, **kw)
            cur["loss"].append(float(out[0].detach().double().cpu()))
            return out
        return g

    M.initiliaze_parameters = initialise
    torch.optim.Adam.step = step
    M._pgcn.masked_loss, M._pgcn.masked_bce_loss = with_loss(M._pgcn.masked_loss), with_loss(M._pgcn.masked_bce_loss)
    got = {}

    def fn(r, size, nlayers, nfeatures, path_A, path_partvec, backend, **kw):
        buf = io.StringIO()
        with redirect_stdout(buf):
            model = M.run(r, size, nlayers, nfeatures, path_A, path_partvec, backend, **kw)
        eng = M._engine_current
        load = M._nodedata.load_multilabel if opts["task"] == "multilabel" else M._nodedata.load
        data = load(kw["features"], kw["labels"], kw["split"], eng.part.owned, int(np.load(kw["split"]).shape[0]), device=M.device)
        model.eval()
        with torch.no_grad():
            ev = model(data.features).cpu().numpy()
        got.update(history=model.history, best=model.best, widths=model.widths, stdout=buf.getvalue(), own=eng.part.owned.cpu().numpy(),
                   names=[k for k, _ in model.named_parameters()], eval_logits=ev, hip=type(eng.k).__name__,
                   fused=[bool(m._state.fused) for m in model])

    t = paths[opts["task"]]
    kw = dict(features=t["features"], labels=t["labels"], split=t["split"], hidden=opts["hidden"], out_heads=opts["Ko"], epochs=epochs,
              lr=lr, task=opts["task"])
    if opts["dropout"] > 0:
        kw.update(dropout=opts["dropout"], dropout_seed=DROPOUT_SEED)
    if opts["bias"]:
        kw["bias"] = True
    if optimizer is not None:
        kw["optimizer"] = optimizer
    M.init_process(rank, P, fn, opts["nlayers"], 0, paths["A"], paths["pv%d" % P], "gloo", kw)
    got.update(rank=rank, grads=cur["grads"], logits=cur["logits"], loss=cur["loss"], drawn=cur["drawn"])
    q.put(got)


def spawn(worker, P, paths, gpu, **kw):
    """BW.spawn_run (ranks that die answer at once; on the GPU the ranks share device 0) with one of this file's workers."""
    saved = BW.run_worker
    BW.run_worker = worker
    try:
        return sorted(BW.spawn_run(P, paths, gpu, **kw), key=lambda r: r["rank"])
    finally:
        BW.run_worker = saved


def rows(per_rank, pick, n):
    out = None
    for r in per_rank:
        v = pick(r)
        out = np.zeros((n,) + v.shape[1:], v.dtype) if out is None else out
        out[r["own"]] = v
    return out


def hold_steps(where, ranks, ref, n, steps):
    """Loss, logits and every reduced gradient of every step against model64 and its twin; returns how many tensors were held."""
    from conftest import held_to_fixture
    held = 0
    for s in range(steps):
        m64, twin = ref["m64"]["steps"][s], ref["twin"]["steps"][s]
        at = "%s/step%d" % (where, s)
        held_to_fixture(at, "loss", np.array([sum(r["loss"][s] for r in ranks)]), twin["loss"].numpy().reshape(1), m64["loss"].numpy().reshape(1))
        held_to_fixture(at, "logits", rows(ranks, lambda r, s=s: r["logits"][s], n), twin["logits"].numpy(), m64["logits"].numpy())
        held += 2
        for i, r in enumerate(ranks):
            assert sorted(r["grads"][s]) == sorted(ref["params"]), (at, sorted(r["grads"][s]))
            for name in ref["params"]:
                held_to_fixture(at + "/rank%d" % i, "grad " + name, r["grads"][s][name], twin["grads"][name].numpy(), m64["grads"][name].numpy())
                held += 1
    return held


# ---- data -----------------------------------------------------------------------------------------------------------------------------------

def make_datasets(dirname):
    """GW.make_datasets (the planted single-label and multi-label problems at n = 1100 on one graph) as ONE paths dictionary:
    {"A", "pv1" .., "single": {features, labels, split}, "multilabel": {...}} and {task: arrays}."""
    sets = GW.make_datasets(dirname)
    paths = {k: v for k, v in sets["single"][0].items() if k == "A" or k.startswith("pv")}
    for task in GW.TASKS:
        paths[task] = {k: sets[task][0][k] for k in ("features", "labels", "split")}
    assert (sets["single"][1]["A"] != sets["multilabel"][1]["A"]).nnz == 0
    return paths, {task: sets[task][1] for task in GW.TASKS}


def make_karate(dirname):
    """Zachary's club with planted labels: two classes by the sign of (id - 16.5), features = a class centre + noise, a split that
    leaves two rows in no set; part vectors for 1 and 2 ranks.  Returns (paths, {"single": arrays})."""
    import scipy.sparse as sp
    from conftest import gpath, read_partvec
    from scipy.io import mmread
    A = sp.csr_matrix(mmread(gpath("karate.A.mtx")))
    A.sum_duplicates()
    n = A.shape[0]
    rng = np.random.default_rng(34)
    y = (np.arange(n) >= n // 2).astype(np.int64)
    centres = rng.standard_normal((2, 6))
    X = (centres[y] + 0.8 * rng.standard_normal((n, 6))).astype(f32)
    split = np.array([1, 2, 3] * 12, np.uint8)[:n]
    split[[5, 20]] = 0
    labels = np.where(split == 0, -1, y).astype(np.int64)
    t = {k: os.path.join(dirname, k + ".npy") for k in ("features", "labels", "split")}
    np.save(t["features"], X)
    np.save(t["labels"], labels)
    np.save(t["split"], split)
    paths = {"A": gpath("karate.A.mtx"), "pv1": gpath("karate.mtx.1.rp"), "pv2": gpath("karate.mtx.2.rp"), "single": t}
    assert len(read_partvec(paths["pv2"])) == n
    return paths, {"single": {"A": A, "X": X, "labels": labels, "split": split}}
