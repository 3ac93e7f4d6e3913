"""The whole model of PGCN.run(features=..., ...) stated once in torch double, the option grid, the seed rule and the worker processes of
tests/test_gradgrid.py and tests/test_gradgrid_gpu.py (spawn start method), in the pattern of tests/_layernorm_workers.py.

``model64`` uses stock operations and torch's own autograd: no backward formula is written here, and of the package it takes
dropout.keep_mask and dropout.threshold alone (the integer host statement of the masks).  The same function in float32 is the TWIN:
its distance from the double run is what fp32 costs the reference itself, and conftest.held_to_fixture holds the model to
max(1e-5, twice that) -- the suite's bar, no new tolerance.

The multi-label loss is binary_cross_entropy_with_logits(reduction="sum") / (n_train C): the MEAN over the train rows' elements,
which is what masked_bce_loss documents, what tests/_multilabel_workers.float64_reference trains with and what every reported loss
is.  (A reference that divides the sum by n_train alone is C times the model's loss and gradient: the reference's error, not the
model's.)

ReLU decisions.  A pre-activation that fp32 and double round to different sides of zero changes a gradient by a whole term; that is
no kernel error, and no element is excused after the fact.  ``pick_seed`` chooses, from the reference alone, the smallest weight seed
in 0 .. 15 for which NO ReLU input of model64 is doubtful at either step: |value| at most 8 times the largest |twin - model64| of that
layer's ReLU input.  A configuration without such a seed fails its group -- unless it is one of ``NO_SEED``, the eleven for which the
reference itself shows that the rule cannot be met.  Those run on their least doubtful seed and are held to the SAME bound, every
element of every tensor: a doubtful ReLU input can only add to the model's distance from the double run, so they ask more of the
kernels than the rule would, not less.

The vectors (biases, scales and shifts of the normalisations) start at zero / one in run(); ``initial_params`` gives them seeded
values away from those, so that a forward pass that ignored one of them, or a gradient that left out a scale, shows.  The worker
checks what run() drew against ``initial_params`` and then writes the reference's parameters into the model, alike on every rank
(on 3 ranks initiliaze_parameters' mean (w + w + w) / 3 is a rounding away from w)."""
import itertools
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
import _multilabel_workers as MW  # noqa: E402
import _nodeclass_workers as NW  # noqa: E402

N, NNZ, COMMUNITY = 1100, 13000, 55          # three 512-row bands with a ragged last one, 17 blocks of 64 rows + 12, ragged 32-row tiles
FIN, CLASSES, LABELS = 24, 7, 41             # 41 labels: two label words with a partly used last one
NLAYERS, HIDDEN, EPOCHS = 4, 32, 2
DROPOUT, DROPOUT_SEED = 0.5, 11
MOMENTUM, EPS = 0.1, 1e-5
TASKS, NORMS = ("single", "multilabel"), ("none", "batch", "node")
SEEDS = range(16)
DOUBT = 8.0
WIDTHS_AXIS = (44, 30, 132)                  # float4 paths and a partly filled mask word; no multiple of 4; above 128

# The configurations for which NO weight seed in 0 .. 15 is free of doubtful ReLU inputs, by the reference alone (the number: the fewest
# doubtful inputs any of the 16 seeds leaves).  The rule counts on a few tenths of a doubtful input per seed.  That holds at width 32:
# 105 600 ReLU inputs a step, the twin's largest error about 1e-6 of their spread, so about 105 600 x 2 x 8e-6 x 0.4 (the density of a
# unit normal at zero) = 0.7.  Width 132 has 435 600 inputs and a twin error that grows with the length of the dot products: 5 - 22
# doubtful inputs per seed, and a seed without one is a matter of e^-5 or less.  The three at widths 32 and 44 expect 1.5 - 2 per seed
# and drew no blank among 16.  Listed configurations still run, on their least doubtful seed, under the same bound with nothing
# excused; a configuration NOT listed here that finds no seed fails its group (``assert_seeded``).
NO_SEED = {("single", "none-h132"): 8, ("single", "batch+root+drop-h132"): 5, ("single", "node+res+drop-h132"): 7,
           ("single", "none+root+bias+res+drop-h132"): 1, ("multilabel", "none-h132"): 2, ("multilabel", "batch+root+drop-h132"): 5,
           ("multilabel", "node+res+drop-h132"): 5, ("multilabel", "none+root+bias+res+drop-h132"): 3,
           ("multilabel", "batch+root+drop-h44"): 1, ("multilabel", "batch+res+drop-h32"): 1, ("multilabel", "batch+bias+res+drop-h32"): 1}


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------

def config(norm="none", root=False, bias=False, residual=False, dropout=0.0, hidden=HIDDEN):
    return {"norm": norm, "root": bool(root), "bias": bool(bias), "residual": bool(residual), "dropout": float(dropout), "hidden": int(hidden)}


def tag(c):
    return "%s%s%s%s%s-h%d" % (c["norm"], "+root" if c["root"] else "", "+bias" if c["bias"] else "", "+res" if c["residual"] else "",
                               "+drop" if c["dropout"] > 0 else "", c["hidden"])


def main_grid(norm):
    """The 16 configurations of one norm: root_weight x bias x residual x dropout."""
    return [config(norm, r, b, s, DROPOUT if d else 0.0) for r, b, s, d in itertools.product((0, 1), repeat=4)]


def rank_subset():
    """What runs on 2 and 3 ranks: per norm the four runs (a, b) of root = a, bias = b, residual = a xor b (under "batch": its
    complement) and dropout = a | b | not (a xor b) for none | batch | node -- every pair of values of every two options occurs
    (``covers_all_pairs``) -- plus the plain layer with a residual link, with and without dropout: the one layer kind whose weight
    gradient can leave the current stream (tuning.wgrad_lane) while a skip connection hands the same gradient tensor to a second
    consumer.  (The complement under "batch" keeps the subset to configurations for which the seed rule finds a seed in both tasks:
    multilabel batch+bias+res+drop has none, test_gradgrid's docstring.  More ranks change the all-reduce, not the ReLU inputs.)"""
    out = []
    for k, norm in enumerate(NORMS):
        for a, b in itertools.product((0, 1), repeat=2):
            d = (a, b, 1 - (a ^ b))[k]
            out.append(config(norm, a, b, (a ^ b) ^ (norm == "batch"), DROPOUT if d else 0.0))
    return out + [config("none", 0, 0, 1, 0.0), config("none", 0, 0, 1, DROPOUT)]


def covers_all_pairs(configs):
    keys = ("norm", "root", "bias", "residual", "dropout")
    values = {"norm": NORMS, "dropout": (0.0, DROPOUT)}
    for x, y in itertools.combinations(keys, 2):
        want = set(itertools.product(values.get(x, (False, True)), values.get(y, (False, True))))
        if want - {(c[x], c[y]) for c in configs}:
            return False
    return True


def width_axis(hidden):
    """The four configurations of the width axis at one hidden width."""
    return [config(hidden=hidden), config("batch", root=True, dropout=DROPOUT, hidden=hidden),
            config("node", residual=True, dropout=DROPOUT, hidden=hidden),
            config("none", root=True, bias=True, residual=True, dropout=DROPOUT, hidden=hidden)]


def widths_of(task, c):
    return [FIN] + [c["hidden"]] * (NLAYERS - 1) + [LABELS if task == "multilabel" else CLASSES]


# ---- data -------------------------------------------------------------------------------------------------------------------------------

def make_datasets(dirname):
    """{task: (paths, arrays)}: the planted problems of the node-classification and the multi-label tests at n = 1100."""
    out = {}
    for task in TASKS:
        d = os.path.join(dirname, task)
        os.makedirs(d, exist_ok=True)
        if task == "single":
            out[task] = NW.make_dataset(d, n=N, nnz=NNZ, community=COMMUNITY, classes=CLASSES, fin=FIN)
        else:
            out[task] = MW.make_dataset(d, n=N, nnz=NNZ, community=COMMUNITY, labels=LABELS, fin=FIN)
    return out


_adj = {}


def dense_adjacency(data):
    """D_r^-1/2 (P + I) D_c^-1/2 of the pattern as a dense double tensor (as _layernorm_workers.float64_reference builds it)."""
    key = id(data["A"])
    if key not in _adj:
        n = data["A"].shape[0]
        B = (data["A"] + sp.identity(n, format="csr")).astype(np.float64)
        B.data[:] = 1.0
        dr = 1.0 / np.sqrt(np.asarray(B.sum(axis=1)).reshape(-1))
        dc = 1.0 / np.sqrt(np.asarray(B.sum(axis=0)).reshape(-1))
        _adj[key] = (data["A"], torch.from_numpy((sp.diags(dr) @ B @ sp.diags(dc)).toarray()))
    return _adj[key][1]


# ---- the parameters ---------------------------------------------------------------------------------------------------------------------

def parameter_names(widths, c):
    """The reference's own statement of what a model of these options owns, in no particular order.  A normalised layer has its scale
    and shift and NO bias; the output layer is never normalised and keeps the bias it was asked for."""
    L = len(widths) - 1
    names = []
    for l in range(L):
        norm = c["norm"] if l < L - 1 else "none"
        names.append("%d.linear.weight" % l)
        if c["root"]:
            names.append("%d.root.weight" % l)
        if norm == "batch":
            names += ["%d.bn_weight" % l, "%d.bn_bias" % l]
        elif norm == "node":
            names += ["%d.ln_weight" % l, "%d.ln_bias" % l]
        elif c["bias"]:
            names.append("%d.bias" % l)
    return names


def buffer_names(widths, c):
    L = len(widths) - 1
    return [("%d.running_" % l) + s for l in range(L - 1) for s in ("mean", "var")] if c["norm"] == "batch" else []


def initial_params(widths, c, seed):
    """{name: fp32 tensor}: the matrices as run() draws them after torch.manual_seed(seed) -- layer by layer, ``linear`` before ``root``
    -- and seeded vectors: scales in 0.5 .. 1.5, shifts and biases in -0.5 .. 0.5 (module docstring)."""
    torch.manual_seed(seed)
    out = {}
    for l, (a, b) in enumerate(zip(widths, widths[1:])):
        out["%d.linear.weight" % l] = torch.nn.Linear(a, b, bias=False).weight.detach().clone()
        if c["root"]:
            out["%d.root.weight" % l] = torch.nn.Linear(a, b, bias=False).weight.detach().clone()
    for name in parameter_names(widths, c):
        if name not in out:
            l, kind = name.split(".")
            rng = np.random.default_rng([seed, int(l), sum(map(ord, kind))])
            f = widths[int(l) + 1]
            v = rng.uniform(0.5, 1.5, f) if kind.endswith("_weight") else rng.uniform(-0.5, 0.5, f)
            out[name] = torch.from_numpy(v.astype(np.float32))
    return out


# ---- the model in double ----------------------------------------------------------------------------------------------------------------

def model64(data, widths, params, opts, step, training=True, dtype=torch.float64, buffers=None, trace=None):
    """(loss, logits, {name: grad}, buffers after the step) of the model of run(normalize="sym", nlayers=len(widths) - 1, ...) on the
    whole graph, one process.  ``opts``: task, norm, root, bias, residual, dropout (+ dropout_seed).  ``buffers``: {name: tensor}, the
    running statistics BEFORE the step (None: zeros and ones); ``training=False``: eval mode, grads is {} and the loss that of the eval
    logits.  ``trace``: a list that receives every hidden layer's ReLU input."""
    from conftest import pkg
    D = pkg("dropout")
    n = data["A"].shape[0]
    Ad = dense_adjacency(data).to(dtype)
    h = torch.from_numpy(data["X"]).to(dtype)
    p = {k: v.detach().to(dtype).clone().requires_grad_(training) for k, v in params.items()}
    L = len(widths) - 1
    buf = {}
    for name in buffer_names(widths, opts):
        given = None if buffers is None else buffers[name]
        fresh = torch.zeros if name.endswith("mean") else torch.ones
        buf[name] = fresh(widths[int(name.split(".")[0]) + 1], dtype=dtype) if given is None else given.detach().to(dtype).clone()
    thr, scale = D.threshold(opts["dropout"])
    for l in range(L):
        z = (Ad @ h) @ p["%d.linear.weight" % l].t()
        if opts["root"]:
            z = z + h @ p["%d.root.weight" % l].t()
        if l == L - 1:
            logits = z + p["%d.bias" % l] if opts["bias"] else z
            break
        f = z.shape[1]
        if opts["norm"] == "batch":
            t = F.batch_norm(z, buf["%d.running_mean" % l], buf["%d.running_var" % l], p["%d.bn_weight" % l], p["%d.bn_bias" % l],
                             training, MOMENTUM, EPS)
        elif opts["norm"] == "node":
            t = F.layer_norm(z, (f,), p["%d.ln_weight" % l], p["%d.ln_bias" % l], EPS)
        else:
            t = z + p["%d.bias" % l] if opts["bias"] else z
        if trace is not None:
            trace.append(t.detach())
        d = torch.relu(t)
        if training and opts["dropout"] > 0.0:
            keep = D.keep_mask(opts.get("dropout_seed", DROPOUT_SEED), step, l, np.arange(n), f, thr)
            d = torch.where(keep, d * scale, torch.zeros((), dtype=dtype))
        h = h + d if opts["residual"] and widths[l] == widths[l + 1] else d
    train = torch.from_numpy(data["split"] == 1)
    if opts["task"] == "multilabel":
        y = torch.from_numpy(data["labels"] == 1)[train].to(dtype)
        loss = F.binary_cross_entropy_with_logits(logits[train], y, reduction="sum") / (int(train.sum()) * logits.shape[1])
    else:
        loss = F.cross_entropy(logits[train], torch.from_numpy(data["labels"])[train])
    grads = {}
    if training:
        names = list(p)
        grads = dict(zip(names, (g.detach() for g in torch.autograd.grad(loss, [p[k] for k in names]))))
    return loss.detach(), logits.detach(), grads, buf


def reference(data, task, c, seed):
    """Both training steps and the eval forward after them, in double and as the fp32 twin, for one configuration and weight seed:
    {"params", "widths", "steps": [{"m64", "twin", "relu64", "relu32"}] * EPOCHS, "eval": {"m64", "twin"}}, every m64 / twin a dict
    loss, logits, grads, buffers."""
    widths = widths_of(task, c)
    params = initial_params(widths, c, seed)
    opts = dict(c, task=task)
    out = {"params": params, "widths": widths, "steps": [], "seed": seed}
    bufs = {torch.float64: None, torch.float32: None}
    for step in range(EPOCHS):
        rec = {}
        for key, rkey, dt in (("m64", "relu64", torch.float64), ("twin", "relu32", torch.float32)):
            tr = []
            loss, logits, grads, b = model64(data, widths, params, opts, step, True, dt, bufs[dt], tr)
            bufs[dt] = b
            rec[key], rec[rkey] = {"loss": loss, "logits": logits, "grads": grads, "buffers": {k: v.clone() for k, v in b.items()}}, tr
        out["steps"].append(rec)
    out["eval"] = {}
    for key, dt in (("m64", torch.float64), ("twin", torch.float32)):
        loss, logits, _, _ = model64(data, widths, params, opts, EPOCHS, False, dt, bufs[dt])
        out["eval"][key] = {"loss": loss, "logits": logits}
    return out


def doubtful(ref):
    """How many ReLU inputs of the double run lie within DOUBT times the twin's largest error on that layer's ReLU input, over both steps."""
    count = 0
    for rec in ref["steps"]:
        for t64, t32 in zip(rec["relu64"], rec["relu32"]):
            worst = float((t32.double() - t64).abs().max())
            count += int((t64.abs() <= DOUBT * worst).sum())
    return count


_refs = {}


def pick_seed(data, task, c):
    """(seed, reference of that seed, [doubtful count of every seed tried], qualifies): the smallest weight seed in SEEDS without a
    doubtful ReLU input.  Where there is none the configuration does NOT qualify (the test that asked fails for it unless NO_SEED lists
    it); seed and reference are then those of the smallest seed with the fewest doubtful inputs: the run is made and held all the same.
    From the reference alone, deterministic; remembered per (task, configuration)."""
    key = (task, tag(c))
    if key not in _refs:
        counts, best = [], None
        for seed in SEEDS:
            ref = reference(data, task, c, seed)
            counts.append(doubtful(ref))
            for rec in ref["steps"]:                   # (counted: the traces are not needed again)
                del rec["relu64"], rec["relu32"]
            if best is None or counts[-1] < counts[best[0]]:
                best = (seed, ref)
            if counts[-1] == 0:
                break
        _refs[key] = best + (counts, counts[-1] == 0)
    return _refs[key]


# ---- the workers ------------------------------------------------------------------------------------------------------------------------

def run_worker(rank, P, port, paths, gpu, q, task=None, jobs=()):
    """Rank `rank` of `P` over gloo (gpu false: the checker-backed kernels on the CPU; true: the real provider): inside ONE process
    group, PGCN.run(epochs=2, lr=0.0, optimizer="torch", normalize="sym", nlayers=4, ...) once per job and lane.  A job:
    {"config", "seed", "params": {name: numpy}, "lanes": [tuning.wgrad_lane values]}.  Reports per job and lane the parameters after
    initialisation, the gradient of every parameter immediately before each optimiser step (after average_gradients), this rank's
    loss and training logits of each step, the eval-mode logits and the buffers after the run."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M = pkg("PGCN")
    T = pkg("tuning").T
    if gpu:
        M._kernel_provider = None
    else:
        from oracle_kernels import OracleKernels
        M._kernel_provider = OracleKernels()
    M._exchanger = None
    cur = {}

    init = M.initiliaze_parameters

    def initialise(model):
        init(model)
        cur["drawn"] = {name: prm.detach().cpu().numpy().copy() for name, prm in model.named_parameters()}
        with torch.no_grad():
            for name, prm in model.named_parameters():
                prm.copy_(torch.from_numpy(cur["job"]["params"][name]))
        cur["model"] = model
        cur["init"] = {name: prm.detach().cpu().numpy().copy() for name, prm in model.named_parameters()}
        model.register_forward_hook(lambda m, a, out: cur["logits"].append(out.detach().cpu().numpy()) if m.training else None)

    adam_step = torch.optim.Adam.step

    def step(self, *a, **kw):
        cur["grads"].append({name: prm.grad.detach().cpu().numpy().copy() for name, prm in cur["model"].named_parameters()})
        return adam_step(self, *a, **kw)

    def with_loss(f):
        def g(*a, **kw):
            out = f(*a, **kw)
            cur["loss"].append(float(out[0].detach().double().cpu()))
            return out
        return g

    M.initiliaze_parameters = initialise
    torch.optim.Adam.step = step
    M.masked_loss, M.masked_bce_loss = with_loss(M.masked_loss), with_loss(M.masked_bce_loss)
    load = M._nodedata.load_multilabel if task == "multilabel" else M._nodedata.load
    results = []

    def fn(r, size, nlayers, nfeatures, path_A, path_partvec, backend, **_):
        for job in jobs:
            c = job["config"]
            for lane in job["lanes"]:
                cur.update(job=job, grads=[], logits=[], loss=[])
                old = T.wgrad_lane
                T.wgrad_lane = lane
                try:
                    torch.manual_seed(job["seed"])
                    kw = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=c["hidden"], epochs=EPOCHS,
                              lr=0.0, optimizer="torch", task=task)
                    if c["norm"] != "none":
                        kw["norm"] = c["norm"]
                    for name, opt in (("root", "root_weight"), ("bias", "bias"), ("residual", "residual")):
                        if c[name]:
                            kw[opt] = True
                    if c["dropout"] > 0.0:
                        kw.update(dropout=c["dropout"], dropout_seed=DROPOUT_SEED)
                    with redirect_stdout(io.StringIO()):
                        model = M.run(r, size, NLAYERS, c["hidden"], path_A, path_partvec, "gloo", normalize="sym", **kw)
                    data = load(paths["features"], paths["labels"], paths["split"], M._engine_current.part.owned, N, device=M.device)
                    model.eval()
                    with torch.no_grad():
                        ev = model(data.features).cpu().numpy()
                    results.append(dict(tag=tag(c), lane=lane, init=cur["init"], drawn=cur["drawn"], grads=cur["grads"], logits=cur["logits"], loss=cur["loss"],
                                        eval_logits=ev, buffers={k: v.detach().cpu().numpy().copy() for k, v in model.named_buffers()},
                                        history=model.history, own=M._engine_current.part.owned.cpu().numpy(),
                                        hip=type(M._engine_current.k).__name__))
                finally:
                    T.wgrad_lane = old

    M.init_process(rank, P, fn, NLAYERS, HIDDEN, paths["A"], paths["pv%d" % P], "gloo", "sym")
    q.put({"rank": rank, "results": results})


def spawn_run(P, paths, gpu, **kw):
    """BW.spawn_run with this file's worker: [the result list of rank 0, of rank 1, ...]."""
    saved = BW.run_worker
    BW.run_worker = run_worker
    try:
        return [r["results"] for r in BW.spawn_run(P, paths, gpu, **kw)]
    finally:
        BW.run_worker = saved


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------

def make_jobs(data, task, configs, lanes=(0,)):
    """(jobs, references, unseeded) of a worker group.  ``unseeded``: the configurations for which every seed in SEEDS leaves a doubtful
    ReLU input, with their counts -- the caller FAILS when one of them is not in NO_SEED (``assert_seeded``), after the group has run."""
    jobs, refs, unseeded = [], {}, []
    for c in configs:
        seed, ref, counts, ok = pick_seed(data, task, c)
        print("%s %s: doubtful ReLU inputs by weight seed %s -> seed %d%s" % (task, tag(c), counts, seed, "" if ok else " (NONE QUALIFIES)"),
              flush=True)
        if not ok:
            unseeded.append((task, tag(c), counts))
        refs[tag(c)] = ref
        jobs.append({"config": c, "seed": seed, "lanes": list(lanes),
                     "params": {k: v.numpy() for k, v in ref["params"].items()}})
    return jobs, refs, unseeded


def assert_seeded(unseeded):
    """The seed rule's failure: a configuration without a weight seed that NO_SEED does not list."""
    new = [u for u in unseeded if (u[0], u[1]) not in NO_SEED]
    assert not new, "every weight seed in 0 .. 15 leaves a doubtful ReLU input (counts by seed): %s" % (new,)


def _rows(per_rank, pick):
    out = None
    for r in per_rank:
        v = pick(r)
        out = np.zeros((N,) + v.shape[1:], v.dtype) if out is None else out
        out[r["own"]] = v
    return out


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_group(task, configs, res, refs, lanes=(0,), case=""):
    """Every assertion of the grid on the answers ``res`` ([rank][job x lane]) of one worker group.  Returns how many tensors were held."""
    from conftest import held_to_fixture
    P = len(res)
    held = 0
    assert all(len(r) == len(configs) * len(lanes) for r in res)
    for j, c in enumerate(configs):
        ref = refs[tag(c)]
        widths = ref["widths"]
        first = None
        for k, lane in enumerate(lanes):
            ranks = [r[j * len(lanes) + k] for r in res]
            where = "gradgrid%s/%s/%s/P%d/lane%d" % (case, task, tag(c), P, lane)
            for r in ranks:
                assert r["tag"] == tag(c) and r["lane"] == lane
                # the model owns what the reference says it owns, and starts from the reference's parameters
                assert sorted(r["init"]) == sorted(parameter_names(widths, c)), (where, sorted(r["init"]))
                assert sorted(r["buffers"]) == sorted(buffer_names(widths, c)), (where, sorted(r["buffers"]))
                for name, v in ref["params"].items():
                    assert _same_bits(r["init"][name], v.numpy()), (where, name)
                    if v.dim() == 2 and P <= 2:        # run() drew the reference's matrices (the ranks' mean of equal draws: exact for 1 and 2)
                        assert _same_bits(r["drawn"][name], v.numpy()), (where, name)
                    elif v.dim() == 2:                 # (w + w + w) / 3 in fp32: within a rounding of w
                        assert np.abs(r["drawn"][name].astype(np.float64) - v.double().numpy()).max() <= 2.0 ** -22 * float(v.abs().max()), (where, name)
                assert len(r["grads"]) == len(r["logits"]) == len(r["loss"]) == EPOCHS, where
            logits = [_rows(ranks, lambda r, s=s: r["logits"][s]) for s in range(EPOCHS)]
            if c["dropout"] > 0.0:
                assert not np.array_equal(logits[0], logits[1]), where + ": the second step drew the first step's masks"
            else:
                assert _same_bits(logits[0], logits[1]), where + ": lr = 0 and no dropout, yet the steps' logits differ"
            for s, rec in enumerate(ref["steps"]):
                m64, twin = rec["m64"], rec["twin"]
                at = "%s/step%d" % (where, s)
                held_to_fixture(at, "loss", np.array([sum(r["loss"][s] for r in ranks)]), twin["loss"].numpy().reshape(1),
                                m64["loss"].numpy().reshape(1))
                held_to_fixture(at, "logits", logits[s], twin["logits"].numpy(), m64["logits"].numpy())
                held += 2
                for i, r in enumerate(ranks):          # the gradient after the all-reduce: the same bound on every rank
                    for name in ref["params"]:
                        held_to_fixture(at + "/rank%d" % i, "grad " + name.split(".", 1)[1], r["grads"][s][name],
                                        twin["grads"][name].numpy(), m64["grads"][name].numpy())
                        held += 1
            last64, last32 = ref["steps"][-1]["m64"]["buffers"], ref["steps"][-1]["twin"]["buffers"]
            for i, r in enumerate(ranks):
                for name in last64:
                    held_to_fixture(where + "/rank%d" % i, name.split(".", 1)[1], r["buffers"][name], last32[name].numpy(),
                                    last64[name].numpy())
                    held += 1
            ev = _rows(ranks, lambda r: r["eval_logits"])
            held_to_fixture(where, "eval logits", ev, ref["eval"]["twin"]["logits"].numpy(), ref["eval"]["m64"]["logits"].numpy())
            held += 1
            # the weight gradient's side lane: the same bits with and without it
            if first is None:
                first = (ranks, logits, ev)
            else:
                for r0, r1 in zip(first[0], ranks):
                    for s in range(EPOCHS):
                        for name in r0["grads"][s]:
                            assert _same_bits(r0["grads"][s][name], r1["grads"][s][name]), (where, "lane", s, name)
                        assert r0["loss"][s] == r1["loss"][s], (where, "lane", s, "loss")
                    for name in r0["buffers"]:
                        assert _same_bits(r0["buffers"][name], r1["buffers"][name]), (where, "lane", name)
                assert all(_same_bits(a, b) for a, b in zip(first[1], logits)) and _same_bits(first[2], ev), (where, "lane", "logits")
    return held


def run_group(datasets, task, configs, P, gpu, lanes=(0,)):
    """One worker group from the seed rule to the last assertion; prints the time the workers took.  Returns the tensors held."""
    import time
    paths, data = datasets[task]
    jobs, refs, unseeded = make_jobs(data, task, configs, lanes)
    t0 = time.time()
    res = spawn_run(P, paths, gpu, task=task, jobs=jobs)
    print("%s, %d configurations x %d lanes on %d ranks (%s): %.1f s in the workers" % (
        task, len(configs), len(lanes), P, res[0][0]["hip"], time.time() - t0), flush=True)
    try:
        held = check_group(task, configs, res, refs, lanes, "-gpu" if gpu else "")
    finally:
        assert_seeded(unseeded)
    return held
