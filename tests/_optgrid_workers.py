"""The gradient grid of tests/_gradgrid_workers.py with the three layer options that were merged after it -- aggr="max", propagate=K /
ppr_alpha (APPNP) and drop_edge=P -- on it: the configuration, ONE reference, a pairwise-covering list, the seed rule and the worker
processes of tests/test_optgrid.py and tests/test_optgrid_gpu.py (spawn start method).

Nothing is restated that an older file states: the data, the parameters, the seed rule's constants and the double model's norm, bias,
ReLU, dropout mask, residual link, buffers and losses are GG's (_gradgrid_workers); the max aggregation's definition and its
linearisation at a recorded selection are AW's (_aggmax_workers.oracle_max, the gather of model_sel); the propagation's coefficients
are PW's (_propagate_workers.coefficients); the kept pattern and its scales are DW's (_dropedge_workers.dropped_adjacency).
``model64x`` is GG.model64 with two places generalised -- the aggregation of a layer and the K propagation steps after the output
layer -- in stock torch operations under torch's own autograd: no backward formula.  test_optgrid pins it to the four older
statements where their options meet (to GG.model64 bit for bit).

The max aggregation is piecewise linear: which neighbour wins is a decision like a ReLU's, and one that fp32 and double may take
differently at a near-tie.  As in tests/_aggmax_workers.py the model is therefore held in two parts: every recorded (OUT, ARG) of a
run, training and eval, is the definition's on the run's OWN fp32 input bit for bit, and loss, logits, gradients and buffers are held
to the double model UNDER that recorded selection.  The seed rule comes first and knows no run: it is applied to ``model64x`` with
``args=None``, where every model (double and twin) selects by the definition on its own layer input.

bound: conftest.held_to_fixture with the float32 twin as fixture, max(1e-5, 2 err_twin) -- the suite's bar, no new tolerance."""
import itertools
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
import _batchnorm_workers as BW  # noqa: E402
import _dropedge_workers as DW  # noqa: E402
import _gradgrid_workers as GG  # noqa: E402
import _propagate_workers as PW  # noqa: E402

N, NLAYERS, HIDDEN, EPOCHS = GG.N, GG.NLAYERS, GG.HIDDEN, GG.EPOCHS
DROPOUT, DROPOUT_SEED = GG.DROPOUT, GG.DROPOUT_SEED
TASKS, NORMS, WIDTHS_AXIS = GG.TASKS, GG.NORMS, GG.WIDTHS_AXIS
AGGRS = ("sum", "max", "drop")                 # "drop": the sum aggregation with drop_edge = DW.P_DROP
ALPHA = 0.1
PROPS = (None, (1, ALPHA), (3, ALPHA))         # K = 1: the backward's special case, which has no D yet (engine.propagate_backward)

# The configurations for which NO weight seed in 0 .. 15 is free of doubtful ReLU inputs, by the reference alone (model64x with
# args=None; the number: the fewest doubtful inputs any of the 16 seeds leaves), measured on the CPU -- written the way GG.NO_SEED is,
# with GG's arithmetic: 0.7 expected doubtful inputs per seed at width 32, 5 - 22 at width 132.  Listed configurations run on their
# least doubtful seed under the same bound with nothing excused; a configuration NOT listed that finds no seed fails its group.
# All three are the width axis at 132 (435 600 ReLU inputs a step): 1 - 21, 10 - 28 and 2 - 14 doubtful inputs per seed.  The twin is
# an fp32 run of the HOST's matrix products, so the counts move by a few elements with the host's processor: none+root+bias+res+K1
# leaves 4 - 12 per seed and a blank at seed 14 on the host the first two were measured on (any number of threads), and 2 - 14 with NO
# blank (seed 14: 2) on the host of the device runs -- listed with that count, it runs on seed 14 on both.  Everything at widths 32, 44
# and 30 finds a seed on both hosts.
NO_SEED_X = {("single", "node+res+drop-h132+max"): 1, ("single", "batch+root-h132+dropedge+K3"): 10,
             ("single", "none+root+bias+res-h132+K1"): 2}


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------

def config(norm="none", root=False, bias=False, residual=False, dropout=0.0, hidden=HIDDEN, aggr="sum", prop=None, dense=False):
    assert aggr in AGGRS and prop in PROPS
    c = GG.config(norm, root, bias, residual, dropout, hidden)
    c.update(aggr=aggr, prop=prop, dense=bool(dense))
    return c


def tag(c):
    """GG.tag extended; a configuration with sum / None (and aggregating layers) keeps GG's tag."""
    return GG.tag(c) + ("" if c["aggr"] == "sum" else "+max" if c["aggr"] == "max" else "+dropedge") + ("+dense" if c["dense"] else "") + \
        ("" if c["prop"] is None else "+K%d" % c["prop"][0])


def run_options(c):
    """What the configuration adds to the keyword arguments of PGCN.run beyond GG's."""
    kw = {}
    if c["aggr"] == "max":
        kw["aggr"] = "max"
    elif c["aggr"] == "drop":
        kw.update(drop_edge=DW.P_DROP, dropout_seed=DROPOUT_SEED)
    if c["prop"] is not None:
        kw.update(propagate=c["prop"][0], ppr_alpha=c["prop"][1])
    if c["dense"]:
        kw["dense_layers"] = True
    return kw


_D = DROPOUT
_GRID = (  # norm, root, bias, residual, dropout, aggr, prop
    ("none", 0, 1, 0, _D, "sum", None),
    ("none", 1, 1, 1, 0., "max", PROPS[1]),
    ("none", 1, 0, 1, _D, "drop", PROPS[2]),
    ("batch", 0, 0, 1, 0., "sum", PROPS[1]),
    ("batch", 0, 1, 0, _D, "max", PROPS[2]),
    ("batch", 1, 1, 0, 0., "drop", None),
    ("node", 1, 0, 1, 0., "sum", PROPS[2]),
    ("node", 0, 0, 1, _D, "max", None),
    ("node", 0, 0, 0, _D, "drop", PROPS[1]),
    ("node", 0, 1, 0, _D, "max", PROPS[1]),
    # beyond the covering ten: the skip connection on the PLAIN layer kind (the one whose weight gradient can leave the current stream,
    # GG.rank_subset) and under batch norm, with each of the two new aggregations
    ("batch", 0, 0, 1, 0., "max", None),
    ("batch", 1, 0, 1, 0., "drop", PROPS[2]),
    ("none", 0, 0, 1, _D, "drop", None),
    ("none", 0, 0, 1, 0., "max", PROPS[2]),
)
_RANKS = (1, 2, 4, 11, 12, 13)                  # indices into _GRID: what runs on 2 and 3 ranks
_HALF = (0, 1, 2, 3, 4, 5, 13)                  # indices into _GRID: the first of the two device groups on one rank (three max each)


def option_grid():
    """The fixed pairwise-covering list at hidden 32 (``covers_all_pairs``: every pair of values of every two of the seven options),
    14 configurations.  run() refuses drop_edge with max: here two values of ONE option, so no pair is lost."""
    return [config(n, r, b, s, d, HIDDEN, a, p) for n, r, b, s, d, a, p in _GRID]


def dense_configs():
    """dense_layers (goes with neither root weight, max nor DropEdge): batch norm + residual + dropout + K 3, node norm + bias + K 1."""
    return [config("batch", residual=True, dropout=DROPOUT, prop=PROPS[2], dense=True), config("node", bias=True, prop=PROPS[1], dense=True)]


def rank_subset_x():
    """What runs on 2 and 3 ranks, six of the list: max + residual (the plain layer + K 3; root + bias + K 1), DropEdge + residual +
    dropout (the plain layer; root + K 3), and under batch norm max + bias + dropout + K 3 and DropEdge + root + residual + K 3 -- each of
    max + residual, drop + residual + dropout, max + prop and drop + prop twice, two of them under batch norm.  (A group's time on the
    device is the start of its processes; six keep the three-rank group below the gradient grid's.)"""
    g = option_grid()
    return [g[i] for i in _RANKS]


def one_rank_groups():
    """The list and the dense pair as the two worker groups of the device test on one rank (one group takes longer than the slowest
    test of the gradient grid: the seed rule and the selections' oracle run on the host); the CPU test runs them as one."""
    g, d = option_grid(), dense_configs()
    return [[g[i] for i in _HALF] + d[:1], [g[i] for i in range(len(g)) if i not in _HALF] + d[1:]]


def width_groups():
    """(id, configurations) of the width axis' worker groups: one per width, at 132 two (the max configuration's seed rule tries all
    16 seeds with the definition's selection at 435 600 elements a layer)."""
    out = [(str(h), W) for h in WIDTHS_AXIS[:2] for W in [width_axis_x(h)]]
    big = width_axis_x(WIDTHS_AXIS[2])
    return out + [("132-max", big[:1]), ("132-dropedge-sum", big[1:])]


def width_axis_x(hidden):
    """The three configurations of the width axis at one hidden width."""
    return [config("node", residual=True, dropout=DROPOUT, hidden=hidden, aggr="max"),
            config("batch", root=True, hidden=hidden, aggr="drop", prop=PROPS[2]),
            config("none", root=True, bias=True, residual=True, hidden=hidden, prop=PROPS[1])]


def covers_all_pairs(configs):
    """GG.covers_all_pairs over the seven options: every pair of values of every two options occurs."""
    values = {"norm": NORMS, "root": (False, True), "bias": (False, True), "residual": (False, True), "dropout": (0.0, DROPOUT),
              "aggr": AGGRS, "prop": PROPS}
    for x, y in itertools.combinations(list(values), 2):
        if set(itertools.product(values[x], values[y])) - {(c[x], c[y]) for c in configs}:
            return False
    return True


# ---- the model in double ----------------------------------------------------------------------------------------------------------------

_dropped, _pattern = {}, {}


def _dropped_adjacency(data, step):
    """DW.dropped_adjacency, remembered per (matrix, step) the way GG.dense_adjacency remembers its matrix."""
    key = (id(data["A"]), step)
    if key not in _dropped:
        _dropped[key] = (data["A"], DW.dropped_adjacency(data, step))
    return _dropped[key][1]


def _sym_pattern(data):
    key = id(data["A"])
    if key not in _pattern:
        _pattern[key] = (data["A"],) + AW.sym_pattern(data["A"])
    return _pattern[key][1:]


_first = {}


def _own_selection(data, H, l):
    """ARG of AW.oracle_max on the layer input H (int64 tensor).  The first layer's input is the features, whatever the seed and the
    step: its selection is remembered per (features, dtype)."""
    key = (id(data["X"]), H.dtype.str)
    if l == 0 and key in _first:
        return _first[key][1]
    rowptr, col = _sym_pattern(data)
    a = torch.from_numpy(AW.oracle_max(rowptr, col, np.arange(H.shape[0]), H)[1].astype(np.int64))
    if l == 0:
        _first[key] = (data["X"], a)
    return a


def model64x(data, widths, params, opts, step, training=True, dtype=torch.float64, buffers=None, trace=None, args=None):
    """GG.model64 (its docstring; the same returns) with two places generalised.  ``opts`` additionally: aggr, prop, dense.
    Aggregation of layer l: sum -- Ad @ h; drop -- DW.dropped_adjacency(data, step) @ h in training, Ad @ h in eval; max -- the gather
    h[args[l][i, c], c], 0 where -1 (AW.model_sel), ``args`` the recorded selection per layer (global ids) or None: the definition's own
    (AW.oracle_max) on THIS model's layer input; dense -- h itself.  After the output layer, with prop = (K, alpha): K steps
    b (Ad @ Z) + a z with (a, b) = PW.coefficients(alpha) and the UNDROPPED Ad."""
    from conftest import pkg
    D = pkg("dropout")
    n = data["A"].shape[0]
    Ad = GG.dense_adjacency(data).to(dtype)
    A_step = _dropped_adjacency(data, step).to(dtype) if opts["aggr"] == "drop" and training else Ad
    h = torch.from_numpy(data["X"]).to(dtype)
    p = {k: v.detach().to(dtype).clone().requires_grad_(training) for k, v in params.items()}
    L = len(widths) - 1
    buf = {}
    for name in GG.buffer_names(widths, opts):
        given = None if buffers is None else buffers[name]
        fresh = torch.zeros if name.endswith("mean") else torch.ones
        buf[name] = fresh(widths[int(name.split(".")[0]) + 1], dtype=dtype) if given is None else given.detach().to(dtype).clone()
    thr, scale = D.threshold(opts["dropout"])
    for l in range(L):
        if opts["dense"]:
            agg = h
        elif opts["aggr"] == "max":
            if args is None:
                a = _own_selection(data, h.detach().numpy(), l)
            else:
                a = torch.from_numpy(args[l].astype(np.int64))
            agg = torch.where(a >= 0, torch.gather(h, 0, a.clamp(min=0)), torch.zeros((), dtype=dtype))
        else:
            agg = A_step @ h
        z = agg @ p["%d.linear.weight" % l].t()
        if opts["root"]:
            z = z + h @ p["%d.root.weight" % l].t()
        if l == L - 1:
            logits = z + p["%d.bias" % l] if opts["bias"] else z
            break
        f = z.shape[1]
        if opts["norm"] == "batch":
            t = F.batch_norm(z, buf["%d.running_mean" % l], buf["%d.running_var" % l], p["%d.bn_weight" % l], p["%d.bn_bias" % l],
                             training, GG.MOMENTUM, GG.EPS)
        elif opts["norm"] == "node":
            t = F.layer_norm(z, (f,), p["%d.ln_weight" % l], p["%d.ln_bias" % l], GG.EPS)
        else:
            t = z + p["%d.bias" % l] if opts["bias"] else z
        if trace is not None:
            trace.append(t.detach())
        d = torch.relu(t)
        if training and opts["dropout"] > 0.0:
            keep = D.keep_mask(opts.get("dropout_seed", DROPOUT_SEED), step, l, np.arange(n), f, thr)
            d = torch.where(keep, d * scale, torch.zeros((), dtype=dtype))
        h = h + d if opts["residual"] and widths[l] == widths[l + 1] else d
    if opts["prop"] is not None:
        K, alpha = opts["prop"]
        a, b = (float(x) for x in PW.coefficients(alpha))
        z = logits
        for _ in range(K):
            logits = b * (Ad @ logits) + a * z
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


def reference(data, task, c, seed, args=None, with_eval=True):
    """GG.reference on ``model64x``.  ``args`` (max alone): {"steps": [[ARG of every layer] per step], "eval": [ARG of every layer]}, the
    recorded selection; None: every model selects for itself.  ``with_eval`` false: the training steps alone (what the seed rule
    counts on); ``add_eval`` completes such a reference."""
    widths = GG.widths_of(task, c)
    params = GG.initial_params(widths, c, seed)
    opts = dict(c, task=task)
    out = {"params": params, "widths": widths, "steps": [], "seed": seed}
    bufs = out["_buffers"] = {torch.float64: None, torch.float32: None}
    for step in range(EPOCHS):
        rec = {}
        for key, rkey, dt in (("m64", "relu64", torch.float64), ("twin", "relu32", torch.float32)):
            tr = []
            loss, logits, grads, b = model64x(data, widths, params, opts, step, True, dt, bufs[dt], tr, None if args is None else args["steps"][step])
            bufs[dt] = b
            rec[key], rec[rkey] = {"loss": loss, "logits": logits, "grads": grads, "buffers": {k: v.clone() for k, v in b.items()}}, tr
        out["steps"].append(rec)
    return add_eval(data, task, c, out, args) if with_eval else out


def add_eval(data, task, c, ref, args=None):
    """The eval forward after the training steps of ``ref`` (their buffers), in double and as the twin."""
    ref["eval"] = {}
    for key, dt in (("m64", torch.float64), ("twin", torch.float32)):
        loss, logits, _, _ = model64x(data, ref["widths"], ref["params"], dict(c, task=task), EPOCHS, False, dt, ref["_buffers"][dt], None,
                                      None if args is None else args["eval"])
        ref["eval"][key] = {"loss": loss, "logits": logits}
    return ref


_refs = {}


def pick_seed(data, task, c):
    """GG.pick_seed (its rule, SEEDS and DOUBT unchanged) on this file's reference with args=None: from the reference alone.  The rule
    counts ReLU inputs of the two training steps; the eval forward is made for the chosen seed only."""
    key = (task, tag(c))
    if key not in _refs:
        counts, best = [], None
        for seed in GG.SEEDS:
            ref = reference(data, task, c, seed, with_eval=False)
            counts.append(GG.doubtful(ref))
            for rec in ref["steps"]:
                del rec["relu64"], rec["relu32"]
            if best is None or counts[-1] < counts[best[0]]:
                best = (seed, ref)
            if counts[-1] == 0:
                break
        _refs[key] = (best[0], add_eval(data, task, c, best[1]), counts, counts[-1] == 0)
    return _refs[key]


# ---- the workers ------------------------------------------------------------------------------------------------------------------------

def run_worker(rank, P, port, paths, gpu, q, task=None, jobs=()):
    """GG.run_worker's protocol and report (its docstring) with the configuration's aggr / drop_edge / propagate, ppr_alpha /
    dense_layers passed to run(), and per job and lane additionally: every call of forward_max -- (model in training mode?, input, OUT,
    ARG), eval-mode calls too -- and whether the engine's max / DropEdge structures are the composed ones (None: never built).  On the
    device the composed propagation steps raise: a run that answers ran the step kernels."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    from conftest import pkg
    M, E = pkg("PGCN"), pkg("engine")
    T = pkg("tuning").T
    if gpu:
        M._kernel_provider = None

        def refuse(*a, **k):
            raise AssertionError("the composed propagation route ran on the device")
        E.ppr_step_composed = E.ppr_step_backward_composed = refuse
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
        cur["modules"] = [type(m).__name__ for m in model]
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

    forward_max = E.AggregationEngine.forward_max

    def recorded(self, H):
        OUT, ARG = forward_max(self, H)
        cur["calls"].append((bool(cur["model"].training), H.detach().cpu().numpy().copy(), OUT.cpu().numpy().copy(), ARG.cpu().numpy().copy()))
        return OUT, ARG

    M.initiliaze_parameters = initialise
    torch.optim.Adam.step = step
    M.masked_loss, M.masked_bce_loss = with_loss(M.masked_loss), with_loss(M.masked_bce_loss)
    E.AggregationEngine.forward_max = recorded
    load = M._nodedata.load_multilabel if task == "multilabel" else M._nodedata.load
    results = []

    def fn(r, size, nlayers, nfeatures, path_A, path_partvec, backend, **_):
        for job in jobs:
            c = job["config"]
            for lane in job["lanes"]:
                cur.update(job=job, grads=[], logits=[], loss=[], calls=[])
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
                    kw.update(run_options(c))
                    with redirect_stdout(io.StringIO()):
                        model = M.run(r, size, NLAYERS, c["hidden"], path_A, path_partvec, "gloo", normalize="sym", **kw)
                    eng = M._engine_current
                    data = load(paths["features"], paths["labels"], paths["split"], eng.part.owned, N, device=M.device)
                    model.eval()
                    with torch.no_grad():
                        ev = model(data.features).cpu().numpy()
                    results.append(dict(tag=tag(c), lane=lane, init=cur["init"], drawn=cur["drawn"], grads=cur["grads"], logits=cur["logits"],
                                        loss=cur["loss"], calls=cur["calls"], modules=cur["modules"], eval_logits=ev,
                                        buffers={k: v.detach().cpu().numpy().copy() for k, v in model.named_buffers()},
                                        history=model.history, own=eng.part.owned.cpu().numpy(), hip=type(eng.k).__name__,
                                        composed_max=None if eng._max is None else bool(eng._max.composed),
                                        composed_drop=None if eng._drop is None else bool(eng._drop.composed)))
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
    """GG.make_jobs on this file's seed rule: (jobs, references, unseeded)."""
    jobs, refs, unseeded = [], {}, []
    for c in configs:
        seed, ref, counts, ok = pick_seed(data, task, c)
        print("%s %s: doubtful ReLU inputs by weight seed %s -> seed %d%s" % (task, tag(c), counts, seed, "" if ok else " (NONE QUALIFIES)"),
              flush=True)
        if not ok:
            unseeded.append((task, tag(c), counts))
        refs[tag(c)] = ref
        jobs.append({"config": c, "seed": seed, "lanes": list(lanes), "params": {k: v.numpy() for k, v in ref["params"].items()}})
    return jobs, refs, unseeded


def assert_seeded(unseeded):
    """The seed rule's failure: a configuration without a weight seed that NO_SEED_X does not list."""
    new = [u for u in unseeded if (u[0], u[1]) not in NO_SEED_X]
    assert not new, "every weight seed in 0 .. 15 leaves a doubtful ReLU input (counts by seed): %s" % (new,)


_under = []


def _held_max(data, task, c, ranks, ref, where):
    """The max aggregation of one run: every recorded (OUT, ARG), training and eval, is AW.oracle_max on the run's own fp32 input bit
    for bit, rows gathered over the ranks; returns the reference under the recorded selection (the eval selection: the last eval
    forward's, the one whose logits are reported)."""
    rowptr, col = _sym_pattern(data)
    gid = np.arange(N)
    ncalls = len(ranks[0]["calls"])
    assert all(len(r["calls"]) == ncalls for r in ranks), where
    modes = [ranks[0]["calls"][k][0] for k in range(ncalls)]
    assert all([r["calls"][k][0] for k in range(ncalls)] == modes for r in ranks), where
    train = [k for k in range(ncalls) if modes[k]]
    evals = [k for k in range(ncalls) if not modes[k]]
    assert len(train) == NLAYERS * EPOCHS and len(evals) >= NLAYERS and len(evals) % NLAYERS == 0, (where, len(train), len(evals))
    ARGS = {}
    for k in range(ncalls):
        Hg, OUT, ARG = (GG._rows(ranks, lambda r, i=i: r["calls"][k][i]) for i in (1, 2, 3))
        want_out, want_arg = AW.oracle_max(rowptr, col, gid, Hg)
        assert ARG.dtype == np.int32 and np.array_equal(ARG, want_arg), (where, "call", k, modes[k], "ARG", int((ARG != want_arg).sum()))
        assert np.array_equal(AW.bits(OUT), AW.bits(want_out)), (where, "call", k, modes[k], "OUT")
        ARGS[k] = ARG
    args = {"steps": [[ARGS[train[s * NLAYERS + l]] for l in range(NLAYERS)] for s in range(EPOCHS)],
            "eval": [ARGS[k] for k in evals[-NLAYERS:]]}
    key = (task, tag(c), ref["seed"], b"".join(a.tobytes() for a in sum(args["steps"], []) + args["eval"]))
    if _under[:1] != [key]:                            # (the second lane records the first lane's selection: one reference serves both)
        under = reference(data, task, c, ref["seed"], args)
        _under[:] = [key, under, GG.doubtful(under)]
    print("%s: %d doubtful ReLU inputs under the recorded selection" % (where, _under[2]), flush=True)
    return _under[1]


def check_group_x(data, task, configs, res, refs, lanes=(0,), case="", gpu=False):
    """Every assertion of GG.check_group on the answers ``res`` ([rank][job x lane]) of one worker group, the references those of
    ``model64x``; for max the recorded selections first (``_held_max``) and the double model and its twin under them.  The two
    steps' logits are bit-identical exactly when the configuration has neither dropout nor DropEdge.  Returns the tensors held."""
    from conftest import held_to_fixture
    P = len(res)
    held = 0
    assert all(len(r) == len(configs) * len(lanes) for r in res)
    for j, c in enumerate(configs):
        seeded = refs[tag(c)]
        widths = seeded["widths"]
        first = None
        for k, lane in enumerate(lanes):
            ranks = [r[j * len(lanes) + k] for r in res]
            where = "optgrid%s/%s/%s/P%d/lane%d" % (case, task, tag(c), P, lane)
            for r in ranks:
                assert r["tag"] == tag(c) and r["lane"] == lane
                assert r["modules"] == ["PGCN"] * NLAYERS + ["Propagate"] * (c["prop"] is not None), (where, r["modules"])
                if gpu:
                    assert r["hip"] == "HipKernels", (where, r["hip"])
                want = False if gpu else True
                assert r["composed_max"] == (want if c["aggr"] == "max" else None), (where, "max structures", r["composed_max"])
                assert r["composed_drop"] == (want if c["aggr"] == "drop" else None), (where, "DropEdge structures", r["composed_drop"])
                assert (len(r["calls"]) > 0) == (c["aggr"] == "max"), where
                # the model owns what the reference says it owns, and starts from the reference's parameters
                assert sorted(r["init"]) == sorted(GG.parameter_names(widths, c)), (where, sorted(r["init"]))
                assert sorted(r["buffers"]) == sorted(GG.buffer_names(widths, c)), (where, sorted(r["buffers"]))
                for name, v in seeded["params"].items():
                    assert GG._same_bits(r["init"][name], v.numpy()), (where, name)
                    if v.dim() == 2 and P <= 2:        # run() drew the reference's matrices (the ranks' mean of equal draws: exact for 1 and 2)
                        assert GG._same_bits(r["drawn"][name], v.numpy()), (where, name)
                    elif v.dim() == 2:                 # (w + w + w) / 3 in fp32: within a rounding of w
                        assert np.abs(r["drawn"][name].astype(np.float64) - v.double().numpy()).max() <= 2.0 ** -22 * float(v.abs().max()), (where, name)
                assert len(r["grads"]) == len(r["logits"]) == len(r["loss"]) == EPOCHS, where
            ref = _held_max(data, task, c, ranks, seeded, where) if c["aggr"] == "max" else seeded
            logits = [GG._rows(ranks, lambda r, s=s: r["logits"][s]) for s in range(EPOCHS)]
            if c["dropout"] > 0.0 or c["aggr"] == "drop":
                assert not np.array_equal(logits[0], logits[1]), where + ": the second step drew the first step's masks"
            else:
                assert GG._same_bits(logits[0], logits[1]), where + ": lr = 0, neither dropout nor DropEdge, yet the steps' logits differ"
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
            ev = GG._rows(ranks, lambda r: r["eval_logits"])
            held_to_fixture(where, "eval logits", ev, ref["eval"]["twin"]["logits"].numpy(), ref["eval"]["m64"]["logits"].numpy())
            held += 1
            # the weight gradient's side lane: the same bits with and without it
            if first is None:
                first = (ranks, logits, ev)
            else:
                for r0, r1 in zip(first[0], ranks):
                    for s in range(EPOCHS):
                        for name in r0["grads"][s]:
                            assert GG._same_bits(r0["grads"][s][name], r1["grads"][s][name]), (where, "lane", s, name)
                        assert r0["loss"][s] == r1["loss"][s], (where, "lane", s, "loss")
                    for name in r0["buffers"]:
                        assert GG._same_bits(r0["buffers"][name], r1["buffers"][name]), (where, "lane", name)
                assert all(GG._same_bits(a, b) for a, b in zip(first[1], logits)) and GG._same_bits(first[2], ev), (where, "lane", "logits")
    return held


def run_group_x(datasets, task, configs, P, gpu, lanes=(0,)):
    """One worker group from the seed rule to the last assertion; prints the time the workers took.  Returns the tensors held."""
    import time
    paths, data = datasets[task]
    jobs, refs, unseeded = make_jobs(data, task, configs, lanes)
    t0 = time.time()
    res = spawn_run(P, paths, gpu, task=task, jobs=jobs)
    print("%s, %d configurations x %d lanes on %d ranks (%s): %.1f s in the workers" % (
        task, len(configs), len(lanes), P, res[0][0]["hip"], time.time() - t0), flush=True)
    try:
        held = check_group_x(data, task, configs, res, refs, lanes, "-gpu" if gpu else "", bool(gpu))
    finally:
        assert_seeded(unseeded)
    return held
