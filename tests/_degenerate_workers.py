"""The degenerate part vectors -- a rank that owns nothing, a rank whose rows are in no set, a rank of one row -- the fixed configuration
lists and the groups of tests/test_degenerate.py and tests/test_degenerate_gpu.py.

Nothing is restated here.  The data, the float64 models, the seed rule, the workers and every held comparison are those of
_gradgrid_workers (GG), _optgrid_workers (OX) and _gat_tail_workers (GT): the double models know no partition, so their references and
weight seeds are the balanced tests'.  A group hands those files' own runners a copy of ``paths`` whose one key "pv<P>" names the
vector written here, looks at what the workers answered BEFORE the runner compares it (``_watch``) -- the vector is what its row of
VECTORS says, an empty rank reports losses of exactly 0.0 and logits of no rows -- and then lets the runner hold loss, logits, every
rank's reduced gradients, the buffers and the eval logits through conftest.held_to_fixture as it does under a balanced vector."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _gat_tail_workers as GT  # noqa: E402
import _gradgrid_workers as GG  # noqa: E402
import _optgrid_workers as OX  # noqa: E402

N = GG.N
VECTOR_SEED = 5
SET_LESS_ROWS = 37
BAND = 512

# name: (ranks, the rank the row is about).  E2: all zeros -- rank 1 owns nothing, rank 0 everything: both exchange rounds are empty
# on both sides.  E3: 1 + rng.integers(0, 2, n) -- rank 0, the one that reports, owns nothing; ranks 1 and 2 exchange with each other
# only.  S2: zeros, 1 on the first 37 vertices in no set -- rank 1's train, val and test records are empty, yet it has a halo and
# sends rows.  O2: zeros, 1 on the first train vertex with a neighbour -- rank 1 owns one row: the first row of a 512-row band alone.
VECTORS = {"E2": (2, 1), "E3": (3, 0), "S2": (2, 1), "O2": (2, 1)}


def degrees(data):
    """Neighbours of every vertex (stored entries of its row off the diagonal; the planted graphs are undirected)."""
    A = data["A"].tocoo()
    return np.bincount(A.row[A.row != A.col], minlength=A.shape[0])


def part_vector(name, data):
    """The vector ``name`` for the task whose arrays ``data`` are, as an int array of n entries."""
    rng = np.random.default_rng(VECTOR_SEED)
    n = data["A"].shape[0]
    pv = np.zeros(n, np.int64)
    if name == "E3":
        pv = 1 + rng.integers(0, 2, n)
    elif name == "S2":
        pv[np.flatnonzero(data["split"] == 0)[:SET_LESS_ROWS]] = 1
    elif name == "O2":
        pv[np.flatnonzero((data["split"] == 1) & (degrees(data) >= 1))[:1]] = 1
    else:
        assert name == "E2", name
    return pv


def with_vector(paths, name, data, dirname, task):
    """A copy of ``paths`` whose "pv<P>" is the vector ``name``, written in the format of sbm.P.rp."""
    P = VECTORS[name][0]
    path = os.path.join(dirname, "%s.%s.%d.rp" % (name, task, P))
    with open(path, "w") as fh:
        fh.write(" ".join(map(str, part_vector(name, data).tolist())) + "\n")
    return dict(paths, **{"pv%d" % P: path})


def check_vector(name, owns, data):
    """Conditions on the INPUT, from the ranks' reported ``own`` arrays and the split: the vector is what its row says."""
    P, who = VECTORS[name]
    assert len(owns) == P and sorted(np.concatenate(owns).tolist()) == list(range(N)), name
    split = data["split"]
    if name in ("E2", "E3"):
        assert owns[who].size == 0, (name, owns[who].size)
    if name == "E3":
        assert all(owns[r].size >= BAND + 1 for r in (1, 2)), (name, [o.size for o in owns])
    if name == "S2":
        assert owns[who].size == SET_LESS_ROWS and (split[owns[who]] == 0).all(), (name, owns[who].size)
    if name == "O2":
        assert owns[who].size == 1 and split[owns[who][0]] == 1 and degrees(data)[owns[who][0]] >= 1, (name, owns[who])


def check_empty_rank(name, answers, classes, epochs, where):
    """An empty rank's answers (one per configuration and lane): ``epochs`` losses of exactly 0.0 and logits of shape (0, C), training
    and eval; with max aggregation every recorded (input, OUT, ARG) has no rows -- the rank made the calls and is not passed over."""
    if name not in ("E2", "E3"):
        return
    for a in answers[VECTORS[name][1]]:
        at = (where, name, a["tag"])
        assert a["loss"] == [0.0] * epochs, (at, a["loss"])
        assert [v.shape for v in a["logits"]] == [(0, classes)] * epochs and a["eval_logits"].shape == (0, classes), at
        for _, H, OUT, ARG in a.get("calls", ()):
            assert H.shape[0] == OUT.shape[0] == ARG.shape[0] == 0 and OUT.shape == ARG.shape and ARG.dtype == np.int32, at


# ---- the configuration lists ------------------------------------------------------------------------------------------------------------

def pgcn_configs():
    """The plain layer with dropout and a skip connection (the kind whose backward unpacks the sign mask); width 30, where the fused
    kernels refuse on the device, so that the library route and the keep-words kernel run: plain with dropout, batch norm + root weight
    + dropout, node norm + residual + dropout."""
    return [GG.config("none", residual=True, dropout=GG.DROPOUT), GG.config("none", dropout=GG.DROPOUT, hidden=30),
            GG.width_axis(30)[1], GG.width_axis(30)[2]]


def newer_configs(half=None):
    """Max aggregation, DropEdge and APPNP with K = 1 and K = 3: the six of the balanced two- and three-rank groups, as they stand.
    ``half`` 0 / 1: the first / the last three of them (``newer_cases``)."""
    six = OX.rank_subset_x()
    return six if half is None else six[3 * half:3 * half + 3]


def gat_configs(task):
    return [GT.options(K=2, hidden=8, Ko=Ko, bias=b, elu=True, dropout=d, task=task)
            for b in (0, 1) for d in (0.0, GT.DROPOUT) for Ko in (1, 2)]


# vector: (tasks of the PGCN list, of the newer-options list, of the GAT list) -- 14 groups, of which ``newer_cases`` runs two as two
# worker groups each: 16, the same on the CPU and on the device
GROUPS = {"E2": (GG.TASKS, GG.TASKS, ("single",)), "E3": (("multilabel",), ("single",), ("multilabel",)),
          "S2": (("single",), ("multilabel",), ("multilabel",)), "O2": (("multilabel",), ("single",), ("single",))}


def cases(kind):
    return [(v, task) for v in GROUPS for task in GROUPS[v][("pgcn", "newer", "gat").index(kind)]]


def newer_cases():
    """(vector, task, half) of the newer-options groups.  A multi-label group of all six on two ranks took 8.3 - 9.9 s on the device,
    lane 0 alone, against the 7.8 - 8.3 s of the balanced test_gradgrid_gpu.test_ranks_hold_the_reduced_gradient[single-2-lanes0],
    the longest a group here may take: most of it on the host (the seed rule, the definition of every recorded selection at 41
    labels, a double reference under the recorded selection per max configuration).  Those run as two worker groups of three."""
    return [(v, task, half) for v, task in cases("newer")
            for half in ((0, 1) if task == "multilabel" and VECTORS[v][0] == 2 else (None,))]


# ---- the groups ---------------------------------------------------------------------------------------------------------------------------

def lanes_of(name, gpu):
    """The PGCN groups on two ranks on the device: with and without the weight gradient's side lane, as the balanced test."""
    return (0, 1) if gpu and VECTORS[name][0] == 2 else (0,)


class _watch:
    """While it is entered, ``module.spawn_run`` hands its answer to ``look`` before the module's runner compares it."""

    def __init__(self, module, look):
        self.module, self.look = module, look

    def __enter__(self):
        self.saved = spawn = self.module.spawn_run

        def watched(*a, **kw):
            res = spawn(*a, **kw)
            self.look(res)
            return res
        self.module.spawn_run = watched

    def __exit__(self, *exc):
        self.module.spawn_run = self.saved


def _logged(f):
    """f() -> (its answer, the number of pairs it sent to the parity log, the largest err_hip / bound among them)."""
    from conftest import OBSERVED_LOG
    import json
    start = os.path.getsize(OBSERVED_LOG) if os.path.exists(OBSERVED_LOG) else 0
    out = f()
    pairs = []
    if os.path.exists(OBSERVED_LOG):
        with open(OBSERVED_LOG) as fh:
            fh.seek(start)
            pairs = [json.loads(line) for line in fh if line.strip()]
    return out, len(pairs), max([p["err_hip"] / p["bound"] for p in pairs], default=0.0)


def _report(kind, name, task, gpu, held, pairs, worst, t0):
    import time
    print("degenerate%s %s %s %s: %d tensors held, %d pairs in the parity log, largest err_hip / bound %.3f, %.1f s" % (
        "-gpu" if gpu else "", kind, name, task, held, pairs, worst, time.time() - t0), flush=True)


def _grid_group(kind, W, run, configs, datasets, dirname, name, task, gpu, lanes=None):
    import time
    t0 = time.time()
    paths, data = datasets[task]
    P = VECTORS[name][0]
    lanes = lanes_of(name, gpu) if lanes is None else lanes
    classes = GG.widths_of(task, configs[0])[-1]

    def look(res):
        assert all(len(r) == len(configs) * len(lanes) for r in res)
        for k in range(len(res[0])):
            check_vector(name, [r[k]["own"] for r in res], data)
        check_empty_rank(name, res, classes, GG.EPOCHS, kind)
        if gpu:
            assert all(a["hip"] == "HipKernels" for r in res for a in r), kind

    with _watch(W, look):
        held, pairs, worst = _logged(lambda: run({task: (with_vector(paths, name, data, dirname, task), data)}, task, configs, P, gpu, lanes=lanes))
    assert held > 0
    _report(kind, name, task, gpu, held, pairs, worst, t0)
    return held


def pgcn_group(datasets, dirname, name, task, gpu, configs=None, lanes=None):
    """GG.run_group of the PGCN list under the vector ``name``; returns the tensors held."""
    return _grid_group("pgcn", GG, GG.run_group, pgcn_configs() if configs is None else configs, datasets, dirname, name, task, gpu, lanes)


def newer_group(datasets, dirname, name, task, gpu, half=None):
    """OX.run_group_x of the newer options under the vector ``name``: it holds every recorded (OUT, ARG) of max aggregation to the
    definition bit for bit with the rows of EVERY rank scattered by ``own`` -- an empty rank contributes its calls and no rows.
    Lane 0 alone, on the device too: with the side lane's repeat a two-rank group of these six took longer there than the balanced
    test_gradgrid_gpu.test_ranks_hold_the_reduced_gradient[single-2-lanes0], the longest a group here may take (8.3 - 10.0 s against
    7.8 s; the seed rule and the selections' oracle run on the host).  The PGCN groups keep the repeat.  ``half``: ``newer_cases``."""
    return _grid_group("newer", OX, OX.run_group_x, newer_configs(half), datasets, dirname, name, task, gpu, lanes=(0,))


def gat_group(gat_datasets, dirname, name, task, gpu):
    """GT.grad_worker on the eight GAT configurations under the vector ``name``, held exactly as
    test_gat_tail.test_whole_model_gradients_of_every_option holds its grid: GT.hold_steps, the dropout / no-dropout comparison of the
    two steps' logits, the eval logits."""
    import time
    from conftest import held_to_fixture
    t0 = time.time()
    paths, data = gat_datasets
    P = VECTORS[name][0]
    grid = gat_configs(task)
    assert len(grid) == 8
    refs = [GT.reference(data[task], o, 0, 2, 0.0) for o in grid]
    jobs = [{"opts": o, "params": {k: v.numpy() for k, v in r["params"].items()}} for o, r in zip(grid, refs)]
    res = GT.spawn(GT.grad_worker, P, with_vector(paths, name, data[task], dirname, task), gpu, jobs=jobs, n=N)
    answers = [r["results"] for r in res]
    assert all(len(a) == len(grid) for a in answers)
    check_vector(name, [a[0]["own"] for a in answers], data[task])
    check_empty_rank(name, answers, GT.classes_of(data[task], grid[0]), 2, "gat")
    if gpu:
        assert all(x["hip"] == "HipKernels" for a in answers for x in a)

    def hold():
        held = 0
        for j, (o, ref) in enumerate(zip(grid, refs)):
            ranks = [dict(r["results"][j], rank=r["rank"]) for r in res]
            where = "degenerate%s/gat/%s/%s/P%d" % ("-gpu" if gpu else "", name, GT.tag(o), P)
            assert all(r["tag"] == GT.tag(o) for r in ranks)
            held += GT.hold_steps(where, ranks, ref, N, 2)
            logits = [GT.rows(ranks, lambda r, s=s: r["logits"][s], N) for s in range(2)]
            if o["dropout"] > 0:
                assert not np.array_equal(logits[0], logits[1]), where + ": the second step drew the first step's masks"
            else:
                assert np.array_equal(logits[0], logits[1]), where
            held_to_fixture(where, "eval logits", GT.rows(ranks, lambda r: r["eval_logits"], N), ref["twin"]["eval"][-1].numpy(),
                            ref["m64"]["eval"][-1].numpy())
            held += 1
        return held

    held, pairs, worst = _logged(hold)
    assert held > 0
    _report("gat", name, task, gpu, held, pairs, worst, t0)
    return held
