"""Data, float64 definitions, bounds and worker processes of tests/test_predict.py and tests/test_predict_gpu.py (spawn start method), in
the pattern of tests/_layernorm_workers.py: the prediction kernel (csrc/pgcn_predict.hip) and checkpoint.py in both launchers."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _nodeclass_workers as NW          # noqa: E402
import _multilabel_workers as MW         # noqa: E402
import _gat_tail_workers as TW           # noqa: E402

SETS = NW.SETS
N, HIDDEN, NLAYERS = NW.N, NW.HIDDEN, NW.NLAYERS
EPOCHS, FIRST_LEG, LR, WEIGHT_SEED = 12, 5, NW.LR, NW.WEIGHT_SEED
DROPOUT, DROPOUT_SEED = NW.DROPOUT, NW.DROPOUT_SEED
# Runs whose best epoch is not the last one: at these step sizes Adam overshoots on the planted-community data and the validation
# score falls back after its first peak (the tests assert that it does).  Measured on the CPU, 12 epochs: without dropout at 0.3 the
# peak is epoch 7 (0.9948) and the last epoch scores 0.9775, 10 validation rows fewer; with dropout 0.5 at 1.5 the peak is epoch 6
# (0.9809) against 0.9671 at the end, 8 rows fewer; the GAT classifier at 0.3 peaks at epoch 2 (0.3131; at most 0.2897 later).
LR_OVERSHOOT, LR_OVERSHOOT_DROPOUT = 0.3, 1.5
# Rows that may be predicted either way when the rank count changes: a top-two gap below NEAR * max |logit|, the rule of
# _nodeclass_workers._stats64, which test_nodeclass.py holds every run to.  The same constant bounds what a probability may move.
NEAR = 1e-4

# the three configurations of the exact-resume tests: every kind of state a checkpoint carries
CONFIGS = {
    "plain": dict(launcher="PGCN", kw={}),                                                    # weights, torch's Adam
    "buffers": dict(launcher="PGCN", kw=dict(dropout=DROPOUT, dropout_seed=DROPOUT_SEED, norm="batch", optimizer="fused",
                                             weight_decay=5e-4)),                             # running statistics, dropout step, arena
    "gat": dict(launcher="PGAT", kw=dict(dropout=DROPOUT, dropout_seed=DROPOUT_SEED, optimizer="fused", lr=LR_OVERSHOOT)),
}
GAT_HEADS, GAT_HIDDEN = 2, 8

# ---- the kernel's shape grid and planted rows -------------------------------------------------------------------------------------------
GRID_C = (1, 2, 3, 4, 5, 7, 32, 33, 41, 100, 128, 256, 260, 1024)       # 256 / 260: one wave's last row width, two waves' first
GRID_N = (0, 1, 63, 64, 65, 128, 129, 513)                              # 128 / 129: a band and one row more
U = 2.0 ** -24                      # unit roundoff of fp32
EXPF_ULPS = 1.0                     # the stated bound of expf in the HIP math library: 1 ulp (= 2 U relative)
TINY = 2.0 ** -126                  # below the smallest normal number a relative bound means nothing: results there are held to this


def make_logits(n, C, seed=0, scale=3.0):
    """Random fp32 logits with the planted rows (where the shape has room): equal maxima at columns (3, 4), (0, C - 1), (255, 256); an
    all-equal row; -inf everywhere but one column; a row of +0.0 / -0.0.  Returns (X, {name: row})."""
    rng = np.random.default_rng(1000 * C + n + seed)
    X = (scale * rng.standard_normal((n, C))).astype(np.float32)
    planted, r = {}, 0

    def take(name):
        nonlocal r
        if r < n:
            planted[name] = r
            r += 1
            return r - 1
        return None

    for a, b in ((3, 4), (0, C - 1), (255, 256)):
        if b < C and a != b:
            i = take("tie%d_%d" % (a, b))
            if i is not None:
                X[i, a] = X[i, b] = np.abs(X[i]).max() + 1.0
    i = take("equal")
    if i is not None:
        X[i] = 0.75
    i = take("neginf")
    if i is not None:
        X[i] = -np.inf
        X[i, C // 2] = 1.5
    i = take("zeros")
    if i is not None:
        X[i] = np.where(np.arange(C) % 2 == 0, 0.0, -0.0).astype(np.float32)
    return X, planted


def argmax_first(X):
    """The first of a row's equal maxima, a NaN dropped and equal to nothing (-1: a row of NaN only): the rule of pgcn_masked_nll_f32."""
    n, C = X.shape
    Z = np.where(np.isnan(X), -np.inf, X)
    m = Z.max(axis=1, keepdims=True) if n else np.zeros((0, 1), X.dtype)
    first = np.where(X == m, np.arange(C)[None, :], C).min(axis=1) if n else np.zeros(0, np.int64)
    return np.where(first == C, -1, first).astype(np.int64)


def softmax64(X):
    X = X.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = X - np.where(np.isnan(X), -np.inf, X).max(axis=1, keepdims=True)
        e = np.exp(d)
        return e / e.sum(axis=1, keepdims=True), d


def sigmoid64(X):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-X.astype(np.float64)))


def sum_depth(C):
    """Additions on the longest path of the kernel's row sum: three inside a thread's quad, then one per level of the tree over the
    TPR = 2^ceil(log2(ceil(C / 4))) threads of a row (the cross-wave step of TPR = 128 / 256 is part of those levels)."""
    quads = (C + 3) // 4
    return 3 + int(np.ceil(np.log2(quads))) if quads > 1 else 3


def softmax_bounds(X):
    """(bound of prob [n, C], of conf [n], of |sum_j prob_j - 1| [n]) from the arithmetic of pgcn_predict_f32, to first order in U with every term rounded
    up: d = x - max is one rounding, |d| U on the argument, which expf turns into a relative |d| U; expf itself EXPF_ULPS ulps = 2 U
    EXPF_ULPS relative; the sum of C non-negative terms inherits at most the worst term's relative error (max |d| U + 2 U EXPF_ULPS)
    and adds one rounding per level, sum_depth(C) U; the division one more U.  conf = 1 / s takes the sum's share and the division;
    prob = e_j / s the element's share too.  Values below the smallest normal number are held to TINY instead."""
    P, d = softmax64(X)
    d = np.where(np.isfinite(d), np.abs(d), 0.0)             # (an element at -inf is an exact 0: no argument rounding)
    e_term = d * U + 2 * U * EXPF_ULPS
    s_term = e_term.max(axis=1) + sum_depth(X.shape[1]) * U
    slack = 1.0 + 64 * U                                    # the second-order terms
    conf_rel = (s_term + U) * slack
    prob_rel = (e_term + s_term[:, None] + U) * slack
    rows = prob_rel.max(axis=1) + X.shape[1] * TINY if X.shape[0] else np.zeros(0)       # |sum_j prob_j - 1| <= the worst relative error
    return prob_rel * P + TINY, conf_rel * P.max(axis=1) + TINY, rows


def sigmoid_bound(X):
    """1 / (1 + expf(-x)): the negation is exact, expf EXPF_ULPS ulps on e, of which p = 1 / (1 + e) sees the share e / (1 + e) <= 1;
    the addition and the division one rounding each."""
    return (2 * U * EXPF_ULPS + 2 * U) * (1.0 + 64 * U) * sigmoid64(X) + TINY


# ---- counts recomputed from prediction files ----------------------------------------------------------------------------------------------

def counts_from_files(prefix, labels, split, task="single"):
    """{"correct": {set: count}} or {"tp" / "fp" / "fn": {set: count}} from <prefix>.pred.npy and the label and split arrays."""
    pred = np.load(prefix + ".pred.npy")
    if task == "single":
        return {"correct": {name: int(((pred == labels) & (split == k)).sum()) for k, name in enumerate(SETS, 1)}}
    y, p = labels != 0, pred != 0
    out = {"tp": {}, "fp": {}, "fn": {}}
    for k, name in enumerate(SETS, 1):
        m = (split == k)[:, None]
        out["tp"][name], out["fp"][name], out["fn"][name] = int((p & y & m).sum()), int((p & ~y & m).sum()), int((~p & y & m).sum())
    return out


def same_entry(a, b):
    """Two history entries equal value for value (a NaN equals a NaN: an empty set's score)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same_entry(a[k], b[k]) for k in a)
    if isinstance(a, float) and isinstance(b, float) and a != a:
        return b != b
    return type(a) is type(b) and a == b


def same_state(a, b):
    """Two (nested) states equal bit for bit: the names of what differs."""
    bad = []

    def walk(x, y, at):
        if isinstance(x, torch.Tensor) or isinstance(y, torch.Tensor):
            if not (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.dtype == y.dtype and torch.equal(x, y)):
                bad.append(at)
        elif isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            if not (isinstance(x, np.ndarray) and isinstance(y, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape
                    and x.tobytes() == y.tobytes()):
                bad.append(at)
        elif isinstance(x, dict):
            if not isinstance(y, dict) or sorted(map(str, x)) != sorted(map(str, y)):
                bad.append(at + " keys")
            else:
                for k in x:
                    walk(x[k], y[k], "%s/%s" % (at, k))
        elif isinstance(x, (list, tuple)):
            if not isinstance(y, (list, tuple)) or len(x) != len(y):
                bad.append(at + " length")
            else:
                for i, (u, v) in enumerate(zip(x, y)):
                    walk(u, v, "%s/%d" % (at, i))
        elif not same_entry(x, y):
            bad.append(at)

    walk(a, b, "")
    return bad


# ---- the workers --------------------------------------------------------------------------------------------------------------------------

def _module(launcher, gpu):
    from conftest import pkg
    M = pkg(launcher)
    provider = None
    if not gpu:
        from oracle_kernels import OracleKernels
        provider = OracleKernels()              # test-only checker-backed kernels: no predict, no masked loss -> the compositions
    M._kernel_provider = provider
    M._exchanger = None
    if launcher == "PGAT":
        M.mode, M.heads = "standard", GAT_HEADS
    return M


def run_worker(rank, P, port, paths, gpu, q, launcher="PGCN", jobs=()):
    """Rank `rank` of `P` over gloo (the checker-backed kernels on the CPU, the real ones on the GPU): one process group, then
    ``launcher``.run(...) once per job, in order.  A job: {"kw": run's keyword arguments, "paths": another data set's, "nlayers",
    "pv": the part vector's key, "stub": "raise"
    (checkpoint.Hooks raises when built: the run must not touch it), "logits": True (also this rank's eval logits under the weights the
    predictions were made from)}.  Per job: history, best, stdout, the final state_dict, the owned ids -- or {"error": (type, text)} of
    a ValueError."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    import io
    from contextlib import redirect_stdout
    import torch.distributed as dist
    from conftest import pkg
    M = _module(launcher, gpu)
    CK = pkg("checkpoint")
    dist.init_process_group("gloo", rank=rank, world_size=P)
    results = []
    for job in jobs:
        kw, jp, nlayers = dict(job["kw"]), job.get("paths") or paths, job.get("nlayers", NLAYERS)
        pv = jp[job.get("pv") or "pv%d" % P]
        hooks = CK.Hooks
        if job.get("stub") == "raise":
            def refuse(*a, **k):
                raise AssertionError("checkpoint.Hooks built in a run without --save / --load / --predict / --proba")
            CK.Hooks = refuse
        buf, got = io.StringIO(), {"rank": rank}
        try:
            torch.manual_seed(WEIGHT_SEED)             # every rank draws the same initial weights (PGAT seeds itself)
            with redirect_stdout(buf):
                if launcher == "PGCN":
                    model = M.run(rank, P, nlayers, HIDDEN, jp["A"], pv, "gloo", normalize="sym", **kw)
                else:
                    model = M.run(rank, P, nlayers, 0, jp["A"], pv, "gloo", **kw)
            eng = M._engine_current
            got.update(history=model.history, best=model.best, widths=model.widths, own=eng.part.owned.cpu().numpy(),
                       state={k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()},
                       snapshot=getattr(model, "best_state", None) is not None, hip=type(eng.k).__name__)
            if job.get("logits"):
                task = M._nodeloss.TASKS[kw.get("task") or "single"]
                data = task.load(kw["features"], kw["labels"], kw["split"], eng.part.owned, int(np.load(kw["split"]).shape[0]),
                                 device=M.device)
                if model.best_state is not None:
                    CK.put_state(model, model.best_state)
                model.eval()
                with torch.no_grad():
                    got["logits"] = model(data.features).cpu().numpy()
        except ValueError as e:
            got["error"] = (type(e).__name__, str(e))
        finally:
            CK.Hooks = hooks
        got["stdout"] = buf.getvalue()
        results.append(got)
    if gpu:
        torch.cuda.synchronize()
    q.put({"rank": rank, "jobs": results})
    if M._exchanger is not None:
        M._exchanger.close()
        M._exchanger = None
    dist.barrier()
    dist.destroy_process_group()


def spawn_jobs(P, paths, gpu, launcher, jobs):
    """[per rank [per job]] of ``run_worker`` on `P` ranks (TW.spawn: a rank that dies answers at once; on the GPU the ranks share
    device 0)."""
    res = TW.spawn(run_worker, P, paths, gpu, launcher=launcher, jobs=jobs)
    return [r["jobs"] for r in res]


def data_kw(paths, task="single", **more):
    t = paths[task] if task in paths else paths
    kw = dict(features=t["features"], labels=t["labels"], split=t["split"], lr=LR)
    if task != "single":
        kw["task"] = task
    kw.update(more)
    return kw


def config_kw(name, paths, **more):
    """run's keyword arguments of one of CONFIGS on its data set."""
    c = CONFIGS[name]
    kw = data_kw(paths, hidden=GAT_HIDDEN if c["launcher"] == "PGAT" else HIDDEN, **c["kw"])
    kw.update(more)
    return kw
