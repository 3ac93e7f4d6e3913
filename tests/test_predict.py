"""checkpoint.py and the prediction rules on the CPU (the checker-backed provider, world sizes 1 and 2 over gloo; 3 for loading): the
composition of pgcn_predict_f32's rules, exact resume in three configurations, the best snapshot against the best record, the
prediction files, partition independence, the refusals, the unchanged path without the options, and the command lines."""
import os

import numpy as np
import pytest
import torch

import _predict_workers as W
from conftest import gpath, pkg


# ---- the rules, from framework operations -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 4, 5, 33, 260])
def test_composed_predictions_follow_the_kernels_rules(C):
    NL, ND = pkg("nodeloss"), pkg("nodedata")
    n = 65
    X, planted = W.make_logits(n, C)
    X[40, C // 2] = np.nan                                   # a NaN is dropped from the maximum and equals nothing
    X[41] = np.nan                                           # a row of NaN only: no class
    Xt = torch.from_numpy(X)
    single = NL.predict_composed(Xt, "single", want_conf=True, want_prob=True)
    multi = NL.predict_composed(Xt, "multilabel", want_prob=True)
    want = W.argmax_first(X)
    assert want[41] == -1 and single.cls.dtype is torch.int64 and np.array_equal(single.cls.numpy(), want)
    assert multi.bits.dtype is torch.int32 and np.array_equal(multi.bits.numpy().view(np.uint32), ND.pack_label_words(X > 0))
    assert single.bits is None and multi.cls is None and multi.conf is None
    ok = ~np.isnan(X).any(axis=1)
    # the sums of torch's CPU kernels have their own order: the bound of the kernel with a sequential sum's depth, C - 1 roundings
    P64, _ = W.softmax64(X[ok])
    bp, bc, _ = W.softmax_bounds(X[ok])
    extra = (C * W.U) * P64
    assert (np.abs(single.prob.numpy()[ok].astype(np.float64) - P64) <= bp + extra).all()
    assert (np.abs(single.conf.numpy()[ok].astype(np.float64) - P64.max(axis=1)) <= bc + extra.max(axis=1)).all()
    assert (np.abs(multi.prob.numpy()[ok].astype(np.float64) - W.sigmoid64(X[ok])) <= W.sigmoid_bound(X[ok])).all()
    only = NL.predict_composed(Xt, "single", want_conf=False)
    assert only.conf is None and only.prob is None and torch.equal(only.cls, single.cls)
    assert NL.predict_kernels(object(), Xt) is None and NL.predict_kernels(None, Xt) is None        # the gate: CPU tensors, no provider


# ---- end to end over gloo -----------------------------------------------------------------------------------------------------------------

RESUMED = ("plain", "buffers")


def _resume_jobs(d, name, paths):
    kw = W.config_kw(name, paths)
    return [dict(kw=dict(kw, epochs=W.EPOCHS, save="%s/%s_straight.pt" % (d, name))),
            dict(kw=dict(kw, epochs=W.FIRST_LEG, save="%s/%s_leg.pt" % (d, name))),
            dict(kw=dict(kw, epochs=W.EPOCHS - W.FIRST_LEG, load="%s/%s_leg.pt" % (d, name), save="%s/%s_resumed.pt" % (d, name)))]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("predict"))
    paths, data = W.NW.make_dataset(d)
    os.makedirs(d + "/ml")
    ml_paths, ml_data = W.MW.make_dataset(d + "/ml")
    return d, paths, data, ml_paths, ml_data


_groups = {}


def _group(P, dataset):
    """One group of `P` ranks, every PGCN job of this file in order, run once: (P, directory, {name: per-rank results})."""
    if (P, dataset[0]) not in _groups:
        _groups[(P, dataset[0])] = _run_group(P, dataset)
    return _groups[(P, dataset[0])]


@pytest.fixture(params=[1, 2])
def pgcn(request, dataset):
    return _group(request.param, dataset)


def _run_group(P, dataset):
    d, paths, data, ml_paths, ml_data = dataset
    d = "%s/P%d" % (d, P)
    os.makedirs(d)
    names, jobs = [], []
    for name in RESUMED:
        names += [name + "_straight", name + "_leg", name + "_resumed"]
        jobs += _resume_jobs(d, name, paths)
    plain = W.config_kw("plain", paths, epochs=W.EPOCHS)
    names += ["untouched", "nodrop", "drop", "multilabel"]
    jobs += [dict(kw=plain, stub="raise"),
             dict(kw=dict(plain, lr=W.LR_OVERSHOOT, predict=d + "/nodrop")),
             dict(kw=dict(plain, lr=W.LR_OVERSHOOT_DROPOUT, dropout=W.DROPOUT, dropout_seed=W.DROPOUT_SEED, save=d + "/drop.pt",
                          predict=d + "/drop", proba=True), logits=True),
             dict(kw=W.data_kw(ml_paths, task="multilabel", hidden=W.HIDDEN, epochs=W.EPOCHS, lr=W.LR_OVERSHOOT, predict=d + "/ml", proba=True),
                  paths=ml_paths)]
    res = W.spawn_jobs(P, paths, False, "PGCN", jobs)
    for r in res:
        assert [j.get("error") for j in r] == [None] * len(jobs)
    return P, d, {name: [r[i] for r in res] for i, name in enumerate(names)}


def _check_exact_resume(d, name, straight_job, resumed_job, best_in_first_leg=False):
    straight, resumed = (torch.load("%s/%s_%s.pt" % (d, name, leg), weights_only=True) for leg in ("straight", "resumed"))
    assert straight["epochs"] == resumed["epochs"] == W.EPOCHS
    keys = ("format", "launcher", "arch", "model", "optimizer", "dropout_step", "best")
    assert W.same_state({k: straight[k] for k in keys}, {k: resumed[k] for k in keys}) == []          # bit for bit
    assert straight["optimizer"]["kind"] == W.CONFIGS[name]["kw"].get("optimizer", "torch")
    assert straight["dropout_step"] == (W.EPOCHS if "dropout" in W.CONFIGS[name]["kw"] else 0)
    assert [h["epoch"] for h in resumed["history"]] == list(range(W.EPOCHS))
    for a, b in zip(straight["history"], resumed["history"]):
        assert W.same_entry(a, b), (a, b)
    for a, b in zip(straight_job, resumed_job):                                                      # on every rank
        assert W.same_state(a["state"], b["state"]) == [] and W.same_entry(a["best"], b["best"])
        assert [h["epoch"] for h in b["history"][W.FIRST_LEG:]] == list(range(W.FIRST_LEG, W.EPOCHS))
    if best_in_first_leg:
        assert 0 <= straight["best"]["entry"]["epoch"] < W.FIRST_LEG
    return straight


@pytest.mark.parametrize("name", RESUMED)
def test_exact_resume(pgcn, name):
    """Twelve epochs straight against five, save, load, seven more (eval_every = 1): the model, the optimiser state, the dropout step,
    the history and ``best`` are equal bit for bit -- plain layers with torch's Adam; dropout + batch norm + the fused optimiser +
    weight decay (buffers, dropout step, arena)."""
    P, d, res = pgcn
    ck = _check_exact_resume(d, name, res[name + "_straight"], res[name + "_resumed"])
    if name == "buffers":
        assert any("running_mean" in k for k in ck["model"]) and ck["optimizer"]["state"]["step"] == W.EPOCHS
        leg = torch.load("%s/%s_leg.pt" % (d, name), weights_only=True)
        assert leg["dropout_step"] == leg["epochs"] == leg["optimizer"]["state"]["step"] == W.FIRST_LEG


@pytest.mark.parametrize("P", [1, 2])
def test_exact_resume_of_the_gat_classifier(tmp_path, P):
    """The PGAT classifier with dropout and the fused optimiser; its best epoch lies inside the first leg and carries over."""
    d = str(tmp_path)
    paths, _ = W.TW.make_datasets(d)
    res = W.spawn_jobs(P, paths, False, "PGAT", _resume_jobs(d, "gat", paths))
    for r in res:
        assert [j.get("error") for j in r] == [None] * 3
    ck = _check_exact_resume(d, "gat", [r[0] for r in res], [r[2] for r in res], best_in_first_leg=True)
    assert ck["launcher"] == "PGAT" and ck["arch"]["heads"] == W.GAT_HEADS and ck["arch"]["out_heads"] == 1


def test_without_the_options_nothing_is_touched(pgcn):
    """A run without the four options builds no checkpoint.Hooks (the stub raises if it were), prints the lines and returns the weights,
    bit for bit, of the same run with --save, whose hooks only read."""
    P, d, res = pgcn
    for plain, saved in zip(res["untouched"], res["plain_straight"]):
        lines = lambda r: [l for l in r["stdout"].splitlines() if not l.startswith("Elapsed time")]      # noqa: E731
        assert lines(plain) == lines(saved)
        assert plain["rank"] != 0 or len([l for l in lines(plain) if l.startswith("Epoch ")]) == W.EPOCHS
        assert W.same_state(plain["state"], saved["state"]) == []
        assert all(W.same_entry(a, b) for a, b in zip(plain["history"], saved["history"])) and W.same_entry(plain["best"], saved["best"])
        assert not plain["snapshot"] and sorted(plain["best"]) == sorted(saved["best"])


@pytest.mark.parametrize("path", ["nodrop", "drop"])
def test_predictions_of_the_best_snapshot_recompute_the_best_record(pgcn, dataset, path):
    """The best epoch is not the last one; the files written from the snapshot give exactly ``best["correct"]`` per set.  Without
    dropout (and without batch norm) the record is the training step's own: the values before that step's update; with dropout it is
    ``evaluate``'s after the update."""
    P, d, res = pgcn
    _, _, data, _, _ = dataset
    r = res[path][0]
    best = r["best"]
    got = W.counts_from_files("%s/%s" % (d, path), data["labels"], data["split"])
    print("P = %d, %s: best epoch %d, correct %r, from pred.npy %r; last epoch %r" % (P, path, best["epoch"], best["correct"], got["correct"],
                                                                                     r["history"][-1]["correct"]))
    assert 0 <= best["epoch"] < W.EPOCHS - 1, "the best epoch must not be the last one"
    assert r["history"][-1]["correct"] != best["correct"]
    assert got["correct"] == best["correct"]
    assert r["snapshot"] and "Predicting with the weights of the best epoch %05d" % best["epoch"] in r["stdout"]
    assert all("Predicting" not in other["stdout"] for other in res[path][1:])                       # rank 0 alone prints


def test_multilabel_predictions_recompute_tp_fp_fn(pgcn, dataset):
    P, d, res = pgcn
    _, _, _, _, ml = dataset
    best = res["multilabel"][0]["best"]
    got = W.counts_from_files(d + "/ml", ml["labels"], ml["split"], task="multilabel")
    print("P = %d, multilabel: best epoch %d, tp %r fp %r fn %r" % (P, best["epoch"], best["tp"], best["fp"], best["fn"]))
    assert got == {k: best[k] for k in ("tp", "fp", "fn")}


def test_prediction_files(pgcn, dataset):
    """Shapes and dtypes of the table; pred.npy is accepted as --labels; rows in no set are predicted; no temporary file is left."""
    P, d, res = pgcn
    _, paths, data, ml_paths, ml = dataset
    ND = pkg("nodedata")
    n, C = W.N, W.NW.CLASSES
    pred, conf, prob = (np.load("%s/drop.%s.npy" % (d, k)) for k in ("pred", "conf", "prob"))
    assert (pred.dtype, pred.shape, conf.dtype, conf.shape, prob.dtype, prob.shape) == (np.int64, (n,), np.float32, (n,), np.float32, (n, C))
    assert not os.path.exists(d + "/nodrop.prob.npy") and os.path.exists(d + "/nodrop.conf.npy")      # --proba was not given
    ND.open_checked(paths["features"], d + "/drop.pred.npy", paths["split"], n)
    none = data["split"] == 0
    assert none.sum() > 100 and ((pred[none] >= 0) & (pred[none] < C)).all() and (conf[none] > 1.0 / C - 1e-6).all()
    assert np.array_equal(conf, prob[np.arange(n), pred]) and np.array_equal(conf, prob.max(axis=1))
    assert np.abs(prob.sum(axis=1) - 1.0).max() < 1e-5
    mp_, mprob = np.load(d + "/ml.pred.npy"), np.load(d + "/ml.prob.npy")
    L = W.MW.LABELS
    assert (mp_.dtype, mp_.shape, mprob.dtype, mprob.shape) == (np.uint8, (n, L), np.float32, (n, L)) and not os.path.exists(d + "/ml.conf.npy")
    assert set(np.unique(mp_)) <= {0, 1} and (mprob[mp_ != 0] >= 0.5).all() and (mprob[mp_ == 0] <= 0.5).all()
    ND.open_checked_multilabel(ml_paths["features"], d + "/ml.pred.npy", ml_paths["split"], n)
    assert mp_[ml["split"] == 0].any()
    assert not [f for f in os.listdir(d) if f.endswith(".tmp")]


@pytest.mark.parametrize("Q", [1, 3])
def test_a_checkpoint_of_two_ranks_loads_on_one_and_on_three(dataset, Q):
    """--load --epochs 0 --predict --proba under the other part vectors: prob.npy within W.NEAR max |logit| (the margin the suite gives
    logits across rank counts), pred.npy equal on every row that _nodeclass_workers._stats64 does not call near."""
    P, d, res = _group(2, dataset)
    _, paths, data, _, _ = dataset
    kw = W.config_kw("plain", paths, epochs=0, lr=W.LR_OVERSHOOT_DROPOUT, dropout=W.DROPOUT, dropout_seed=W.DROPOUT_SEED, load=d + "/drop.pt",
                     predict="%s/from%d" % (d, Q), proba=True)
    got = W.spawn_jobs(Q, paths, False, "PGCN", [dict(kw=kw)])
    assert all(r[0].get("error") is None for r in got)
    assert W.same_entry(got[0][0]["best"], res["drop"][0]["best"]) and len(got[0][0]["history"]) == W.EPOCHS
    assert "Epoch " not in got[0][0]["stdout"]                                                       # nothing is trained
    logits = W.NW.gather_rows(res["drop"], "logits", W.N)
    near = W.NW._stats64(torch.from_numpy(logits).double(), data["labels"], data["split"])["near_rows"]
    prob2, probq = np.load(d + "/drop.prob.npy"), np.load("%s/from%d.prob.npy" % (d, Q))
    pred2, predq = np.load(d + "/drop.pred.npy"), np.load("%s/from%d.pred.npy" % (d, Q))
    worst, tol = float(np.abs(prob2 - probq).max()), W.NEAR * float(np.abs(logits).max())
    print("2 ranks -> %d: largest probability difference %.3g (tolerance %.3g), %d near rows, %d predictions differ"
          % (Q, worst, tol, int(near.sum()), int((pred2 != predq).sum())))
    assert worst <= tol and not ((pred2 != predq) & ~near).any()
    assert near.sum() <= 0.01 * W.N
    # every row was written by its owner under the other part vector
    assert sorted(np.concatenate([r[0]["own"] for r in got]).tolist()) == list(range(W.N))


def test_refusals_raise_on_every_rank_before_any_collective(dataset, tmp_path):
    """A checkpoint of another width, layer count, task, norm, optimiser kind or launcher, a truncated file, --proba without
    --predict, an option without the data files: a ValueError on BOTH ranks (a rank that went on into a collective alone would hang
    the group, and the job after the refusals would never report)."""
    P, d, res = _group(2, dataset)
    _, paths, data, ml_paths, _ = dataset
    ck = d + "/plain_straight.pt"
    cut = str(tmp_path / "cut.pt")
    with open(ck, "rb") as f, open(cut, "wb") as g:
        g.write(f.read()[:4000])
    base = W.config_kw("plain", paths, epochs=0, load=ck)
    bad = [("widths differs", dict(kw=dict(base, hidden=16))), ("layers differs", dict(kw=base, nlayers=3)),
           ("task differs", dict(kw=W.data_kw(ml_paths, task="multilabel", hidden=W.HIDDEN, epochs=0, load=ck), paths=ml_paths)),
           ("norm differs", dict(kw=dict(base, norm="batch"))), ("optimizer differs", dict(kw=dict(base, optimizer="fused"))),
           ("dropout differs", dict(kw=dict(base, dropout=0.25))),
           ("not a readable checkpoint", dict(kw=dict(base, load=cut))),
           ("proba needs predict", dict(kw=dict(base, proba=True))),
           ("need features, labels and split", dict(kw=dict(save=d + "/x.pt"))), ("need features, labels and split", dict(kw=dict(load=ck))),
           ("need features, labels and split", dict(kw=dict(predict=d + "/x"))), ("need features, labels and split", dict(kw=dict(proba=True)))]
    jobs = [j for _, j in bad] + [dict(kw=dict(base, predict=d + "/after"))]
    got = W.spawn_jobs(2, paths, False, "PGCN", jobs)
    for r in got:
        for (text, _), j in zip(bad, r):
            assert j.get("error") is not None and j["error"][0] == "ValueError" and text in j["error"][1], (text, j.get("error"))
        assert r[-1].get("error") is None
    assert os.path.exists(d + "/after.pred.npy") and not os.path.exists(d + "/x.pt")
    # the other launcher
    g = str(tmp_path / "gat")
    os.makedirs(g)
    gpaths, _ = W.TW.make_datasets(g)
    got = W.spawn_jobs(2, gpaths, False, "PGAT", [dict(kw=W.config_kw("gat", gpaths, epochs=0, load=ck)),
                                                  dict(kw=W.config_kw("gat", gpaths, epochs=0, proba=True))])
    for r in got:
        assert r[0]["error"][0] == "ValueError" and "launcher differs" in r[0]["error"][1] and "proba needs predict" in r[1]["error"][1]


def test_checkpoint_module_round_trip(tmp_path):
    """checkpoint.save / load on their own: the fields, weights_only loading, the temporary name, the differing field named."""
    CK = pkg("checkpoint")
    path = str(tmp_path / "m.pt")
    arch = CK.architecture([4, 8, 3], "single", dropout=0.5, dropout_seed=7, norm="batch")
    model = {"0.linear.weight": torch.randn(8, 4), "0.bn.running_mean": torch.zeros(8)}
    entry = {"epoch": 3, "val": 0.5, "test": float("nan"), "correct": {"train": 1, "val": 2, "test": 3}}
    calls = []
    CK.save(path, "PGCN", arch, model, "fused", {"step": 4, "state": {0: {"exp_avg": torch.ones(3), "exp_avg_sq": torch.ones(3)}}}, 4, 4,
            [entry], entry, model, rank=0, barrier=lambda: calls.append(1))
    assert calls == [1] and os.listdir(str(tmp_path)) == ["m.pt"]
    CK.save(str(tmp_path / "other.pt"), "PGCN", arch, model, "fused", {}, 4, 4, [], rank=1, barrier=lambda: calls.append(2))
    assert calls == [1, 2] and os.listdir(str(tmp_path)) == ["m.pt"]                                 # rank 0 alone writes
    ck = CK.load(path, "PGCN", arch, "fused")
    assert ck["format"] == CK.FORMAT_VERSION and ck["epochs"] == 4 and ck["dropout_step"] == 4 and W.same_entry(ck["history"][0], entry)
    assert W.same_state(ck["model"], model) == [] and W.same_state(ck["best"]["model"], model) == [] and ck["optimizer"]["state"]["step"] == 4
    for field, other in (("widths", CK.architecture([4, 9, 3], "single", 0.5, 7, "batch")), ("layers", CK.architecture([4, 8, 8, 3], "single", 0.5, 7, "batch")),
                         ("task", CK.architecture([4, 8, 3], "multilabel", 0.5, 7, "batch")), ("norm", CK.architecture([4, 8, 3], "single", 0.5, 7)),
                         ("dropout_seed", CK.architecture([4, 8, 3], "single", 0.5, 8, "batch")),
                         ("root_weight", CK.architecture([4, 8, 3], "single", 0.5, 7, "batch", root_weight=True)),
                         ("heads", CK.architecture([4, 8, 3], "single", 0.5, 7, "batch", heads=2))):
        with pytest.raises(ValueError, match=field + " differs"):
            CK.load(path, "PGCN", other, "fused")
    with pytest.raises(ValueError, match="launcher differs"):
        CK.load(path, "PGAT", arch, "fused")
    with pytest.raises(ValueError, match="optimizer differs"):
        CK.load(path, "PGCN", arch, "torch")
    with pytest.raises(ValueError, match="not a readable checkpoint"):
        CK.load(str(tmp_path / "absent.pt"))
    torch.save({"format": 1}, str(tmp_path / "foreign.pt"))
    with pytest.raises(ValueError, match="not a checkpoint of this project"):
        CK.load(str(tmp_path / "foreign.pt"))


# ---- the command lines --------------------------------------------------------------------------------------------------------------------

BASE = ["-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"), "-b", "gloo", "-s", "1", "-l", "2", "-f", "16"]


def _keep_cli_state(monkeypatch, M):
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        if k in os.environ:
            monkeypatch.setenv(k, os.environ[k])
        else:
            monkeypatch.delenv(k, raising=False)
    for name in ("path_A", "path_partvec"):
        monkeypatch.setattr(M, name, getattr(M, name, None), raising=False)
    if hasattr(M, "mode"):                                   # (PGAT's main keeps the module's values where a flag is absent)
        monkeypatch.setattr(M, "mode", "standard")
        monkeypatch.setattr(M, "heads", 1)


class _Inline:
    tuples = []

    def __init__(self, target, args):
        self.target, self.args, self.exitcode = target, args, None
        _Inline.tuples.append(args)

    def start(self):
        self.target(*self.args)
        self.exitcode = 0

    def join(self):
        pass


@pytest.mark.parametrize("launcher", ["PGCN", "PGAT"])
def test_cli_forwards_the_options(monkeypatch, dataset, tmp_path, launcher):
    M = pkg(launcher)
    _keep_cli_state(monkeypatch, M)
    paths = dataset[1]
    seen = []
    _Inline.tuples = []
    monkeypatch.setattr(M.mp, "Process", _Inline)
    monkeypatch.setattr(M.mp, "set_start_method", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "init_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "destroy_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M, "run", lambda *a, **k: seen.append((a, k)))
    files = ["--features", paths["features"], "--labels", paths["labels"], "--split", paths["split"]]
    ck = str(tmp_path / "m.pt")
    open(ck, "wb").close()
    M.main(BASE + files)
    M.main(BASE + files + ["--save", ck])
    M.main(BASE + files + ["--load", ck, "--epochs", "0", "--predict", "out", "--proba"])
    three = {"features": paths["features"], "labels": paths["labels"], "split": paths["split"]}
    assert seen[0][1] == three                                                                       # none given: the call of before
    assert seen[1][1] == dict(three, save=ck)
    assert seen[2][1] == dict(three, load=ck, epochs=0, predict="out", proba=True)
    if launcher == "PGCN":           # the argument tuple grows only when one of the four is given
        assert [len(t) for t in _Inline.tuples] == [19, 30, 30] and _Inline.tuples[1][-4:] == (ck, None, None, None)


@pytest.mark.parametrize("launcher", ["PGCN", "PGAT"])
@pytest.mark.parametrize("bad,text", [(["--save", "m.pt"], "need them"), (["--load", "m.pt"], "need them"), (["--predict", "out"], "need them"),
                                      (["--proba"], "need them"), ("FILES+--proba", "--proba needs --predict"),
                                      ("FILES+--load /nonexistent/m.pt", "--load: no such file")])
def test_cli_refusals(monkeypatch, dataset, capsys, launcher, bad, text):
    M = pkg(launcher)
    _keep_cli_state(monkeypatch, M)
    paths = dataset[1]
    if isinstance(bad, str):
        bad = ["--features", paths["features"], "--labels", paths["labels"], "--split", paths["split"]] + bad.split("+")[1].split()
    with pytest.raises(SystemExit) as e:
        M.main(BASE + bad)
    out = capsys.readouterr().out
    assert e.value.code == 2 and text in out, out
    if text == "need them":
        assert "--save, --load, --predict, --proba" in out and bad[0] in out.split("got ")[1]
