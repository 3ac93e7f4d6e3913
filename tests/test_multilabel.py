"""Multi-label node classification (nodedata.load_multilabel / pack_label_words, PGCN.masked_bce_loss / masked_bce_stats /
evaluate_multilabel, run(task="multilabel"), --task) -- the CPU side: the packed label words, the loader, the framework composition
of the masked BCE against float64 numpy, partition independence over gloo with the checker-backed kernels against a float64
restatement of the model, and the command line.  The kernels are held in test_multilabel_gpu.py."""
import os

import numpy as np
import pytest
import torch

import _multilabel_workers as W
from conftest import gpath, pkg


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("multilabel")))


@pytest.fixture(scope="module")
def reference(dataset):
    return W.float64_reference(dataset[1], [W.FIN, W.HIDDEN, W.LABELS])


# ---- the packed label words ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 31, 32, 33, 100])
def test_pack_unpack_round_trip(C):
    nd, P = pkg("nodedata"), pkg("PGCN")
    rng = np.random.default_rng(C)
    a = (rng.random((37, C)) < 0.4).astype(np.uint8)
    a[0, :], a[1, :] = 0, 1
    w = nd.pack_label_words(a)
    assert w.dtype == np.uint32 and w.shape == (37, (C + 31) // 32)
    for i, j in ((1, 0), (1, C - 1), (5, C // 2), (36, C - 1)):                           # bit b of word w = label 32 w + b
        assert (int(w[i, j // 32]) >> (j % 32)) & 1 == int(a[i, j])
    if C % 32:
        assert not (w[:, -1] >> np.uint32(C % 32)).any()                                 # nothing at or above C
    assert np.array_equal(nd.unpack_label_words(w, C), a)
    assert np.array_equal(nd.unpack_label_words(w.view(np.int32), C), a)
    assert np.array_equal(nd.pack_label_words(a * 7), w)                                 # any nonzero is a 1
    words = torch.from_numpy(w.view(np.int32))
    assert np.array_equal(P.unpack_label_bits(words, C).numpy(), a.astype(bool))
    # bits at or above C are ignored by the composition
    x = torch.from_numpy(rng.standard_normal((37, C)).astype(np.float32))
    s = torch.from_numpy(rng.integers(0, 4, 37).astype(np.uint8))
    dirty = w.copy()
    if C % 32:
        dirty[:, -1] |= np.uint32((0xffffffff << (C % 32)) & 0xffffffff)
    st0 = P.masked_bce_stats_composed(x, words, s)
    st1 = P.masked_bce_stats_composed(x, torch.from_numpy(dirty.view(np.int32)), s)
    assert all(torch.equal(p, q) for p, q in zip(st0, st1))
    with pytest.raises(ValueError):
        nd.pack_label_words(np.zeros(5, np.uint8))
    with pytest.raises(ValueError):
        nd.unpack_label_words(w, C + 32)


# ---- the loader --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [2, 3])
def test_loader_rows_are_the_owned_rows(dataset, P):
    nd = pkg("nodedata")
    paths, data = dataset
    pv = np.array(list(map(int, open(paths["pv%d" % P]).readline().split())))
    seen = np.zeros(W.N, bool)
    for rank in range(P):
        owned = np.nonzero(pv == rank)[0]
        got = nd.load_multilabel(paths["features"], paths["labels"], paths["split"], torch.from_numpy(owned), W.N)
        assert got.features.dtype is torch.float32 and got.labels.dtype is torch.int32 and got.split.dtype is torch.uint8
        assert got.labels.shape == (owned.size, 1) and got.labels.is_contiguous()
        assert np.array_equal(got.features.numpy(), data["X"][owned])
        assert np.array_equal(got.split.numpy(), data["split"][owned])
        assert np.array_equal(nd.unpack_label_words(got.labels.numpy(), W.LABELS), (data["labels"][owned] != 0).astype(np.uint8))
        assert got.fin == W.FIN and got.classes == W.LABELS
        assert got.counts == tuple(int((data["split"] == k).sum()) for k in range(4))
        seen[owned] = True
    assert seen.all()


def test_loader_error_cases(dataset, tmp_path):
    nd = pkg("nodedata")
    paths, data = dataset
    ok = (paths["features"], paths["labels"], paths["split"])

    def save(name, a):
        np.save(str(tmp_path / name), a)
        return str(tmp_path / name)

    assert nd.open_checked_multilabel(*ok, W.N)[3:5] == (W.FIN, W.LABELS)
    with pytest.raises(ValueError, match="dtype"):                                       # a wrong dtype
        nd.open_checked_multilabel(ok[0], save("i64.npy", data["labels"].astype(np.int64)), ok[2], W.N)
    with pytest.raises(ValueError, match="dimensions"):                                  # a 1-D file
        nd.open_checked_multilabel(ok[0], save("flat.npy", data["labels"][:, 0].copy()), ok[2], W.N)
    with pytest.raises(ValueError, match="vertices"):                                    # the row count
        nd.open_checked_multilabel(ok[0], save("short.npy", data["labels"][:-1]), ok[2], W.N)
    with pytest.raises(ValueError, match="vertices"):
        nd.open_checked_multilabel(*ok, W.N + 1)
    with pytest.raises(ValueError, match="no columns"):
        nd.open_checked_multilabel(ok[0], save("empty.npy", np.zeros((W.N, 0), np.uint8)), ok[2], W.N)
    in_set = int(np.nonzero(data["split"] == 2)[0][3])
    two = data["labels"].copy()
    two[in_set, 4] = 2
    with pytest.raises(ValueError, match="vertex %d .*val.* value 2" % in_set):          # 2 on a row of a set: names the vertex
        nd.open_checked_multilabel(ok[0], save("two.npy", two), ok[2], W.N)
    free = data["labels"].copy()
    free[data["split"] == 0] = 2                                                         # 2 on rows in no set: accepted
    assert (data["split"] == 0).sum() > 100
    assert nd.open_checked_multilabel(ok[0], save("free.npy", free), ok[2], W.N)[4] == W.LABELS
    four = data["split"].copy()
    four[7] = 4
    with pytest.raises(ValueError, match="code 4"):
        nd.open_checked_multilabel(ok[0], ok[1], save("four.npy", four), W.N)
    # the single-label loader is what it was: it refuses this label file
    with pytest.raises(ValueError, match="dtype"):
        nd.open_checked(*ok, W.N)


# ---- masked_bce_stats: the composition --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 7, 33, 121])
def test_composition_against_float64(C):
    P, nd = pkg("PGCN"), pkg("nodedata")
    n = 257
    rng = np.random.default_rng(C)
    x = (rng.standard_normal((n, C)) * 4).astype(np.float32)
    y = rng.random((n, C)) < 0.3
    s = rng.integers(0, 4, n).astype(np.uint8)
    s[:8] = [1, 1, 1, 1, 2, 3, 0, 1]
    x[0, :] = 0.0                                                  # exactly 0: predicts negative
    x[1, 0], y[1, 0] = np.inf, True                                # costs 0
    x[2, 0], y[2, 0] = -np.inf, False                              # costs 0
    x[6, :] = np.nan                                               # a row in no set: counts for nothing
    words = torch.from_numpy(nd.pack_label_words(y).view(np.int32))
    xt, st_ = torch.from_numpy(x), torch.from_numpy(s)
    st = P.masked_bce_stats(xt, words, st_)                        # CPU tensors: the composition
    want = W.stats64(x, y, s)
    assert st.loss_sum.dtype is torch.float64 and st.tp.dtype is torch.int64
    assert st.tp.tolist() == want["tp"] and st.fp.tolist() == want["fp"] and st.fn.tolist() == want["fn"]
    assert st.rows.tolist() == want["rows"] and float(st.loss_sum[0]) == 0.0
    for k in (1, 2, 3):
        assert np.isfinite(want["loss_sum"][k])
        assert abs(float(st.loss_sum[k]) - want["loss_sum"][k]) <= 1e-5 * max(1.0, abs(want["loss_sum"][k]))
    # the autograd node against the float64 mean over the train rows' elements and its gradient scale * (sigmoid - y)
    n_train = int((s == 1).sum()) + 5
    xg = xt.clone().requires_grad_(True)
    loss, st2 = P.masked_bce_loss(xg, words, st_, n_train)
    (loss * 3.0).backward()
    train = torch.from_numpy(s == 1)
    # (torch's own binary_cross_entropy_with_logits makes inf * 0 = NaN of the infinite logits: the numpy restatement instead)
    ref = want["loss_sum"][1] / (n_train * C)
    with np.errstate(over="ignore"):
        gref = 3.0 / (n_train * C) * (1.0 / (1.0 + np.exp(-x.astype(np.float64))) - y)
    assert abs(float(loss.detach()) - ref) <= 1e-5 * max(1.0, abs(ref))
    assert float(np.abs(xg.grad.double().numpy() - gref)[s == 1].max()) <= 2e-6
    assert torch.equal(xg.grad[~train], torch.zeros_like(xg.grad[~train]))           # exactly zero off the train set
    assert all(torch.equal(p, q) for p, q in zip(st, st2))
    # -inf against a set label costs +inf in that set only; a NaN on a val row poisons the val loss only
    x[3, 0], y[3, 0] = -np.inf, True
    x[4, C - 1] = np.nan
    words = torch.from_numpy(nd.pack_label_words(y).view(np.int32))
    st = P.masked_bce_stats_composed(torch.from_numpy(x), words, st_)
    want2 = W.stats64(x, y, s)
    assert float(st.loss_sum[1]) == np.inf and bool(torch.isnan(st.loss_sum[2]))
    assert abs(float(st.loss_sum[3]) - want["loss_sum"][3]) <= 1e-5 * max(1.0, abs(want["loss_sum"][3]))
    assert st.tp.tolist() == want2["tp"] and st.fp.tolist() == want2["fp"] and st.fn.tolist() == want2["fn"]


def test_global_stats_micro_f1():
    P, K = pkg("PGCN"), pkg("kernels")
    st = K.MaskedBCEStats(torch.tensor([0.0, 12.0, 3.0, 0.0], dtype=torch.float64), torch.tensor([0, 6, 0, 0]), torch.tensor([0, 2, 0, 0]),
                          torch.tensor([0, 2, 5, 0]), torch.tensor([9, 4, 2, 0]))
    P.world_size = 1
    out = P._global_stats_multilabel(st, 3)
    assert out["micro_f1"]["train"] == 12 / 16 and out["micro_f1"]["val"] == 0.0 and np.isnan(out["micro_f1"]["test"])
    assert out["loss"]["train"] == 1.0 and out["loss"]["val"] == 0.5 and np.isnan(out["loss"]["test"])
    assert out["tp"] == {"train": 6, "val": 0, "test": 0} and out["rows"] == {"train": 4, "val": 2, "test": 0}


# ---- end to end over gloo ------------------------------------------------------------------------------------------------------------

def test_ranks_over_gloo_against_one_rank_and_float64(dataset, reference):
    """The planted problem, 1, 2 and 3 ranks with the checker-backed kernels (masked BCE by composition) against the float64
    reference of tests/_multilabel_workers.py: losses within 1e-5, TP / FP / FN within the reference's near-zero logits."""
    paths, data = dataset
    ref, final = reference
    one = None
    for P in (1, 2, 3):
        res = W.spawn_run(P, paths, False)
        worst = W.check_against_reference(res, ref, final, data)
        print("P = %d: largest relative loss error against float64 %.3g" % (P, worst))
        assert res[0]["widths"] == [W.FIN, W.HIDDEN, W.LABELS]
        if one is None:
            one = res
        else:
            for a, b in zip(one[0]["history"], res[0]["history"]):
                assert a["rows"] == b["rows"]                          # the set sizes: exactly
    hist = one[0]["history"]
    print("train micro-F1: first epoch %.4f, last %.4f (float64 reference %.4f -> %.4f)"
          % (hist[0]["train"], hist[-1]["train"], ref[0]["micro_f1"]["train"], ref[-1]["micro_f1"]["train"]))
    assert hist[-1]["train"] > hist[0]["train"]
    lines = one[0]["stdout"].strip().splitlines()
    assert lines[-1].startswith("Best Val F1 ") and " | Test F1 " in lines[-1]
    epochs = [l for l in lines if l.startswith("Epoch ")]
    assert len(epochs) == W.EPOCHS and " | Train F1 " in epochs[0] and " | Val F1 " in epochs[0] and " | Test F1 " in epochs[0]
    assert one[0]["best"]["val"] == max(h["val"] for h in hist)


def test_dropout_reports_from_evaluate_after_the_update(dataset):
    paths, data = dataset
    ref, final = W.float64_reference(data, [W.FIN, W.HIDDEN, W.LABELS], dropout=W.DROPOUT)
    res = W.spawn_run(2, paths, False, dropout=W.DROPOUT)
    worst = W.check_against_reference(res, ref, final, data)
    print("P = 2, dropout %.1f: largest relative loss error against float64 %.3g" % (W.DROPOUT, worst))


# ---- the command line ------------------------------------------------------------------------------------------------------------------

def _keep_cli_state(monkeypatch, M):
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        if k in os.environ:
            monkeypatch.setenv(k, os.environ[k])
        else:
            monkeypatch.delenv(k, raising=False)
    for name in ("path_A", "path_partvec"):
        monkeypatch.setattr(M, name, getattr(M, name, None), raising=False)


BASE = ["-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"), "-b", "gloo", "-s", "1", "-l", "2", "-f", "16"]


@pytest.mark.parametrize("bad", [["--task", "multilabel"], ["--task", "single"], ["--task", "multilabel", "--features", "F"],
                                 ["--features", "F", "--labels", "L", "--split", "S", "--task", "multiclass"],
                                 ["--features", "F", "--labels", "L", "--split", "S", "--task", ""]])
def test_cli_rejects_task_without_files_or_unknown(monkeypatch, capsys, dataset, bad):
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    paths = dataset[0]
    argv = [{"F": paths["features"], "L": paths["labels"], "S": paths["split"]}.get(a, a) for a in bad]
    with pytest.raises(SystemExit) as e:
        M.main(BASE + argv)
    assert e.value.code == 2
    assert "--task" in capsys.readouterr().out                      # refused as a use of --task, not as an option nobody knows


def test_cli_forwards_task_and_nothing_else(monkeypatch, dataset):
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    paths = dataset[0]
    seen = []

    class InlineProcess:
        def __init__(self, target, args):
            self.target, self.args, self.exitcode = target, args, None

        def start(self):
            self.target(*self.args)
            self.exitcode = 0

        def join(self):
            pass

    monkeypatch.setattr(M.mp, "Process", InlineProcess)
    monkeypatch.setattr(M.mp, "set_start_method", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "init_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "destroy_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M, "run", lambda *a, **k: seen.append((a, k)))
    files = ["--features", paths["features"], "--labels", paths["labels"], "--split", paths["split"]]
    M.main(BASE)
    M.main(BASE + files)
    M.main(BASE + files + ["--task", "multilabel"])
    M.main(BASE + files + ["--epochs", "9", "--task", "multilabel", "--dropout", "0.5"])
    args = (0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo")
    three = {"features": paths["features"], "labels": paths["labels"], "split": paths["split"]}
    assert seen[0] == (args, {})                                     # no option: today's call
    assert seen[1] == (args, three)                                  # no --task: nothing new
    assert seen[2] == (args, dict(three, task="multilabel"))
    assert seen[3] == (args, dict(three, epochs=9, task="multilabel", dropout=0.5, dropout_seed=0))


def test_run_refuses_task_without_files_or_unknown(dataset):
    M = pkg("PGCN")
    paths = dataset[0]
    with pytest.raises(ValueError, match="needs features"):
        M.run(0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo", task="multilabel")
    with pytest.raises(ValueError, match="task takes"):
        M.run(0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo", features=paths["features"], labels=paths["labels"],
              split=paths["split"], task="multiclass")


# ---- the per-set record (csrc/pgcn_setrecord.h) -------------------------------------------------------------------------------------

@pytest.mark.parametrize("planes,views,fields", [(1, "masked_stats_views", ("loss_sum", "correct", "rows")),
                                                 (3, "masked_bce_stats_views", ("loss_sum", "tp", "fp", "fn", "rows"))])
def test_record_views_are_the_fields_in_the_documented_order(planes, views, fields):
    """double loss_sum[4], then `planes` planes of int64[4], then int64 rows[4]: every view aliases its four words of the record."""
    k = pkg("kernels")
    record = torch.arange(100, 100 + 4 * (2 + planes), dtype=torch.int64)       # hand-filled: word w holds 100 + w
    st = getattr(k, views)(record)
    assert st._fields == fields and len(k.set_record_views(record, planes)) == planes + 2
    assert st.loss_sum.dtype is torch.float64 and st.loss_sum.shape == (4,) and st.loss_sum.data_ptr() == record.data_ptr()
    assert st.loss_sum.view(torch.int64).tolist() == [100, 101, 102, 103]
    for q in range(1, planes + 2):
        assert st[q].dtype is torch.int64 and st[q].tolist() == [100 + 4 * q + j for j in range(4)]
        assert st[q].data_ptr() == record.data_ptr() + 32 * q
    st.loss_sum[2] = 1.5                                                        # the float64 view aliases words 0-3 ...
    assert record[2].item() == int(np.float64(1.5).view(np.int64))
    record[1] = int(np.float64(-2.25).view(np.int64))
    assert st.loss_sum[1].item() == -2.25
    st.rows[3] = 7                                                              # ... and the last view the last four
    assert record[-1].item() == 7
