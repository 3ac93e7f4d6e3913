"""Node classification on real inputs (nodedata.py, PGCN(relu=False), PGCN.masked_loss / evaluate, run(features=..., labels=...,
split=...), --features / --labels / --split / --hidden / --epochs / --lr / --eval-every) -- the CPU side: the loader, the framework
composition of the masked loss against float64, the layer without ReLU, partition independence over gloo with the checker-backed
kernels against a float64 restatement of the model, and the command line.  The kernels are held in test_nodeclass_gpu.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _nodeclass_workers as W
from conftest import gpath, pkg


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("nodeclass")))


@pytest.fixture(scope="module")
def reference(dataset):
    return W.float64_reference(dataset[1], [W.FIN, W.HIDDEN, W.CLASSES])


# ---- nodedata ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 2, 3])
def test_nodedata_rows_are_the_owned_rows(dataset, P):
    nd = pkg("nodedata")
    paths, data = dataset
    pv = np.array(list(map(int, open(paths["pv%d" % P]).readline().split())))
    seen = np.zeros(W.N, bool)
    for rank in range(P):
        owned = torch.from_numpy(np.nonzero(pv == rank)[0])
        got = nd.load(paths["features"], paths["labels"], paths["split"], owned, W.N)
        assert got.features.dtype is torch.float32 and got.labels.dtype is torch.int64 and got.split.dtype is torch.uint8
        assert np.array_equal(got.features.numpy(), data["X"][owned.numpy()])
        assert np.array_equal(got.labels.numpy(), data["labels"][owned.numpy()])
        assert np.array_equal(got.split.numpy(), data["split"][owned.numpy()])
        assert got.fin == W.FIN and got.classes == W.CLASSES
        assert got.counts == tuple(int((data["split"] == k).sum()) for k in range(4))
        seen[owned.numpy()] = True
    assert seen.all()
    assert nd.load(paths["features"], paths["labels"], paths["split"], torch.arange(5), W.N, classes=9).classes == 9


def test_nodedata_error_cases(dataset, tmp_path):
    nd = pkg("nodedata")
    paths, data = dataset
    ok = (paths["features"], paths["labels"], paths["split"])

    def save(name, a):
        np.save(str(tmp_path / name), a)
        return str(tmp_path / name)

    with pytest.raises(ValueError, match="vertices"):
        nd.open_checked(*ok, W.N + 1)                                                       # a wrong n
    for k, a in ((0, data["X"][:-1]), (1, data["labels"][:-1]), (2, data["split"][:-1])):
        bad = list(ok)
        bad[k] = save("short%d.npy" % k, a)
        with pytest.raises(ValueError, match="vertices"):
            nd.open_checked(*bad, W.N)
    for k, a in ((0, data["X"].astype(np.float64)), (1, data["labels"].astype(np.int32)), (2, data["split"].astype(np.int8)),
                 (0, data["X"][:, 0].copy()), (1, data["labels"].reshape(-1, 1)), (2, data["split"].reshape(-1, 1))):
        bad = list(ok)
        bad[k] = save("bad%d.npy" % k, a)
        with pytest.raises(ValueError, match="dtype|dimensions"):                           # a wrong dtype or rank
            nd.open_checked(*bad, W.N)
    four = data["split"].copy()
    four[7] = 4
    with pytest.raises(ValueError, match="code 4"):
        nd.open_checked(ok[0], ok[1], save("four.npy", four), W.N)
    in_set = int(np.nonzero(data["split"] == 2)[0][0])
    for v in (-1, W.CLASSES + 3):
        lab = data["labels"].copy()
        lab[in_set] = v
        with pytest.raises(ValueError, match="outside"):
            nd.open_checked(ok[0], save("lab.npy", lab), ok[2], W.N, classes=W.CLASSES)
    with pytest.raises(ValueError, match="outside"):
        nd.open_checked(*ok, W.N, classes=W.CLASSES - 1)
    lab = data["labels"].copy()
    lab[data["split"] == 0] = 10 ** 6                                                       # rows in no set: anything goes
    assert nd.open_checked(ok[0], save("free.npy", lab), ok[2], W.N, classes=W.CLASSES)[4] == W.CLASSES
    with pytest.raises(ValueError):
        nd.open_checked(str(tmp_path / "missing.npy"), ok[1], ok[2], W.N)


# ---- masked_loss: the composition -------------------------------------------------------------------------------------------------

def _loss_case(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g) * 4
    y = torch.randint(0, C, (n,), generator=g)
    s = torch.randint(0, 4, (n,), generator=g).to(torch.uint8)
    y[s == 0] = -1
    return x, y, s


@pytest.mark.parametrize("n,C", [(500, 7), (333, 41), (64, 128), (1, 3), (90, 172)])
def test_masked_loss_composition_against_float64(n, C):
    P = pkg("PGCN")
    x0, y, s = _loss_case(n, C, n + C)
    if n > 3:
        x0[1, 0] = float("-inf")
        x0[2, :] = 3.0                                              # equal maxima: the lowest index
    n_train = max(int((s == 1).sum()), 1) + 5
    x = x0.clone().requires_grad_(True)
    loss, st = P.masked_loss(x, y, s, n_train)
    (loss * 3.0).backward()
    xd = x0.double().requires_grad_(True)
    train = s == 1
    ref = F.cross_entropy(xd[train], y[train], reduction="sum") / n_train
    (ref * 3.0).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5 * max(1.0, abs(float(ref.detach())))
    assert float((x.grad.double() - xd.grad).abs().max()) <= 2e-6
    assert torch.equal(x.grad[~train], torch.zeros_like(x.grad[~train]))           # exactly zero off the train set
    pred = np.argmax(x0.numpy(), 1)
    for k in (1, 2, 3):
        m = s == k
        assert int(st.rows[k]) == int(m.sum())
        assert int(st.correct[k]) == int((pred[m.numpy()] == y[m].numpy()).sum())
        want = float(F.cross_entropy(x0.double()[m], y[m], reduction="sum")) if int(m.sum()) else 0.0
        assert abs(float(st.loss_sum[k]) - want) <= 1e-5 * max(1.0, abs(want))
    assert int(st.rows[0]) == int((s == 0).sum()) and st.loss_sum.dtype is torch.float64 and st.correct.dtype is torch.int64


def test_masked_loss_out_of_range_label_poisons_its_set_only():
    P = pkg("PGCN")
    x, y, s = _loss_case(200, 7, 1)
    i = int(torch.nonzero(s == 2)[0])
    y[i] = 7
    _, st = P.masked_loss(x, y, s, 10)
    assert bool(torch.isnan(st.loss_sum[2])) and not bool(torch.isnan(st.loss_sum[1])) and not bool(torch.isnan(st.loss_sum[3]))
    pred = x.argmax(1)
    assert int(st.correct[2]) == int(((pred == y) & (s == 2)).sum())


# ---- PGCN(relu=False) ------------------------------------------------------------------------------------------------------------------

class _Eng:
    class part:
        owned = torch.arange(50)

    def forward(self, H):
        return H * 2.0

    def backward(self, g):
        return g * 2.0


def test_layer_without_relu_and_the_default():
    P = pkg("PGCN")
    torch.manual_seed(0)
    H = torch.randn(50, 16)
    last = P.PGCN(_Eng(), 16, 7, relu=False)
    out = last(H)
    assert torch.equal(out, P.mm_nt(H * 2.0, last.linear.weight)) and bool((out < 0).any())
    drop = P.PGCN(_Eng(), 16, 7, dropout=0.5, relu=False)          # no dropout on a layer without ReLU
    drop.linear.weight.data.copy_(last.linear.weight.data)
    drop.train()
    assert torch.equal(drop(H), out)
    # gradients: those of the plain product
    Hg = H.clone().requires_grad_(True)
    last(Hg).square().sum().backward()
    Hd, wd = H.double().requires_grad_(True), last.linear.weight.detach().double().requires_grad_(True)
    ((Hd * 2.0) @ wd.t()).square().sum().backward()
    assert float((Hg.grad.double() - Hd.grad).abs().max()) <= 1e-4 * float(Hd.grad.abs().max())
    assert float((last.linear.weight.grad.double() - wd.grad).abs().max()) <= 1e-4 * float(wd.grad.abs().max())
    # the default: today's layer, bit for bit
    a, b = P.PGCN(_Eng(), 16, 16), P.PGCN(_Eng(), 16, 16, relu=True)
    b.linear.weight.data.copy_(a.linear.weight.data)
    assert a.relu is True and torch.equal(a(H), b(H)) and torch.equal(a(H), P._LinearReluNoBias.apply(H * 2.0, a.linear.weight))


# ---- end to end over gloo ------------------------------------------------------------------------------------------------------------

def test_reference_learns(dataset, reference):
    """The float64 reference after W.EPOCHS = 12 epochs of Adam (lr 0.02) on the planted-community data: test accuracy 0.984 at the
    last training step, 0.987 for the trained model, against a majority-class rate of 0.184 (measured on the CPU).  Margin: 0.5
    above the majority rate -- far below what the reference reaches, far above chance.  The engine is held to the reference
    (check_against_reference), not to this margin.  Its near-tie rows (top-two gap below 1e-4 max |logit|) stay under 1 % of
    every set at every epoch (at most 6 of ~1500 rows)."""
    paths, data = dataset
    ref, final = reference
    test = data["split"] == 3
    majority = np.bincount(data["labels"][test], minlength=W.CLASSES).max() / test.sum()
    acc = final["correct"]["test"] / final["rows"]["test"]
    print("float64 reference: test accuracy %.4f, majority class %.4f" % (acc, majority))
    assert acc >= majority + 0.5
    assert ref[-1]["correct"]["test"] / ref[-1]["rows"]["test"] >= majority + 0.5
    for r in ref + [final]:
        for name in W.SETS:
            assert r["near"][name] <= 0.01 * r["rows"][name]
    assert (data["labels"][data["split"] == 0] == -1).all() and (data["split"] == 0).sum() > 100


@pytest.mark.parametrize("dropout", [0.0, W.DROPOUT])
def test_ranks_over_gloo_against_one_rank_and_float64(dataset, reference, dropout):
    paths, data = dataset
    ref, final = reference if dropout == 0.0 else W.float64_reference(data, [W.FIN, W.HIDDEN, W.CLASSES], dropout=dropout)
    one = None
    for P in (1, 2, 3):
        res = W.spawn_run(P, paths, False, dropout=dropout)
        worst = W.check_against_reference(res, ref, final, data)
        print("P = %d, dropout %.1f: largest relative loss error against float64 %.3g" % (P, dropout, worst))
        assert res[0]["widths"] == [W.FIN, W.HIDDEN, W.CLASSES]
        if one is None:
            one = res
        else:
            for a, b in zip(one[0]["history"], res[0]["history"]):
                assert a["rows"] == b["rows"]                          # the set sizes: exactly
    lines = one[0]["stdout"].strip().splitlines()
    assert lines[-1].startswith("Best Val ") and len([l for l in lines if l.startswith("Epoch ")]) == W.EPOCHS


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


@pytest.mark.parametrize("bad", [["--features", "F"], ["--labels", "L", "--split", "S"], ["--epochs", "5"], ["--hidden", "8"],
                                 ["--lr", "0.1"], ["--eval-every", "2"], ["--features", "F", "--labels", "L", "--split", "S", "--epochs", "x"],
                                 ["--features", "F", "--labels", "L", "--split", "S", "--lr", "-1"],
                                 ["--features", "F", "--labels", "L", "--split", "S", "--hidden", "0"],
                                 ["--features", "F", "--labels", "L", "--split", "S", "--eval-every", "0"],
                                 ["--features", "/nonexistent/F.npy", "--labels", "L", "--split", "S"]])
def test_cli_rejects_bad_or_partial_options(monkeypatch, dataset, bad):
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    paths = dataset[0]
    argv = [{"F": paths["features"], "L": paths["labels"], "S": paths["split"]}.get(a, a) for a in bad]
    with pytest.raises(SystemExit) as e:
        M.main(BASE + argv)
    assert e.value.code == 2


def test_cli_forwards_the_data_options_and_nothing_else(monkeypatch, dataset):
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
    M.main(BASE + files + ["--hidden", "32", "--epochs", "9", "--lr", "0.05", "--eval-every", "3", "--dropout", "0.5"])
    args = (0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo")
    three = {"features": paths["features"], "labels": paths["labels"], "split": paths["split"]}
    assert seen[0] == (args, {})                                     # no data option: today's call
    assert seen[1] == (args, three)
    assert seen[2] == (args, dict(three, hidden=32, epochs=9, lr=0.05, eval_every=3, dropout=0.5, dropout_seed=0))
    # init_process itself, called the old way
    seen.clear()
    M.init_process(0, 1, M.run, 2, 16, "A", "pv", "gloo")
    M.init_process(0, 1, M.run, 2, 16, "A", "pv", "gloo", "sym", 0.5, 3)
    assert seen == [((0, 1, 2, 16, "A", "pv", "gloo"), {}),
                    ((0, 1, 2, 16, "A", "pv", "gloo"), {"normalize": "sym", "dropout": 0.5, "dropout_seed": 3})]


def test_run_refuses_partial_files(dataset):
    M = pkg("PGCN")
    with pytest.raises(ValueError, match="go together"):
        M.run(0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo", features=dataset[0]["features"])
