"""The tail of a GAT layer (head mean, bias, ELU, dropout) and training PGAT on data, on the CPU: the framework composition of PGAT.py
against its fp32 statement in numpy and against float64 autograd, the layer's defaults, every refusal, run() on a planted problem on
one and two ranks, and whole-model gradients of every option against a dense float64 GAT (tests/_gat_tail_workers.py).  The HIP
kernels are covered by tests/test_gat_tail_gpu.py."""
import itertools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gat_tail_workers as W
from conftest import gpath, held_to_fixture, pkg, read_partvec, rel_err

SEED, LAYER = 77, 1


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- the composition --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,d", [(1, 3), (4, 8), (3, 5), (2, 50)])
def test_composed_against_the_fp32_statement_and_float64_autograd(K, d):
    M, D = pkg("PGAT"), pkg("dropout")
    n = 97
    rng = np.random.default_rng(10 * K + d)
    x = rng.standard_normal((n, K * d)).astype(np.float32)
    ids = torch.arange(n, dtype=torch.int64) * 3 + 1
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(SEED, "cpu")
    state.step.fill_(4)
    for mean, has_bias, act, drop in itertools.product((False, True), (False, True), (0, 1), (False, True)):
        fout = d if mean else K * d
        b = rng.standard_normal(fout).astype(np.float32) if has_bias else None
        G = rng.standard_normal((n, fout)).astype(np.float32)
        keep = D.keep_mask(SEED, 4, LAYER, ids, fout, thr).numpy() if drop else None
        bt = torch.from_numpy(b) if has_bias else None
        Y = M.gat_tail_composed(torch.from_numpy(x), K, d, mean, bt, act, ids, state if drop else None, LAYER, thr if drop else 0,
                                scale if drop else 1.0)
        want, exact = W.tail32(x, K, d, mean, b, act, keep, scale)
        Yn = Y.numpy()
        case = (K, d, mean, has_bias, act, drop)
        assert Yn.shape == (n, fout) and np.array_equal(_bits(Yn[exact]), _bits(want[exact])), case
        assert W.ulps(Yn, want).max() <= 3 + (1 if drop else 0), case                    # (torch's own expm1 on the host)
        dX, db = M.gat_tail_backward_composed(torch.from_numpy(G), Y, K, d, mean, act, ids, state if drop else None, LAYER,
                                              thr if drop else 0, scale if drop else 1.0)
        dx32, gm32 = W.tail_backward32(G, Yn, K, d, mean, act, keep, scale)
        assert np.array_equal(_bits(dX.numpy()), _bits(dx32)), case
        err, bound = W.dbias_error_and_bound(db.numpy(), gm32)
        assert (err <= bound).all(), case
        # float64 autograd of the same function
        X64 = torch.from_numpy(x).double().requires_grad_(True)
        b64 = torch.from_numpy(b).double().requires_grad_(True) if has_bias else None
        t = X64.view(n, K, d).mean(1) if mean else X64
        t = t + b64 if has_bias else t
        a = F.elu(t) if act else t
        if drop:
            a = torch.where(torch.from_numpy(keep), a * scale, torch.zeros((), dtype=torch.float64))
        grads = torch.autograd.grad((a * torch.from_numpy(G).double()).sum(), [X64] + ([b64] if has_bias else []))
        # a handful of fp32 roundings per element (2^-24 each) against values of order one: 1e-6 of the largest value
        assert rel_err(Yn, a.detach().numpy()) < 1e-6 and rel_err(dX.numpy(), grads[0].numpy()) < 1e-6, case
        if has_bias:
            assert rel_err(db.numpy(), grads[1].numpy()) < 1e-6, case


def test_autograd_node_on_the_cpu_is_the_composition():
    M, D = pkg("PGAT"), pkg("dropout")
    n, K, d = 40, 3, 5
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((n, K * d)).astype(np.float32)).requires_grad_(True)
    b = torch.from_numpy(rng.standard_normal(d).astype(np.float32)).requires_grad_(True)
    G = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32))
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(SEED, "cpu")
    ids = torch.arange(n, dtype=torch.int64)
    Y = M._GatTail.apply(x, b, K, d, True, 1, ids, state, LAYER, thr, scale)
    dx, db = torch.autograd.grad((Y * G).sum(), (x, b))
    Yc = M.gat_tail_composed(x, K, d, True, b, 1, ids, state, LAYER, thr, scale)
    dxc, dbc = M.gat_tail_backward_composed(G, Yc, K, d, True, 1, ids, state, LAYER, thr, scale)
    assert torch.equal(Y, Yc) and torch.equal(dx, dxc) and torch.equal(db, dbc)
    assert bool((Y == 0).any()) and bool((Y != 0).any())


# ---- the layer --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture()
def cpu_engine():
    """PGAT on the checker-backed provider, one rank, karate; the module's state comes back afterwards."""
    from oracle_kernels import OracleKernels
    from scipy.io import mmread
    M = pkg("PGAT")
    names = ("_kernel_provider", "myrank", "world_size", "device", "mode", "heads", "_exchanger", "_engine_current", "send_map", "recv_map",
             "path_A", "path_partvec")
    saved = {k: getattr(M, k) for k in names}
    M._kernel_provider = OracleKernels()
    M.myrank, M.world_size, M.device, M.mode, M.heads, M._exchanger = 0, 1, torch.device("cpu"), "standard", 1, None
    A = mmread(gpath("karate.A.mtx"))
    part = read_partvec(gpath("karate.mtx.1.rp"))
    M.send_map, M.recv_map = M.compute_communication_maps(A, part, 0, 1)
    eng = M.get_partitiont_of_adjacency_matrix(A, part, 0)
    try:
        yield M, eng
    finally:
        for k, v in saved.items():
            setattr(M, k, v)


def test_layer_defaults_are_the_layer_of_before(cpu_engine):
    M, eng = cpu_engine
    torch.manual_seed(5)
    plain = M.PGAT(eng, 6, 8, heads=2)
    torch.manual_seed(5)
    full = M.PGAT(eng, 6, 8, heads=2, bias=False, activation=None, concat=True, dropout=0.0, layer=0, state=None)
    assert list(plain.state_dict()) == list(full.state_dict()) == ["attention", "linear.weight"]
    assert [k for k, _ in full.named_parameters()] == [k for k, _ in plain.named_parameters()] == ["attention", "linear.weight"]
    assert not full._has_tail
    H = torch.from_numpy(np.random.default_rng(1).standard_normal((eng.part.n_local, 6)).astype(np.float32))
    called = []
    apply = M._GatTail.apply
    M._GatTail.apply = lambda *a: called.append(1) or apply(*a)
    try:
        assert torch.equal(plain(H), full(H)) and not called                       # none of the four: the tail is not called at all
        opt = M.PGAT(eng, 6, 8, heads=2, bias=True, concat=False)
        out = opt(H)
        assert called and out.shape == (eng.part.n_local, 4) and opt.out_features == 8
    finally:
        M._GatTail.apply = apply
    assert [k for k, _ in opt.named_parameters()] == ["attention", "bias", "linear.weight"]
    assert tuple(opt.bias.shape) == (4,) and not bool(opt.bias.any())
    assert tuple(M.PGAT(eng, 6, 8, heads=2, bias=True).bias.shape) == (8,)


def test_layer_options_against_the_composition(cpu_engine):
    M, eng = cpu_engine
    D = pkg("dropout")
    n = eng.part.n_local
    H = torch.from_numpy(np.random.default_rng(2).standard_normal((n, 6)).astype(np.float32))
    state = D.DropoutState(3, "cpu")
    torch.manual_seed(7)
    base = M.PGAT(eng, 6, 8, heads=2)
    torch.manual_seed(7)
    layer = M.PGAT(eng, 6, 8, heads=2, bias=True, activation="elu", dropout=0.5, layer=2, state=state)
    with torch.no_grad():
        layer.bias.copy_(torch.arange(8.0) / 8 - 0.5)
    X = base(H).detach()
    thr, scale = D.threshold(0.5)
    ids = eng.part.owned.to(torch.int64)
    assert torch.equal(layer(H), M.gat_tail_composed(X, 2, 4, False, layer.bias, 1, ids, state, 2, thr, scale))
    layer.eval()
    assert torch.equal(layer(H), M.gat_tail_composed(X, 2, 4, False, layer.bias, 1))           # eval: the tail without dropout


def test_constructor_refusals():
    M, D = pkg("PGAT"), pkg("dropout")
    ref = types.SimpleNamespace(mode="reference")
    with pytest.raises(ValueError, match="activation takes"):
        M.PGAT(None, 4, 4, heads=1, activation="relu")
    with pytest.raises(ValueError, match="needs state"):
        M.PGAT(None, 4, 4, heads=1, dropout=0.5)
    with pytest.raises(ValueError, match="probability"):
        M.PGAT(None, 4, 4, heads=1, dropout=1.0, state=D.DropoutState(0))
    with pytest.raises(ValueError, match="divisible"):
        M.PGAT(None, 4, 6, heads=4, bias=True)
    for kw in ({"bias": True}, {"activation": "elu"}, {"concat": False}, {"dropout": 0.5, "state": D.DropoutState(0)}):
        with pytest.raises(ValueError, match="reference layer"):
            M.PGAT(ref, 4, 4, heads=1, **kw)
    M.PGAT(ref, 4, 4, heads=1)                                                               # the plain reference layer is still there


def _files(tmp_path):
    out = []
    for k in ("features", "labels", "split"):
        p = tmp_path / (k + ".npy")
        np.save(p, np.zeros((2, 2), np.float32))
        out += ["--" + k, str(p)]
    return out


@pytest.mark.parametrize("args,text", [
    (["--features", "x.npy"], "--features, --labels and --split go together"),
    (["--hidden", "8"], "--features, --labels and --split go together"),
    (["--bias"], "need them); got --bias"),
    (["--adamw", "--dropout", "0.5"], "got --adamw, --dropout"),
    (["--task", "multi"], "--task takes single|multilabel, got 'multi'"),
    (["--hidden", "0"], "--hidden takes a positive integer, got '0'"),
    (["--out-heads", "two"], "--out-heads takes a positive integer, got 'two'"),
    (["--epochs", "-1"], "--epochs takes a positive integer, got '-1'"),
    (["--eval-every", "0"], "--eval-every takes a positive integer, got '0'"),
    (["--lr", "0"], "--lr takes a positive number, got '0'"),
    (["--dropout", "1.5"], "--dropout takes a probability in [0, 1), got '1.5'"),
    (["--dropout-seed", "x"], "--dropout-seed takes an integer, got 'x'"),
    (["--weight-decay", "-1"], "--weight-decay takes a number >= 0, got '-1'"),
    (["--optimizer", "sgd"], "--optimizer takes torch|fused, got 'sgd'"),
    (["--features", "/nonexistent/f.npy", "--labels", "l.npy", "--split", "s.npy"], "--features: no such file '/nonexistent/f.npy'"),
    ("FILES+--mode reference", "--mode reference has no bias"),
    ("FILES+--heads 3 --hidden 8", "--hidden takes a multiple of --heads (3), got '8'"),
])
def test_main_refusals(args, text, tmp_path, capsys):
    M = pkg("PGAT")
    saved = (M.path_A, M.path_partvec, M.mode, M.heads)
    if isinstance(args, str):
        args = _files(tmp_path) + args.split("+")[1].split()
    M.mode, M.heads = "standard", 1                   # (main keeps the module's values where a flag is absent)
    try:
        with pytest.raises(SystemExit) as e:
            M.main(["-a", "A.mtx", "-p", "A.part"] + args)
    finally:
        M.path_A, M.path_partvec, M.mode, M.heads = saved
    out = capsys.readouterr().out
    assert e.value.code == 2 and text in out and len(out.strip().splitlines()) == 1, out


def test_run_refusals():
    M = pkg("PGAT")
    with pytest.raises(ValueError, match="go together"):
        M.run(0, 1, 2, 4, "A.mtx", "pv", "gloo", features="x.npy")
    with pytest.raises(ValueError, match="go together"):
        M.run(0, 1, 2, 4, "A.mtx", "pv", "gloo", hidden=8)
    with pytest.raises(ValueError, match="task takes"):
        M.run(0, 1, 2, 4, "A.mtx", "pv", "gloo", features="x", labels="y", split="s", task="multi")
    with pytest.raises(ValueError, match="optimizer takes"):
        M.run(0, 1, 2, 4, "A.mtx", "pv", "gloo", features="x", labels="y", split="s", optimizer="sgd")


# ---- run() on data ----------------------------------------------------------------------------------------------------------------------

EPOCHS, LR = 4, 0.01


@pytest.fixture(scope="module")
def karate(tmp_path_factory):
    paths, data = W.make_karate(str(tmp_path_factory.mktemp("gat_tail_karate")))
    opts = W.options(K=2, hidden=8, Ko=2, bias=True, elu=True, dropout=W.DROPOUT)
    return paths, data["single"], opts, W.reference(data["single"], opts, 0, EPOCHS, LR)


@pytest.fixture(scope="module")
def karate_runs(karate):
    paths, data, opts, ref = karate
    params = {k: v.numpy() for k, v in ref["params"].items()}
    return {P: W.spawn(W.run_worker, P, paths, False, opts=opts, params=params, epochs=EPOCHS, lr=LR) for P in (1, 2)}


@pytest.mark.parametrize("P", [1, 2])
def test_run_on_data_against_the_float64_model(karate, karate_runs, P):
    paths, data, opts, ref = karate
    res = karate_runs[P]
    n = data["A"].shape[0]
    r0 = res[0]
    assert sorted(r0["names"]) == sorted(ref["params"]) and r0["widths"] == [6, 8, 2] and len(r0["history"]) == EPOCHS
    assert all(r["history"] == r0["history"] and r["best"] == r0["best"] for r in res)
    W.hold_steps("gat_tail/karate/P%d" % P, res, ref, n, EPOCHS)
    for e, h in enumerate(r0["history"]):                        # with dropout: the record of an eval pass after the update
        a64, a32 = W.accuracy(ref["m64"]["eval"][e], data), W.accuracy(ref["twin"]["eval"][e], data)
        for j, what in enumerate(("loss", "accuracy")):
            got = np.array([h["losses"][s] if j == 0 else h[s] for s in W.SETS])
            held_to_fixture("gat_tail/karate/P%d/epoch%d" % (P, e), what, got, np.array([a32[s][j] for s in W.SETS]),
                            np.array([a64[s][j] for s in W.SETS]))
    lines = r0["stdout"].strip().splitlines()
    assert len(lines) == EPOCHS + 2 and lines[0].startswith("Epoch 00000 | Loss ") and " | Train " in lines[0] and " | Test " in lines[0]
    assert lines[-1].startswith("Best Val %.4f at epoch %05d | Test " % (r0["best"]["val"], r0["best"]["epoch"]))
    held_to_fixture("gat_tail/karate/P%d" % P, "eval logits", W.rows(res, lambda r: r["eval_logits"], n),
                    ref["twin"]["eval"][-1].numpy(), ref["m64"]["eval"][-1].numpy())


def test_two_ranks_print_the_losses_of_one(karate_runs):
    one, two = karate_runs[1][0], karate_runs[2][0]
    assert [ln for ln in one["stdout"].splitlines() if ln.startswith(("Epoch", "Best"))] == \
        [ln for ln in two["stdout"].splitlines() if ln.startswith(("Epoch", "Best"))]
    # the same masks: the first training pass at the same parameters gives the same logits row for row, up to the sums' order
    n = 34
    a, b = W.rows(karate_runs[1], lambda r: r["logits"][0], n), W.rows(karate_runs[2], lambda r: r["logits"][0], n)
    assert rel_err(a, b) < 1e-5


def test_every_rank_count_draws_the_same_initial_parameters(karate, karate_runs):
    """run() draws the classifier's parameters under the dropout seed on every rank alike: one rank and two start from the same
    bits (the mean of two equal draws is that draw), whatever the caller's generator holds."""
    paths, data, opts, ref = karate
    one = karate_runs[1][0]["drawn"]
    for r in karate_runs[2]:
        assert sorted(r["drawn"]) == sorted(one) and all(np.array_equal(_bits(r["drawn"][k]), _bits(one[k])) for k in one)
    assert all(np.abs(one[k]).max() > 0 for k in one if not k.endswith("bias"))
    other = W.spawn(W.run_worker, 1, paths, False, opts=dict(opts, dropout=0.0), params=None, epochs=1, lr=LR)[0]["drawn"]
    assert not np.array_equal(other["0.linear.weight"], one["0.linear.weight"])              # dropout off: seed 0, not DROPOUT_SEED


def test_fused_optimizer_trains_like_torch(karate, karate_runs):
    paths, data, opts, ref = karate
    params = {k: v.numpy() for k, v in ref["params"].items()}
    got = W.spawn(W.run_worker, 2, paths, False, opts=opts, params=params, epochs=EPOCHS, lr=LR, optimizer="fused")[0]
    want = karate_runs[2][0]
    for a, b in zip(got["history"], want["history"]):
        assert abs(a["loss"] - b["loss"]) <= 1e-5 * max(1.0, abs(b["loss"])) and a["train"] == b["train"]


# ---- whole-model gradients --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return W.make_datasets(str(tmp_path_factory.mktemp("gat_tail_grid")))


def _grid(task):
    return [W.options(K=2, hidden=8, Ko=Ko, bias=b, elu=e, dropout=W.DROPOUT if dr else 0.0, task=task)
            for b, e, dr, Ko in itertools.product((0, 1), (0, 1), (0, 1), (1, 2))]


@pytest.mark.parametrize("task,P", [("single", 1), ("multilabel", 1), ("single", 2)])
def test_whole_model_gradients_of_every_option(datasets, task, P):
    paths, data = datasets
    grid = _grid(task)
    assert len(grid) == 16
    refs = [W.reference(data[task], o, 0, 2, 0.0) for o in grid]
    jobs = [{"opts": o, "params": {k: v.numpy() for k, v in r["params"].items()}} for o, r in zip(grid, refs)]
    res = W.spawn(W.grad_worker, P, paths, False, jobs=jobs, n=W.GW.N)
    held = 0
    for j, (o, ref) in enumerate(zip(grid, refs)):
        ranks = [dict(r["results"][j], rank=r["rank"]) for r in res]
        where = "gat_tail/grid/%s/P%d" % (W.tag(o), P)
        assert all(r["tag"] == W.tag(o) for r in ranks)
        held += W.hold_steps(where, ranks, ref, W.GW.N, 2)
        logits = [W.rows(ranks, lambda r, s=s: r["logits"][s], W.GW.N) for s in range(2)]
        if o["dropout"] > 0:
            assert not np.array_equal(logits[0], logits[1]), where + ": the second step drew the first step's masks"
        else:
            assert np.array_equal(logits[0], logits[1]), where
        held_to_fixture(where, "eval logits", W.rows(ranks, lambda r: r["eval_logits"], W.GW.N), ref["twin"]["eval"][-1].numpy(),
                        ref["m64"]["eval"][-1].numpy())
    print("%s on %d ranks: %d tensors held" % (task, P, held + 16))
