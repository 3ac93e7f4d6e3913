"""Batch normalisation over all vertices of the graph, fused with ReLU and dropout (csrc/pgcn_norm.hip, PGCN._BatchNormReluDropout,
PGCN(norm="batch"), run(norm=...), --norm) -- the CPU side: the float64 definition against torch.nn.BatchNorm1d, the framework
composition against the definition, the entry points' refusals on the loaded library, global statistics over gloo against a
one-process float64 loop, eval mode, and the command line.  The kernels are held in test_batchnorm_gpu.py."""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import _batchnorm_workers as W
from conftest import gpath, pkg

U = 2.0 ** -24


def _case(n, f, seed, spread=True):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, f))
    if spread:
        X = X * rng.uniform(0.1, 3.0, f) + rng.uniform(-2.0, 2.0, f)
    return X, rng.uniform(0.5, 1.5, f), rng.uniform(-0.5, 0.5, f), rng.standard_normal((n, f))


# ---- the definition ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,f", [(1, 1), (2, 3), (65, 7), (300, 33)])
def test_definition_is_torch_batchnorm_in_float64(n, f):
    """bn64 / bn_backward64 / running64 against torch.nn.BatchNorm1d in double followed by relu, autograd included, three steps."""
    bn = torch.nn.BatchNorm1d(f, eps=W.EPS, momentum=W.MOMENTUM).double()
    X, gamma, beta, G = _case(n, f, 100 * n + f)
    bn.weight.data.copy_(torch.from_numpy(gamma))
    bn.bias.data.copy_(torch.from_numpy(beta))
    rm, rv = np.zeros(f), np.ones(f)
    for step in range(3):
        Xs = X + 0.25 * step
        if n == 1:                          # torch refuses one value per channel in training mode: the definition's limit var = 0
            Y, mean, invstd = W.bn64(Xs, gamma, beta)
            assert np.array_equal(mean, Xs[0]) and np.allclose(invstd, 1 / np.sqrt(W.EPS), rtol=1e-15)
            assert np.allclose(Y, np.maximum(beta, 0)[None], atol=1e-12)
            rm, rv = W.running64(rm, rv, mean, np.zeros(f), n)
            dX, dg, db, _, _ = W.bn_backward64(G, Y, Xs, mean, invstd, gamma)
            assert np.abs(dX).max() <= 1e-12 and np.allclose(db, np.where(Y > 0, G, 0).sum(0)) and np.abs(dg).max() <= 1e-12
            continue
        xt = torch.from_numpy(Xs).requires_grad_(True)
        bn.zero_grad()
        yt = torch.relu(bn(xt))
        yt.backward(torch.from_numpy(G))
        Y, mean, invstd = W.bn64(Xs, gamma, beta)
        m, var, _ = W.stats64(Xs)
        rm, rv = W.running64(rm, rv, m, var, n)
        dX, dg, db, _, _ = W.bn_backward64(G, Y, Xs, mean, invstd, gamma)
        for got, want in ((Y, yt), (dX, xt.grad), (dg, bn.weight.grad), (db, bn.bias.grad), (rm, bn.running_mean), (rv, bn.running_var)):
            want = want.detach().numpy()
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (step, np.abs(got - want).max())
    if n == 1:
        assert np.allclose(rv, 0.9 ** 3)                            # N = 1: the biased variance (0) enters the running one


# ---- the composition -------------------------------------------------------------------------------------------------------------------

def _forward_bound(X, mean, invstd, gamma, beta, scale=1.0):
    return 4 * U * scale * (np.abs(gamma) * invstd * (np.abs(X) + np.abs(mean)) + np.abs(beta))


def _backward_bounds(G, Y, X, mean, invstd, gamma, scale, n):
    gm = np.abs(np.where(Y > 0, G.astype(np.float64) * scale, 0.0))
    xh = np.abs((X - mean) * invstd)
    R = np.abs(mean) * invstd
    S1 = np.abs(np.where(Y > 0, G * scale, 0.0).sum(0))
    S2 = np.abs((np.where(Y > 0, G * scale, 0.0) * ((X - mean) * invstd)).sum(0))
    return (16 * U * np.abs(gamma) * invstd * (gm + S1 / n + (xh + R) * S2 / n), 4 * U * (gm * (xh + R)).sum(0), 2 * U * gm.sum(0))


@pytest.mark.parametrize("n,f,p", [(65, 7, 0.0), (300, 33, 0.0), (300, 33, 0.5), (129, 128, 0.3), (1, 1, 0.0)])
def test_composition_against_the_definition(n, f, p):
    P, D = pkg("PGCN"), pkg("dropout")
    P.world_size = 1
    X64, gamma64, beta64, G64 = _case(n, f, 7 * n + f)
    X, gamma, beta, G = (torch.from_numpy(a.astype(np.float32)) for a in (X64, gamma64, beta64, G64))
    Xd, gd, bd, Gd = (t.double().numpy() for t in (X, gamma, beta, G))
    thr, scale = D.threshold(p)
    state = D.DropoutState(5, "cpu") if p > 0 else None
    if state is not None:
        state.step.fill_(3)
    ids = torch.arange(n, dtype=torch.int64) * 7 + 11
    rm, rv = torch.zeros(f), torch.ones(f)
    x = X.clone().requires_grad_(True)
    g_, b_ = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    Y = P._BatchNormReluDropout.apply(x, g_, b_, (rm, rv), True, W.MOMENTUM, W.EPS, n, ids if p > 0 else None, state, 2, thr, scale)
    Y.backward(G)
    keep = D.keep_mask(5, 3, 2, ids, f, thr).numpy() if p > 0 else None
    Y64, mean, invstd = W.bn64(Xd, gd, bd, keep=keep, scale=scale)
    err = np.abs(Y.detach().double().numpy() - Y64)
    bound = _forward_bound(Xd, mean, invstd, gd, bd, scale)
    print("n %d f %d p %.1f: forward error / bound %.3g" % (n, f, p, (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    if p > 0:
        pre = gd * (Xd - mean) * invstd + bd
        clear = pre > 1e-4                                               # pre-activation positive beyond any rounding
        assert np.array_equal((Y.detach().numpy() == 0)[clear], ~keep[clear])
        assert 0.2 < (~keep).mean() < 0.8
    Yn = Y.detach().numpy()
    dX64, dg64, db64, _, _ = W.bn_backward64(Gd, Yn, Xd, mean, invstd, gd, scale)
    bx, bg, bb = _backward_bounds(Gd, Yn, Xd, mean, invstd, gd, scale, n)
    assert (np.abs(x.grad.double().numpy() - dX64) <= bx + 1e-30).all()
    assert (np.abs(g_.grad.double().numpy() - dg64) <= bg + 1e-30).all()
    assert (np.abs(b_.grad.double().numpy() - db64) <= bb + 1e-30).all()
    m, var, _ = W.stats64(Xd)
    wm, wv = W.running64(np.zeros(f), np.ones(f), m, var, n)
    assert np.abs(rm.double().numpy() - wm).max() <= 1e-6 * max(1.0, np.abs(wm).max())
    assert np.abs(rv.double().numpy() - wv).max() <= 1e-6 * max(1.0, np.abs(wv).max())


# ---- the entry points without a device -------------------------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every refusal of include/pgcn_hip.h's batch-norm section, on the loaded library: the answer comes before any launch."""
    _lib, kernels = pkg("_lib"), pkg("kernels")
    L = _lib.lib()
    EINVAL, EUNSUP, ENOMEM = -1, _lib.PGCN_EUNSUPPORTED, -4
    buf = (ctypes.c_double * 4096)()
    a = ctypes.addressof(buf)
    M, V, S, WS, ST = a, a + 8192, a + 12288, a + 16384, a + 24576          # matrix, vectors, sums, work-space, step
    nan, inf = float("nan"), float("inf")
    wsb = L.pgcn_bn_colstats_ws_bytes
    assert wsb(0, 4) == wsb(1, 4) == wsb(kernels.BN_STAT_ROWS, 4) == 2 * 4 * 8          # one record per band, at least one
    assert wsb(kernels.BN_STAT_ROWS + 1, 4) == 2 * wsb(1, 4) and wsb(4 * kernels.BN_STAT_ROWS + 1, 1024) == 5 * 2 * 1024 * 8
    assert wsb(-1, 4) == -1 and wsb(4, 0) == -1 and wsb(4, 1025) == -1

    def colstats(X=M, ldx=8, n=4, f=8, sums=S, ws=WS, wb=1 << 12):
        return L.pgcn_bn_colstats_f32(X, ldx, n, f, sums, ws, wb, None)

    def prepare(sums=S, f=8, eps=1e-5, mom=0.1, tr=1, rm=V, rv=V + 64, mean=V + 128, invstd=V + 192):
        return L.pgcn_bn_prepare_f32(sums, f, eps, mom, tr, rm, rv, mean, invstd, None)

    def apply(X=M, ldx=8, n=4, f=8, mean=V, invstd=V + 64, g=V + 128, b=V + 192, ids=None, step=None, Y=M + 1024, ldy=8):
        return L.pgcn_bn_relu_apply_f32(X, ldx, n, f, mean, invstd, g, b, ids, 1, step, 0, 1 << 31, Y, ldy, None)

    def bstats(G=M, ldg=8, Y=M + 1024, ldy=8, X=M + 2048, ldx=8, n=4, f=8, mean=V, invstd=V + 64, scale=2.0, sums=S, dg=V + 128,
               db=V + 192, ws=WS, wb=1 << 12):
        return L.pgcn_bn_backward_stats_f32(G, ldg, Y, ldy, X, ldx, n, f, mean, invstd, scale, sums, dg, db, ws, wb, None)

    def backward(G=M, ldg=8, Y=M + 1024, ldy=8, X=M + 2048, ldx=8, n=4, f=8, mean=V, invstd=V + 64, g=V + 128, sums=S, N=10, scale=2.0,
                 dX=M + 3072, ldd=8):
        return L.pgcn_bn_relu_backward_f32(G, ldg, Y, ldy, X, ldx, n, f, mean, invstd, g, sums, N, scale, dX, ldd, None)

    cases = [
        (colstats, "pgcn_bn_colstats_f32", [dict(X=None), dict(sums=None), dict(ws=None), dict(n=-1), dict(f=0), dict(f=-3), dict(ldx=7),
                                            dict(sums=S + 4), dict(ws=WS + 4)]),
        (prepare, "pgcn_bn_prepare_f32", [dict(sums=None), dict(mean=None), dict(invstd=None), dict(f=0), dict(f=-1), dict(eps=0.0),
                                          dict(eps=-1e-5), dict(eps=nan), dict(eps=inf), dict(mom=-0.1), dict(mom=1.5), dict(mom=nan),
                                          dict(tr=0, rm=None), dict(tr=0, rv=None), dict(sums=S + 4)]),
        (apply, "pgcn_bn_relu_apply_f32", [dict(X=None), dict(Y=None), dict(mean=None), dict(invstd=None), dict(g=None), dict(b=None),
                                           dict(n=-1), dict(f=0), dict(ldx=7), dict(ldy=7), dict(step=ST + 4), dict(ids=ST + 4)]),
        (bstats, "pgcn_bn_backward_stats_f32", [dict(G=None), dict(Y=None), dict(X=None), dict(mean=None), dict(invstd=None),
                                                dict(sums=None), dict(ws=None), dict(n=-1), dict(f=0), dict(ldg=7), dict(ldy=7), dict(ldx=7),
                                                dict(scale=0.0), dict(scale=-1.0), dict(scale=nan), dict(scale=inf)]),
        (backward, "pgcn_bn_relu_backward_f32", [dict(G=None), dict(Y=None), dict(X=None), dict(dX=None), dict(mean=None), dict(invstd=None),
                                                 dict(g=None), dict(sums=None), dict(n=-1), dict(f=0), dict(ldg=7), dict(ldy=7), dict(ldx=7),
                                                 dict(ldd=7), dict(N=0), dict(N=-5), dict(scale=nan), dict(scale=0.0)]),
    ]
    for fn, name, bads in cases:
        for bad in bads:
            assert fn(**bad) == EINVAL, (name, bad)
            assert name.encode() in L.pgcn_last_error(), (name, bad)
        wide = dict(f=1025)
        wide.update({k: 1025 for k in ("ldx", "ldy", "ldg", "ldd") if k in fn.__code__.co_varnames})
        assert fn(**wide) == EUNSUP, name                                # above 1024 columns
    assert colstats(wb=63) == ENOMEM and bstats(wb=63) == ENOMEM
    assert apply(n=0, X=None, Y=None) == _lib.PGCN_OK and backward(n=0, G=None, Y=None, X=None, dX=None) == _lib.PGCN_OK      # nothing to do
    assert not any(buf)                                                  # and nothing was written


def test_binding_answers_none_for_what_the_kernels_do_not_cover():
    kernels = pkg("kernels")
    k = object.__new__(kernels.HipKernels)
    k.device, k.lib = torch.device("cuda:0"), None
    X, v = torch.zeros(4, 8), torch.zeros(8)
    assert k.bn_colstats(X) is None and k.bn_relu_apply(X, v, v, v, v) is None
    assert k.bn_prepare(None, 2000, 1e-5, 0.1, True, None, None) is None
    assert k.bn_backward_stats(X, X, X, v, v, 1.0) is None
    assert k.bn_relu_backward(X, X, X, v, v, v, torch.zeros(16, dtype=torch.float64), 4, 1.0) is None


# ---- global statistics over gloo ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("batchnorm")))


WIDTHS = [W.FIN, W.HIDDEN, W.HIDDEN, W.CLASSES]


@pytest.fixture(scope="module")
def references(dataset):
    return {p: W.float64_reference(dataset[1], WIDTHS, dropout=p) for p in (0.0, W.DROPOUT)}


@pytest.mark.parametrize("dropout,partvec,optimizer", [(0.0, "cpv", None), (W.DROPOUT, "pv", None), (0.0, "pv", "fused"),
                                                       (W.DROPOUT, "cpv", "fused")])
def test_ranks_over_gloo_against_a_float64_loop(dataset, references, dropout, partvec, optimizer):
    """1, 2 and 3 ranks, 3 layers, norm="batch": every epoch's loss of every set within 1e-5 (relative, floor 1: the suite's multi-rank
    bound) of the one-process float64 loop that implements the definition, the final running statistics within 1e-5 of its.  The
    features are shifted and scaled per community, so under the contiguous part vector a rank's own statistics are far from the
    graph's.  Seen to fail with the forward all-reduce of the composition skipped (P = 2, contiguous part
    vector: train loss off by 2.1e-2 at epoch 0) and with the backward one skipped (9.9e-3 at epoch 1, the first epoch that sees the
    wrong gradient)."""
    paths, data = dataset
    ref, final, running = references[dropout]
    for P in (1, 2, 3):
        res = W.spawn_run(P, paths, False, dropout=dropout, partvec=partvec, optimizer=optimizer)
        worst = W.check_losses(res, ref)
        wr = W.check_running(res, running)
        print("P = %d, dropout %.1f, %s, optimizer %s: largest loss error %.3g, running statistics %.3g" % (P, dropout, partvec, optimizer,
                                                                                                           worst, wr))
        assert res[0]["widths"] == WIDTHS and len(res[0]["running"]) == 2
        lines = res[0]["stdout"].strip().splitlines()
        assert lines[-1].startswith("Best Val ") and len([l for l in lines if l.startswith("Epoch ")]) == W.EPOCHS


# ---- eval mode, and the model without norm ---------------------------------------------------------------------------------------------

class _Eng:
    class part:
        owned = torch.arange(50)
        n = 50

    def forward(self, H):
        return H * 2.0

    def backward(self, g):
        return g * 2.0


def test_eval_mode_uses_the_running_statistics_and_leaves_them():
    P = pkg("PGCN")
    P.world_size = 1
    torch.manual_seed(0)
    H = torch.randn(50, 16) * 3 + 1
    layer = P.PGCN(_Eng(), 16, 12, norm="batch", dropout=0.5, layer=1)
    assert [n for n, _ in layer.named_parameters()] == ["bn_weight", "bn_bias", "linear.weight"]
    assert torch.equal(layer.bn_weight.data, torch.ones(12)) and torch.equal(layer.bn_bias.data, torch.zeros(12))
    assert sorted(n for n, _ in layer.named_buffers()) == ["running_mean", "running_var"]
    layer.train()
    y_train = layer(H)
    rm, rv = layer.running_mean.clone(), layer.running_var.clone()
    assert not torch.equal(rm, torch.zeros(12)) and bool((y_train == 0).any())
    model = torch.nn.Sequential(layer, P.PGCN(_Eng(), 12, 3, relu=False))
    labels, split = torch.arange(50) % 3, (torch.arange(50) % 4).to(torch.uint8)
    ev = P.evaluate(model, H, labels, split)
    assert model.training and np.isfinite(ev["loss"]["train"])
    assert torch.equal(layer.running_mean, rm) and torch.equal(layer.running_var, rv)          # evaluate() left them alone
    layer.eval()
    y_eval = layer(H)
    assert torch.equal(layer.running_mean, rm) and torch.equal(layer.running_var, rv)
    X = P.mm_nt(H * 2.0, layer.linear.weight).detach().double().numpy()
    want, _, _ = W.bn64(X, np.ones(12), np.zeros(12), mean=rm.double().numpy(), var=rv.double().numpy())
    assert np.abs(y_eval.detach().double().numpy() - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    layer.train()
    layer(H)
    assert not torch.equal(layer.running_mean, rm)                       # training mode updates them
    with pytest.raises(ValueError, match="relu=True"):
        P.PGCN(_Eng(), 16, 7, relu=False, norm="batch")
    with pytest.raises(ValueError, match="norm takes"):
        P.PGCN(_Eng(), 16, 7, norm="layer")


def test_models_without_norm_are_unchanged(dataset):
    """norm=None / "none": no new parameter, buffer or launch -- the state dict, the outputs and a whole data run are those of a model
    built without the argument, bit for bit."""
    P = pkg("PGCN")
    torch.manual_seed(3)
    H = torch.randn(50, 16)
    torch.manual_seed(4)
    a = P.PGCN(_Eng(), 16, 16)
    torch.manual_seed(4)
    b = P.PGCN(_Eng(), 16, 16, norm=None)
    torch.manual_seed(4)
    c = P.PGCN(_Eng(), 16, 16, norm="none")
    assert list(a.state_dict()) == list(b.state_dict()) == list(c.state_dict()) == ["linear.weight"]
    assert torch.equal(a(H), b(H)) and torch.equal(a(H), c(H))
    paths = dataset[0]
    runs = [W.spawn_run(1, paths, False, norm=norm, nlayers=2, epochs=3) for norm in (None, "none")]
    assert runs[0][0]["history"] == runs[1][0]["history"] and runs[0][0]["stdout"].split("Elapsed")[0] == runs[1][0]["stdout"].split("Elapsed")[0]
    for x, y in zip(runs[0][0]["params"], runs[1][0]["params"]):
        assert np.array_equal(x, y)
    assert len(runs[0][0]["params"]) == 2 and runs[0][0]["running"] == []


# ---- run() and the command line -----------------------------------------------------------------------------------------------------------

BASE = ["-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"), "-b", "gloo", "-s", "1", "-l", "2", "-f", "16"]


def test_run_refuses_norm_without_files_or_an_unknown_norm(dataset):
    M = pkg("PGCN")
    with pytest.raises(ValueError, match="needs features, labels and split"):
        M.run(0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo", norm="batch")
    p = dataset[0]
    with pytest.raises(ValueError, match="norm takes"):
        M.run(0, 1, 2, 16, p["A"], p["pv1"], "gloo", features=p["features"], labels=p["labels"], split=p["split"], norm="layer")


def _keep_cli_state(monkeypatch, M):
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        if k in os.environ:
            monkeypatch.setenv(k, os.environ[k])
        else:
            monkeypatch.delenv(k, raising=False)
    for name in ("path_A", "path_partvec"):
        monkeypatch.setattr(M, name, getattr(M, name, None), raising=False)


@pytest.mark.parametrize("bad", [["--norm", "batch"], ["--norm", "layer"], ["--features", "F", "--labels", "L", "--split", "S", "--norm", "x"]])
def test_cli_rejects_norm_without_files_or_an_unknown_norm(monkeypatch, dataset, bad, capsys):
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    paths = dataset[0]
    argv = [{"F": paths["features"], "L": paths["labels"], "S": paths["split"]}.get(a, a) for a in bad]
    with pytest.raises(SystemExit) as e:
        M.main(BASE + argv)
    assert e.value.code == 2
    out = capsys.readouterr().out
    assert "--norm" in out


def test_cli_forwards_norm_and_nothing_else(monkeypatch, dataset):
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
    M.main(BASE + ["--norm", "none"])
    M.main(BASE + files)
    M.main(BASE + files + ["--norm", "none"])
    M.main(BASE + files + ["--norm", "batch"])
    M.main(BASE + files + ["--norm", "batch", "--optimizer", "fused", "--dropout", "0.5"])
    args = (0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo")
    three = {"features": paths["features"], "labels": paths["labels"], "split": paths["split"]}
    assert seen[0] == seen[1] == (args, {})                          # no option, or the default spelled out: today's call
    assert seen[2] == seen[3] == (args, three)
    assert seen[4] == (args, dict(three, norm="batch"))
    assert seen[5] == (args, dict(three, norm="batch", optimizer="fused", dropout=0.5, dropout_seed=0))


def test_cli_norm_batch_prints_the_usual_lines(monkeypatch, dataset):
    """--norm batch with the three files, one rank over gloo in this process (the checker-backed provider): the usual lines."""
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    from conftest import free_port
    from oracle_kernels import OracleKernels
    paths = dataset[0]

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
    monkeypatch.setenv("MASTER_PORT", str(free_port()))
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setattr(M, "_kernel_provider", OracleKernels())
    monkeypatch.setattr(M, "_exchanger", None)
    buf = io.StringIO()
    with redirect_stdout(buf):
        M.main(["-a", paths["A"], "-p", paths["pv1"], "-b", "gloo", "-s", "1", "-l", "3", "-f", "16", "--normalize", "sym", "--features",
                paths["features"], "--labels", paths["labels"], "--split", paths["split"], "--hidden", "16", "--epochs", "3", "--lr", "0.01",
                "--norm", "batch"])
    lines = buf.getvalue().strip().splitlines()
    assert [l[:11] for l in lines if l.startswith("Epoch ")] == ["Epoch 00000", "Epoch 00001", "Epoch 00002"]
    assert any(l.startswith("Elapsed time ") for l in lines) and lines[-1].startswith("Best Val ")
