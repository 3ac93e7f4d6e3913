"""GraphSAGE-style layers: root weight and bias, fused with ReLU and dropout (csrc/pgcn_combine.hip, PGCN._CombineBiasReluDropout,
PGCN(root_weight=, bias=), run(root_weight=, bias=), --root-weight / --bias) -- the CPU side: the framework composition against
float64 autograd, the module's structure, the batch-norm rule, data runs against a float64 numpy loop, partition independence over
gloo, and the command line.  The kernels are held in test_rootweight_gpu.py."""
import os

import numpy as np
import pytest
import torch

import _rootweight_workers as W
from conftest import gpath, pkg


# ---- the composition ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f", [1, 5, 128])
@pytest.mark.parametrize("relu", [True, False])
def test_composition_against_float64_autograd(f, relu):
    """The node on CPU tensors (the composition) at n = 37: forward and Gm bit-equal to the fp32 expression, both within rounding of
    float64 autograd of relu((z1 + z2) + b) * keep * scale, dbias within ulp32(ref64) + n 2^-52 sum |Gm|."""
    P, D = pkg("PGCN"), pkg("dropout")
    n = 37
    rng = np.random.default_rng(10 * f + relu)
    z1, z2, G = (rng.standard_normal((n, f)).astype(np.float32) for _ in range(3))
    b = rng.standard_normal(f).astype(np.float32)
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(5, "cpu")
    state.step.fill_(3)
    ids = torch.arange(n, dtype=torch.int64) * 7 + 11
    keep = D.keep_mask(5, 3, 2, ids, f, thr).numpy() if relu else None
    old = P._kernel_provider
    P._kernel_provider = None
    try:
        t1, t2, tb = (torch.from_numpy(a.copy()).requires_grad_(True) for a in (z1, z2, b))
        Y = P._CombineBiasReluDropout.apply(t1, t2, tb, relu, ids if relu else None, state if relu else None, 2, thr if relu else 0,
                                            scale if relu else 1.0)
        Y.backward(torch.from_numpy(G))
    finally:
        P._kernel_provider = old
    want = W.combine32(z1, z2, b, relu, keep, scale)
    Yn = Y.detach().numpy()
    assert np.array_equal(Yn.view(np.int32), want.view(np.int32))
    Gm = W.masked_grad32(G, Yn, relu, scale)
    assert np.array_equal(t1.grad.numpy().view(np.int32), Gm.view(np.int32))
    assert np.array_equal(t2.grad.numpy().view(np.int32), Gm.view(np.int32))
    err, bound = W.dbias_error_and_bound(tb.grad.numpy(), Gm)
    print("f %d relu %s: dbias error / bound %.3g" % (f, relu, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    # float64 autograd of the definition on the same fp32 inputs
    d1, d2, db = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (z1, z2, b))
    t = (d1 + d2) + db
    y64 = torch.relu(t) * torch.from_numpy(keep).double() * float(scale) if relu else t
    y64.backward(torch.from_numpy(G.astype(np.float64)))
    agree = (t.detach().numpy() > 0) == (W.combine32(z1, z2, b, False) > 0)         # the sign of a sum near 0 may round either way
    assert agree.mean() > 0.99
    u = 2.0 ** -24
    tol = 4 * u * float(scale) * (np.abs(z1) + np.abs(z2) + np.abs(b)[None]).astype(np.float64)
    assert (np.abs(Yn - y64.detach().numpy())[agree] <= tol[agree]).all()
    assert (np.abs(Gm - d1.grad.numpy())[agree] <= 2 * u * np.abs(G * scale)[agree]).all()
    assert torch.equal(d1.grad, d2.grad)
    exact = np.where(agree, Gm.astype(np.float64), d1.grad.numpy()).sum(0)          # where the signs differ the definition's own element
    assert np.abs(db.grad.numpy() - exact).max() <= 4 * u * np.abs(G * scale).sum(0).max()


def test_absent_terms_are_not_added_and_no_dropout_without_relu():
    P = pkg("PGCN")
    z1 = torch.tensor([[-0.0, 1.0, -2.0]])
    assert np.signbit(P.combine_composed(z1, None, None, relu=False).numpy()[0, 0])           # -0.0 + nothing stays -0.0
    assert not np.signbit(P.combine_composed(z1, torch.zeros(1, 3), None, relu=False).numpy()[0, 0])
    assert P.combine_composed(z1, None, None, relu=False).data_ptr() != z1.data_ptr()
    Gm, db = P.combine_backward_composed(torch.ones(1, 3), None, relu=False)
    assert torch.equal(Gm, torch.ones(1, 3)) and torch.equal(db, torch.ones(3))
    Gm, db = P.combine_backward_composed(torch.ones(1, 3), torch.tensor([[0.0, 2.0, 0.0]]), relu=True, scale=2.0, want_dbias=False)
    assert torch.equal(Gm, torch.tensor([[0.0, 2.0, 0.0]])) and db is None


def test_binding_answers_none_for_what_the_kernels_do_not_cover():
    kernels = pkg("kernels")
    k = object.__new__(kernels.HipKernels)
    k.device, k.lib = torch.device("cuda:0"), None
    X = torch.zeros(4, 8)
    assert k.combine_forward(X, X, torch.zeros(8), True) is None and k.combine_backward(X, X, True) is None
    assert kernels.COMBINE_SUM_ROWS == 512 and kernels.COMBINE_MAX_F == 1024


def test_entry_points_refuse_bad_arguments_without_a_device():
    """The refusals of include/pgcn_hip.h's combine section on the loaded library: the answer comes before any launch."""
    import ctypes
    _lib = pkg("_lib")
    L = _lib.lib()
    EINVAL, EUNSUP, ENOMEM = -1, _lib.PGCN_EUNSUPPORTED, -4
    buf = (ctypes.c_double * 4096)()
    a = ctypes.addressof(buf)
    M, V, WS, ST = a, a + 8192, a + 16384, a + 24576
    wsb = L.pgcn_combine_ws_bytes
    assert wsb(0, 4) == wsb(1, 4) == wsb(512, 4) == 4 * 8 and wsb(513, 4) == 2 * 4 * 8 and wsb(2049, 1024) == 5 * 1024 * 8
    assert wsb(-1, 4) == -1 and wsb(4, 0) == -1 and wsb(4, 1025) == -1

    def fwd(Z1=M, ld1=8, Z2=M + 1024, ld2=8, bias=V, n=4, f=8, relu=1, ids=None, step=None, Y=M + 2048, ldy=8):
        return L.pgcn_combine_forward_f32(Z1, ld1, Z2, ld2, bias, n, f, relu, ids, 1, step, 0, 1 << 31, Y, ldy, None)

    def bwd(G=M, ldg=8, Y=M + 1024, ldy=8, n=4, f=8, relu=1, scale=2.0, Gm=M + 2048, ldgm=8, db=V, ws=WS, wb=1 << 12):
        return L.pgcn_combine_backward_f32(G, ldg, Y, ldy, n, f, relu, scale, Gm, ldgm, db, ws, wb, None)

    nan, inf = float("nan"), float("inf")
    for fn, name, bads in (
            (fwd, "pgcn_combine_forward_f32", [dict(Z1=None), dict(Y=None), dict(n=-1), dict(f=0), dict(f=-2), dict(ld1=7), dict(ld2=7),
                                               dict(ldy=7), dict(step=ST + 4), dict(ids=ST + 4), dict(Y=M, ldy=16)]),
            (bwd, "pgcn_combine_backward_f32", [dict(G=None), dict(Y=None), dict(n=-1), dict(f=0), dict(ldg=7), dict(ldy=7), dict(ldgm=7),
                                                dict(ws=None), dict(ws=WS + 4), dict(scale=0.0), dict(scale=-1.0), dict(scale=nan),
                                                dict(scale=inf), dict(Gm=M, ldgm=16)])):
        for bad in bads:
            assert fn(**bad) == EINVAL, (name, bad)
            assert name.encode() in L.pgcn_last_error(), (name, bad)
    assert fwd(f=1028, ld1=1028, ld2=1028, ldy=1028) == EUNSUP and bwd(f=1028, ldg=1028, ldy=1028, ldgm=1028) == EUNSUP
    assert bwd(wb=63) == ENOMEM
    assert fwd(n=0, Z1=None, Y=None) == _lib.PGCN_OK and bwd(n=0, G=None, Y=None, Gm=None, db=None, ws=None) == _lib.PGCN_OK
    assert bwd(Gm=None, db=None, ws=None) == _lib.PGCN_OK                  # nothing asked for
    assert not any(buf)                                                  # and nothing was written


# ---- the module ------------------------------------------------------------------------------------------------------------------------------

class _Eng:
    class part:
        owned = torch.arange(50) * 3 + 1
        n = 200

    def forward(self, H):
        return H * 2.0

    def backward(self, g):
        return g * 2.0


def test_module_structure_and_defaults_off():
    P = pkg("PGCN")
    torch.manual_seed(3)
    H = torch.randn(50, 16)
    layer = P.PGCN(_Eng(), 16, 12, root_weight=True, bias=True)
    assert sorted(n for n, _ in layer.named_parameters()) == ["bias", "linear.weight", "root.weight"]
    assert layer.root.weight.shape == (12, 16) and torch.equal(layer.bias.data, torch.zeros(12))
    only_root, only_bias = P.PGCN(_Eng(), 16, 12, root_weight=True), P.PGCN(_Eng(), 16, 12, bias=True)
    assert sorted(only_root.state_dict()) == ["linear.weight", "root.weight"] and sorted(only_bias.state_dict()) == ["bias", "linear.weight"]
    torch.manual_seed(4)
    a = P.PGCN(_Eng(), 16, 16)
    torch.manual_seed(4)
    b = P.PGCN(_Eng(), 16, 16, root_weight=False, bias=False)
    assert list(a.state_dict()) == list(b.state_dict()) == ["linear.weight"]
    assert not hasattr(b, "root") and not hasattr(b, "bias")
    assert torch.equal(a(H), b(H))
    for kw in (dict(relu=False), dict(dropout=0.5, layer=1), dict(norm="batch")):
        torch.manual_seed(4)
        a = P.PGCN(_Eng(), 16, 16, **kw)
        torch.manual_seed(4)
        b = P.PGCN(_Eng(), 16, 16, root_weight=False, bias=False, **kw)
        assert list(a.state_dict()) == list(b.state_dict()) and torch.equal(a(H), b(H))
        ga, gb = a(H).grad_fn, b(H).grad_fn
        assert type(ga).__name__ == type(gb).__name__ and "Combine" not in type(gb).__name__          # the same autograd node


def test_layer_is_the_definition_and_its_gradients():
    """y = drop(relu(2 H W_n^T + H W_r^T + b)) with the stub engine (A H = 2 H), against float64 autograd; dH sums both paths."""
    P, D = pkg("PGCN"), pkg("dropout")
    torch.manual_seed(7)
    H = torch.randn(50, 16, requires_grad=True)
    G = torch.randn(50, 12)
    for relu, p in ((True, 0.0), (True, 0.5), (False, 0.0)):
        layer = P.PGCN(_Eng(), 16, 12, root_weight=True, bias=True, relu=relu, dropout=p, layer=1, state=D.DropoutState(9, "cpu"))
        with torch.no_grad():
            layer.bias.copy_(torch.randn(12))
        layer.train()
        Y = layer(H)
        grads = torch.autograd.grad(Y, (H, layer.linear.weight, layer.root.weight, layer.bias), G)
        Hd = H.detach().double().requires_grad_(True)
        wn, wr, b = (t.detach().double().requires_grad_(True) for t in (layer.linear.weight, layer.root.weight, layer.bias))
        t = ((2.0 * Hd) @ wn.t() + Hd @ wr.t()) + b
        if relu:
            thr, scale = D.threshold(p)
            keep = D.keep_mask(9, 0, 1, _Eng.part.owned, 12, thr).double() if p > 0 else torch.ones(50, 12, dtype=torch.float64)
            t = torch.relu(t) * keep * (float(scale) if p > 0 else 1.0)
        want = torch.autograd.grad(t, (Hd, wn, wr, b), G.double())
        assert float((Y.detach().double() - t.detach()).abs().max()) <= 1e-5
        for got, w in zip(grads, want):
            assert float((got.double() - w).abs().max()) <= 1e-4 * max(1.0, float(w.abs().max()))
        if p > 0:
            assert 0.3 < float((Y == 0).float().mean()) < 0.9
        layer.eval()
        if relu:
            assert float((layer(H).double() - torch.relu(((2.0 * Hd) @ wn.t() + Hd @ wr.t()) + b)).detach().abs().max()) <= 1e-5      # eval: no dropout


def test_a_normalised_hidden_layer_owns_no_bias():
    P = pkg("PGCN")
    P.world_size = 1
    layer = P.PGCN(_Eng(), 16, 12, norm="batch", root_weight=True, bias=True)
    assert sorted(n for n, _ in layer.named_parameters()) == ["bn_bias", "bn_weight", "linear.weight", "root.weight"]
    assert not hasattr(layer, "bias")
    torch.manual_seed(1)
    H = torch.randn(50, 16)
    layer.train()
    Y = layer(H)
    X = (2.0 * H.double()) @ layer.linear.weight.double().t() + H.double() @ layer.root.weight.double().t()
    want = torch.relu((X - X.mean(0)) / torch.sqrt(X.var(0, unbiased=False) + 1e-5))
    assert float((Y.double() - want).abs().max()) <= 1e-4
    out = P.PGCN(_Eng(), 16, 7, relu=False, root_weight=True, bias=True)      # the output layer keeps its bias
    assert sorted(n for n, _ in out.named_parameters()) == ["bias", "linear.weight", "root.weight"]


# ---- data runs ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("rootweight")))


@pytest.fixture(scope="module")
def references(dataset):
    return {p: W.float64_reference(dataset[1], dropout=p) for p in (0.0, W.DROPOUT)}


@pytest.fixture(scope="module")
def one_rank_with_dropout(dataset):
    return W.spawn_run(1, dataset[0], False, dropout=W.DROPOUT, masks=True)


@pytest.mark.parametrize("dropout,optimizer", [(0.0, None), (W.DROPOUT, None), (0.0, "fused"), (W.DROPOUT, "fused")])
def test_data_run_against_a_float64_numpy_loop(dataset, references, one_rank_with_dropout, dropout, optimizer):
    """3 layers with root weight and bias on one rank against the float64 numpy restatement of the loop (the same initial weights, Adam,
    the keep function of dropout.py): every reported loss within 1e-5 (relative, floor 1), the same best-validation epoch."""
    paths, _ = dataset
    ref, best = references[dropout]
    res = one_rank_with_dropout if (dropout > 0 and optimizer is None) else W.spawn_run(1, paths, False, dropout=dropout, optimizer=optimizer)
    worst = W.check_losses(res, ref)
    print("dropout %.1f optimizer %s: largest loss error %.3g; best epochs %d / %d" % (dropout, optimizer, worst, res[0]["best"]["epoch"], best))
    assert res[0]["best"]["epoch"] == best
    assert res[0]["widths"] == W.WIDTHS and len(res[0]["params"]) == 9
    assert sorted(res[0]["names"]) == sorted("%d.%s" % (i, n) for i in range(3) for n in ("bias", "linear.weight", "root.weight"))
    assert all(np.abs(p).max() > 0 for p in res[0]["params"])                                  # every bias moved off zero: it is trained
    lines = res[0]["stdout"].strip().splitlines()
    assert lines[-1].startswith("Best Val ") and len([l for l in lines if l.startswith("Epoch ")]) == W.EPOCHS


@pytest.mark.parametrize("P,partvec", [(2, "pv"), (2, "cpv"), (3, "pv"), (3, "cpv")])
def test_ranks_under_any_part_vector_reproduce_one_rank(dataset, one_rank_with_dropout, P, partvec):
    """World sizes 2 and 3 under a random and a contiguous part vector against one rank, dropout on: losses within 1e-5 (relative, floor
    1) and the first hidden layer's train-mode masks equal element for element in global row order -- and equal to dropout.py's keep
    function of the global row ids."""
    D = pkg("dropout")
    paths, _ = dataset
    one = one_rank_with_dropout
    res = W.spawn_run(P, paths, False, dropout=W.DROPOUT, partvec=partvec, masks=True)
    worst = 0.0
    for a, b in zip(res[0]["history"], one[0]["history"]):
        assert a["epoch"] == b["epoch"]
        for name in W.SETS:
            worst = max(worst, abs(a["losses"][name] - b["losses"][name]) / max(1.0, abs(b["losses"][name])))
    print("P = %d %s: largest loss difference to one rank %.3g" % (P, partvec, worst))
    assert len(res[0]["history"]) == W.EPOCHS and worst <= 1e-5
    yt, ye = W.gather_rows(res, "y_train"), W.gather_rows(res, "y_eval")
    yt1, ye1 = W.gather_rows(one, "y_train"), W.gather_rows(one, "y_eval")
    clear = (ye > 1e-4) & (ye1 > 1e-4)                                            # pre-activation positive beyond any rounding
    thr, _ = D.threshold(W.DROPOUT)
    keep = D.keep_mask(W.DROPOUT_SEED, W.MASK_STEP, 0, np.arange(W.N), W.HIDDEN, thr).numpy()
    assert clear.mean() > 0.2 and 0.45 < (~keep).mean() < 0.55
    assert np.array_equal((yt != 0)[clear], (yt1 != 0)[clear])
    assert np.array_equal((yt != 0)[clear], keep[clear]) and not (yt != 0)[~keep].any()


# ---- run() and the command line ----------------------------------------------------------------------------------------------------------------

BASE = ["-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"), "-b", "gloo", "-s", "1", "-l", "2", "-f", "16"]


def _keep_cli_state(monkeypatch, M):
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        if k in os.environ:
            monkeypatch.setenv(k, os.environ[k])
        else:
            monkeypatch.delenv(k, raising=False)
    for name in ("path_A", "path_partvec"):
        monkeypatch.setattr(M, name, getattr(M, name, None), raising=False)


def test_run_refuses_the_options_without_files():
    M = pkg("PGCN")
    for kw in (dict(root_weight=True), dict(bias=True)):
        with pytest.raises(ValueError, match="need features, labels and split"):
            M.run(0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo", **kw)


@pytest.mark.parametrize("bad", [["--root-weight"], ["--bias"], ["--root-weight", "--bias", "--features", "F"]])
def test_cli_rejects_the_flags_without_the_files(monkeypatch, bad, capsys):
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    with pytest.raises(SystemExit) as e:
        M.main(BASE + bad)
    assert e.value.code == 2
    out = capsys.readouterr().out
    assert "go together" in out and "--root-weight, --bias need them" in out and bad[0] in out.split("got")[1]


def test_cli_forwards_the_flags_and_nothing_else(monkeypatch, dataset):
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
    M.main(BASE + files)
    M.main(BASE + files + ["--root-weight"])
    M.main(BASE + files + ["--bias"])
    M.main(BASE + files + ["--root-weight", "--bias", "--norm", "batch", "--weight-decay", "0.01", "--dropout", "0.5"])
    args = (0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo")
    three = {"features": paths["features"], "labels": paths["labels"], "split": paths["split"]}
    assert seen[0] == (args, three)                                   # no new flag: today's call
    assert seen[1] == (args, dict(three, root_weight=True))
    assert seen[2] == (args, dict(three, bias=True))
    assert seen[3] == (args, dict(three, root_weight=True, bias=True, norm="batch", weight_decay=0.01, dropout=0.5, dropout_seed=0))
