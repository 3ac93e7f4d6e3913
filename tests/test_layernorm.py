"""Layer normalisation of a vertex over its features and residual links, fused with ReLU and dropout (csrc/pgcn_layernorm.hip,
PGCN._LayerNormReluDropout, PGCN(norm="node", residual=True), run(norm=..., residual=...), --norm node, --residual) -- the CPU side:
the float64 definition against torch.nn.functional.layer_norm, the framework composition against the definition within the bounds of
tests/_layernorm_workers.py, the entry points' refusals on the loaded library, the module's structure, an 8-layer data run on 1 - 3
ranks over gloo against a one-process float64 loop, and the command line.  The kernels are held in test_layernorm_gpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _layernorm_workers as W
from conftest import gpath, pkg


# ---- the definition ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,f", [(2, 3), (65, 7), (300, 33)])
def test_definition_is_torch_layer_norm_in_float64(n, f):
    """ln64 / ln_backward64 against torch.nn.functional.layer_norm in double followed by relu, autograd included, to 1e-12."""
    X, gamma, beta, G, _ = (a.astype(np.float64) for a in W.make_case(n, f, 100 * n + f))
    xt, gt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (X, gamma, beta))
    yt = torch.relu(torch.nn.functional.layer_norm(xt, (f,), gt, bt, W.EPS))
    yt.backward(torch.from_numpy(G))
    ref = W.ln64(X, gamma, beta)
    back = W.ln_backward64(G, X, ref["mean"], ref["rstd"], gamma, ref["t"] > 0)
    for name, got, want in (("Y", ref["Y"], yt), ("dX", back["dX"], xt.grad), ("dgamma", back["dgamma"], gt.grad),
                            ("dbeta", back["dbeta"], bt.grad)):
        want = want.detach().numpy()
        e = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        print("n %d f %d %s: %.3g" % (n, f, name, e))
        assert e <= 1e-12, (name, e)
    assert abs(ref["rstd"][2] * np.sqrt(W.EPS) - 1.0) <= 1e-6 if n > 2 else True        # the constant row: variance 0


# ---- the composition -------------------------------------------------------------------------------------------------------------------

def _run_node(P, X, gamma, beta, G, R, drop, seed=5, step=3, layer=2, p=0.5):
    """The autograd node on CPU tensors -> (got of W.check_case, keep, scale, x.grad of R)."""
    D = pkg("dropout")
    n, f = X.shape
    thr, scale = D.threshold(p if drop else 0.0)
    state = D.DropoutState(seed, "cpu") if drop else None
    if state is not None:
        state.step.fill_(step)
    ids = torch.arange(n, dtype=torch.int64) * 7 + 11
    x, g_, b_ = (torch.from_numpy(a).clone().requires_grad_(True) for a in (X, gamma, beta))
    r = torch.from_numpy(R).clone().requires_grad_(True) if R is not None else None
    Y = P._LayerNormReluDropout.apply(x, g_, b_, r, True, W.EPS, ids if drop else None, state, layer, thr, scale)
    saved = Y.grad_fn.saved_tensors
    assert len(saved) == 5 and saved[0] is not None                     # X, gamma, mean, rstd and the bits: nothing else
    mean, rstd, bits = saved[2], saved[3], saved[4]
    Y.backward(torch.from_numpy(G))
    keep = D.keep_mask(seed, step, layer, ids, f, thr).numpy() if drop else None
    got = {"Y": Y.detach().numpy(), "mean": mean.numpy(), "rstd": rstd.numpy(), "bits": bits.numpy().astype(bool),
           "dX": x.grad.numpy(), "dgamma": g_.grad.numpy(), "dbeta": b_.grad.numpy()}
    return got, keep, scale, (r.grad if r is not None else None)


@pytest.mark.parametrize("drop,with_r", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("n,f", [(5, 1), (65, 3), (65, 100), (513, 32), (5, 1024)])
def test_composition_meets_the_bounds(n, f, drop, with_r):
    P = pkg("PGCN")
    P.world_size = 1
    X, gamma, beta, G, R = W.make_case(n, f, 7 * n + f)
    got, keep, scale, rgrad = _run_node(P, X, gamma, beta, G, R if with_r else None, drop)
    W.check_case("composition%s%s" % (" dropout" if drop else "", " R" if with_r else ""), X, gamma, beta, G, got, keep, scale,
                 R if with_r else None)
    if with_r:
        assert torch.equal(rgrad, torch.from_numpy(G))                    # the residual's gradient is G itself
    if drop:
        ref = W.ln64(X, gamma, beta)
        _, cmp_, _ = W.forward_bounds(X, gamma, beta, ref, scale)
        d = got["Y"].astype(np.float64) - (R if with_r else 0.0)
        sel = cmp_ & (ref["t"] > 0)
        if with_r:                                                       # (R + d == R does not say d == 0 in fp32: use the bits)
            assert np.array_equal(got["bits"][sel], keep[sel])
        else:
            assert np.array_equal((d != 0)[sel], keep[sel])              # every zero under dropout is a zero of dropout.keep_mask
        if n * f >= 1000:
            assert 0.4 < (~keep).mean() < 0.6


def test_only_the_residual_wants_a_gradient():
    """Frozen parameters, X without a gradient, R with one: nothing is saved and R's gradient is G itself."""
    P = pkg("PGCN")
    X, gamma, beta, G, R = (torch.from_numpy(a) for a in W.make_case(65, 33, 2))
    r = R.clone().requires_grad_(True)
    Y = P._LayerNormReluDropout.apply(X, gamma, beta, r, True, W.EPS, None, None, 0, 0, 1.0)
    assert len(Y.grad_fn.saved_tensors) == 0
    Y.backward(G)
    assert torch.equal(r.grad, G)


def test_composition_eval_mode_saves_nothing_and_drops_nothing():
    P, D = pkg("PGCN"), pkg("dropout")
    X, gamma, beta, _, R = (torch.from_numpy(a) for a in W.make_case(65, 33, 1))
    state = D.DropoutState(5, "cpu")
    thr, scale = D.threshold(0.5)
    a = P._LayerNormReluDropout.apply(X, gamma, beta, R, False, W.EPS, torch.arange(65), state, 0, thr, scale)
    b = P._LayerNormReluDropout.apply(X, gamma, beta, R, True, W.EPS, None, None, 0, 0, 1.0)
    assert torch.equal(a, b) and a.grad_fn is None


# ---- the entry points without a device -------------------------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every refusal of include/pgcn_hip.h's layer-norm section, on the loaded library: the answer comes before any launch."""
    _lib, kernels = pkg("_lib"), pkg("kernels")
    L = _lib.lib()
    EINVAL, EUNSUP, ENOMEM = -1, _lib.PGCN_EUNSUPPORTED, -4
    buf = (ctypes.c_double * 8192)()
    a = ctypes.addressof(buf)
    M, V, WS, ST = a, a + 40960, a + 49152, a + 57344                    # matrices, vectors, work-space, step / row ids
    nan, inf = float("nan"), float("inf")
    assert kernels.LN_MAX_F == 1024 and kernels.LN_STAT_ROWS == 512
    wsb = L.pgcn_ln_ws_bytes
    one = 2 * 4 * 8
    assert [wsb(n, 4) for n in (0, 1, 512, 513, 2049)] == [one, one, one, 2 * one, 5 * one]     # one record per band, at least one
    assert wsb(2049, 1024) == 5 * 2 * 1024 * 8
    assert wsb(-1, 4) == -1 and wsb(4, 0) == -1 and wsb(4, 1025) == -1

    def forward(X=M, ldx=8, n=4, f=8, g=V, b=V + 64, eps=1e-5, R=M + 1024, ldr=8, ids=None, step=None, Y=M + 2048, ldy=8, mean=V + 128,
                rstd=V + 256, mask=V + 384):
        return L.pgcn_ln_relu_forward_f32(X, ldx, n, f, g, b, eps, R, ldr, ids, 1, step, 0, 1 << 31, Y, ldy, mean, rstd, mask, None)

    def backward(G=M, ldg=8, X=M + 1024, ldx=8, n=4, f=8, mean=V, rstd=V + 64, g=V + 128, mask=V + 256, scale=2.0, dX=M + 2048, ldd=8,
                 dg=V + 384, db=V + 512, ws=WS, wb=1 << 12):
        return L.pgcn_ln_relu_backward_f32(G, ldg, X, ldx, n, f, mean, rstd, g, mask, scale, dX, ldd, dg, db, ws, wb, None)

    cases = [
        (forward, "pgcn_ln_relu_forward_f32", [
            dict(X=None), dict(Y=None), dict(g=None), dict(b=None), dict(n=-1), dict(f=0), dict(f=-3), dict(ldx=7), dict(ldy=7), dict(ldr=7),
            dict(eps=0.0), dict(eps=-1e-5), dict(eps=nan), dict(eps=inf), dict(step=ST + 4), dict(ids=ST + 4), dict(mask=V + 386),
            dict(R=M + 2048, ldr=16, ldy=8, Y=M + 2048),                    # in place with differing leading dimensions
            dict(mean=None), dict(rstd=None), dict(mask=None), dict(mean=None, rstd=None), dict(mean=None, mask=None),
            dict(rstd=None, mask=None)]),                                 # only some of mean, rstd, mask
        (backward, "pgcn_ln_relu_backward_f32", [
            dict(G=None), dict(X=None), dict(dX=None), dict(mean=None), dict(rstd=None), dict(g=None), dict(mask=None), dict(n=-1), dict(f=0),
            dict(ldg=7), dict(ldx=7), dict(ldd=7), dict(scale=0.0), dict(scale=-1.0), dict(scale=nan), dict(scale=inf), dict(ws=None),
            dict(ws=WS + 4), dict(mask=V + 258), dict(dg=None), dict(db=None)]),
    ]
    for fn, name, bads in cases:
        for bad in bads:
            assert fn(**bad) == EINVAL, (name, bad)
            assert name.encode() in L.pgcn_last_error(), (name, bad)
        wide = dict(f=1025)
        wide.update({k: 1025 for k in ("ldx", "ldy", "ldr", "ldg", "ldd") if k in fn.__code__.co_varnames})
        assert fn(**wide) == EUNSUP, name                                # above 1024 columns
    assert backward(wb=2 * 8 * 8 - 1) == ENOMEM and backward(n=513, wb=2 * 2 * 8 * 8 - 1) == ENOMEM
    # nothing to do: no launch, nothing written (with sums asked for and no rows the second level would run: not here)
    assert forward(n=0, X=None, Y=None, R=None, mean=None, rstd=None, mask=None) == _lib.PGCN_OK
    assert backward(n=0, G=None, X=None, dX=None, mean=None, rstd=None, mask=None, dg=None, db=None, ws=None, wb=0) == _lib.PGCN_OK
    assert not any(buf)


def test_binding_answers_none_for_what_the_kernels_do_not_cover():
    kernels = pkg("kernels")
    k = object.__new__(kernels.HipKernels)
    k.device, k.lib = torch.device("cuda:0"), None
    X, v, r = torch.zeros(4, 8), torch.zeros(8), torch.zeros(4)
    assert k.ln_relu_forward(X, v, v, 1e-5) is None
    assert k.ln_relu_backward(X, X, r, r, v, torch.zeros((4, 1), dtype=torch.int32)) is None


# ---- the module -------------------------------------------------------------------------------------------------------------------------

class _Eng:
    class part:
        owned = torch.arange(50) * 3 + 1
        n = 200

    def forward(self, H):
        return H * 2.0

    def backward(self, g):
        return g * 2.0


def test_module_structure_and_refused_settings():
    P = pkg("PGCN")
    P.world_size = 1
    assert P.NORMS == ("none", "batch", "node")
    layer = P.PGCN(_Eng(), 16, 12, norm="node", dropout=0.5, layer=1, bias=True)
    assert [n for n, _ in layer.named_parameters()] == ["ln_weight", "ln_bias", "linear.weight"]      # no `bias` under norm="node"
    assert torch.equal(layer.ln_weight.data, torch.ones(12)) and torch.equal(layer.ln_bias.data, torch.zeros(12)) and layer.ln_eps == 1e-5
    assert list(layer.named_buffers()) == []
    rooted = P.PGCN(_Eng(), 16, 16, norm="node", root_weight=True, residual=True)
    assert [n for n, _ in rooted.named_parameters()] == ["ln_weight", "ln_bias", "linear.weight", "root.weight"]
    with pytest.raises(ValueError, match="norm takes"):
        P.PGCN(_Eng(), 16, 7, norm="layer")
    with pytest.raises(ValueError, match="relu=True"):
        P.PGCN(_Eng(), 16, 7, relu=False, norm="node")
    with pytest.raises(ValueError, match="in_features == out_features"):
        P.PGCN(_Eng(), 16, 12, residual=True)
    with pytest.raises(ValueError, match="relu=True"):
        P.PGCN(_Eng(), 16, 16, relu=False, residual=True)
    # eval(): the same statistics without dropout; train(): zeros of the dropout
    torch.manual_seed(0)
    H = torch.randn(50, 16) * 3 + 1
    layer.train()
    yt = layer(H)
    layer.eval()
    ye = layer(H)
    X = P.mm_nt(H * 2.0, layer.linear.weight).detach().double().numpy()
    want = W.ln64(X, np.ones(12), np.zeros(12))["Y"]
    assert np.abs(ye.detach().double().numpy() - want).max() <= 1e-5
    keep = pkg("dropout").keep_mask(0, 0, 1, _Eng.part.owned, 12, layer.dropout_thr).numpy()
    assert not (yt.detach().numpy() != 0)[~keep].any() and bool((yt == 0).any()) and 0.3 < (~keep).mean() < 0.7
    # the node with a root weight and a residual: H + relu(LN(Z1 + Z2)), gradients through every path
    Hr = H.clone().requires_grad_(True)
    y = rooted(Hr)
    Z = P.mm_nt(H * 2.0, rooted.linear.weight) + P.mm_nt(H, rooted.root.weight)
    want = H.double().numpy() + W.ln64(Z.detach().double().numpy(), np.ones(16), np.zeros(16))["Y"]
    assert np.abs(y.detach().double().numpy() - want).max() <= 1e-5
    y.sum().backward()
    assert Hr.grad is not None and rooted.root.weight.grad is not None and rooted.ln_weight.grad is not None


def test_models_without_the_options_are_unchanged():
    """No new parameter, buffer or branch without the options: state dict keys and outputs are those of a model built without them."""
    P = pkg("PGCN")
    P.world_size = 1
    torch.manual_seed(3)
    H = torch.randn(50, 16)
    nodes = ("_LinearReluNoBiasBackward", "_LinearReluDropoutNoBiasBackward", "_BatchNormReluDropoutBackward",
             "_CombineBiasReluDropoutBackward", "_LinearNoBiasBackward")                  # the autograd node each layer kind had before
    for node, kw in zip(nodes, ({}, {"dropout": 0.5, "layer": 1}, {"norm": "batch"}, {"root_weight": True, "bias": True}, {"relu": False})):
        torch.manual_seed(4)
        a = P.PGCN(_Eng(), 16, 16, **kw)
        torch.manual_seed(4)
        b = P.PGCN(_Eng(), 16, 16, residual=False, **kw)
        assert list(a.state_dict()) == list(b.state_dict()) and not any(k.startswith("ln_") for k in a.state_dict())
        assert a.residual is False
        ya, yb = a(H), b(H)
        assert torch.equal(ya, yb)
        assert type(ya.grad_fn).__name__ == node and type(yb.grad_fn).__name__ == node
    # the plain layer against its definition written out: relu((A H) W^T) with this engine's A H = 2 H
    torch.manual_seed(4)
    a = P.PGCN(_Eng(), 16, 16)
    assert torch.equal(a(H), torch.relu(P.mm_nt(H * 2.0, a.linear.weight)))


@pytest.mark.parametrize("kw", [{}, {"dropout": 0.5, "layer": 1}, {"norm": "batch"}, {"norm": "batch", "dropout": 0.5}, {"root_weight": True},
                                {"root_weight": True, "bias": True, "dropout": 0.5}, {"bias": True}])
def test_residual_on_the_other_layer_kinds_is_a_framework_addition(kw):
    """residual=True on a layer that is not norm="node": H + layer(H) of the same weights, bit for bit."""
    P = pkg("PGCN")
    P.world_size = 1
    torch.manual_seed(3)
    H = torch.randn(50, 16)
    torch.manual_seed(4)
    a = P.PGCN(_Eng(), 16, 16, **kw)
    torch.manual_seed(4)
    b = P.PGCN(_Eng(), 16, 16, residual=True, **kw)
    assert list(a.state_dict()) == list(b.state_dict())
    for s in a.state_dict():
        assert torch.equal(a.state_dict()[s], b.state_dict()[s])
    assert torch.equal(b(H), H + a(H))


# ---- an 8-layer data run ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("layernorm")))


WIDTHS = [W.FIN] + [W.HIDDEN] * 7 + [W.CLASSES]


@pytest.fixture(scope="module")
def references(dataset):
    return {p: W.float64_reference(dataset[1], WIDTHS, dropout=p) for p in (0.0, W.DROPOUT)}


@pytest.fixture(scope="module")
def one_rank_with_dropout(dataset):
    return W.spawn_run(1, dataset[0], False, dropout=W.DROPOUT, masks=True)


@pytest.mark.parametrize("dropout,optimizer", [(0.0, None), (W.DROPOUT, None), (0.0, "fused"), (W.DROPOUT, "fused")])
def test_deep_data_run_against_a_float64_loop(dataset, references, one_rank_with_dropout, dropout, optimizer):
    """8 layers, hidden 32, norm="node", residual=True, 8 epochs, lr 0.01 on one rank: every epoch's loss of every set within 1e-5
    relative of the one-process float64 loop (dense A, torch double autograd, keep_mask, Adam written out), the same best epoch."""
    paths, _ = dataset
    ref, best = references[dropout]
    res = one_rank_with_dropout if (dropout > 0 and optimizer is None) else W.spawn_run(1, paths, False, dropout=dropout, optimizer=optimizer)
    W.check_losses(res, ref)
    print("best epoch %d, the float64 loop's %d" % (res[0]["best"]["epoch"], best))
    assert res[0]["best"]["epoch"] == best
    assert res[0]["widths"] == WIDTHS and res[0]["buffers"] == []
    assert res[0]["residual"] == [False] + [True] * 6 + [False]           # every layer but the last whose two widths are equal
    assert res[0]["names"][:3] == ["0.ln_weight", "0.ln_bias", "0.linear.weight"] and res[0]["names"][-1] == "7.linear.weight"
    assert len(res[0]["names"]) == 3 * 7 + 1
    lines = res[0]["stdout"].strip().splitlines()
    assert lines[-1].startswith("Best Val ") and len([l for l in lines if l.startswith("Epoch ")]) == W.EPOCHS


@pytest.mark.parametrize("P,partvec", [(2, "pv"), (2, "cpv"), (3, "pv"), (3, "cpv")])
def test_ranks_under_any_part_vector_reproduce_one_rank(dataset, one_rank_with_dropout, P, partvec):
    """World sizes 2 and 3 under a random and a contiguous part vector against one rank, dropout 0.5: losses within 1e-5 relative and
    the first hidden layer's train-mode zeros equal element for element in global row order -- the zeros of dropout.py's keep function
    of the global row ids."""
    D = pkg("dropout")
    paths, _ = dataset
    one = one_rank_with_dropout
    res = W.spawn_run(P, paths, False, dropout=W.DROPOUT, partvec=partvec, masks=True)
    W.check_losses(res, one[0]["history"])
    assert res[0]["best"]["epoch"] == one[0]["best"]["epoch"]
    yt, ye = W.gather_rows(res, "y_train"), W.gather_rows(res, "y_eval")
    yt1, ye1 = W.gather_rows(one, "y_train"), W.gather_rows(one, "y_eval")
    clear = (ye > 1e-4) & (ye1 > 1e-4)                                            # pre-activation positive beyond any rounding
    thr, _ = D.threshold(W.DROPOUT)
    keep = D.keep_mask(W.DROPOUT_SEED, W.MASK_STEP, 0, np.arange(W.N), W.HIDDEN, thr).numpy()
    assert clear.mean() > 0.2 and 0.45 < (~keep).mean() < 0.55
    assert np.array_equal((yt != 0)[clear], (yt1 != 0)[clear])
    assert np.array_equal((yt != 0)[clear], keep[clear]) and not (yt != 0)[~keep].any()


# ---- run() and the command line -----------------------------------------------------------------------------------------------------------

BASE = ["-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"), "-b", "gloo", "-s", "1", "-l", "2", "-f", "16"]


def test_run_refuses_the_options_without_files():
    M = pkg("PGCN")
    with pytest.raises(ValueError, match="norm='node' needs features, labels and split"):
        M.run(0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo", norm="node")
    with pytest.raises(ValueError, match="needs features, labels and split"):
        M.run(0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo", residual=True)


def _keep_cli_state(monkeypatch, M):
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        if k in os.environ:
            monkeypatch.setenv(k, os.environ[k])
        else:
            monkeypatch.delenv(k, raising=False)
    for name in ("path_A", "path_partvec"):
        monkeypatch.setattr(M, name, getattr(M, name, None), raising=False)


@pytest.mark.parametrize("bad", [["--norm", "node"], ["--residual"], ["--norm", "node", "--residual"]])
def test_cli_rejects_the_options_without_files(monkeypatch, bad, capsys):
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    with pytest.raises(SystemExit) as e:
        M.main(BASE + bad)
    assert e.value.code == 2
    out = capsys.readouterr().out
    assert "--norm, --residual, --root-weight, --bias need them" in out
    for opt in bad:
        if opt.startswith("--"):
            assert opt in out.split("got ")[1]


def test_cli_forwards_the_options_and_nothing_else(monkeypatch, dataset):
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    paths = dataset[0]
    seen = []

    class InlineProcess:
        def __init__(self, target, args):
            self.target, self.args, self.exitcode = target, args, None
            tuples.append(args)

        def start(self):
            self.target(*self.args)
            self.exitcode = 0

        def join(self):
            pass

    tuples = []
    monkeypatch.setattr(M.mp, "Process", InlineProcess)
    monkeypatch.setattr(M.mp, "set_start_method", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "init_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "destroy_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M, "run", lambda *a, **k: seen.append((a, k)))
    files = ["--features", paths["features"], "--labels", paths["labels"], "--split", paths["split"]]
    M.main(BASE + files)
    M.main(BASE + files + ["--norm", "node"])
    M.main(BASE + files + ["--residual"])
    M.main(BASE + files + ["--norm", "node", "--residual", "--dropout", "0.5"])
    M.main(BASE + files + ["--norm", "batch"])
    M.main(BASE + files + ["--root-weight"])
    args = (0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo")
    three = {"features": paths["features"], "labels": paths["labels"], "split": paths["split"]}
    assert seen[0] == (args, three)
    assert seen[1] == (args, dict(three, norm="node"))
    assert seen[2] == (args, dict(three, residual=True))
    assert seen[3] == (args, dict(three, norm="node", residual=True, dropout=0.5, dropout_seed=0))
    assert seen[4] == (args, dict(three, norm="batch")) and seen[5] == (args, dict(three, root_weight=True))
    # the argument tuple handed to init_process grows only when --residual is given
    assert [len(t) for t in tuples] == [19, 23, 26, 26, 23, 25] and tuples[2][-1] is True and tuples[3][-1] is True
