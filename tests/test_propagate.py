"""Personalised-PageRank propagation of the logits (APPNP) on the CPU: the composed step functions against the numpy fp32 formula bit
for bit, the engine's propagate / propagate_backward on karate against the float64 recursion (one rank and over gloo with the golden
part vectors), the adjoint identity, the whole model against a double model, PGCN(aggregate=False), run(propagate=...) /
--propagate / --ppr-alpha / --dense-layers, checkpoints, the defaults, and the C entry points' argument checks (no device).

tests/_propagate_workers.py has the definition and the bound: (K + 1) x 1e-5 against the float64 recursion."""
import os

import numpy as np
import pytest
import torch

from conftest import gpath, pkg, rel_err

import _predict_workers as PW
import _propagate_workers as W


# ---- the composed steps are the formula ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", [0.0, 0.1, 0.5])
def test_composed_steps_are_the_fp32_formula_bit_for_bit(alpha):
    E = pkg("engine")
    rng = np.random.default_rng(int(alpha * 10))
    n, f = 37, 7
    S, H, G, T, D = (rng.standard_normal((n, f)).astype(np.float32) * 3 for _ in range(5))
    S[3, 2], H[5, 1] = np.float32(-0.0), np.float32(-0.0)
    t = torch.from_numpy
    a, b = E.ppr_coefficients(alpha)
    assert (np.float32(a), np.float32(b)) == W.coefficients(alpha) and a == float(np.float32(alpha))
    want = W.step_np(S, H, alpha)
    assert np.array_equal(W.bits(E.ppr_step_composed(t(S), t(H), alpha).numpy()), W.bits(want))
    Sc = t(S.copy())
    assert E.ppr_step_composed(Sc, t(H), alpha, out=Sc) is Sc and np.array_equal(W.bits(Sc.numpy()), W.bits(want))       # in place
    # first (no D), middle and last step of the adjoint
    for Din, last in ((None, False), (D, False), (D, True), (None, True)):
        wg, wd = W.step_backward_np(G, T, Din, alpha, last)
        gout, dout = E.ppr_step_backward_composed(t(G), t(T), None if Din is None else t(Din), alpha, last)
        assert np.array_equal(W.bits(dout.numpy()), W.bits(wd)), (alpha, last)
        assert (gout is None) if last else np.array_equal(W.bits(gout.numpy()), W.bits(wg)), (alpha, last)
        Tc, Dc = t(T.copy()), (t(T.copy()) if Din is None and last else None if Din is None else t(Din.copy()))
        gout, dout = E.ppr_step_backward_composed(t(G), Tc, None if Din is None else Dc, alpha, last, gout=None if last else Tc, dout=Dc)
        assert np.array_equal(W.bits(dout.numpy()), W.bits(wd)) and (Dc is None or dout is Dc), (alpha, last, "in place")
        assert last or (gout is Tc and np.array_equal(W.bits(Tc.numpy()), W.bits(wg)))
    if alpha == 0.0:                                   # the propagation of before the teleport: Z <- A Z exactly
        assert np.array_equal(W.bits(want), W.bits(S + np.float32(0.0) * H))


# ---- the engine on karate -----------------------------------------------------------------------------------------------------------

def _karate_engine():
    from oracle_kernels import OracleKernels
    P, E, I = pkg("partition"), pkg("engine"), pkg("ingest")
    A = I.mmread(gpath("karate.mtx")).tocoo()
    n = A.shape[0]
    part = P.build_partition(torch.from_numpy(A.row.astype(np.int64)), torch.from_numpy(A.col.astype(np.int64)),
                             torch.from_numpy(A.data.astype(np.float32)), n, torch.zeros(n, dtype=torch.int64), 0, 1, normalize="sym")
    return E.AggregationEngine(part, OracleKernels(), torch.device("cpu")), W.sym_normalised(A), n


@pytest.fixture(scope="module")
def karate():
    eng, Ad, n = _karate_engine()
    assert np.array_equal(Ad, Ad.T) and np.linalg.norm(Ad, 2) <= 1.0 + 1e-12
    return eng, Ad, n


@pytest.mark.parametrize("K,alpha,C", W.KARATE_CASES)
def test_propagate_on_karate_against_the_float64_recursion(karate, K, alpha, C):
    eng, Ad, n = karate
    own = eng.part.owned.numpy()
    Hg, Gg = W.seeded_operands(n, K, alpha, C)
    H = torch.from_numpy(Hg[own]).requires_grad_(True)
    M = pkg("PGCN")
    Z = M.Propagate(eng, K, alpha)(H)
    Z.backward(torch.from_numpy(Gg[own]))
    bound = (K + 1) * W.TOL
    ez = rel_err(Z.detach().numpy(), W.propagate64(Ad, Hg, K, alpha)[own])
    ed = rel_err(H.grad.numpy(), W.propagate_backward64(Ad, Gg, K, alpha)[own])
    print("K=%d alpha=%g C=%d: forward %.3g, dH %.3g (bound %.3g)" % (K, alpha, C, ez, ed, bound))
    assert ez <= bound and ed <= bound
    # the adjoint identity <propagate(X), Y> = <X, propagate_backward(Y)>
    D = eng.propagate_backward(torch.from_numpy(Gg[own]), K, alpha)
    assert torch.equal(D, H.grad)
    lhs, rhs = float((Z.detach().double() * torch.from_numpy(Gg[own]).double()).sum()), float((H.detach().double() * D.double()).sum())
    assert abs(lhs - rhs) <= bound * np.linalg.norm(Hg.astype(np.float64)) * np.linalg.norm(Gg.astype(np.float64))
    # the engine's steps ARE the composed formula around its own aggregation: one step by hand, bit for bit
    if K == 1:
        S = eng.forward(H.detach())
        assert np.array_equal(W.bits(Z.detach().numpy()), W.bits(W.step_np(S.numpy(), H.detach().numpy(), alpha)))


def test_propagate_saves_nothing_and_skips_a_backward_nobody_needs(karate, monkeypatch):
    eng, _, n = karate
    M = pkg("PGCN")
    H = torch.rand(n, 4)
    for K, alpha in ((0, 0.1), (2, 1.0), (2, float("inf")), (2, 1.0 - 1e-9)):        # (the last rounds to 1.0f)
        with pytest.raises(ValueError):
            eng.propagate(H, K, alpha)
        with pytest.raises(ValueError):
            eng.propagate_backward(H, K, alpha)
    out = M.PPropagate.apply(eng, H.clone().requires_grad_(True), 3, 0.1)
    assert tuple(out.grad_fn.saved_tensors) == ()
    calls = []
    monkeypatch.setattr(type(eng), "propagate_backward", lambda self, *a: calls.append(a) or torch.zeros(n, 4))
    joined = []
    monkeypatch.setattr(type(eng), "join_wgrad", lambda self: joined.append(1))
    w = torch.ones(4, requires_grad=True)
    (M.PPropagate.apply(eng, H, 3, 0.1) * w).sum().backward()             # H needs no gradient: the node is not even entered
    assert calls == [] and w.grad is not None
    Hg = H.clone().requires_grad_(True)
    M.PPropagate.apply(eng, Hg, 3, 0.1).sum().backward()
    assert len(calls) == 1 and calls[0][1:] == (3, 0.1) and joined == [1]       # join_wgrad at the end, as PSpMM.backward
    mod = M.Propagate(eng, 3)
    assert mod.alpha == 0.1 and list(mod.parameters()) == [] and list(mod.buffers()) == [] and mod.state_dict() == {}
    a = mod.train()(H)
    assert torch.equal(a, mod.eval()(H))
    for bad in (dict(K=0), dict(K=1.5), dict(K=True), dict(K=2, alpha=1.0), dict(K=2, alpha=-0.1), dict(K=2, alpha=float("nan"))):
        with pytest.raises(ValueError):
            M.Propagate(eng, **bad)


def test_an_engine_that_never_propagates_holds_nothing_new():
    eng, _, n = _karate_engine()
    held = set(vars(eng))
    H = torch.rand(n, 6)
    eng.backward(eng.forward(H))
    assert set(vars(eng)) == held and eng._max is None and eng._buf == {}
    assert not [k for k in held if "ppr" in k or "propag" in k]
    eng.propagate_backward(eng.propagate(H, 10, 0.1), 10, 0.1)
    assert set(vars(eng)) == held and eng._max is None                  # and one that does keeps nothing either


def test_scratch_does_not_grow_with_the_number_of_steps(karate, monkeypatch):
    """Besides the result at most two n_local x f matrices, whatever K is."""
    eng, _, n = karate
    made = []
    empty = torch.empty

    def counted(*a, **k):
        t = empty(*a, **k)
        if tuple(t.shape) == (n, 5):
            made.append(t)
        return t

    E = pkg("engine")
    H = torch.rand(n, 5)
    monkeypatch.setattr(E.torch, "empty", counted)
    for K in (1, 2, 10):
        for fn, most in ((eng.propagate, 2), (eng.propagate_backward, 3)):
            made.clear()
            fn(H, K, 0.1)
            assert len(made) <= most, (K, fn.__name__, len(made))


@pytest.mark.parametrize("P,pv", [(2, "karate.mtx.2.rp"), (3, "karate.mtx.3.hp")])
def test_ranks_over_gloo_against_one_rank(karate, P, pv):
    _, Ad, n = karate
    paths = {"A": gpath("karate.mtx"), "one": gpath("karate.mtx.1.rp"), "parts": gpath(pv)}
    cases = [(K, alpha, 7) for K in (1, 3, 10) for alpha in (0.0, 0.1, 0.5)]
    one = W.check_engine(W.spawn_engine(1, paths, False, cases=cases, normalize="sym", pv="one"), Ad, cases, "karate")
    res = W.spawn_engine(P, paths, False, cases=cases, normalize="sym", pv="parts")
    assert all(r["hip"] == "OracleKernels" for r in res) and sum(r["cases"][0]["fwd"]["send_volume"] for r in res) > 0
    W.check_same(one, W.check_engine(res, Ad, cases, "karate"), cases, "karate P=%d against one rank" % P)


# ---- the whole model ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("propagate")))


@pytest.mark.parametrize("P", [1, 2])
def test_model_gradients_against_the_double_model(dataset, P):
    paths, data = dataset
    configs = W.model_configs()
    res = W.spawn_model(P, paths, False, configs, data)
    assert W.check_models(data, configs, res) > 0
    if P == 2:                              # dense layers exchange nothing but the K propagation steps, forward and backward
        for rank in res:
            dense, gcn = rank[0]["stats"], rank[1]["stats"]
            assert dense["send_nmsg"] == W.EPOCHS * 2 * configs[0]["K"] * (P - 1) and dense["send_volume"] > 0, dense
            assert gcn["send_nmsg"] > W.EPOCHS * 2 * configs[1]["K"] * (P - 1), gcn


# ---- PGCN(aggregate=False) ----------------------------------------------------------------------------------------------------------

def test_a_dense_layer_is_the_torch_expression():
    M = pkg("PGCN")

    class NoEngine:                           # any use of the engine by a layer that does not aggregate fails
        def __getattr__(self, name):
            raise AssertionError("a dense layer touched the engine: %s" % name)

    torch.manual_seed(3)
    H = torch.randn(50, 6)
    for kw, expr in ((dict(), lambda m, h: torch.relu(h @ m.linear.weight.t())),
                     (dict(relu=False), lambda m, h: h @ m.linear.weight.t()),
                     (dict(bias=True), lambda m, h: torch.relu(h @ m.linear.weight.t() + m.bias)),
                     (dict(relu=False, bias=True), lambda m, h: h @ m.linear.weight.t() + m.bias)):
        dense, usual = M.PGCN(NoEngine(), 6, 4, aggregate=False, **kw), M.PGCN(None, 6, 4, **kw)
        assert sorted(dense.state_dict()) == sorted(usual.state_dict()) and dense.aggregate is False and usual.aggregate is True
        if "bias" in kw:
            with torch.no_grad():
                dense.bias.copy_(torch.randn(4))
        dense.eval()
        got, want = dense(H), expr(dense, H)
        assert rel_err(got.detach().numpy(), want.detach().numpy()) <= 1e-6, kw
    for extra in (dict(norm="batch"), dict(norm="node"), dict(root_weight=False, bias=True, norm="node")):
        assert sorted(M.PGCN(None, 6, 6, aggregate=False, **extra).state_dict()) == sorted(M.PGCN(None, 6, 6, **extra).state_dict())
    with pytest.raises(ValueError, match="aggregate=False"):
        M.PGCN(None, 6, 4, aggregate=False, aggr="max")
    with pytest.raises(ValueError, match="aggregate=False"):
        M.PGCN(None, 6, 4, aggregate=False, root_weight=True)


# ---- the defaults are today's -------------------------------------------------------------------------------------------------------

def test_defaults_are_todays():
    CK, M = pkg("checkpoint"), pkg("PGCN")
    today = {"widths": [24, 32, 7], "layers": 2, "task": "single", "norm": "none", "root_weight": False, "bias": False, "residual": False,
             "heads": None, "out_heads": None, "dropout": 0.0, "dropout_seed": 0}
    assert CK.architecture([24, 32, 7], "single") == today == CK.architecture([24, 32, 7], "single", propagate=None, dense_layers=None)
    assert CK.architecture([24, 32, 7], "single", dense_layers=False) == today
    assert CK.architecture([24, 32, 7], "single", propagate=(10, 0.1)) == dict(today, propagate=[10, 0.1])
    assert CK.architecture([24, 32, 7], "single", dense_layers=True) == dict(today, dense_layers=True)
    assert CK.ARCH_FIELDS[-2:] == ("propagate", "dense_layers") and M.AGGRS == ("sum", "max") and M.PPR_ALPHA == 0.1
    assert M._architecture(24, 7, 2, 32, None, False, 0.0, 0, None, None, None, None) == today
    assert M._architecture(24, 7, 2, 32, None, False, 0.0, 0, None, None, None, None, None, 3, None, True) == \
        dict(today, propagate=[3, 0.1], dense_layers=True)


class _Inline:
    seen = []

    def __init__(self, target, args, kwargs=None):
        _Inline.seen.append((args, kwargs))
        self.exitcode = 0

    def start(self):
        pass

    def join(self):
        pass


def test_cli_takes_the_three_flags_and_refuses_bad_values(monkeypatch, capsys, tmp_path):
    M = pkg("PGCN")
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.setenv(k, os.environ[k]) if k in os.environ else monkeypatch.delenv(k, raising=False)
    for name in ("path_A", "path_partvec"):
        monkeypatch.setattr(M, name, getattr(M, name, None), raising=False)
    monkeypatch.setattr(M.mp, "Process", _Inline)
    monkeypatch.setattr(M.mp, "set_start_method", lambda *a, **k: None)
    base = ["-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"), "-b", "gloo", "-s", "1", "-l", "2", "-f", "16"]
    files = []
    for k in ("features", "labels", "split"):
        open(str(tmp_path / k), "wb").close()
        files += ["--" + k, str(tmp_path / k)]
    _Inline.seen = []
    M.main(base)
    M.main(base + files)
    M.main(base + files + ["--propagate", "10"])
    M.main(base + files + ["--propagate", "3", "--ppr-alpha", "0.25", "--dense-layers", "--bias"])
    M.main(base + files + ["--dense-layers"])
    assert [kw for _, kw in _Inline.seen] == [None, None, {"propagate": 10}, {"propagate": 3, "ppr_alpha": 0.25, "dense_layers": True},
                                              {"dense_layers": True}]
    # without the new flags: the argument tuples of today (9 positional arguments; with the files 19)
    assert _Inline.seen[0][0] == (0, 1, M.run, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo", None)
    assert _Inline.seen[1][0] == _Inline.seen[0][0] + (0.0, 0) + tuple(str(tmp_path / k) for k in ("features", "labels", "split")) + (None,) * 5
    assert _Inline.seen[2][0] == _Inline.seen[1][0]                       # the new options never ride in the tuple
    three = "--features, --labels and --split go together"
    for bad, text in ((files + ["--propagate", "0"], "--propagate takes an integer >= 1"),
                      (files + ["--propagate", "x"], "--propagate takes an integer >= 1"),
                      (files + ["--propagate", "2", "--ppr-alpha", "1"], "--ppr-alpha takes a number >= 0 and < 1"),
                      (files + ["--propagate", "2", "--ppr-alpha", "-0.1"], "--ppr-alpha takes a number >= 0 and < 1"),
                      (files + ["--propagate", "2", "--ppr-alpha", "nan"], "--ppr-alpha takes a number >= 0 and < 1"),
                      (files + ["--ppr-alpha", "0.2"], "--ppr-alpha needs --propagate"),
                      (files + ["--dense-layers", "--aggr", "max"], "--dense-layers does not go with --aggr max"),
                      (files + ["--dense-layers", "--root-weight"], "--dense-layers does not go with --root-weight"),
                      (["--propagate", "2"], three), (["--propagate", "2", "--ppr-alpha", "0.2"], three), (["--dense-layers"], three)):
        with pytest.raises(SystemExit) as e:
            M.main(base + bad)
        out = capsys.readouterr().out
        assert e.value.code == 2 and text in out and len(out.strip().splitlines()) == 1, (bad, out)
    with pytest.raises(SystemExit):
        M.main(base + ["--dense-layers"])
    out = capsys.readouterr().out                                         # the message names the flags and keeps what earlier tests pin
    assert "--aggr, --propagate, --ppr-alpha, --dense-layers," in out and "--save, --load, --predict, --proba" in out and \
        "--norm, --residual, --root-weight, --bias need them" in out and "got --dense-layers" in out
    # init_process hands them to run() by name, only when given
    got = []
    monkeypatch.setattr(M.dist, "init_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "destroy_process_group", lambda *a, **k: None)
    M.init_process(0, 1, lambda *a, **k: got.append((len(a), k)), 2, 16, "A", "p", "gloo", propagate=4, ppr_alpha=0.3, dense_layers=True)
    M.init_process(0, 1, lambda *a, **k: got.append((len(a), k)), 2, 16, "A", "p", "gloo", propagate=4)
    M.init_process(0, 1, lambda *a, **k: got.append((len(a), k)), 2, 16, "A", "p", "gloo")
    assert got == [(7, {"propagate": 4, "ppr_alpha": 0.3, "dense_layers": True}), (7, {"propagate": 4}), (7, {})]


# ---- run(propagate=...), checkpoints, predictions -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trained(tmp_path_factory, dataset):
    d = str(tmp_path_factory.mktemp("propagate_cli"))
    paths, data = dataset
    three = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=W.HIDDEN, lr=0.02)
    appnp = dict(three, propagate=4, ppr_alpha=0.2, dense_layers=True, dropout=0.5, dropout_seed=3)
    whole, leg, pred = d + "/whole.pt", d + "/leg.pt", d + "/pred"
    jobs = [dict(kw=dict(appnp, epochs=8, save=whole, predict=pred), logits=True),          # 0: the uninterrupted run
            dict(kw=dict(appnp, epochs=5, save=leg)),                                          # 1: its first leg ...
            dict(kw=dict(appnp, epochs=3, load=leg, save=d + "/resumed.pt")),                  # 2: ... and the rest
            dict(kw=dict(appnp, epochs=0, load=whole, propagate=5)),                           # 3: another K
            dict(kw=dict(appnp, epochs=0, load=whole, ppr_alpha=0.1)),                         # 4: another alpha
            dict(kw=dict({k: v for k, v in appnp.items() if k != "dense_layers"}, epochs=0, load=whole)),      # 5: another layer kind
            dict(kw=dict({k: v for k, v in appnp.items() if k not in ("propagate", "ppr_alpha")}, epochs=0, load=whole)),   # 6: no propagation
            dict(kw=dict(three, epochs=1, save=d + "/plain.pt")),                              # 7: a checkpoint of today
            dict(kw=dict(three, epochs=0, load=d + "/plain.pt")),                              # 8
            dict(kw=dict(three, epochs=0, load=d + "/plain.pt", propagate=2)),                 # 9
            dict(kw=dict(three, epochs=1, propagate=0)), dict(kw=dict(three, epochs=1, ppr_alpha=0.1)),          # 10, 11
            dict(kw=dict(three, epochs=1, propagate=2, ppr_alpha=1.0)), dict(kw=dict(propagate=2)),               # 12, 13
            dict(kw=dict(three, epochs=1, dense_layers=True, aggr="max")), dict(kw=dict(dense_layers=True))]      # 14, 15
    for j in jobs:
        j["nlayers"] = 2
    return PW.spawn_jobs(2, paths, False, "PGCN", jobs), d, data


def test_run_trains_resumes_bit_for_bit_and_predicts_through_the_propagation(trained):
    res, d, data = trained
    for rank in res:
        whole, leg, rest = rank[0], rank[1], rank[2]
        assert all("error" not in r for r in (whole, leg, rest)), [r.get("error") for r in (whole, leg, rest)]
        losses = [h["losses"]["train"] for h in whole["history"]]
        assert len(losses) == 8 and np.isfinite(losses).all() and losses[-1] < losses[0], losses
        assert [h["epoch"] for h in rest["history"]] == list(range(8))
        assert PW.same_state(whole["history"], rest["history"]) == [] and PW.same_state(whole["state"], rest["state"]) == []
        assert sorted(whole["state"]) == ["0.linear.weight", "1.linear.weight"]              # the Propagate module owns nothing
    a, b = torch.load(d + "/whole.pt", weights_only=True), torch.load(d + "/resumed.pt", weights_only=True)
    assert a["arch"]["propagate"] == [4, 0.2] and a["arch"]["dense_layers"] is True
    assert PW.same_state({k: a[k] for k in ("model", "optimizer", "epochs", "dropout_step", "best")},
                         {k: b[k] for k in ("model", "optimizer", "epochs", "dropout_step", "best")}) == []
    plain = torch.load(d + "/plain.pt", weights_only=True)["arch"]
    assert "propagate" not in plain and "dense_layers" not in plain
    # the prediction files hold the arg-max of the PROPAGATED logits: they differ from the MLP's own where the propagation decides
    logits = W.rows([dict(own=r[0]["own"], v=r[0]["logits"]) for r in res], lambda r: r["v"], W.N)
    pred = np.load(d + "/pred.pred.npy")
    assert pred.shape == (W.N,) and np.array_equal(pred, logits.argmax(1))
    w = a["best"]["model"] if a["best"] else a["model"]
    h = torch.relu(torch.from_numpy(data["X"]).double() @ w["0.linear.weight"].double().t()) @ w["1.linear.weight"].double().t()
    Ad = W.GG.dense_adjacency(data).numpy()
    want = W.propagate64(Ad, h.numpy(), 4, 0.2)
    # (K + 1) TOL for the propagation and one TOL, the suite's bar for a model's logits, for the two layers in front of it
    assert rel_err(logits, want) <= (4 + 2) * W.TOL and (h.numpy().argmax(1) != want.argmax(1)).any()
    near = np.sort(want, 1)[:, -1] - np.sort(want, 1)[:, -2] < PW.NEAR * np.abs(want).max()
    assert np.array_equal(pred[~near], want.argmax(1)[~near])


def test_checkpoints_name_the_field_and_todays_still_load(trained):
    res, _, _ = trained
    for rank in res:                                            # every rank raises alike
        for k, field in ((3, "propagate"), (4, "propagate"), (5, "dense_layers"), (6, "propagate"), (9, "propagate")):
            assert rank[k].get("error", ("", ""))[0] == "ValueError" and field + " differs" in rank[k]["error"][1], (k, rank[k].get("error"))
        assert "error" not in rank[7] and "error" not in rank[8]
        assert "propagate takes an integer >= 1" in rank[10]["error"][1] and "ppr_alpha needs propagate" in rank[11]["error"][1]
        assert "ppr_alpha takes" in rank[12]["error"][1] and "need features, labels and split" in rank[13]["error"][1]
        assert "dense_layers does not go with" in rank[14]["error"][1] and "need features, labels and split" in rank[15]["error"][1]


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_without_a_device():
    L = pkg("_lib").lib()
    one, two = 16, 4096       # non-null addresses that are never dereferenced: every refusal below happens before any HIP call
    step = lambda **k: L.pgcn_ppr_step_f32(k.get("S", one), k.get("lds", 8), k.get("H", two), k.get("ldh", 8), k.get("n", 4), k.get("f", 8),
                                           k.get("alpha", 0.1), k.get("Y", 3 * two), k.get("ldy", 8), None)
    back = lambda **k: L.pgcn_ppr_step_backward_f32(k.get("G", one), k.get("ldg", 8), k.get("T", two), k.get("ldt", 8), k.get("D", 2 * two),
                                                    k.get("ldd", 8), k.get("n", 4), k.get("f", 8), k.get("alpha", 0.1), k.get("last", 0),
                                                    k.get("Gout", 3 * two), k.get("ldgo", 8), k.get("Dout", 4 * two), k.get("lddo", 8), None)
    alphas = [dict(alpha=a) for a in (1.0, -0.1, float("nan"), float("inf"), 1.5)]
    for call, name, bad in ((step, b"pgcn_ppr_step_f32", [dict(S=None), dict(H=None), dict(Y=None), dict(n=-1), dict(f=0), dict(lds=7), dict(ldh=7),
                                                         dict(ldy=7), dict(Y=one, ldy=12)] + alphas),
                            (back, b"pgcn_ppr_step_backward_f32", [dict(G=None), dict(T=None), dict(Dout=None), dict(Gout=None), dict(n=-1),
                                                                   dict(f=0), dict(ldg=7), dict(ldt=7), dict(ldd=7), dict(ldgo=7), dict(lddo=7),
                                                                   dict(Gout=two, ldgo=12), dict(Dout=2 * two, lddo=12),
                                                                   dict(last=1, Dout=None)] + alphas)):
        for k in bad:
            assert call(**k) == -1 and name in L.pgcn_last_error(), (name, k)
        assert call(f=1025, lds=1025, ldh=1025, ldy=1025, ldg=1025, ldt=1025, ldd=1025, ldgo=1025, lddo=1025) == pkg("_lib").PGCN_EUNSUPPORTED
        assert call(n=0) == 0                         # nothing to do: no launch, no device
    assert back(n=0, last=1, Gout=None) == 0 and back(n=0, D=None) == 0          # Gout is optional at the last step, D at the first
