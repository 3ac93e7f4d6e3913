"""Generalised-PageRank propagation with learned hop weights (GPR-GNN) on the CPU: the definition in numpy fp32 and float64 (it is APPNP
under the PPR coefficients, the backward is the adjoint, dgamma matches a finite difference), the composed step functions bit for bit,
the engine's gpr / gpr_backward on karate against float64 (one rank and over gloo with the golden part vectors), the whole model against
a double model with gamma's gradient, run(gpr=...) / --gpr / --gpr-init / --gpr-alpha, checkpoints, and the C entry points' argument
checks (no device).

tests/_gpr_workers.py has the definition and the bounds."""
import os

import numpy as np
import pytest
import torch

from conftest import gpath, pkg, rel_err

import _fused_adam_workers as FA
import _predict_workers as PW
import _gpr_workers as R
import _propagate_workers as W


# ---- the definition -----------------------------------------------------------------------------------------------------------------

def _karate_dense():
    A = pkg("ingest").mmread(gpath("karate.mtx")).tocoo()
    return A, W.sym_normalised(A)


@pytest.mark.parametrize("K,alpha", [(1, 0.1), (3, 0.5), (10, 0.1), (10, 0.0)])
def test_definition_is_appnp_under_the_ppr_coefficients(K, alpha):
    _, Ad = _karate_dense()
    rng = np.random.default_rng(K)
    H = rng.standard_normal((Ad.shape[0], 5))
    a, b = (float(x) for x in W.coefficients(alpha))
    gamma = [a * b ** k for k in range(K)] + [b ** K]                    # exact in the coefficients propagate64 uses
    want = W.propagate64(Ad, H, K, alpha)
    assert np.abs(R.gpr64(Ad, H, gamma) - want).max() <= 1e-12 * np.abs(want).max()
    # and the "ppr" initialisation is those weights rounded once from Python doubles
    g = R.ppr_gamma(K, alpha)
    assert g.dtype == np.float32 and g[K] == np.float32((1.0 - alpha) ** K) and g[0] == np.float32(alpha)
    assert torch.equal(pkg("PGCN").gpr_initial(K, "ppr", alpha), torch.from_numpy(g))
    assert torch.equal(pkg("PGCN").gpr_initial(K, "uniform"), torch.full((K + 1,), 1.0 / (K + 1), dtype=torch.float64).float())


def test_backward64_is_the_adjoint_and_dgamma_a_finite_difference():
    _, Ad = _karate_dense()
    rng = np.random.default_rng(1)
    n, K = Ad.shape[0], 4
    H, G = rng.standard_normal((n, 6)), rng.standard_normal((n, 6))
    gamma = rng.uniform(-1, 1, K + 1)
    D, dg, _ = R.gpr_backward64(Ad, G, H, gamma)
    lhs, rhs = float((R.gpr64(Ad, H, gamma) * G).sum()), float((H * D).sum())
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(H) * np.linalg.norm(G)
    for k in range(K + 1):
        e = np.zeros(K + 1)
        e[k] = 1e-3
        fd = float(((R.gpr64(Ad, H, gamma + e) - R.gpr64(Ad, H, gamma - e)) * G).sum()) / 2e-3       # the map is linear in gamma: exact
        assert abs(fd - dg[k]) <= 1e-9 * max(1.0, abs(dg[k])), (k, fd, dg[k])


def test_composed_steps_are_the_fp32_formula_bit_for_bit():
    E = pkg("engine")
    rng = np.random.default_rng(2)
    n, f = 37, 7
    X, Y, H = (rng.standard_normal((n, f)).astype(np.float32) * 3 for _ in range(3))
    X[3, 2] = np.float32(-0.0)
    g = np.array([0.3, -0.7, 0.0], np.float32)
    t = torch.from_numpy
    for k in range(3):
        for Yin in (None, Y):
            want = R.step_np(X, Yin, g[k])
            got = E.gpr_step_composed(t(X), None if Yin is None else t(Yin), t(g), k)
            assert np.array_equal(R.bits(got.numpy()), R.bits(want)), (k, Yin is None)
            Yc = t(Y.copy())
            assert E.gpr_step_composed(t(X), None if Yin is None else Yc, t(g), k, out=Yc) is Yc and np.array_equal(R.bits(Yc.numpy()), R.bits(want))
            dots = []
            (d,) = E.gpr_step_backward_composed(t(X), t(H), None if Yin is None else t(Yin), t(g), k, dots)
            assert np.array_equal(R.bits(d.numpy()), R.bits(want)) and dots[0].dtype is torch.float64
            ref = float(np.dot(X.astype(np.float64).reshape(-1), H.astype(np.float64).reshape(-1)))
            assert abs(float(dots[0]) - ref) <= R.dot_bound(ref, X, H)
            assert E.gpr_step_backward_composed(t(X), t(H), None, t(g), k, dots, need_d=False) == (None,) and len(dots) == 2
    assert np.signbit(E.gpr_step_composed(t(X), None, t(g), 0).numpy()[3, 2])         # an absent Yin is not added: -0.0 survives


# ---- the engine on karate -----------------------------------------------------------------------------------------------------------

def _karate_engine():
    from oracle_kernels import OracleKernels
    P, E = pkg("partition"), pkg("engine")
    A, Ad = _karate_dense()
    n = A.shape[0]
    part = P.build_partition(torch.from_numpy(A.row.astype(np.int64)), torch.from_numpy(A.col.astype(np.int64)),
                             torch.from_numpy(A.data.astype(np.float32)), n, torch.zeros(n, dtype=torch.int64), 0, 1, normalize="sym")
    return E.AggregationEngine(part, OracleKernels(), torch.device("cpu")), Ad, n


@pytest.fixture(scope="module")
def karate():
    return _karate_engine()


@pytest.mark.parametrize("K,C", R.KARATE_CASES)
def test_gpr_on_karate_against_float64(karate, K, C):
    eng, Ad, n = karate
    own = eng.part.owned.numpy()
    Hg, Gg, g = R.seeded_case(n, K, C)
    H = torch.from_numpy(Hg[own]).requires_grad_(True)
    mod = pkg("PGCN").Gpr(eng, K)
    with torch.no_grad():
        mod.gamma.copy_(torch.from_numpy(g))
    OUT = mod(H)
    assert {tuple(s.shape) for s in OUT.grad_fn.saved_tensors} == {(n, C), (K + 1,)}          # H and gamma, nothing else
    OUT.backward(torch.from_numpy(Gg[own]))
    D64, dg64, norms = R.gpr_backward64(Ad, Gg, Hg, g)
    bound = (K + 1) * R.TOL
    eo, ed = rel_err(OUT.detach().numpy(), R.gpr64(Ad, Hg, g)[own]), rel_err(H.grad.numpy(), D64[own])
    print("K=%d C=%d: forward %.3g, dH %.3g (bound %.3g)" % (K, C, eo, ed, bound))
    assert eo <= bound and ed <= bound
    hn = np.linalg.norm(Hg.astype(np.float64))
    for k in range(K + 1):
        assert abs(float(mod.gamma.grad[k]) - dg64[k]) <= (k + 1) * R.TOL * norms[k] * hn, k
    if K == 1:              # the engine's steps ARE the formula around its own aggregation: by hand, bit for bit
        S = eng.forward(H.detach())
        want = R.step_np(S.numpy(), R.step_np(H.detach().numpy(), None, g[0]), g[1])
        assert np.array_equal(R.bits(OUT.detach().numpy()), R.bits(want))


def test_module_parameter_scratch_and_the_skipped_chain(karate, monkeypatch):
    eng, _, n = karate
    M, E = pkg("PGCN"), pkg("engine")
    mod = M.Gpr(eng, 3, init="uniform")
    assert [k for k, _ in mod.named_parameters()] == ["gamma"] and mod.gamma.dtype is torch.float32 and tuple(mod.gamma.shape) == (4,)
    assert "K=3" in repr(mod) and "uniform" in repr(mod) and "ppr(alpha=0.25)" in repr(M.Gpr(eng, 2, alpha=0.25))
    assert "per-parameter groups" in M.Gpr.__doc__
    for bad in (dict(K=0), dict(K=1.5), dict(K=True), dict(K=2, alpha=1.5), dict(K=2, alpha=-0.1), dict(K=2, alpha=float("nan")),
                dict(K=2, init="ones")):
        with pytest.raises(ValueError):
            M.Gpr(eng, **bad)
    H = torch.rand(n, 5)
    assert torch.equal(mod.train()(H), mod.eval()(H))
    for bad in (torch.ones(1), torch.ones(3, dtype=torch.float64), [0.5, 0.5]):
        with pytest.raises(ValueError):
            eng.gpr(H, bad)
    # H needs no gradient: the D chain is skipped, dgamma is still formed; join_wgrad at the end, as PSpMM.backward
    calls, joined = [], []
    real = type(eng).gpr_backward
    monkeypatch.setattr(type(eng), "gpr_backward", lambda self, *a: calls.append(a[3]) or real(self, *a))
    monkeypatch.setattr(type(eng), "join_wgrad", lambda self: joined.append(1), raising=False)
    mod(H).sum().backward()
    assert calls == [False] and joined == [1] and mod.gamma.grad is not None and float(mod.gamma.grad.abs().sum()) > 0
    # two ping-pong buffers and the accumulator, whatever K is; nothing new kept on the engine
    made, empty, held = [], torch.empty, set(vars(eng))

    def counted(*a, **k):
        t = empty(*a, **k)
        if tuple(t.shape) == (n, 5):
            made.append(t)
        return t

    monkeypatch.setattr(E.torch, "empty", counted)
    for K in (1, 2, 10):
        g = torch.full((K + 1,), 0.1)
        made.clear()
        eng.gpr(H, g)
        assert len(made) <= 2, (K, len(made))
        made.clear()
        eng.gpr_backward(H, H, g, True)
        assert len(made) <= 2, (K, len(made))
    assert set(vars(eng)) == held


@pytest.mark.parametrize("P,pv", [(2, "karate.mtx.2.rp"), (3, "karate.mtx.3.hp")])
def test_ranks_over_gloo_against_one_rank(P, pv):
    _, Ad = _karate_dense()
    paths = {"A": gpath("karate.mtx"), "one": gpath("karate.mtx.1.rp"), "parts": gpath(pv)}
    cases = R.KARATE_CASES
    one = R.check_engine(R.spawn_engine(1, paths, False, cases=cases, normalize="sym", pv="one"), Ad, cases, "karate")
    res = R.spawn_engine(P, paths, False, cases=cases, normalize="sym", pv="parts")
    assert all(r["hip"] == "OracleKernels" for r in res) and sum(r["cases"][0]["fwd"]["send_volume"] for r in res) > 0
    R.check_same(one, R.check_engine(res, Ad, cases, "karate"), Ad, cases, "karate P=%d against one rank" % P)


# ---- the whole model ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return R.make_dataset(str(tmp_path_factory.mktemp("gpr")))


@pytest.mark.parametrize("P", [1, 2])
def test_model_gradients_against_the_double_model(dataset, P):
    paths, data = dataset
    configs = R.model_configs()
    res = R.spawn_model(P, paths, False, configs, data)
    assert R.check_models(data, configs, res) > 0


# ---- the defaults, the command line --------------------------------------------------------------------------------------------------

def test_architecture_record_carries_gpr_only_when_given():
    CK, M = pkg("checkpoint"), pkg("PGCN")
    today = CK.architecture([24, 32, 7], "single")
    assert "gpr" not in today and "gpr" in CK.ARCH_FIELDS and CK.architecture([24, 32, 7], "single", gpr=None) == today
    assert CK.architecture([24, 32, 7], "single", gpr=(10, "ppr", 0.1)) == dict(today, gpr=[10, "ppr", 0.1])
    assert M._architecture(24, 7, 2, 32, None, False, 0.0, 0, None, None, None, None) == today
    assert M._architecture(24, 7, 2, 32, None, False, 0.0, 0, None, None, None, None, gpr=3) == dict(today, gpr=[3, "ppr", 0.1])
    assert M._architecture(24, 7, 2, 32, None, False, 0.0, 0, None, None, None, None, gpr=3, gpr_init="uniform", gpr_alpha=0.5) == \
        dict(today, gpr=[3, "uniform", 0.5])
    assert M.GPR_INITS == ("ppr", "uniform") and M.GPR_ALPHA == 0.1
    ck = {"launcher": "PGCN", "arch": dict(today, gpr=[3, "ppr", 0.1]), "optimizer": {"kind": "torch"}}
    CK.check(ck, "PGCN", dict(today, gpr=[3, "ppr", 0.1]), "torch")
    for other in (today, dict(today, gpr=[4, "ppr", 0.1]), dict(today, gpr=[3, "uniform", 0.1])):
        with pytest.raises(ValueError, match="gpr differs"):
            CK.check(ck, "PGCN", other, "torch")


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
    M.main(base + files)
    M.main(base + files + ["--gpr", "10"])
    M.main(base + files + ["--gpr", "3", "--gpr-init", "uniform", "--dense-layers"])
    M.main(base + files + ["--gpr", "3", "--gpr-alpha", "1", "--gpr-init", "ppr"])
    assert [kw for _, kw in _Inline.seen] == [None, {"gpr": 10}, {"gpr": 3, "gpr_init": "uniform", "dense_layers": True},
                                              {"gpr": 3, "gpr_alpha": 1.0, "gpr_init": "ppr"}]
    assert _Inline.seen[1][0] == _Inline.seen[0][0]                       # the new options never ride in the tuple
    three = "--features, --labels and --split go together"
    for bad, text in ((files + ["--gpr", "0"], "--gpr takes an integer >= 1"), (files + ["--gpr", "x"], "--gpr takes an integer >= 1"),
                      (files + ["--gpr", "2", "--gpr-alpha", "1.5"], "--gpr-alpha takes a number >= 0 and <= 1"),
                      (files + ["--gpr", "2", "--gpr-alpha", "-0.1"], "--gpr-alpha takes a number >= 0 and <= 1"),
                      (files + ["--gpr", "2", "--gpr-alpha", "nan"], "--gpr-alpha takes a number >= 0 and <= 1"),
                      (files + ["--gpr", "2", "--gpr-init", "ones"], "--gpr-init takes ppr|uniform"),
                      (files + ["--gpr-alpha", "0.2"], "--gpr-init and --gpr-alpha need --gpr"),
                      (files + ["--gpr-init", "uniform"], "--gpr-init and --gpr-alpha need --gpr"),
                      (files + ["--gpr", "2", "--propagate", "2"], "--gpr does not go with --propagate"),
                      (["--gpr", "2"], three), (["--gpr", "2", "--gpr-init", "uniform"], three)):
        with pytest.raises(SystemExit) as e:
            M.main(base + bad)
        out = capsys.readouterr().out
        assert e.value.code == 2 and text in out and len(out.strip().splitlines()) == 1, (bad, out)
    with pytest.raises(SystemExit):
        M.main(base + ["--gpr", "2"])
    assert "--softmax-aggr, --gpr, --gpr-init, --gpr-alpha," in capsys.readouterr().out
    got = []
    monkeypatch.setattr(M.dist, "init_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "destroy_process_group", lambda *a, **k: None)
    M.init_process(0, 1, lambda *a, **k: got.append((len(a), k)), 2, 16, "A", "p", "gloo", gpr=4, gpr_init="uniform", gpr_alpha=0.3)
    M.init_process(0, 1, lambda *a, **k: got.append((len(a), k)), 2, 16, "A", "p", "gloo", gpr=4)
    M.init_process(0, 1, lambda *a, **k: got.append((len(a), k)), 2, 16, "A", "p", "gloo")
    assert got == [(7, {"gpr": 4, "gpr_init": "uniform", "gpr_alpha": 0.3}), (7, {"gpr": 4}), (7, {})]


def test_run_refuses_by_message():
    M = pkg("PGCN")
    base = (0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo")
    three = dict(features="f.npy", labels="l.npy", split="s.npy")
    for kw, text in ((dict(three, gpr=2, propagate=2), "gpr does not go with propagate"), (dict(three, gpr_init="uniform"), "gpr_init and gpr_alpha need gpr"),
                     (dict(three, gpr_alpha=0.2), "gpr_init and gpr_alpha need gpr"), (dict(gpr=2), "gpr needs features, labels and split"),
                     (dict(three, gpr=0), "gpr takes an integer >= 1"), (dict(three, gpr=True), "gpr takes an integer >= 1"),
                     (dict(three, gpr=2, gpr_alpha=1.5), "gpr_alpha takes a number with 0 <= alpha <= 1"),
                     (dict(three, gpr=2, gpr_alpha=float("nan")), "gpr_alpha takes a number with 0 <= alpha <= 1"),
                     (dict(three, gpr=2, gpr_init="ones"), "gpr_init takes ppr | uniform")):
        with pytest.raises(ValueError, match=text.replace("|", r"\|")):
            M.run(*base, **kw)


# ---- run(gpr=...), checkpoints, predictions, the two optimisers -----------------------------------------------------------------------

LR = 0.02


@pytest.fixture(scope="module")
def trained(tmp_path_factory, dataset):
    d = str(tmp_path_factory.mktemp("gpr_cli"))
    paths, data = dataset
    three = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=R.HIDDEN, lr=LR)
    gpr = dict(three, gpr=4, gpr_alpha=0.2, dense_layers=True, dropout=0.5, dropout_seed=3)
    whole, leg, pred = d + "/whole.pt", d + "/leg.pt", d + "/pred"
    jobs = [dict(kw=dict(gpr, epochs=8, save=whole, predict=pred), logits=True),           # 0: the uninterrupted run
            dict(kw=dict(gpr, epochs=5, save=leg)),                                           # 1: its first leg ...
            dict(kw=dict(gpr, epochs=3, load=leg, save=d + "/resumed.pt")),                   # 2: ... and the rest
            dict(kw=dict(gpr, epochs=0, load=whole, gpr=5)),                                  # 3: another K
            dict(kw=dict(gpr, epochs=0, load=whole, gpr_init="uniform")),                     # 4: another initialisation
            dict(kw=dict({k: v for k, v in gpr.items() if k not in ("gpr", "gpr_alpha")}, epochs=0, load=whole)),      # 5: no gpr
            dict(kw=dict(three, epochs=1)),                                                   # 6: a run of today
            dict(kw=dict(three, epochs=3, gpr=10, dense_layers=True, optimizer="torch"), nlayers=R.NLAYERS),     # 7, 8: the two optimisers
            dict(kw=dict(three, epochs=3, gpr=10, dense_layers=True, optimizer="fused"), nlayers=R.NLAYERS)]
    for j in jobs:
        j.setdefault("nlayers", 2)
    return {P: PW.spawn_jobs(P, paths, False, "PGCN", jobs if P == 2 else jobs[7:]) for P in (1, 2)}, d, data


def test_run_trains_resumes_bit_for_bit_and_predicts(trained):
    res, d, data = trained
    for rank in res[2]:
        whole, leg, rest = rank[0], rank[1], rank[2]
        assert all("error" not in r for r in (whole, leg, rest)), [r.get("error") for r in (whole, leg, rest)]
        losses = [h["losses"]["train"] for h in whole["history"]]
        assert len(losses) == 8 and np.isfinite(losses).all() and losses[-1] < losses[0], losses
        assert PW.same_state(whole["history"], rest["history"]) == [] and PW.same_state(whole["state"], rest["state"]) == []
        assert sorted(whole["state"]) == ["0.linear.weight", "1.linear.weight", "2.gamma"]
        assert not np.array_equal(whole["state"]["2.gamma"], R.ppr_gamma(4, 0.2))              # gamma was trained ...
        assert np.array_equal(R.bits(whole["state"]["2.gamma"]), R.bits(res[2][0][0]["state"]["2.gamma"]))      # ... alike on every rank
        for k in (3, 4, 5):
            assert rank[k].get("error", ("", ""))[0] == "ValueError" and "gpr differs" in rank[k]["error"][1], (k, rank[k].get("error"))
    a, b = torch.load(d + "/whole.pt", weights_only=True), torch.load(d + "/resumed.pt", weights_only=True)
    assert a["arch"]["gpr"] == [4, "ppr", 0.2] and a["arch"]["dense_layers"] is True and "propagate" not in a["arch"]
    assert PW.same_state({k: a[k] for k in ("model", "optimizer", "epochs", "dropout_step", "best")},
                         {k: b[k] for k in ("model", "optimizer", "epochs", "dropout_step", "best")}) == []
    # the prediction files hold the arg-max of the logits propagated with the TRAINED gamma
    logits = R.rows([dict(own=r[0]["own"], v=r[0]["logits"]) for r in res[2]], lambda r: r["v"], R.N)
    pred = np.load(d + "/pred.pred.npy")
    assert pred.shape == (R.N,) and np.array_equal(pred, logits.argmax(1))
    w = a["best"]["model"] if a["best"] else a["model"]
    h = torch.relu(torch.from_numpy(data["X"]).double() @ w["0.linear.weight"].double().t()) @ w["1.linear.weight"].double().t()
    want = R.gpr64(W.GG.dense_adjacency(data).numpy(), h.numpy(), w["2.gamma"].double().numpy())
    scale = float(np.abs(w["2.gamma"].double().numpy()).sum())          # the trained weights no longer sum to 1: the bound scales with them
    assert rel_err(logits, want) <= (4 + 2) * R.TOL * max(1.0, scale)


def test_gamma_line_is_printed_only_with_gpr(trained):
    res, _, _ = trained
    lines = res[2][0][0]["stdout"].strip().splitlines()
    assert lines[-1].startswith("gamma ") and len(lines[-1].split()) == 1 + 5 and not any(l.startswith("gamma ") for l in lines[:-1])
    assert np.allclose([float(x) for x in lines[-1].split()[1:]], res[2][0][0]["state"]["2.gamma"], rtol=1e-5)
    assert "gamma " not in res[2][1][0]["stdout"] and "gamma " not in res[2][0][6]["stdout"]      # rank 1; a run without --gpr


def test_fused_and_torch_agree_on_gamma_after_three_steps(trained, dataset):
    """The bound of the fused-Adam tests between the two optimisers: twice the error of torch's own fp32 optimiser against float64
    plus one rounding (_fused_adam_workers.errors_and_bound); the float64 run is the double model with torch's Adam in double."""
    res, _, _ = trained
    _, data = dataset
    c = R.config(True, K=10)
    params = W.GG.initial_params(W.widths_of(c), c, PW.WEIGHT_SEED)
    params[R.GAMMA] = torch.from_numpy(R.ppr_gamma(10, 0.1))
    ref = R.train64(data, c, params, 3, LR)[R.GAMMA]
    for P in (1, 2):
        yard, fused = (res[P][0][j if P == 2 else j - 7] for j in (7, 8))
        assert "error" not in yard and "error" not in fused
        e, e_torch, bound = FA.errors_and_bound(fused["state"][R.GAMMA], yard["state"][R.GAMMA], ref)
        print("P=%d gamma after 3 steps: fused %.3g torch %.3g bound %.3g" % (P, e, e_torch, bound))
        assert e <= bound and np.abs(ref - R.ppr_gamma(10, 0.1)).max() > LR / 2      # and it has moved


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_without_a_device():
    _lib = pkg("_lib")
    L = _lib.lib()
    one, two = 16, 4096       # non-null addresses that are never dereferenced: every refusal below happens before any HIP call
    big = 1 << 20
    step = lambda **k: L.pgcn_gpr_step_f32(k.get("X", one), k.get("ldx", 8), k.get("Yin", two), k.get("ldyin", 8), k.get("gamma", 5 * two),
                                           k.get("k", 1), k.get("K", 3), k.get("n", 4), k.get("f", 8), k.get("Y", 3 * two), k.get("ldy", 8), None)
    back = lambda **k: L.pgcn_gpr_step_backward_f32(k.get("T", one), k.get("ldt", 8), k.get("H", two), k.get("ldh", 8), k.get("Din", 2 * two),
                                                    k.get("lddin", 8), k.get("gamma", 5 * two), k.get("k", 1), k.get("K", 3), k.get("n", 4),
                                                    k.get("f", 8), k.get("Dout", 4 * two), k.get("lddo", 8), k.get("ws", 6 * two),
                                                    k.get("ws_bytes", big), None)
    fin = lambda **k: L.pgcn_gpr_dot_finish_f32(k.get("ws", 6 * two), k.get("ws_bytes", big), k.get("n", 4), k.get("f", 8), k.get("K", 3),
                                                k.get("dgamma", two), None)
    ks = [dict(k=-1), dict(k=4), dict(K=-1)]
    for call, name, bad in ((step, b"pgcn_gpr_step_f32", [dict(X=None), dict(Y=None), dict(gamma=None), dict(n=-1), dict(f=0), dict(ldx=7),
                                                         dict(ldyin=7), dict(ldy=7), dict(Y=two, ldy=12), dict(Y=one, ldy=12)] + ks),
                            (back, b"pgcn_gpr_step_backward_f32", [dict(T=None), dict(H=None), dict(gamma=None), dict(ws=None), dict(n=-1),
                                                                   dict(f=0), dict(ldt=7), dict(ldh=7), dict(lddin=7), dict(lddo=7),
                                                                   dict(Dout=2 * two, lddo=12), dict(Dout=one, lddo=12), dict(ws=6 * two + 4)] + ks),
                            (fin, b"pgcn_gpr_dot_finish_f32", [dict(ws=None), dict(dgamma=None), dict(n=-1), dict(f=0), dict(K=-1),
                                                               dict(ws=6 * two + 4)])):
        for k in bad:
            assert call(**k) == -1 and name in L.pgcn_last_error(), (name, k)
        assert call(f=1025, ldx=1025, ldyin=1025, ldy=1025, ldt=1025, ldh=1025, lddin=1025, lddo=1025) == _lib.PGCN_EUNSUPPORTED
    assert step(n=0) == 0 and back(n=0) == 0 and step(n=0, Yin=None) == 0 and back(n=0, Din=None, Dout=None) == 0       # no launch, no device
    assert back(ws_bytes=8) == fin(ws_bytes=8) == -4                      # PGCN_ENOMEM: a work-space below pgcn_gpr_ws_bytes
    # the work-space: K + 1 regions of a count and one record per band of 512 rows (or of the flat view, whichever has more)
    assert L.pgcn_gpr_ws_bytes(0, 8, 3) == 4 * 2 * 8 and L.pgcn_gpr_ws_bytes(513, 8, 0) == (1 + 2) * 8
    assert L.pgcn_gpr_ws_bytes(1100, 128, 10) == 11 * (1 + 3) * 8 and L.pgcn_gpr_ws_bytes(1100, 1023, 1) == 2 * (1 + 19) * 8
    assert L.pgcn_gpr_ws_bytes(4, 1025, 3) == -1 and L.pgcn_gpr_ws_bytes(-1, 8, 3) == -1 and L.pgcn_gpr_ws_bytes(4, 8, -1) == -1
    assert L.pgcn_abi_version() == 3
