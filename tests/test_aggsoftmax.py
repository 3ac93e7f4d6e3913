"""The softmax aggregation on the CPU: the composed routes against the float64 definition, the merge rule, the engine over gloo (the
checker-backed provider has no softmax kernels) on 1, 2 and 3 ranks, the whole model against the float64 model,
run(softmax_beta=...) / --softmax-aggr, checkpoints, validation, the defaults, and the C entry points' size checks (no device)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import gpath, pkg

import _aggsoftmax_workers as W
import _batchnorm_workers as BW
import _predict_workers as PW


def _pattern(rng, nrows, ncols, lens):
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([rng.choice(ncols, k, replace=False) for k in lens] + [np.zeros(0, np.int64)]).astype(np.int64)
    return rowptr, col


def _host_csr(rowptr, col, nrows, ncols):
    P = pkg("partition")
    return P.HostCSR(nrows, ncols, torch.from_numpy(rowptr), torch.from_numpy(col.astype(np.int32)), torch.ones(col.size))


@pytest.mark.parametrize("f", [1, 5, 32])
def test_composed_routes_are_the_definition_and_splits_accumulate(f):
    """aggsoftmax_composed within the forward bound, whole and as two column-disjoint halves (the second accumulating, both orders);
    aggsoftmax_backward_composed within the backward bound."""
    E = pkg("engine")
    rng = np.random.default_rng(f)
    nrows, ncols = 60, 90
    lens = rng.integers(0, 25, nrows)
    lens[[3, 17]] = 0
    lens[5] = 1
    rowptr, col = _pattern(rng, nrows, ncols, lens)
    gid = rng.permutation(ncols) + 1000
    dev = torch.device("cpu")
    whole = E.composed_max_csr(_host_csr(rowptr, col, nrows, ncols), torch.from_numpy(gid), dev)
    rowi = np.repeat(np.arange(nrows), lens)
    halves = []
    for keep in (col < 45, col >= 45):
        rp = np.concatenate([[0], np.cumsum(np.bincount(rowi[keep], minlength=nrows))]).astype(np.int64)
        halves.append(E.composed_max_csr(_host_csr(rp, col[keep], nrows, ncols), torch.from_numpy(gid), dev))
    T = sp.csr_matrix((np.ones(col.size), col, rowptr), shape=(nrows, ncols)).T.tocsr()
    AT = E.composed_max_csr(_host_csr(T.indptr.astype(np.int64), T.indices.astype(np.int64), ncols, nrows), None, dev)
    G = rng.random((nrows, f), dtype=np.float32) * 2 - 1
    for fam, H in W.families(rng, ncols, f).items():
        for beta in (0.0, 1.0, 8.0):
            o = W.oracle_softmax(rowptr, col, H, beta)
            Ht = torch.from_numpy(H)
            for parts in ([whole], halves, halves[::-1]):
                OUT, LSE = torch.full((nrows, f), 9.0), torch.full((nrows, f), 7.0)
                for k, A in enumerate(parts):
                    E.aggsoftmax_composed(A, Ht, OUT, LSE, beta, accumulate=k > 0)
                W.assert_forward(OUT.numpy(), LSE.numpy(), o, beta, (fam, beta, len(parts)))
            D = torch.full((ncols, f), 5.0)
            E.aggsoftmax_backward_composed(AT, Ht, torch.from_numpy(G), OUT, LSE, D, beta)
            W.assert_backward(D.numpy(), rowptr, col, H, G, OUT.numpy(), LSE.numpy(), beta, (fam, beta))


def test_merge_rule_is_associative_within_the_bound_and_handles_absent_groups():
    """Random splits of a row's candidates into groups, merged in fp32 left to right, right to left and pairwise: each within the
    forward bound of the float64 definition.  -inf groups are absent; two absent groups merge to absent, without a NaN."""
    rng = np.random.default_rng(3)
    f, ncols = 6, 400
    for beta, scale, k in [(b, s, k) for b in (0.0, 1.0, 8.0, 50.0) for s in (1.0, 20.0) for k in (1, 2, 40, 300)]:
        H = ((rng.random((ncols, f), dtype=np.float32) * 2 - 1) * scale).astype(np.float32)
        c = rng.choice(ncols, k, replace=False)
        rowptr = np.array([0, k], np.int64)
        o = W.oracle_softmax(rowptr, c, H, beta)
        cuts = np.sort(rng.choice(np.arange(1, k), min(k - 1, 3), replace=False)) if k > 1 else np.zeros(0, np.int64)
        groups = []
        for g in np.split(c, cuts):
            go = W.oracle_softmax(np.array([0, g.size], np.int64), g, H, beta)
            groups.append((go["OUT"].astype(np.float32), go["LSE"].astype(np.float32)))
        groups.insert(1, (np.zeros((1, f), np.float32), np.full((1, f), -np.inf, np.float32)))      # an absent group in the middle
        for order in (groups, groups[::-1]):
            acc = (np.zeros((1, f), np.float32), np.full((1, f), -np.inf, np.float32))
            for g in order:
                acc = tuple(a.astype(np.float32) for a in W.merge(*acc, *g))
            W.assert_forward(acc[0], acc[1], o, beta, (beta, scale, k))
        pairs = list(groups)
        while len(pairs) > 1:
            pairs = [tuple(a.astype(np.float32) for a in W.merge(*pairs[i], *pairs[i + 1])) if i + 1 < len(pairs) else pairs[i]
                     for i in range(0, len(pairs), 2)]
        W.assert_forward(pairs[0][0], pairs[0][1], o, beta, (beta, scale, k, "pairwise"))
    none = (np.zeros((1, f), np.float32), np.full((1, f), -np.inf, np.float32))
    with np.errstate(all="raise"):
        out, lse = W.merge(*none, *none)
    assert (out == 0).all() and np.isneginf(lse).all()
    E = pkg("engine")
    t = [torch.from_numpy(a) for a in none]
    out, lse = E.softmax_merge(*t, *t)
    assert bool((out == 0).all()) and bool(torch.isneginf(lse).all())
    out, lse = E.softmax_merge(*t, torch.full((1, f), 3.0), torch.full((1, f), -2.0))
    assert bool((out == 3).all()) and bool((lse == -2).all())


# ---- engine level: the composed route over gloo -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("aggsoftmax")))


@pytest.mark.parametrize("P,partvec", [(1, "pv"), (2, "pv"), (2, "cpv"), (3, "pv"), (3, "cpv")])
def test_engine_composed_route_over_gloo(dataset, P, partvec):
    paths, data = dataset
    res = W.spawn_engine(P, paths, False, partvec=partvec)
    assert all(r["composed"] and r["hip"] == "OracleKernels" for r in res)
    W.check_engine(res, data, P)


# ---- model level ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 2, 3])
def test_model_against_the_double_model(dataset, P):
    paths, data = dataset
    configs = W.model_configs() if P == 1 else W.rank_subset()
    jobs = W.make_jobs(configs)
    res = W.spawn_model(P, paths, False, W.strip(jobs))
    assert all(r["composed"] and r["kinds"] == ["method:_aggregate_softmax"] for rank in res for r in rank)
    assert W.check_models(data, configs, jobs, res, "") > 0


# ---- interface --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("aggsoftmax_cli"))
    paths, data = BW.make_dataset(d)
    three = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=BW.HIDDEN, lr=0.01)
    a, b, sm = d + "/a.pt", d + "/b.pt", d + "/sum.pt"
    jobs = [dict(kw=dict(three, epochs=30, softmax_beta=1.0)),                              # 0: trains
            dict(kw=dict(three, epochs=20, softmax_beta=1.0, save=a)),                      # 1: the first 20 ...
            dict(kw=dict(three, epochs=10, softmax_beta=1.0, load=a, save=b)),              # 2: ... and 10 more: job 0 bit for bit
            dict(kw=dict(three, epochs=0, load=a)),                                         # 3: without the option: refused
            dict(kw=dict(three, epochs=0, load=a, softmax_beta=2.0)),                       # 4: another beta: refused
            dict(kw=dict(three, epochs=1, save=sm)),                                        # 5
            dict(kw=dict(three, epochs=0, load=sm)),                                        # 6: an old checkpoint still loads
            dict(kw=dict(three, epochs=0, load=sm, softmax_beta=0.0)),                      # 7: beta = 0 is a value: refused
            dict(kw=dict(three, epochs=1, softmax_beta=-1.0)),                              # 8
            dict(kw=dict(three, epochs=1, softmax_beta=True)),                              # 9
            dict(kw=dict(three, epochs=1, softmax_beta=1.0, aggr="max")),                   # 10
            dict(kw=dict(three, epochs=1, softmax_beta=1.0, dense_layers=True, propagate=2)),     # 11
            dict(kw=dict(three, epochs=1, softmax_beta=1.0, drop_edge=0.5)),                # 12
            dict(kw=dict(softmax_beta=1.0)),                                                # 13
            dict(kw=dict(three, epochs=2, softmax_beta=0, propagate=2))]                    # 14: Propagate keeps PSpMM; 0 is taken
    for j in jobs:
        j["nlayers"] = 3
    return PW.spawn_jobs(2, paths, False, "PGCN", jobs), (a, b, sm)


def test_run_with_softmax_beta_trains_and_resumes_bit_for_bit(trained):
    res, (a, b, sm) = trained
    for rank in res:
        whole, first, resumed = rank[0], rank[1], rank[2]
        assert all("error" not in r for r in (whole, first, resumed, rank[14])), [r.get("error") for r in (whole, first, resumed, rank[14])]
        losses = [h["losses"]["train"] for h in whole["history"]]
        assert len(losses) == 30 and all(np.isfinite(h["losses"][s]) for h in whole["history"] for s in BW.SETS)
        assert losses[-1] < losses[0], losses
        assert [h["epoch"] for h in resumed["history"]][-10:] == list(range(20, 30))
        assert [h["losses"] for h in resumed["history"]][-10:] == [h["losses"] for h in whole["history"]][-10:]      # bit for bit
        assert len(rank[14]["history"]) == 2
    ck = torch.load(b, weights_only=True)
    assert ck["arch"]["softmax_beta"] == 1.0 and isinstance(ck["arch"]["softmax_beta"], float) and ck["epochs"] == 30
    assert "softmax_beta" not in torch.load(sm, weights_only=True)["arch"]


def test_checkpoints_name_softmax_beta_and_old_ones_still_load(trained):
    res, _ = trained
    for rank in res:                                            # every rank raises alike
        for k in (3, 4, 7):
            assert rank[k].get("error", ("", ""))[0] == "ValueError" and "softmax_beta differs" in rank[k]["error"][1], rank[k].get("error")
        assert "error" not in rank[5] and "error" not in rank[6]
        for k in (8, 9):
            assert "softmax_beta takes a finite number >= 0" in rank[k]["error"][1], rank[k]["error"]
        assert 'softmax_beta does not go with aggr="max"' in rank[10]["error"][1]
        assert "softmax_beta does not go with dense_layers" in rank[11]["error"][1]
        assert "softmax_beta does not go with drop_edge" in rank[12]["error"][1]
        assert "needs features, labels and split" in rank[13]["error"][1]


class _Inline:
    seen = []

    def __init__(self, target, args, kwargs=None):
        _Inline.seen.append((args, kwargs))
        self.exitcode = 0

    def start(self):
        pass

    def join(self):
        pass


def test_cli_takes_softmax_aggr(monkeypatch, capsys, tmp_path):
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
    M.main(base + files + ["--softmax-aggr", "1.5"])
    M.main(base + files + ["--softmax-aggr", "0", "--root-weight", "--bias"])
    M.main(base + files + ["--aggr", "max"])                          # --aggr is no prefix of the new option: parsed as before
    M.main(base + files + ["--softmax", "2"])                         # a unique prefix, as getopt takes them
    assert [kw for _, kw in _Inline.seen] == [None, {"softmax_beta": 1.5}, {"softmax_beta": 0.0}, {"aggr": "max"}, {"softmax_beta": 2.0}]
    assert _Inline.seen[0][0] == _Inline.seen[1][0] == _Inline.seen[3][0]      # the argument tuple of before
    for value in ("-1", "inf", "nan", "x", ""):
        with pytest.raises(SystemExit) as e:
            M.main(base + files + ["--softmax-aggr", value])
        assert e.value.code == 2 and "--softmax-aggr takes a finite number >= 0, got %r" % value in capsys.readouterr().out
    for bad, text in ((files + ["--softmax-aggr", "1", "--aggr", "max"], "--softmax-aggr does not go with --aggr max"),
                      (files + ["--softmax-aggr", "1", "--dense-layers"], "--softmax-aggr does not go with --dense-layers"),
                      (files + ["--softmax-aggr", "1", "--normalize", "sym", "--drop-edge", "0.5"], "--softmax-aggr does not go with --drop-edge"),
                      (["--softmax-aggr", "1"], "need them"), (files + ["--aggr", "mean"], "--aggr takes sum|max")):
        with pytest.raises(SystemExit) as e:
            M.main(base + bad)
        assert e.value.code == 2 and text in capsys.readouterr().out
    # init_process hands it to run() by name, and only when given
    got = []
    monkeypatch.setattr(M.dist, "init_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "destroy_process_group", lambda *a, **k: None)
    M.init_process(0, 1, lambda *a, **k: got.append(k), 2, 16, "A", "p", "gloo", softmax_beta=0.0)
    M.init_process(0, 1, lambda *a, **k: got.append(k), 2, 16, "A", "p", "gloo")
    assert got == [{"softmax_beta": 0.0}, {}]


def test_defaults_are_todays():
    CK, M, D = pkg("checkpoint"), pkg("PGCN"), pkg("dropout")
    today = {"widths": [24, 32, 7], "layers": 2, "task": "single", "norm": "none", "root_weight": False, "bias": False, "residual": False,
             "heads": None, "out_heads": None, "dropout": 0.0, "dropout_seed": 0}
    assert CK.architecture([24, 32, 7], "single") == today == CK.architecture([24, 32, 7], "single", softmax_beta=None)
    assert CK.architecture([24, 32, 7], "single", softmax_beta=0) == dict(today, softmax_beta=0.0)
    assert CK.ARCH_FIELDS[-3:] == ("softmax_beta", "propagate", "dense_layers") and M.AGGRS == ("sum", "max")
    plain, soft = M.PGCN(None, 4, 3, root_weight=True, bias=True), M.PGCN(None, 4, 3, root_weight=True, bias=True, softmax_beta=0)
    assert sorted(plain.state_dict()) == sorted(soft.state_dict()) == ["bias", "linear.weight", "root.weight"]
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in soft.named_modules()]
    assert plain._aggregate == M.PSpMM.apply and not hasattr(plain, "softmax_beta") and soft.softmax_beta == 0.0
    assert M.PGCN(None, 4, 3, softmax_beta=None)._aggregate == M.PSpMM.apply
    for bad in (True, False, -0.5, float("inf"), float("nan"), "1"):
        with pytest.raises(ValueError, match="softmax_beta takes a finite number >= 0"):
            M.PGCN(None, 4, 3, softmax_beta=bad)
    with pytest.raises(ValueError, match='softmax_beta does not go with aggr="max"'):
        M.PGCN(None, 4, 3, softmax_beta=1.0, aggr="max")
    with pytest.raises(ValueError, match="softmax_beta does not go with aggregate=False"):
        M.PGCN(None, 4, 3, softmax_beta=1.0, aggregate=False)
    with pytest.raises(ValueError, match="softmax_beta does not go with drop_edge"):
        M.PGCN(None, 4, 3, softmax_beta=1.0, drop_edge=D.EdgeDrop(0.5, D.DropoutState(1, torch.device("cpu"))))
    M.PGCN(None, 4, 3, softmax_beta=1.0, drop_edge=D.EdgeDrop(0.0, D.DropoutState(1, torch.device("cpu"))))      # (not active)


def test_an_engine_that_never_calls_it_builds_no_max_structures():
    from oracle_kernels import OracleKernels
    P, E, I = pkg("partition"), pkg("engine"), pkg("ingest")
    A = I.mmread(gpath("karate.mtx")).tocoo()
    n = A.shape[0]
    part = P.build_partition(torch.from_numpy(A.row.astype(np.int64)), torch.from_numpy(A.col.astype(np.int64)),
                             torch.from_numpy(A.data.astype(np.float32)), n, torch.zeros(n, dtype=torch.int64), 0, 1, normalize="sym")
    eng = E.AggregationEngine(part, OracleKernels(), torch.device("cpu"))
    H = torch.rand(n, 6)
    eng.backward(eng.forward(H))
    assert eng._max is None
    OUT, LSE, halo = eng.forward_softmax(H, 2.0)
    assert eng._max is not None and eng._max.composed and halo is None
    own = part.owned.numpy()
    Hg = np.zeros((n, 6), np.float32)
    Hg[own] = H.numpy()
    rowptr, col = W.sym_pattern(A)
    o = W.oracle_softmax(rowptr, col, Hg, 2.0)
    W.assert_forward(OUT.numpy(), LSE.numpy(), {k: v[own] for k, v in o.items()}, 2.0, "karate")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------

def test_entry_points_refuse_bad_sizes_without_a_device():
    L = pkg("_lib").lib()
    one = 16        # a non-null address that is never dereferenced: every refusal below happens before any HIP call
    fwd = lambda **k: L.pgcn_aggsoftmax_csr_plan_f32(k.get("rowptr", one), k.get("pairs", one), None, k.get("rows", 4), None,
                                                     k.get("nslices", 1), None, 0, k.get("B", one), k.get("ldb", 8), k.get("OUT", one),
                                                     k.get("ldo", 8), k.get("LSE", one), k.get("ldl", 8), k.get("beta", 1.0), k.get("f", 8),
                                                     None, 0, 0, 0, None)
    bwd = lambda **k: L.pgcn_aggsoftmax_backward_csr_plan_f32(k.get("rowptr", one), k.get("col", one), None, None, k.get("rows", 4), None,
                                                              k.get("nslices", 1), None, 0, k.get("X", one), k.get("ldx", 8),
                                                              k.get("G", one), k.get("ldg", 8), k.get("OUT", one), k.get("ldo", 8),
                                                              k.get("LSE", one), k.get("ldl", 8), k.get("D", one), k.get("ldd", 8),
                                                              k.get("beta", 1.0), k.get("f", 8), None, 0, 0, 0, None)
    betas = [dict(beta=-1.0), dict(beta=float("inf")), dict(beta=float("nan")), dict(beta=-float("inf"))]
    for call, name, bad in ((fwd, b"pgcn_aggsoftmax_csr_plan_f32", [dict(f=0), dict(ldb=7), dict(ldo=7), dict(ldl=7), dict(rows=-1),
                                                                      dict(B=None), dict(OUT=None), dict(LSE=None), dict(pairs=None),
                                                                      dict(rowptr=None), dict(nslices=0), dict(nslices=9),
                                                                      dict(nslices=8)] + betas),
                            (bwd, b"pgcn_aggsoftmax_backward_csr_plan_f32", [dict(f=0), dict(ldx=7), dict(ldg=7), dict(ldo=7), dict(ldl=7),
                                                                               dict(ldd=7), dict(rows=-1), dict(X=None), dict(G=None),
                                                                               dict(OUT=None), dict(LSE=None), dict(D=None), dict(col=None),
                                                                               dict(rowptr=None), dict(nslices=0), dict(nslices=9),
                                                                               dict(nslices=8)] + betas)):
        for k in bad:
            assert call(**k) == -1 and name in L.pgcn_last_error(), (name, k)
        assert call(rows=0) == 0 and call(rows=0, beta=0.0) == 0          # nothing to do: no launch, no device
