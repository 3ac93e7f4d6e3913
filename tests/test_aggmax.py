"""The max aggregation on the CPU: the definition against its update rule, the composed route of the engine over gloo (the
checker-backed provider has no max kernels) on 1, 2 and 3 ranks, the whole model against a double model under the run's own selection,
run(aggr="max") / --aggr max, checkpoints, validation, the defaults, and the C entry points' size checks (no device)."""
import os

import numpy as np
import pytest
import torch

from conftest import gpath, pkg

import _aggmax_workers as W
import _batchnorm_workers as BW
import _predict_workers as PW


def _pattern(rng, nrows, ncols, lens):
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([rng.choice(ncols, k, replace=False) for k in lens] + [np.zeros(0, np.int64)]).astype(np.int64)
    return rowptr, col


def test_the_oracle_is_the_update_rule_in_any_order():
    rng = np.random.default_rng(0)
    lens = np.array([0, 1, 7, 0, 30, 2, 64, 0])
    rowptr, col = _pattern(rng, len(lens), 80, lens)
    gid = rng.permutation(80)
    for H in (W.tie_features(80, 5, 1), (rng.random((80, 5), dtype=np.float32) - 2), np.full((80, 5), -3.0, np.float32)):
        want = W.oracle_max(rowptr, col, gid, H)
        for order in (None, lambda k: np.arange(k)[::-1], lambda k: np.random.default_rng(k).permutation(k)):
            got = W.rule_max(rowptr, col, gid, H, order)
            assert np.array_equal(got[1], want[1]) and np.array_equal(W.bits(got[0]), W.bits(want[0]))
    assert (want[1][[0, 3, 7]] == -1).all() and (want[0][[0, 3, 7]] == 0).all() and (want[0][1] == -3).all()


def _host_csr(rowptr, col, nrows, ncols):
    P = pkg("partition")
    return P.HostCSR(nrows, ncols, torch.from_numpy(rowptr), torch.from_numpy(col.astype(np.int32)), torch.ones(col.size))


@pytest.mark.parametrize("f", [1, 5, 32])
def test_composed_route_is_the_definition_and_splits_accumulate(f):
    """aggmax_composed bit for bit, whole and as two column-disjoint halves (the second accumulating, both orders); the composed
    backward exactly on integer gradients."""
    E = pkg("engine")
    rng = np.random.default_rng(f)
    nrows, ncols = 60, 90
    lens = rng.integers(0, 25, nrows)
    lens[[3, 17]] = 0
    rowptr, col = _pattern(rng, nrows, ncols, lens)
    gid = rng.permutation(ncols) + 1000
    dev = torch.device("cpu")
    whole = E.composed_max_csr(_host_csr(rowptr, col, nrows, ncols), torch.from_numpy(gid), dev)
    rowi = np.repeat(np.arange(nrows), lens)
    halves = []
    for keep in (col < 45, col >= 45):
        rp = np.concatenate([[0], np.cumsum(np.bincount(rowi[keep], minlength=nrows))]).astype(np.int64)
        halves.append(E.composed_max_csr(_host_csr(rp, col[keep], nrows, ncols), torch.from_numpy(gid), dev))
    for H in (W.tie_features(ncols, f, 3), rng.random((ncols, f), dtype=np.float32) - 3):
        want_out, want_arg = W.oracle_max(rowptr, col, gid, H)
        Ht = torch.from_numpy(H)
        for parts in ([whole], halves, halves[::-1]):
            OUT, ARG = torch.full((nrows, f), 9.0), torch.full((nrows, f), 7, dtype=torch.int32)
            for k, A in enumerate(parts):
                E.aggmax_composed(A, Ht, OUT, ARG, accumulate=k > 0)
            assert np.array_equal(ARG.numpy(), want_arg) and np.array_equal(W.bits(OUT.numpy()), W.bits(want_out))
    # backward: the transposed pattern, rows = columns of the forward structure, ARG in the forward's global ids
    T = __import__("scipy.sparse", fromlist=["x"]).csr_matrix((np.ones(col.size), col, rowptr), shape=(nrows, ncols)).T.tocsr()
    AT = E.composed_max_csr(_host_csr(T.indptr.astype(np.int64), T.indices.astype(np.int64), ncols, nrows), None, dev)
    G = rng.integers(-8, 9, (nrows, f)).astype(np.float32)
    D = torch.full((ncols, f), 5.0)
    E.aggmax_backward_composed(AT, torch.from_numpy(gid.astype(np.int32)), torch.from_numpy(G), torch.from_numpy(want_arg), D)
    inv = np.full(gid.max() + 1, -1)
    inv[gid] = np.arange(ncols)
    local = np.where(want_arg >= 0, inv[np.maximum(want_arg, 0)], -1)
    D64, _, K = W.oracle_max_backward(local, G, ncols)
    assert np.array_equal(D.numpy().astype(np.float64), D64) and K.sum() == (want_arg >= 0).sum()


# ---- engine level: the composed route over gloo -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("aggmax")))


@pytest.mark.parametrize("P,partvec", [(1, "pv"), (2, "pv"), (2, "cpv"), (3, "pv"), (3, "cpv")])
def test_engine_composed_route_over_gloo(dataset, P, partvec):
    paths, data = dataset
    res = W.spawn_engine(P, paths, False, partvec=partvec)
    assert all(r["composed"] and r["hip"] == "OracleKernels" for r in res)
    W.check_engine(res, data, P)


# ---- model level ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 2, 3])
def test_model_against_the_double_model_under_its_own_selection(dataset, P):
    paths, data = dataset
    configs = W.model_configs() if P == 1 else W.rank_subset()
    jobs = W.make_jobs(configs)
    res = W.spawn_model(P, paths, False, [{k: v for k, v in j.items() if k != "torch_params"} for j in jobs])
    assert all(r["composed"] for rank in res for r in rank)
    assert W.check_models(data, configs, jobs, res, "") > 0


# ---- interface --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("aggmax_cli"))
    paths, data = BW.make_dataset(d)
    three = dict(features=paths["features"], labels=paths["labels"], split=paths["split"], hidden=BW.HIDDEN, lr=0.01)
    mx, sm = d + "/max.pt", d + "/sum.pt"
    jobs = [dict(kw=dict(three, epochs=8, aggr="max", root_weight=True, bias=True, save=mx)),
            dict(kw=dict(three, epochs=2, aggr="max", root_weight=True, bias=True, load=mx)),
            dict(kw=dict(three, epochs=0, root_weight=True, bias=True, load=mx)),
            dict(kw=dict(three, epochs=1, save=sm)),
            dict(kw=dict(three, epochs=0, load=sm)),
            dict(kw=dict(three, epochs=0, load=sm, aggr="sum")),
            dict(kw=dict(three, epochs=0, load=sm, aggr="max")),
            dict(kw=dict(three, epochs=1, aggr="mean")),
            dict(kw=dict(aggr="max"))]
    for j in jobs:
        j["nlayers"] = 3
    return PW.spawn_jobs(2, paths, False, "PGCN", jobs), (mx, sm)


def test_run_with_aggr_max_trains_and_resumes(trained):
    res, (mx, sm) = trained
    for rank in res:
        first, resumed = rank[0], rank[1]
        losses = [h["losses"]["train"] for h in first["history"]]
        assert len(losses) == 8 and all(np.isfinite(h["losses"][s]) for h in first["history"] for s in BW.SETS)
        assert losses[-1] < losses[0], losses
        assert [h["epoch"] for h in resumed["history"]][-2:] == [8, 9] and "error" not in resumed
    ck = torch.load(mx, weights_only=True)
    assert ck["arch"]["aggr"] == "max" and "aggr" not in torch.load(sm, weights_only=True)["arch"]


def test_checkpoints_name_aggr_and_old_ones_still_load(trained):
    res, _ = trained
    for rank in res:                                            # every rank raises alike
        for k in (2, 6):
            assert rank[k].get("error", ("", ""))[0] == "ValueError" and "aggr differs" in rank[k]["error"][1], rank[k].get("error")
        assert "error" not in rank[4] and "error" not in rank[5]
        assert "aggr takes" in rank[7]["error"][1] and "needs features, labels and split" in rank[8]["error"][1]


class _Inline:
    seen = []

    def __init__(self, target, args, kwargs=None):
        _Inline.seen.append((args, kwargs))
        self.exitcode = 0

    def start(self):
        pass

    def join(self):
        pass


def test_cli_takes_aggr(monkeypatch, capsys, tmp_path):
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
    M.main(base + files + ["--aggr", "sum"])
    M.main(base + files + ["--aggr", "max", "--root-weight", "--bias"])
    assert [kw for _, kw in _Inline.seen] == [None, None, {"aggr": "max"}]
    assert _Inline.seen[0][0] == _Inline.seen[1][0]                   # --aggr sum: the argument tuple of before
    for bad, text in ((files + ["--aggr", "mean"], "--aggr takes sum|max"), (["--aggr", "max"], "need them")):
        with pytest.raises(SystemExit) as e:
            M.main(base + bad)
        assert e.value.code == 2 and text in capsys.readouterr().out
    # init_process hands it to run() by name
    got = []
    monkeypatch.setattr(M.dist, "init_process_group", lambda *a, **k: None)
    monkeypatch.setattr(M.dist, "destroy_process_group", lambda *a, **k: None)
    M.init_process(0, 1, lambda *a, **k: got.append(k), 2, 16, "A", "p", "gloo", aggr="max")
    M.init_process(0, 1, lambda *a, **k: got.append(k), 2, 16, "A", "p", "gloo")
    assert got == [{"aggr": "max"}, {}]


def test_defaults_are_todays():
    CK, M = pkg("checkpoint"), pkg("PGCN")
    today = {"widths": [24, 32, 7], "layers": 2, "task": "single", "norm": "none", "root_weight": False, "bias": False, "residual": False,
             "heads": None, "out_heads": None, "dropout": 0.0, "dropout_seed": 0}
    assert CK.architecture([24, 32, 7], "single") == today == CK.architecture([24, 32, 7], "single", aggr="sum")
    assert CK.architecture([24, 32, 7], "single", aggr="max") == dict(today, aggr="max") and "aggr" in CK.ARCH_FIELDS
    assert M.AGGRS == ("sum", "max")
    keys = sorted(M.PGCN(None, 4, 3, root_weight=True, bias=True).state_dict())
    assert keys == sorted(M.PGCN(None, 4, 3, root_weight=True, bias=True, aggr=None).state_dict()) == \
        sorted(M.PGCN(None, 4, 3, root_weight=True, bias=True, aggr="max").state_dict()) == ["bias", "linear.weight", "root.weight"]
    with pytest.raises(ValueError, match="aggr takes"):
        M.PGCN(None, 4, 3, aggr="mean")


def test_a_sum_only_engine_never_builds_the_max_structures():
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
    OUT, ARG = eng.forward_max(H)
    assert eng._max is not None and eng._max.composed
    own = part.owned.numpy()
    Hg = np.zeros((n, 6), np.float32)
    Hg[own] = H.numpy()
    rowptr, col = W.sym_pattern(A)
    want_out, want_arg = W.oracle_max(rowptr, col, np.arange(n), Hg)
    assert np.array_equal(ARG.numpy(), want_arg[own]) and np.array_equal(W.bits(OUT.numpy()), W.bits(want_out[own]))


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------

def test_entry_points_refuse_bad_sizes_without_a_device():
    L = pkg("_lib").lib()
    one = 16        # a non-null address that is never dereferenced: every refusal below happens before any HIP call
    fwd = lambda **k: L.pgcn_aggmax_csr_plan_f32(k.get("rowptr", one), k.get("pairs", one), None, k.get("rows", 4), None, k.get("nslices", 1),
                                                 None, 0, k.get("B", one),
                                                 k.get("ldb", 8), k.get("OUT", one), k.get("ldo", 8), k.get("ARG", one), k.get("lda", 8),
                                                 k.get("f", 8), None, 0, 0, 0, None)
    bwd = lambda **k: L.pgcn_aggmax_backward_csr_plan_f32(k.get("rowptr", one), k.get("col", one), k.get("gid", one), None, None,
                                                          k.get("rows", 4), None, k.get("nslices", 1), None, 0, k.get("G", one), k.get("ldg", 8), k.get("ARG", one),
                                                          k.get("lda", 8), k.get("D", one), k.get("ldd", 8), k.get("f", 8), None, 0, 0, 0, None)
    for call, name, bad in ((fwd, b"pgcn_aggmax_csr_plan_f32", [dict(f=0), dict(ldb=7), dict(ldo=7), dict(lda=7), dict(rows=-1),
                                                                  dict(B=None), dict(OUT=None), dict(ARG=None), dict(pairs=None),
                                                                  dict(rowptr=None), dict(nslices=0), dict(nslices=9), dict(nslices=8)]),
                            (bwd, b"pgcn_aggmax_backward_csr_plan_f32", [dict(f=0), dict(ldg=7), dict(lda=7), dict(ldd=7), dict(rows=-1),
                                                                           dict(G=None), dict(ARG=None), dict(D=None), dict(col=None),
                                                                           dict(gid=None), dict(nslices=0), dict(nslices=9),
                                                                           dict(nslices=8)])):
        for k in bad:
            assert call(**k) == -1 and name in L.pgcn_last_error(), (name, k)
        assert call(rows=0) == 0                      # nothing to do: no launch, no device
