"""GATv2 layers on the CPU: the composed route and the engine's kernel path (numpy stand-ins of csrc/pgcn_gatv2.hip) against the float64
definition under 1, 2 and 3 ranks, the whole model's gradients against float64 autograd, PGAT.run over gloo, the options' refusals, the
checkpoint record and the library's exports.  Every comparison is conftest.held_to_fixture with its defaults."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch
from scipy.io import mmread

from conftest import ROOT, gpath, held_to_fixture, pkg, read_partvec, rel_err

import _gatv2_workers as W

K_, D_ = 2, 32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _graph_paths(name, tmp_path_factory):
    if name == "karate":
        return {"A": gpath("karate.A.mtx"), "pv1": gpath("karate.mtx.1.rp"), "pv2": gpath("karate.mtx.2.rp"), "pv3": gpath("karate.mtx.3.hp")}
    n = mmread(gpath("cora.A.mtx")).shape[0]
    pv3 = str(tmp_path_factory.mktemp("gatv2_cora") / "cora.3.pv")        # (1 and 2 ranks: the committed vectors; 3: a seeded one)
    with open(pv3, "w") as f:
        f.write(" ".join(map(str, np.random.default_rng(3).integers(0, 3, n).tolist())) + "\n")
    return {"A": gpath("cora.A.mtx"), "pv1": gpath("cora.A.mtx.1.rp"), "pv2": gpath("cora.A.mtx.2.rp"), "pv3": pv3}


@pytest.fixture(scope="module", params=["karate", "cora"])
def layer_case(request, tmp_path_factory):
    paths = _graph_paths(request.param, tmp_path_factory)
    A = mmread(paths["A"])
    n = A.shape[0]
    er, ec = W.pattern(A)
    x = W.layer_inputs(n, n, K_, D_, 5)
    return request.param, paths, n, {"m64": W.aggregate64(er, ec, x, K_, D_), "twin": W.aggregate64(er, ec, x, K_, D_, torch.float32)}


def _gather(res, n):
    got = {k: W.rows(res, lambda r, k=k: r[k], n) for k in ("out", "dZt", "dZs")}
    got["da"] = sum(r["da"].astype(np.float64) for r in res).astype(np.float32)          # the ranks' partial sums, as the reduction adds them
    return got


@pytest.mark.parametrize("provider", ["composed", "v2"])
def test_engine_forward_backward_any_partition(layer_case, provider):
    """The composed route (a provider without the new methods) and the kernel route (V2Kernels) against the one-rank float64 result."""
    name, paths, n, ref = layer_case
    got = {}
    for P in (1, 2, 3):
        res = W.spawn(W.engine_worker, P, paths, False, provider=None if provider == "composed" else "v2", K=K_, d=D_, seed=5, n=n)
        where = "gatv2/engine/%s/%s/P%d" % (name, provider, P)
        got[P] = _gather(res, n)
        for k in ("out", "dZt", "dZs", "da"):
            held_to_fixture(where, k, got[P][k], ref["twin"][k], ref["m64"][k])
        for r in res:
            assert r["composed"] == (provider == "composed"), where
            if provider == "v2":               # the log shows the kernel route: every pass over every entry exactly once
                assert [c[0] for c in r["log"]] == ["scores", "softmax", "grad_rows", "grad_cols"], (where, r["log"])
                assert all(c[3] == r["nnz"] for c in r["log"]), where
    for P in (2, 3):                           # the same global result under every part vector (each is within its bound of float64)
        for k in ("out", "dZt", "dZs", "da"):
            bound = 2 * max(1e-5, 2 * rel_err(ref["twin"][k], ref["m64"][k]))
            assert rel_err(got[P][k], got[1][k]) <= bound, (name, provider, P, k)


@pytest.mark.parametrize("provider", [None, "v2"])
def test_a_rank_without_halo_rows_still_takes_part_in_the_exchange(tmp_path, provider):
    """Two rings of six vertices, one per rank, and ONE directed entry: vertex 2 (rank 0) attends to vertex 8 (rank 1).  Rank 1 sends
    a row and receives none: it has no halo, and must make the all-to-all-v of the forward all the same -- rank 0 waits in it (a
    forward that skipped it there left the ranks' collectives mismatched, which over gloo and RCCL is a hang, here a dead worker)."""
    import scipy.sparse as sp
    from scipy.io import mmwrite
    n = 12
    r = np.array([i for i in range(n)] * 2 + [2])
    c = np.array([(i + 1) % 6 + 6 * (i // 6) for i in range(n)] + [(i - 1) % 6 + 6 * (i // 6) for i in range(n)] + [8])
    A = sp.coo_matrix((np.ones(r.size), (r, c)), shape=(n, n))
    paths = {"A": str(tmp_path / "rings.mtx"), "pv2": str(tmp_path / "rings.2.pv")}
    mmwrite(paths["A"], A)
    with open(paths["pv2"], "w") as f:
        f.write(" ".join(["0"] * 6 + ["1"] * 6) + "\n")
    er, ec = W.pattern(A)
    x = W.layer_inputs(n, n, K_, D_, 9)
    ref64, ref32 = W.aggregate64(er, ec, x, K_, D_), W.aggregate64(er, ec, x, K_, D_, torch.float32)
    res = W.spawn(W.engine_worker, 2, paths, False, provider=provider, K=K_, d=D_, seed=9, n=n)
    assert [r["halo"] for r in res] == [1, 0] and [r["nnz"] for r in res] == [13, 12]
    got = _gather(res, n)
    for k in ("out", "dZt", "dZs", "da"):
        held_to_fixture("gatv2/engine/no-halo-rank/%s" % (provider or "composed"), k, got[k], ref32[k], ref64[k])
    assert np.abs(got["dZs"][8]).max() > 0                      # (the row that travelled got its gradient back)


def test_a_row_without_entries_gives_zeros_and_no_gradient():
    gat, partition = pkg("gat"), pkg("partition")
    n = 6
    row, col = torch.tensor([0, 0, 1, 3, 3, 3]), torch.tensor([1, 2, 0, 0, 3, 5])          # rows 2, 4, 5 are empty; columns 4 unreferenced
    part = partition.build_partition(row, col, torch.ones(6), n, torch.zeros(n, dtype=torch.int64), 0, 1, with_transpose=False)
    x = W.layer_inputs(n, n, 2, 32, 1)
    ref = W.aggregate64(row.numpy(), col.numpy(), x, 2, 32)
    for prov in (W.OK.OracleKernels(), W.V2Kernels()):
        eng = gat.GatEngine(part, prov, torch.device("cpu"), None)
        st = eng.new_layer_state(2, 32)
        own = eng.part.owned.numpy()                   # (the engine's row order; back to the global one below)
        inv = np.empty(n, np.int64)
        inv[own] = np.arange(n)
        out = eng.forward_v2(st, torch.from_numpy(x["Zt"][own]), torch.from_numpy(x["Zs"][own]), torch.from_numpy(x["a"]))
        dZt, dZs, da = eng.backward_v2(st, torch.from_numpy(x["dOut"][own]))
        out, dZt, dZs = out[inv], dZt[inv], dZs[inv]
        for t in (out, dZt, dZs, da):
            assert torch.isfinite(t).all()
        assert (out[[2, 4, 5]] == 0).all() and (dZt[[2, 4, 5]] == 0).all() and (dZs[4] == 0).all()
        for k, v in (("out", out), ("dZt", dZt), ("dZs", dZs), ("da", da)):
            held_to_fixture("gatv2/engine/empty-rows/%s" % type(prov).__name__, k, v.numpy(), W.aggregate64(row.numpy(), col.numpy(), x, 2, 32, torch.float32)[k], ref[k])


def test_engine_refusals():
    gat, partition, synth, D = pkg("gat"), pkg("partition"), pkg("synth"), pkg("dropout")
    n, row, col, val = synth.make_graph(60, 300, seed=2)
    part = partition.build_partition(row, col, val, n, torch.zeros(n, dtype=torch.int64), 0, 1)
    x = torch.zeros(n, 8), torch.zeros(n, 8), torch.zeros(8, 1)
    eng = gat.GatEngine(part, W.OK.OracleKernels(), torch.device("cpu"), None, mode="reference")
    with pytest.raises(ValueError, match="standard"):
        eng.forward_v2(eng.new_layer_state(1, 8), *x)
    eng = gat.GatEngine(part, W.OK.OracleKernels(), torch.device("cpu"), None)
    st = eng.new_layer_state(1, 8)
    st.drop = D.AttnDrop(0.5, D.DropoutState(0))
    with pytest.raises(ValueError, match="attention dropout"):
        eng.forward_v2(st, *x)
    with pytest.raises(ValueError, match="expected"):
        eng.forward_v2(eng.new_layer_state(1, 8), x[0], x[1], torch.zeros(16, 1))          # (the v1 shape of the attention parameter)


# ---- the whole model --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return W.make_datasets(str(tmp_path_factory.mktemp("gatv2_grid")))


@pytest.mark.parametrize("P,provider,hidden", [(1, None, 8), (2, "v2", 64), (3, "v2", 64)])
def test_whole_model_gradients_against_float64_autograd(datasets, P, provider, hidden):
    """Two layers: K concatenated heads + bias + ELU + dropout, then the mean of two heads with bias; with and without shared weights.
    Loss, logits and EVERY parameter's reduced gradient (attention and linear_t included) of two steps."""
    paths, data = datasets
    n = W.GT.GW.N
    grid = [W.options(K=2, hidden=hidden, Ko=2, bias=True, dropout=W.GT.DROPOUT, share=sh) for sh in (False, True)]
    refs = [W.reference(data["single"], o, 0, 2, 0.0) for o in grid]
    jobs = [{"opts": o, "params": {k: v.numpy() for k, v in r["params"].items()}} for o, r in zip(grid, refs)]
    res = W.spawn(W.grad_worker, P, paths, False, jobs=jobs, n=n, provider=provider)
    for j, (o, ref) in enumerate(zip(grid, refs)):
        ranks = [dict(r["results"][j], rank=r["rank"]) for r in res]
        where = "gatv2/model/%s/h%d/P%d" % (W.tag(o), hidden, P)
        names = sorted(ref["params"])
        assert ("0.linear_t.weight" in names) == (not o["share"]) and "0.attention" in names and "1.attention" in names
        held = W.hold_steps(where, ranks, ref, n, 2)
        assert held == 2 * (2 + P * len(names))
        held_to_fixture(where, "eval logits", W.rows(ranks, lambda r: r["eval_logits"], n), ref["twin"]["eval"][-1].numpy(),
                        ref["m64"]["eval"][-1].numpy())
        for r in ranks:                        # hidden 64 (d = 32) on the stand-ins: the kernels' path; the last layer's d = the classes: composed
            assert r["composed"] == [provider is None, True], where
    if provider == "v2":
        assert all(any(c[0] == "grad_cols" for c in r["log"]) for r in res)


EPOCHS, LR = 3, 0.01


@pytest.fixture(scope="module")
def karate(tmp_path_factory):
    paths, data = W.make_karate(str(tmp_path_factory.mktemp("gatv2_karate")))
    paths["pv3"] = gpath("karate.mtx.3.hp")
    return paths, data["single"]


@pytest.mark.parametrize("P", [2, 3])
def test_run_over_gloo_against_the_float64_model(karate, P):
    """PGAT.run(attention="v2") on P ranks: loss, logits and every reduced gradient of every epoch, and the eval logits after the
    run, against the float64 run -- the rule of tests/test_attndrop.py and tests/test_gat_tail.py on the same data."""
    paths, data = karate
    opts = W.options(K=2, hidden=8, Ko=2, bias=True, dropout=W.GT.DROPOUT, share=(P == 3))
    ref = W.reference(data, opts, 0, EPOCHS, LR)
    res = W.spawn(W.run_worker, P, paths, False, share=opts["share"], opts=opts, params={k: v.numpy() for k, v in ref["params"].items()},
                  epochs=EPOCHS, lr=LR)
    n = data["A"].shape[0]
    assert len(res[0]["history"]) == EPOCHS
    W.hold_steps("gatv2/run/karate/P%d" % P, res, ref, n, EPOCHS)
    held_to_fixture("gatv2/run/karate/P%d" % P, "eval logits", W.rows(res, lambda r: r["eval_logits"], n),
                    ref["twin"]["eval"][-1].numpy(), ref["m64"]["eval"][-1].numpy())
    assert sorted(res[0]["names"]) == sorted(ref["params"])


# ---- the options: layer, refusals, checkpoint record, resume, command line ----------------------------------------------------------------

def test_layer_parameters_and_the_default():
    M = pkg("PGAT")
    torch.manual_seed(1)
    v1 = M.PGAT(None, 6, 16, heads=2)
    torch.manual_seed(1)
    same = M.PGAT(None, 6, 16, heads=2, attention="v1", share_weights=False)
    assert list(v1.state_dict()) == list(same.state_dict()) == ["attention", "linear.weight"]
    assert all(torch.equal(a, b) for a, b in zip(v1.state_dict().values(), same.state_dict().values()))
    assert tuple(v1.attention.shape) == (16, 2) and v1.projected_width == 16 + 4
    v2 = M.PGAT(None, 6, 16, heads=2, attention="v2")
    assert sorted(v2.state_dict()) == ["attention", "linear.weight", "linear_t.weight"] and tuple(v2.attention.shape) == (8, 2)
    assert tuple(v2.linear_t.weight.shape) == (16, 6) and v2.projected_width == 32
    sh = M.PGAT(None, 6, 16, heads=2, attention="v2", share_weights=True)
    assert sorted(sh.state_dict()) == ["attention", "linear.weight"] and sh.projected_width == 16
    gain = torch.nn.init.calculate_gain("relu")                  # xavier_normal_, gain of relu: std = gain * sqrt(2 / (fan_in + fan_out))
    big = M.PGAT(None, 300, 400, heads=2, attention="v2")
    for w in (big.linear.weight, big.linear_t.weight):
        assert abs(float(w.detach().std()) / (gain * (2.0 / 700) ** 0.5) - 1) < 0.05


def test_constructor_and_run_refusals():
    M, D = pkg("PGAT"), pkg("dropout")
    ref = types.SimpleNamespace(mode="reference")
    with pytest.raises(ValueError, match="attention takes v1 | v2"):
        M.PGAT(None, 4, 4, heads=1, attention="v3")
    with pytest.raises(ValueError, match="share_weights needs attention='v2'"):
        M.PGAT(None, 4, 4, heads=1, share_weights=True)
    with pytest.raises(ValueError, match="attention='v2' needs mode='standard'"):
        M.PGAT(ref, 4, 4, heads=1, attention="v2")
    with pytest.raises(ValueError, match="attention='v2' with attn_dropout is not implemented"):
        M.PGAT(None, 4, 4, heads=1, attention="v2", attn_dropout=0.5, state=D.DropoutState(0))
    files = dict(features="x", labels="y", split="s")
    saved = M.mode
    M.mode = "standard"                        # (module state: an earlier test of the session may have left the other mode)
    try:
        with pytest.raises(ValueError, match="attention takes"):
            M.run(0, 1, 2, 4, "A.mtx", "pv", "gloo", attention="v3", **files)
        with pytest.raises(ValueError, match="share_weights needs attention='v2'"):
            M.run(0, 1, 2, 4, "A.mtx", "pv", "gloo", share_weights=True, **files)
        with pytest.raises(ValueError, match="attn_dropout is not implemented"):
            M.run(0, 1, 2, 4, "A.mtx", "pv", "gloo", attention="v2", attn_dropout=0.5, **files)
        M.mode = "reference"
        with pytest.raises(ValueError, match="static score only"):
            M.run(0, 1, 2, 4, "A.mtx", "pv", "gloo", attention="v2")                      # (without the data files too)
    finally:
        M.mode = saved


def test_checkpoint_records_the_options_only_for_v2():
    M, C = pkg("PGAT"), pkg("checkpoint")
    saved = M.heads
    M.heads = 2
    try:
        plain = M._architecture(6, 2, 2, "single", 8, 1, 0.0, 0, None)
        v1 = M._architecture(6, 2, 2, "single", 8, 1, 0.0, 0, None, attention="v1", share_weights=False)
        v2 = M._architecture(6, 2, 2, "single", 8, 1, 0.0, 0, None, attention="v2", share_weights=False)
        v2s = M._architecture(6, 2, 2, "single", 8, 1, 0.0, 0, None, attention="v2", share_weights=True)
    finally:
        M.heads = saved
    assert "attention" not in plain and v1 == dict(plain)                                    # a checkpoint without the fields is a v1 model
    assert v2["attention"] == "v2" and v2["share_weights"] is False and v2s["share_weights"] is True
    assert {k: v for k, v in v2.items() if k not in ("attention", "share_weights")} == dict(plain)
    assert "attention" in C.ARCH_FIELDS and "share_weights" in C.ARCH_FIELDS
    ck = {"launcher": "PGAT", "arch": v2, "optimizer": {"kind": "torch"}}
    C.check(ck, "PGAT", v2, "torch")
    with pytest.raises(ValueError, match="attention differs"):
        C.check(ck, "PGAT", plain, "torch")                                                    # a v2 checkpoint under a v1 command line
    with pytest.raises(ValueError, match="attention differs"):
        C.check({"launcher": "PGAT", "arch": plain, "optimizer": {"kind": "torch"}}, "PGAT", v2, "torch")      # and the reverse
    with pytest.raises(ValueError, match="share_weights differs"):
        C.check(ck, "PGAT", v2s, "torch")


def test_resume_is_the_run_that_never_stopped(karate, tmp_path):
    """2 + 2 epochs through save / load equal 4 epochs bit for bit; a v1 command line refuses the v2 checkpoint."""
    paths, data = karate
    opts = W.options(K=2, hidden=8, Ko=1, dropout=W.GT.DROPOUT)
    ck = str(tmp_path / "two.ckpt")
    whole = W.spawn(W.run_worker, 1, paths, False, opts=opts, params=None, epochs=4, lr=LR)[0]
    first = W.spawn(W.run_worker, 1, paths, False, extra={"save": ck}, opts=opts, params=None, epochs=2, lr=LR)[0]
    rest = W.spawn(W.run_worker, 1, paths, False, extra={"load": ck}, opts=opts, params=None, epochs=2, lr=LR)[0]
    assert np.array_equal(_bits(rest["eval_logits"]), _bits(whole["eval_logits"]))
    assert not np.array_equal(_bits(first["eval_logits"]), _bits(whole["eval_logits"]))
    assert len(whole["history"]) == 4 and rest["history"] == whole["history"] and first["history"] == whole["history"][:2]
    assert sorted(whole["names"]) == ["0.attention", "0.linear.weight", "0.linear_t.weight", "1.attention", "1.linear.weight", "1.linear_t.weight"]
    arch = torch.load(ck, weights_only=True)["arch"]
    assert arch["attention"] == "v2" and arch["share_weights"] is False
    other = W.spawn(W.run_worker, 1, paths, False, attention=None, opts=opts, params=None, epochs=1, lr=LR)[0]
    assert sorted(other["names"]) == ["0.attention", "0.linear.weight", "1.attention", "1.linear.weight"]
    C = pkg("checkpoint")
    with pytest.raises(ValueError, match="attention differs"):
        C.load(ck, "PGAT", {k: v for k, v in arch.items() if k not in ("attention", "share_weights")}, "torch")


def _files(tmp_path):
    out = []
    for k in ("features", "labels", "split"):
        p = tmp_path / (k + ".npy")
        np.save(p, np.zeros((2, 2), np.float32))
        out += ["--" + k, str(p)]
    return out


@pytest.mark.parametrize("args,text", [
    (["--attention", "v3"], "--attention takes v1|v2, got 'v3'"),
    (["--share-weights"], "--share-weights needs --attention v2"),
    (["--attention", "v1", "--share-weights"], "--share-weights needs --attention v2"),
    (["--attention", "v2", "--mode", "reference"], "--mode reference has the static score only: --attention v2 needs --mode standard"),
    ("FILES+--attention v2 --attn-dropout 0.6", "--attention v2 with --attn-dropout is not implemented"),
])
def test_main_refuses(args, text, tmp_path, capsys):
    M = pkg("PGAT")
    saved = (M.path_A, M.path_partvec, M.mode, M.heads)
    if isinstance(args, str):
        args = _files(tmp_path) + args.split("+")[1].split()
    M.mode, M.heads = "standard", 1
    try:
        with pytest.raises(SystemExit) as e:
            M.main(["-a", "A.mtx", "-p", "A.part"] + args)
    finally:
        M.path_A, M.path_partvec, M.mode, M.heads = saved
    out = capsys.readouterr().out
    assert e.value.code == 2 and text in out and len(out.strip().splitlines()) == 1, out


def test_main_accepts(tmp_path, monkeypatch):
    """--attention v2 / --share-weights reach run() with and without --features; v1 and the absent option start the process of before."""
    M = pkg("PGAT")
    saved = (M.path_A, M.path_partvec, M.mode, M.heads)
    started = []

    class Proc:
        exitcode = 0

        def __init__(self, target=None, args=()):
            started.append(args)

        def start(self):
            pass

        def join(self):
            pass

    monkeypatch.setattr(M.mp, "Process", Proc)
    monkeypatch.setattr(M.mp, "set_start_method", lambda *a, **k: None)
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("SLURM_PROCID", raising=False)
    M.mode, M.heads = "standard", 1
    try:
        M.main(["-a", "A.mtx", "-p", "A.part", "--heads", "2"] + _files(tmp_path) + ["--attention", "v2", "--share-weights"])
        M.main(["-a", "A.mtx", "-p", "A.part", "--attention", "v2"])
        M.main(["-a", "A.mtx", "-p", "A.part", "--attention", "v1"])
        M.main(["-a", "A.mtx", "-p", "A.part"])
    finally:
        M.path_A, M.path_partvec, M.mode, M.heads = saved
    assert started[0][-1]["attention"] == "v2" and started[0][-1]["share_weights"] is True and "features" in started[0][-1]
    assert started[1][-1] == {"attention": "v2"}
    assert started[2] == started[3] and not isinstance(started[3][-1], dict)                  # the argument tuple of before


def test_synthetic_loop_runs_with_the_option(tmp_path, monkeypatch):
    """PGAT.run without data files: the reference's own loop on v2 layers (checker-backed provider), and the loss falls."""
    import io
    from contextlib import redirect_stdout
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # (the checker-backed provider computes on the host)
    M = W._module(False)
    saved = (M.myrank, M.world_size, M.device)
    buf = io.StringIO()
    try:
        with redirect_stdout(buf):
            torch.manual_seed(0)
            model = M.run(0, 1, 2, 4, gpath("karate.A.mtx"), gpath("karate.mtx.1.rp"), "gloo", epochs=3, attention="v2")
    finally:
        M.myrank, M.world_size, M.device = saved
        M._kernel_provider = None
    assert all(m.version == "v2" and hasattr(m, "linear_t") for m in model)
    losses = [float(line.split()[-1]) for line in buf.getvalue().splitlines() if line.startswith("Epoch")]
    assert len(losses) == 3 and np.isfinite(losses).all()


# ---- the library ------------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_gatv2_entry_points():
    _lib = pkg("_lib")
    src = open(os.path.join(ROOT, "include", "pgcn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(n for n in set(re.findall(r"\b(pgcn_[a-z0-9_]+)\s*\(", src)) if n.startswith("pgcn_gatv2_"))
    assert names == ["pgcn_gatv2_da_ws_elems", "pgcn_gatv2_grad_cols_f32", "pgcn_gatv2_grad_rows_f32", "pgcn_gatv2_scores_f32",
                     "pgcn_gatv2_softmax_f32"]
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(L, n), "libpgcn_hip.so does not export %s" % n
        assert n in _lib.SIGNATURES
    B = _lib.lib()
    assert B.pgcn_abi_version() == 3 and _lib.ABI_VERSION == 3
    assert len(B.pgcn_gatv2_scores_f32.argtypes) == 18 and len(B.pgcn_gatv2_grad_rows_f32.argtypes) == 36
    assert len(B.pgcn_gatv2_grad_cols_f32.argtypes) == 30 and len(B.pgcn_gatv2_softmax_f32.argtypes) == 10
    # host-only behaviour: sizes are checked, shapes refused, before any device call
    assert B.pgcn_gatv2_da_ws_elems(10, None, 0, None, 1, 4, 64) == (3 + 1) * 256
    assert B.pgcn_gatv2_da_ws_elems(10, None, 0, None, 0, 4, 64) == -1
    assert B.pgcn_gatv2_scores_f32(None, None, 5, None, 0, None, 1, None, 8, None, 8, None, 1, 8, 0.2, None, 0, None) == -5      # d = 8
    assert B.pgcn_gatv2_scores_f32(None, None, 5, None, 0, None, 1, None, 320, None, 320, None, 5, 64, 0.2, None, 0, None) == -5  # F = 320
    assert B.pgcn_gatv2_scores_f32(None, None, 5, None, 0, None, 1, None, 16, None, 32, None, 1, 32, 0.2, None, 0, None) == -1    # ld < F
    assert B.pgcn_gatv2_grad_cols_f32(None, None, 0, None, 0, None, 1, None, 0, None, 32, None, 32, None, 32, None, None, 0, None, 0, 1, 32, 0.2,
                                      None, 32, None, 0, 0, 0, None) == 0                                                           # no rows
