"""Dot-product attention layers on the CPU: the composed route and the engine's kernel path (numpy stand-ins of csrc/pgcn_gatdot.hip)
against the float64 definition under 1, 2 and 3 ranks, the whole model's gradients against float64 autograd, PGAT.run over gloo, the
options' refusals, the checkpoint record and the library's exports.  Every comparison is conftest.held_to_fixture with its defaults."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch
from scipy.io import mmread

from conftest import ROOT, gpath, held_to_fixture, pkg, rel_err

import _gatdot_workers as W

K_, D_ = 2, 32
OUTS = ("out", "dZq", "dZk", "dZv")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def layer_case():
    paths = {"A": gpath("karate.A.mtx"), "pv1": gpath("karate.mtx.1.rp"), "pv2": gpath("karate.mtx.2.rp"), "pv3": gpath("karate.mtx.3.hp")}
    A = mmread(paths["A"])
    n = A.shape[0]
    er, ec = W.pattern(A)
    x = W.layer_inputs(n, n, K_, D_, 5)
    return paths, n, {"m64": W.aggregate64(er, ec, x, K_, D_), "twin": W.aggregate64(er, ec, x, K_, D_, torch.float32)}


def _gather(res, n):
    return {k: W.rows(res, lambda r, k=k: r[k], n) for k in OUTS}


@pytest.mark.parametrize("provider", ["composed", "dot"])
def test_engine_forward_backward_any_partition(layer_case, provider):
    """The composed route (a provider without the new methods) and the kernel route (DotKernels) against the one-rank float64 result."""
    paths, n, ref = layer_case
    got = {}
    for P in (1, 2, 3):
        res = W.spawn(W.engine_worker, P, paths, False, provider=None if provider == "composed" else "dot", K=K_, d=D_, seed=5, n=n)
        where = "gatdot/engine/karate/%s/P%d" % (provider, P)
        got[P] = _gather(res, n)
        for k in OUTS:
            held_to_fixture(where, k, got[P][k], ref["twin"][k], ref["m64"][k])
        for r in res:
            assert r["composed"] == (provider == "composed"), where
            if provider == "dot":              # the log shows the kernel route: every pass over every entry exactly once
                assert [c[0] for c in r["log"]] == ["scores", "softmax", "grad_rows", "grad_cols"], (where, r["log"])
                assert all(c[3] == r["nnz"] for c in r["log"]), where
    for P in (2, 3):                           # the same global result under every part vector (each is within its bound of float64)
        for k in OUTS:
            bound = 2 * max(1e-5, 2 * rel_err(ref["twin"][k], ref["m64"][k]))
            assert rel_err(got[P][k], got[1][k]) <= bound, (provider, P, k)


@pytest.mark.parametrize("provider", [None, "dot"])
def test_a_rank_without_halo_rows_still_takes_part_in_the_exchange(tmp_path, provider):
    """Two rings of six vertices, one per rank, and ONE directed entry: vertex 2 (rank 0) attends to vertex 8 (rank 1).  Rank 1 sends
    a row and receives none: it has no halo, and must make the all-to-all-v of the forward all the same -- rank 0 waits in it."""
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
    for k in OUTS:
        held_to_fixture("gatdot/engine/no-halo-rank/%s" % (provider or "composed"), k, got[k], ref32[k], ref64[k])
    assert np.abs(got["dZk"][8]).max() > 0 and np.abs(got["dZv"][8]).max() > 0          # (the row that travelled got both gradients back)


def test_a_row_without_entries_gives_zeros_and_no_gradient():
    gat, partition = pkg("gat"), pkg("partition")
    n = 6
    row, col = torch.tensor([0, 0, 1, 3, 3, 3]), torch.tensor([1, 2, 0, 0, 3, 5])          # rows 2, 4, 5 are empty; column 4 unreferenced
    part = partition.build_partition(row, col, torch.ones(6), n, torch.zeros(n, dtype=torch.int64), 0, 1, with_transpose=False)
    x = W.layer_inputs(n, n, 2, 32, 1)
    ref, twin = W.aggregate64(row.numpy(), col.numpy(), x, 2, 32), W.aggregate64(row.numpy(), col.numpy(), x, 2, 32, torch.float32)
    for prov in (W.OK.OracleKernels(), W.DotKernels()):
        eng = gat.GatEngine(part, prov, torch.device("cpu"), None)
        st = eng.new_layer_state(2, 32)
        own = eng.part.owned.numpy()                   # (the engine's row order; back to the global one below)
        inv = np.empty(n, np.int64)
        inv[own] = np.arange(n)
        out = eng.forward_dot(st, *(torch.from_numpy(x[k][own]) for k in ("Zq", "Zk", "Zv")))
        dZq, dZk, dZv = eng.backward_dot(st, torch.from_numpy(x["dOut"][own]))
        out, dZq, dZk, dZv = out[inv], dZq[inv], dZk[inv], dZv[inv]
        for t in (out, dZq, dZk, dZv):
            assert torch.isfinite(t).all()
        assert (out[[2, 4, 5]] == 0).all() and (dZq[[2, 4, 5]] == 0).all() and (dZk[4] == 0).all() and (dZv[4] == 0).all()
        for k, v in (("out", out), ("dZq", dZq), ("dZk", dZk), ("dZv", dZv)):
            held_to_fixture("gatdot/engine/empty-rows/%s" % type(prov).__name__, k, v.numpy(), twin[k], ref[k])


def test_a_rank_without_entries_launches_nothing():
    """nnz == 0: zeros everywhere, on the kernel route too (the stand-ins are never reached with a null plan)."""
    gat, partition = pkg("gat"), pkg("partition")
    n = 4
    e = torch.zeros(0, dtype=torch.int64)
    part = partition.build_partition(e, e, torch.zeros(0), n, torch.zeros(n, dtype=torch.int64), 0, 1, with_transpose=False)
    x = W.layer_inputs(n, n, 2, 32, 2)
    for prov in (W.OK.OracleKernels(), W.DotKernels()):
        eng = gat.GatEngine(part, prov, torch.device("cpu"), None)
        st = eng.new_layer_state(2, 32)
        out = eng.forward_dot(st, *(torch.from_numpy(x[k]) for k in ("Zq", "Zk", "Zv")))
        grads = eng.backward_dot(st, torch.from_numpy(x["dOut"]))
        assert all((t == 0).all() and t.shape == (n, 64) for t in (out,) + tuple(grads))


def test_engine_refusals():
    gat, partition, synth, D = pkg("gat"), pkg("partition"), pkg("synth"), pkg("dropout")
    n, row, col, val = synth.make_graph(60, 300, seed=2)
    part = partition.build_partition(row, col, val, n, torch.zeros(n, dtype=torch.int64), 0, 1)
    x = torch.zeros(n, 8), torch.zeros(n, 8), torch.zeros(n, 8)
    eng = gat.GatEngine(part, W.OK.OracleKernels(), torch.device("cpu"), None, mode="reference")
    with pytest.raises(ValueError, match="standard"):
        eng.forward_dot(eng.new_layer_state(1, 8), *x)
    eng = gat.GatEngine(part, W.OK.OracleKernels(), torch.device("cpu"), None)
    st = eng.new_layer_state(1, 8)
    st.drop = D.AttnDrop(0.5, D.DropoutState(0))
    with pytest.raises(ValueError, match="attention dropout"):
        eng.forward_dot(st, *x)
    with pytest.raises(ValueError, match="expected"):
        eng.forward_dot(eng.new_layer_state(1, 8), x[0], x[1], torch.zeros(n, 16))


# ---- the whole model --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return W.make_datasets(str(tmp_path_factory.mktemp("gatdot_grid")))


@pytest.mark.parametrize("P,provider,hidden", [(1, None, 8), (2, "dot", 64)])
def test_whole_model_gradients_against_float64_autograd(datasets, P, provider, hidden):
    """Two layers: K concatenated heads + bias + ELU + dropout, then the mean of two heads with bias.  Loss, logits and EVERY
    parameter's reduced gradient (linear, linear_k and linear_q) of two steps."""
    paths, data = datasets
    n = W.GT.GW.N
    o = W.options(K=2, hidden=hidden, Ko=2, bias=True, dropout=W.GT.DROPOUT)
    ref = W.reference(data["single"], o, 0, 2, 0.0)
    jobs = [{"opts": o, "params": {k: v.numpy() for k, v in ref["params"].items()}}]
    res = W.spawn(W.grad_worker, P, paths, False, jobs=jobs, n=n, provider=provider)
    ranks = [dict(r["results"][0], rank=r["rank"]) for r in res]
    where = "gatdot/model/%s/h%d/P%d" % (W.tag(o), hidden, P)
    names = sorted(ref["params"])
    assert names == ["0.bias", "0.linear.weight", "0.linear_k.weight", "0.linear_q.weight",
                     "1.bias", "1.linear.weight", "1.linear_k.weight", "1.linear_q.weight"]
    held = W.hold_steps(where, ranks, ref, n, 2)
    assert held == 2 * (2 + P * len(names))
    held_to_fixture(where, "eval logits", W.rows(ranks, lambda r: r["eval_logits"], n), ref["twin"]["eval"][-1].numpy(),
                    ref["m64"]["eval"][-1].numpy())
    for r in ranks:                            # hidden 64 (d = 32) on the stand-ins: the kernels' path; the last layer's d = the classes: composed
        assert r["composed"] == [provider is None, True], where
    if provider == "dot":
        assert all(any(c[0] == "grad_cols" for c in r["log"]) for r in res)


EPOCHS, LR = 3, 0.01


@pytest.fixture(scope="module")
def karate(tmp_path_factory):
    paths, data = W.make_karate(str(tmp_path_factory.mktemp("gatdot_karate")))
    paths["pv3"] = gpath("karate.mtx.3.hp")
    return paths, data["single"]


def test_run_over_gloo_against_the_float64_model(karate):
    """PGAT.run(attention="dot") on 2 ranks: loss, logits and every reduced gradient of every epoch, and the eval logits after the
    run, against the float64 run."""
    paths, data = karate
    P = 2
    opts = W.options(K=2, hidden=8, Ko=2, bias=True, dropout=W.GT.DROPOUT)
    ref = W.reference(data, opts, 0, EPOCHS, LR)
    res = W.spawn(W.run_worker, P, paths, False, opts=opts, params={k: v.numpy() for k, v in ref["params"].items()}, epochs=EPOCHS, lr=LR)
    n = data["A"].shape[0]
    assert len(res[0]["history"]) == EPOCHS
    W.hold_steps("gatdot/run/karate/P%d" % P, res, ref, n, EPOCHS)
    held_to_fixture("gatdot/run/karate/P%d" % P, "eval logits", W.rows(res, lambda r: r["eval_logits"], n),
                    ref["twin"]["eval"][-1].numpy(), ref["m64"]["eval"][-1].numpy())
    assert sorted(res[0]["names"]) == sorted(ref["params"])


# ---- the options: layer, refusals, checkpoint record, resume, command line ----------------------------------------------------------------

def test_layer_parameters_and_the_default():
    M = pkg("PGAT")
    assert M.ATTENTIONS == ("v1", "v2", "dot")
    torch.manual_seed(1)
    v1 = M.PGAT(None, 6, 16, heads=2)
    torch.manual_seed(1)
    same = M.PGAT(None, 6, 16, heads=2, attention="v1")
    assert list(v1.state_dict()) == list(same.state_dict()) == ["attention", "linear.weight"]          # the state dict of before
    assert all(torch.equal(a, b) for a, b in zip(v1.state_dict().values(), same.state_dict().values()))
    assert tuple(v1.attention.shape) == (16, 2) and v1.projected_width == 16 + 4
    dot = M.PGAT(None, 6, 16, heads=2, attention="dot")
    assert sorted(dot.state_dict()) == ["linear.weight", "linear_k.weight", "linear_q.weight"] and dot.attention is None
    assert [k for k, _ in dot.named_parameters()] == ["linear.weight", "linear_k.weight", "linear_q.weight"]
    assert all(tuple(w.shape) == (16, 6) for w in dot.state_dict().values()) and dot.projected_width == 48
    gain = torch.nn.init.calculate_gain("relu")                  # xavier_normal_, gain of relu: std = gain * sqrt(2 / (fan_in + fan_out))
    big = M.PGAT(None, 300, 400, heads=2, attention="dot")
    for w in (big.linear.weight, big.linear_k.weight, big.linear_q.weight):
        assert abs(float(w.detach().std()) / (gain * (2.0 / 700) ** 0.5) - 1) < 0.05


def test_constructor_and_run_refusals():
    M, D = pkg("PGAT"), pkg("dropout")
    ref = types.SimpleNamespace(mode="reference")
    with pytest.raises(ValueError, match=r"attention takes v1 \| v2 \| dot, got 'v3'"):
        M.PGAT(None, 4, 4, heads=1, attention="v3")
    with pytest.raises(ValueError, match="share_weights needs attention='v2'"):
        M.PGAT(None, 4, 4, heads=1, attention="dot", share_weights=True)
    with pytest.raises(ValueError, match="attention='dot' needs mode='standard'"):
        M.PGAT(ref, 4, 4, heads=1, attention="dot")
    with pytest.raises(ValueError, match="attention='dot' with attn_dropout is not implemented"):
        M.PGAT(None, 4, 4, heads=1, attention="dot", attn_dropout=0.5, state=D.DropoutState(0))
    files = dict(features="x", labels="y", split="s")
    saved = M.mode
    M.mode = "standard"                        # (module state: an earlier test of the session may have left the other mode)
    try:
        with pytest.raises(ValueError, match="share_weights needs attention='v2'"):
            M.run(0, 1, 2, 4, "A.mtx", "pv", "gloo", attention="dot", share_weights=True, **files)
        with pytest.raises(ValueError, match="attention='dot' with attn_dropout is not implemented"):
            M.run(0, 1, 2, 4, "A.mtx", "pv", "gloo", attention="dot", attn_dropout=0.5, **files)
        M.mode = "reference"
        with pytest.raises(ValueError, match="static score only"):
            M.run(0, 1, 2, 4, "A.mtx", "pv", "gloo", attention="dot")                     # (without the data files too)
    finally:
        M.mode = saved


def test_checkpoint_records_the_option_only_for_dot():
    M, C = pkg("PGAT"), pkg("checkpoint")
    saved = M.heads
    M.heads = 2
    try:
        plain = M._architecture(6, 2, 2, "single", 8, 1, 0.0, 0, None)
        v2 = M._architecture(6, 2, 2, "single", 8, 1, 0.0, 0, None, attention="v2", share_weights=False)
        dot = M._architecture(6, 2, 2, "single", 8, 1, 0.0, 0, None, attention="dot")
    finally:
        M.heads = saved
    assert "attention" not in plain and dot["attention"] == "dot" and dot["share_weights"] is False
    assert {k: v for k, v in dot.items() if k not in ("attention", "share_weights")} == dict(plain)
    ck = {"launcher": "PGAT", "arch": dot, "optimizer": {"kind": "torch"}}
    C.check(ck, "PGAT", dot, "torch")
    for other in (plain, v2):                                    # a dot checkpoint under a v1 or v2 command line, and the reverse
        with pytest.raises(ValueError, match="attention differs"):
            C.check(ck, "PGAT", other, "torch")
        with pytest.raises(ValueError, match="attention differs"):
            C.check({"launcher": "PGAT", "arch": other, "optimizer": {"kind": "torch"}}, "PGAT", dot, "torch")


def test_resume_is_the_run_that_never_stopped(karate, tmp_path):
    """2 + 2 epochs through save / load equal 4 epochs bit for bit; a v1 command line refuses the dot checkpoint."""
    paths, data = karate
    opts = W.options(K=2, hidden=8, Ko=1, dropout=W.GT.DROPOUT)
    ck = str(tmp_path / "two.ckpt")
    whole = W.spawn(W.run_worker, 1, paths, False, opts=opts, params=None, epochs=4, lr=LR)[0]
    first = W.spawn(W.run_worker, 1, paths, False, extra={"save": ck}, opts=opts, params=None, epochs=2, lr=LR)[0]
    rest = W.spawn(W.run_worker, 1, paths, False, extra={"load": ck}, opts=opts, params=None, epochs=2, lr=LR)[0]
    assert np.array_equal(_bits(rest["eval_logits"]), _bits(whole["eval_logits"]))
    assert not np.array_equal(_bits(first["eval_logits"]), _bits(whole["eval_logits"]))
    assert len(whole["history"]) == 4 and rest["history"] == whole["history"] and first["history"] == whole["history"][:2]
    assert sorted(whole["names"]) == ["0.linear.weight", "0.linear_k.weight", "0.linear_q.weight",
                                      "1.linear.weight", "1.linear_k.weight", "1.linear_q.weight"]
    saved = torch.load(ck, weights_only=True)
    assert saved["arch"]["attention"] == "dot" and saved["arch"]["share_weights"] is False and "0.attention" not in saved["model"]
    C = pkg("checkpoint")
    with pytest.raises(ValueError, match="attention differs"):
        C.load(ck, "PGAT", {k: v for k, v in saved["arch"].items() if k not in ("attention", "share_weights")}, "torch")


def test_fused_optimizer_takes_the_three_projections(karate):
    """--optimizer fused on the dot layers: the flat arena holds linear, linear_k and linear_q, and the loss falls."""
    paths, data = karate
    opts = W.options(K=2, hidden=8, Ko=1)
    res = W.spawn(W.run_worker, 1, paths, False, opts=opts, params=None, epochs=4, lr=0.05, optimizer="fused")[0]
    losses = [h["loss"] for h in res["history"]]
    assert len(losses) == 4 and np.isfinite(losses).all() and losses[-1] < losses[0]


def _files(tmp_path):
    out = []
    for k in ("features", "labels", "split"):
        p = tmp_path / (k + ".npy")
        np.save(p, np.zeros((2, 2), np.float32))
        out += ["--" + k, str(p)]
    return out


@pytest.mark.parametrize("args,text", [
    (["--attention", "dot", "--share-weights"], "--share-weights needs --attention v2"),
    (["--attention", "dot", "--mode", "reference"], "--mode reference has the static score only: --attention dot needs --mode standard"),
    ("FILES+--attention dot --attn-dropout 0.6", "--attention dot with --attn-dropout is not implemented"),
    (["--attention", "dotty"], "got 'dotty' (or dot, the scaled dot-product score)"),
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
    """--attention dot reaches run() with and without --features; the absent option starts the process of before."""
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
        M.main(["-a", "A.mtx", "-p", "A.part", "--heads", "2"] + _files(tmp_path) + ["--attention", "dot"])
        M.main(["-a", "A.mtx", "-p", "A.part", "--attention", "dot"])
        M.main(["-a", "A.mtx", "-p", "A.part"])
    finally:
        M.path_A, M.path_partvec, M.mode, M.heads = saved
    assert started[0][-1]["attention"] == "dot" and "share_weights" not in started[0][-1] and "features" in started[0][-1]
    assert started[1][-1] == {"attention": "dot"}
    assert not isinstance(started[2][-1], dict)                                               # the argument tuple of before


def test_synthetic_loop_runs_with_the_option(tmp_path, monkeypatch):
    """PGAT.run without data files: the reference's own loop on dot layers (checker-backed provider)."""
    import io
    from contextlib import redirect_stdout
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # (the checker-backed provider computes on the host)
    M = W._module(False)
    saved = (M.myrank, M.world_size, M.device)
    buf = io.StringIO()
    try:
        with redirect_stdout(buf):
            torch.manual_seed(0)
            model = M.run(0, 1, 2, 4, gpath("karate.A.mtx"), gpath("karate.mtx.1.rp"), "gloo", epochs=3, attention="dot")
    finally:
        M.myrank, M.world_size, M.device = saved
        M._kernel_provider = None
    assert all(m.version == "dot" and hasattr(m, "linear_k") and hasattr(m, "linear_q") and m.attention is None for m in model)
    losses = [float(line.split()[-1]) for line in buf.getvalue().splitlines() if line.startswith("Epoch")]
    assert len(losses) == 3 and np.isfinite(losses).all()


# ---- the library ------------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_gatdot_entry_points():
    _lib = pkg("_lib")
    src = open(os.path.join(ROOT, "include", "pgcn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(n for n in set(re.findall(r"\b(pgcn_[a-z0-9_]+)\s*\(", src)) if n.startswith("pgcn_gatdot_"))
    assert names == ["pgcn_gatdot_grad_cols_f32", "pgcn_gatdot_grad_rows_f32", "pgcn_gatdot_scores_f32"]
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(L, n), "libpgcn_hip.so does not export %s" % n
        assert n in _lib.SIGNATURES
    B = _lib.lib()
    assert len(B.pgcn_gatdot_scores_f32.argtypes) == 16 and len(B.pgcn_gatdot_grad_rows_f32.argtypes) == 31
    assert len(B.pgcn_gatdot_grad_cols_f32.argtypes) == 29
    # host-only behaviour: sizes are checked, shapes refused, before any device call
    assert B.pgcn_gatdot_scores_f32(None, None, 5, None, 0, None, 1, None, 8, None, 8, 1, 8, None, 0, None) == -5        # d = 8
    assert B.pgcn_gatdot_scores_f32(None, None, 5, None, 0, None, 1, None, 320, None, 320, 5, 64, None, 0, None) == -5    # F = 320
    assert B.pgcn_gatdot_scores_f32(None, None, 5, None, 0, None, 1, None, 16, None, 32, 1, 32, None, 0, None) == -1      # ld < F
    assert B.pgcn_gatdot_scores_f32(None, None, 5, None, 0, None, 1, None, 66, None, 64, 2, 32, None, 0, None) == -5      # ld % 4
    assert B.pgcn_gatdot_grad_cols_f32(None, None, 0, None, 0, None, 1, None, 0, None, None, 32, None, 32, None, 0, None, 0, 1, 32,
                                       None, 32, None, 32, None, 0, 0, 0, None) == 0                                       # no rows
    assert B.pgcn_gatdot_grad_rows_f32(None, None, 0, None, 0, None, 1, None, 0, None, 32, None, 32, None, 0, None, 32, None, 32, None,
                                       1, 32, None, 0, None, 32, None, 0, 0, 0, None) == 0                                 # no rows
