"""Layer norm and residual links of the GAT layers off the device: the composed twins and a three-layer classifier against float64, the
model on 1 and 2 gloo ranks, the absent options, refusals, the checkpoint record and resume, and the command line."""
import types

import numpy as np
import pytest
import torch
from scipy.io import mmread

import _attndrop_workers as AW
import _gat_norm_workers as W
import _gat_tail_workers as GT
from conftest import gpath, pkg, rel_err
from test_attndrop import cpu_engine  # noqa: F401  (PGAT on a recording checker-backed provider, one rank, karate)

ON = {"norm": "node", "residual": True}


@pytest.mark.parametrize("K,d,mean,n", [(1, 3, 0, 513), (2, 5, 1, 1025), (4, 64, 0, 65)])
def test_composed_twins_against_float64(K, d, mean, n):
    M, D = pkg("PGAT"), pkg("dropout")
    x = W.inputs(n, K, d, mean, 7)
    thr, scale = D.threshold(W.P)
    keep = D.keep_mask(W.SEED, 0, W.LAYER, torch.from_numpy(x["ids"]), d if mean else K * d, thr).numpy()
    want = W.shadow64(x, K, d, mean, True, True, 1, keep, float(scale))
    got = W.run(M, D, x, K, d, mean, True, True, 1, True, torch.device("cpu"))
    errs = {w: rel_err(got[w].numpy(), want[w]) for w in W.WHAT}
    print(errs)
    assert max(errs.values()) <= 2e-6          # fp32 sums of at most 256 terms and three float64 column sums, rounded once


def test_whole_model_gradients_of_a_three_layer_classifier(cpu_engine):
    """build_classifier(norm="node", residual=True, dropout=0.5) in training mode on one rank: the logits and every parameter's
    gradient against the dense float64 model -- G handed through as the residual's gradient, each layer's own masks, X kept per layer."""
    M, eng = cpu_engine
    D = pkg("dropout")
    state, (thr, scale) = D.DropoutState(5), D.threshold(0.5)
    torch.manual_seed(9)
    model, widths = M.build_classifier(eng, 8, 2, 3, 8, 2, 1, 0.5, True, state, **ON)
    assert widths == [8, 8, 8, 2] and [(m.norm, m.residual) for m in model] == [("node", True), ("node", True), (None, False)]
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if "ln_" in name or name.endswith("bias"):
                prm.add_(0.3 * torch.randn_like(prm))
    own = eng.part.owned.cpu()
    H = torch.randn(len(own), 8)
    out = model.train()(H)
    (out * torch.cos(out.detach())).sum().backward()
    edge = torch.from_numpy(mmread(gpath("karate.A.mtx")).toarray() != 0)[own][:, own]       # (the engine's rows are in its own order)
    cfg = [{"K": 2, "concat": True, "elu": True, "residual": True, "keep": D.keep_mask(5, 0, l, own, 8, thr), "scale": float(scale)}
           for l in range(2)] + [{"K": 1, "concat": False, "elu": False, "residual": False}]
    W.hold_model("gat_norm/classifier", model, out, edge, H, cfg)


@pytest.mark.parametrize("attention", ["v1", "dot"])
def test_the_absent_options_make_the_calls_of_before(cpu_engine, attention):
    M, eng = cpu_engine
    rec = eng.k
    H = torch.from_numpy(np.random.default_rng(1).standard_normal((eng.part.n_local, 8)).astype(np.float32))

    def trace(**kw):
        torch.manual_seed(5)
        layer = M.PGAT(eng, 8, 8, heads=2, bias=True, activation="elu", attention=attention, **kw)
        del rec.calls[:]
        out = layer(H)
        out.sum().backward()
        return [c[0] for c in rec.calls], out.detach().clone(), list(layer.state_dict())

    base, off = trace(), trace(norm="none", residual=False)
    assert off[0] == base[0] and torch.equal(off[1], base[1]) and off[2] == base[2]
    res, on = trace(residual=True), trace(**ON)
    assert res[0] == base[0] and torch.equal(res[1], H + base[1]) and res[2] == base[2]      # no norm: _GatTail and a tensor addition
    assert sorted(on[2]) == sorted(base[2] + ["ln_weight", "ln_bias"]) and not torch.equal(on[1], res[1])


def test_refusals_the_record_and_the_command_line(capsys, tmp_path, monkeypatch):
    M, C = pkg("PGAT"), pkg("checkpoint")
    ref = types.SimpleNamespace(mode="reference")
    for kw, text in (({"norm": "batch"}, "belongs to PGCN"), ({"norm": "layer"}, "norm takes"),
                     ({"in_features": 6, "residual": True}, "residual=True needs in_features equal"),
                     ({"heads": 2, "concat": False, "residual": True}, "residual=True needs in_features equal"),     # (2 wide after the mean)
                     ({"A": ref, "norm": "node"}, "reference layer has no norm"), ({"A": ref, "residual": True}, "reference layer has no norm")):
        with pytest.raises(ValueError, match=text):
            M.PGAT(kw.pop("A", None), kw.pop("in_features", 4), 4, **dict({"heads": 1}, **kw))
    layer = M.PGAT(None, 4, 4, heads=1, norm="node")
    assert torch.equal(layer.ln_weight, torch.ones(4)) and torch.equal(layer.ln_bias, torch.zeros(4))
    started = []
    Proc = type("Proc", (), {"exitcode": 0, "__init__": lambda self, target=None, args=(): started.append(args),
                             "start": lambda self: None, "join": lambda self: None})
    monkeypatch.setattr(M.mp, "Process", Proc)
    monkeypatch.setattr(M.mp, "set_start_method", lambda *a, **k: None)
    files = {k: str(tmp_path / (k + ".npy")) for k in ("features", "labels", "split")}
    for v in files.values():
        np.save(v, np.zeros((2, 2), np.float32))
    flags = ["-a", "A.mtx", "-p", "A.part"] + [a for k, v in files.items() for a in ("--" + k, v)]
    saved = (M.path_A, M.path_partvec, M.mode, M.heads)
    M.mode, M.heads = "standard", 2                 # (the module's state is whatever the test before left)
    try:
        with pytest.raises(ValueError, match="belongs to PGCN"):
            M.run(0, 1, 2, 4, "A.mtx", "pv", "gloo", features="x", labels="y", split="s", norm="batch")
        with pytest.raises(ValueError, match="go together"):
            M.run(0, 1, 2, 4, "A.mtx", "pv", "gloo", norm="node")
        for args, text in ((["--norm", "batch"], "belongs to PGCN.py"), (["--norm", "node", "--residual"], "need them); got --norm, --residual")):
            with pytest.raises(SystemExit) as e:
                M.main(["-a", "A.mtx", "-p", "A.part"] + args)
            out = capsys.readouterr().out
            assert e.value.code == 2 and text in out and len(out.strip().splitlines()) == 1, out
        for more in ([], ["--norm", "node", "--residual"], ["--norm", "none"]):      # forwarded when given, and nothing else
            M.main(flags + more)
        plain, off, on = (M._architecture(6, 2, 3, "single", 8, 1, 0.0, 0, None, **kw) for kw in ({}, {"norm": "none", "residual": False}, ON))
    finally:
        M.path_A, M.path_partvec, M.mode, M.heads = saved
    assert [a[-1] for a in started] == [files, dict(files, **ON), dict(files, norm="none")] and len({len(a) for a in started}) == 1
    assert off == plain and (plain["norm"], plain["residual"]) == ("none", False) and (on["norm"], on["residual"]) == ("node", True)
    assert {k: v for k, v in on.items() if k not in ON} == {k: v for k, v in plain.items() if k not in ON}
    with pytest.raises(ValueError, match="norm differs"):
        C.check({"launcher": "PGAT", "arch": on, "optimizer": {"kind": "torch"}}, "PGAT", plain, "torch")


def test_one_and_two_ranks_train_the_same_model_and_resume_is_exact(tmp_path):
    """Three layers with norm, residual and dropout 0.5 on cora.A.mtx with the committed part vectors and a planted two-class problem: 1
    and 2 gloo ranks report the same losses (the tail is row-local, the masks a function of the global ids); 2 + 2 epochs through a
    checkpoint equal 4 epochs bit for bit; another norm is refused by name."""
    n, rng = 2708, np.random.default_rng(3)
    y = (np.arange(n) % 2).astype(np.int64)
    data = {"features": (rng.standard_normal((2, 8))[y] + 0.8 * rng.standard_normal((n, 8))).astype(np.float32), "labels": y,
            "split": np.array([1, 2, 3] * n, np.uint8)[:n]}
    paths = {"A": gpath("cora.A.mtx"), "pv1": gpath("cora.A.mtx.1.rp"), "pv2": gpath("cora.A.mtx.2.rp"),
             "single": {k: str(tmp_path / (k + ".npy")) for k in data}}
    for k, v in data.items():
        np.save(paths["single"][k], v)
    opts = GT.options(K=2, hidden=8, Ko=1, bias=True, dropout=0.5, nlayers=3)

    def train(P, epochs, **extra):
        return AW.spawn(AW.run_worker, P, paths, False, attn=None, extra=dict(ON, **extra), opts=opts, params=None, epochs=epochs, lr=0.01)[0]

    ck = str(tmp_path / "two.ckpt")
    whole, two = train(1, 4), train(2, 4)
    losses = lambda r: ["%.4f" % h["loss"] for h in r["history"]]
    print("1 rank:", losses(whole), "2 ranks:", losses(two))
    assert len(whole["history"]) == 4 and losses(whole) == losses(two) and whole["widths"] == [8, 8, 8, 2]
    train(1, 2, save=ck)
    rest = train(1, 2, load=ck)
    assert np.array_equal(rest["eval_logits"].view(np.int32), whole["eval_logits"].view(np.int32)) and rest["history"] == whole["history"]
    arch = torch.load(ck, weights_only=True)["arch"]
    assert (arch["norm"], arch["residual"]) == ("node", True)
    with pytest.raises(ValueError, match="norm differs"):
        pkg("checkpoint").load(ck, "PGAT", dict(arch, norm="none"), "torch")
