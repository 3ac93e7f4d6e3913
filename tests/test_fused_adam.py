"""The fused Adam / AdamW step (csrc/pgcn_optim.hip: pgcn_adam_step_f32, optim.FlatAdam, run(weight_decay=, decoupled_decay=,
optimizer=), --weight-decay / --adamw / --optimizer) -- the CPU side: the float64 definition against torch's own optimisers, the framework
composition against it, the arena, the entry point's refusals (nothing launches: no device needed), the data loop over gloo with the
checker-backed kernels against a float64 restatement, and the command line.  The kernel is held in test_fused_adam_gpu.py.

Tolerance of every fp32 comparison (F.errors_and_bound): against float64, the error may be twice that of torch's own fp32 optimiser on
the same inputs plus one rounding of the value, 2 e_torch + 2^-23 max(1, max |p|).  Both errors are printed before the assertion."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _fused_adam_workers as F
import _nodeclass_workers as W
from conftest import gpath, pkg

MODES = [(0.0, False), (F.WD, False), (0.0, True), (F.WD, True)]


# ---- the definition ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(7, 50), (16, 7)])
@pytest.mark.parametrize("wd,decoupled", MODES)
def test_adam64_is_torch_adam_in_float64(shape, wd, decoupled):
    n = shape[0] * shape[1]
    rng = np.random.default_rng(n)
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) for _ in range(5)]
    want = F.torch_steps(p0, grads, "cpu", dtype=torch.float64, weight_decay=wd, decoupled=decoupled)
    got = F.reference_steps(p0, grads, weight_decay=wd, decoupled=decoupled)
    for name, a, b in zip("pmv", got, want):
        rel = float(np.abs(a - b).max() / np.abs(b).max())
        print("%s wd %g decoupled %s: %s relative difference %.3g" % (shape, wd, decoupled, name, rel))
        assert rel <= 1e-12


@pytest.mark.parametrize("wd,decoupled", MODES)
@pytest.mark.parametrize("grad_scale", [1.0, F.THIRD])
def test_composition_against_float64(wd, decoupled, grad_scale):
    optim = pkg("optim")
    n = 7 * 50 + 16 * 7
    p0, grads = F.make_case(n, 5, seed=n)
    hyper = dict(weight_decay=wd, decoupled=decoupled, grad_scale=grad_scale)
    ref = F.reference_steps(p0, grads, **hyper)
    yard = F.torch_steps(p0, grads, "cpu", **hyper)
    p, m, v = torch.from_numpy(p0.copy()), torch.zeros(n), torch.zeros(n)
    step = torch.zeros(1, dtype=torch.int64)
    for g in grads:
        gt = torch.from_numpy(g.copy())
        optim.adam_step_composed(p, gt, m, v, step, F.LR, F.BETAS, F.EPS, wd, decoupled, grad_scale, True)
        assert not gt.any()                                         # zeroed in place
        step.add_(1)
    for name, got, y, r in zip("pmv", (p, m, v), yard, ref):
        e, e_torch, bound = F.errors_and_bound(got.numpy(), y, r)
        print("wd %g decoupled %s scale %.3g: %s e_composed %.3g e_torch %.3g bound %.3g" % (wd, decoupled, grad_scale, name, e, e_torch, bound))
        assert e <= bound
    g = torch.from_numpy(grads[0].copy())
    optim.adam_step_composed(p, g, m, v, step, F.LR, F.BETAS, F.EPS, wd, decoupled, grad_scale, False)
    assert np.array_equal(g.numpy(), grads[0])                      # zero_grad off: untouched


# ---- the arena -------------------------------------------------------------------------------------------------------------------------

def _model():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(50, 7, bias=False), torch.nn.Linear(7, 16, bias=True))


def _inside(view, flat):
    off = view.data_ptr() - flat.data_ptr()
    return 0 <= off and off + 4 * view.numel() <= 4 * flat.numel() and off % 256 == 0


def _padding(opt):
    pad = torch.ones(opt.numel, dtype=torch.bool)
    for p, o in zip(opt.params, opt.offsets):
        pad[o:o + p.numel()] = False
    return pad


def test_arena_layout_aliasing_padding_and_state():
    optim = pkg("optim")
    model = _model()
    before = [p.detach().clone() for p in model.parameters()]
    opt = optim.FlatAdam(model.parameters(), lr=F.LR, weight_decay=F.WD)
    params = list(model.parameters())
    assert opt.numel == 384 + 128 + 64 and opt.offsets == [0, 384, 512]          # 350, 112 and 16 floats in segments of 64
    for p, b in zip(params, before):
        assert torch.equal(p.data, b) and p.data.is_contiguous()
        assert _inside(p.data, opt.flat_p) and _inside(p.grad, opt.flat_g)
        assert p.data_ptr() - opt.flat_p.data_ptr() == p.grad.data_ptr() - opt.flat_g.data_ptr()
    assert not opt.flat_g.any() and not opt.exp_avg.any() and not opt.exp_avg_sq.any()
    pad = _padding(opt)
    assert int(pad.sum()) == 34 + 16 + 48 and not opt.flat_p[pad].any()
    x = torch.randn(5, 50)
    ptrs = [p.grad.data_ptr() for p in params]
    for it in range(3):
        model(x).square().sum().backward()
        assert [p.grad.data_ptr() for p in params] == ptrs          # autograd added in place
        assert opt.flat_g[~pad].abs().sum() > 0 and not opt.flat_g[pad].any()
        opt.reduce_gradients(average=False)                         # (one rank: no collective)
        opt.step()
        assert not opt.flat_g.any() and int(opt.step_count) == it + 1
        for buf in (opt.flat_p, opt.flat_g, opt.exp_avg, opt.exp_avg_sq):
            assert not buf[pad].any()                               # p = g = m = v = 0 maps to itself, decay on
    assert [p.data_ptr() - opt.flat_p.data_ptr() for p in params] == [4 * o for o in opt.offsets]
    # accumulation over two backwards, then zero_grad
    model(x).square().sum().backward()
    once = opt.flat_g.clone()
    model(x).square().sum().backward()
    assert torch.allclose(opt.flat_g, 2 * once, rtol=1e-6, atol=0)
    opt.zero_grad()
    assert not opt.flat_g.any()
    # state: a round trip into a second optimiser, then both take the same step
    sd = opt.state_dict()
    assert sd["step"] == 3 and sorted(sd["state"]) == [0, 1, 2]
    assert all(_inside(sd["state"][i]["exp_avg"], opt.exp_avg) and sd["state"][i]["exp_avg"].shape == params[i].shape for i in range(3))
    twin = _model()
    twin.load_state_dict(model.state_dict())
    opt2 = optim.FlatAdam(twin.parameters(), lr=F.LR, weight_decay=F.WD)
    opt2.load_state_dict(sd)
    assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq) and int(opt2.step_count) == 3
    for mdl, o in ((model, opt), (twin, opt2)):
        mdl(x).square().sum().backward()
        o.step()
    assert torch.equal(opt2.flat_p, opt.flat_p)


@pytest.mark.parametrize("wd,decoupled", [(F.WD, False), (F.WD, True)])
def test_flat_adam_and_torch_from_the_same_state(wd, decoupled):
    """state_dict() starts a torch optimiser where this one stands: two more steps of each stay within the tolerance of the float64
    definition started from the same state."""
    optim = pkg("optim")
    model, twin = _model(), _model()
    opt = optim.FlatAdam(model.parameters(), lr=F.LR, weight_decay=wd, decoupled=decoupled)
    xs = [torch.randn(5, 50, generator=torch.Generator().manual_seed(s)) for s in range(4)]
    for x in xs[:2]:
        model(x).square().sum().backward()
        opt.step()
    twin.load_state_dict(model.state_dict())
    sd = opt.state_dict()
    topt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(twin.parameters(), lr=F.LR, weight_decay=wd)
    for i, p in enumerate(twin.parameters()):
        topt.state[p] = {"step": torch.tensor(float(sd["step"])), "exp_avg": sd["state"][i]["exp_avg"].clone(),
                         "exp_avg_sq": sd["state"][i]["exp_avg_sq"].clone()}
    ref = [(p.detach().double().numpy().copy(), sd["state"][i]["exp_avg"].double().numpy().copy(),
            sd["state"][i]["exp_avg_sq"].double().numpy().copy()) for i, p in enumerate(model.parameters())]
    for k, x in enumerate(xs[2:]):
        model(x).square().sum().backward()
        grads = [p.grad.detach().clone() for p in model.parameters()]
        for p, g in zip(twin.parameters(), grads):                  # the same fp32 gradients for all three
            p.grad = g.clone()
        ref = [F.adam64(r[0], g.numpy(), r[1], r[2], sd["step"] + k + 1, weight_decay=wd, decoupled=decoupled) for r, g in zip(ref, grads)]
        opt.step()
        topt.step()
    for p, q, r in zip(model.parameters(), twin.parameters(), ref):
        e, e_torch, bound = F.errors_and_bound(p.detach().numpy(), q.detach().numpy(), r[0])
        print("decoupled %s: e_flat %.3g e_torch %.3g bound %.3g" % (decoupled, e, e_torch, bound))
        assert e <= bound


def test_flat_adam_refuses_what_the_arena_cannot_hold():
    optim = pkg("optim")
    w = torch.nn.Parameter(torch.zeros(3, 3))
    for kw in (dict(lr=-1.0), dict(lr=float("nan")), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.5)), dict(eps=0.0), dict(weight_decay=-1e-3)):
        with pytest.raises(ValueError):
            optim.FlatAdam([w], **kw)
    with pytest.raises(ValueError):
        optim.FlatAdam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError):
        optim.FlatAdam([])


def test_provider_answer_decides_between_kernel_and_composition():
    """A provider whose adam_step answers None (what HipKernels.adam_step does for CPU tensors, another dtype, non-contiguous
    tensors, tensors of different devices) sends the step to the composition; one that answers True is trusted."""
    optim = pkg("optim")
    calls = []

    class Refuses:
        def adam_step(self, *a):
            calls.append(a)
            return None

    class Takes:
        def adam_step(self, *a):
            calls.append(a)
            return True

    for prov, moved in ((Refuses(), True), (Takes(), False), (object(), True)):
        w = torch.nn.Parameter(torch.ones(5))
        opt = optim.FlatAdam([w], lr=0.1, kernels=prov)
        w.grad.fill_(1.0)
        opt.reduce_gradients(average=True)
        opt.step()
        assert bool((w.data != 1.0).all()) == moved and int(opt.step_count) == 1
    assert len(calls) == 2 and calls[0][4] is not None and calls[0][-1] is True and calls[0][-2] == 1.0


def test_binding_answers_none_for_what_the_kernel_does_not_cover():
    """HipKernels.adam_step on a box without a GPU: every tensor is a CPU tensor -> None, before the library is touched."""
    kernels = pkg("kernels")
    k = object.__new__(kernels.HipKernels)                          # (the constructor needs a device; the check under test does not)
    k.device, k.lib = torch.device("cuda:0"), None
    z = torch.zeros(8)
    assert k.adam_step(z, z.clone(), z.clone(), z.clone(), torch.zeros(1, dtype=torch.int64), 1e-3, (0.9, 0.999), 1e-8, 0.0, False, 1.0, True) is None


# ---- the entry point without a device ----------------------------------------------------------------------------------------------------

def test_entry_point_is_exported_and_refuses_bad_arguments_without_a_device():
    _lib = pkg("_lib")
    L = _lib.lib()
    assert "pgcn_adam_step_f32" in _lib.SIGNATURES and hasattr(L, "pgcn_adam_step_f32")
    buf = (ctypes.c_float * 16)()
    step = (ctypes.c_int64 * 1)()
    a = ctypes.addressof(buf)
    s = ctypes.addressof(step)
    ok = dict(n=4, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0)

    def call(p=a, g=a + 16, m=a + 32, v=a + 48, st=s, **kw):
        h = dict(ok, **kw)
        return L.pgcn_adam_step_f32(p, g, m, v, h["n"], h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], 0, 1.0, 1, st, None)

    EINVAL = -1
    assert call(n=0) == _lib.PGCN_OK                               # nothing to do, nothing launched
    assert call(n=0, p=None) == _lib.PGCN_OK
    for bad in (dict(n=-1), dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(st=None), dict(b1=1.0), dict(b2=1.0),
                dict(lr=float("nan")), dict(lr=-1e-3), dict(lr=float("inf")), dict(eps=-1e-8), dict(wd=-5e-4), dict(wd=float("nan")),
                dict(b1=-0.1)):
        assert call(**bad) == EINVAL, bad
        assert b"pgcn_adam_step_f32" in L.pgcn_last_error()
    assert L.pgcn_adam_step_f32(a, a + 16, a + 32, a + 48, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, float("inf"), 1, s, None) == EINVAL
    assert not any(buf)                                             # and nothing was written


# ---- the data loop over gloo ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("fused_adam")))


WIDTHS = [W.FIN, W.HIDDEN, W.CLASSES]


def _check_run(res, yard, reference, data, what):
    ref, final, weights = reference
    worst = W.check_against_reference(res, ref, final, data)         # per-epoch losses within 1e-5 of float64, counts within its near ties
    e, e_torch, bound = F.weight_errors(res, yard, weights)
    print("%s: largest relative loss error %.3g; trained weights e_run %.3g e_torch %.3g bound %.3g" % (what, worst, e, e_torch, bound))
    assert e <= bound
    return worst


def test_fused_and_torch_runs_over_gloo_against_float64(dataset):
    """run(optimizer="fused", weight_decay=5e-4) on 1, 2 and 3 ranks (the composition: the checker-backed provider has no adam_step)
    against the float64 reference written with adam64; run(optimizer="torch") with the same decay as the yardstick of the trained
    weights and held to the same loss bound; the rank counts against each other."""
    paths, data = dataset
    reference = F.float64_reference(data, WIDTHS, weight_decay=F.WD)
    plain = W.float64_reference(data, WIDTHS)[0]
    assert max(abs(a["loss"]["train"] - b["loss"]["train"]) for a, b in zip(reference[0], plain)) > 1e-4      # the decay is felt
    runs = {}
    for P in (1, 2, 3):
        yard = F.spawn_run(P, paths, False, weight_decay=F.WD, optimizer="torch")
        W.check_against_reference(yard, reference[0], reference[1], data)
        runs[P] = F.spawn_run(P, paths, False, weight_decay=F.WD, optimizer="fused")
        _check_run(runs[P], yard, reference, data, "fused, coupled, P = %d" % P)
        assert sorted(runs[P][0]["history"][0]) == sorted(yard[0]["history"][0])       # the same record keys as the torch loop
        assert all(np.array_equal(r["weights"][0], runs[P][0]["weights"][0]) for r in runs[P])        # every rank holds the same weights
    for P in (2, 3):
        for a, b in zip(runs[1][0]["history"], runs[P][0]["history"]):
            assert a["rows"] == b["rows"]
            for name in W.SETS:                                         # both within 1e-5 of the same reference
                assert abs(a["losses"][name] - b["losses"][name]) <= 2e-5 * abs(a["losses"][name])
    lines = runs[1][0]["stdout"].strip().splitlines()
    assert lines[-1].startswith("Best Val ") and len([l for l in lines if l.startswith("Epoch ")]) == W.EPOCHS


def test_decoupled_decay_over_gloo_against_float64(dataset):
    paths, data = dataset
    reference = F.float64_reference(data, WIDTHS, weight_decay=F.WD, decoupled=True)
    coupled = F.float64_reference(data, WIDTHS, weight_decay=F.WD)
    assert max(float(np.abs(a - b).max()) for a, b in zip(reference[2], coupled[2])) > 1e-5            # AdamW is not Adam + L2
    yard = F.spawn_run(2, paths, False, weight_decay=F.WD, decoupled_decay=True, optimizer="torch")
    W.check_against_reference(yard, reference[0], reference[1], data)
    res = F.spawn_run(2, paths, False, weight_decay=F.WD, decoupled_decay=True, optimizer="fused")
    _check_run(res, yard, reference, data, "fused, decoupled, P = 2")


def test_run_refuses_bad_optimiser_options(dataset):
    M = pkg("PGCN")
    paths = dataset[0]
    three = dict(features=paths["features"], labels=paths["labels"], split=paths["split"])
    base = (0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo")
    for kw in (dict(weight_decay=5e-4), dict(decoupled_decay=True), dict(optimizer="fused")):
        with pytest.raises(ValueError, match="need features"):
            M.run(*base, **kw)
    with pytest.raises(ValueError, match="optimizer takes"):
        M.run(*base, optimizer="foo", **three)
    for wd in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight_decay"):
            M.run(*base, weight_decay=wd, **three)


# ---- the command line ------------------------------------------------------------------------------------------------------------------

def _keep_cli_state(monkeypatch, M):
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        if k in os.environ:
            monkeypatch.setenv(k, os.environ[k])
        else:
            monkeypatch.delenv(k, raising=False)
    for name in ("path_A", "path_partvec"):
        monkeypatch.setattr(M, name, getattr(M, name, None), raising=False)


BASE = ["-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"), "-b", "gloo", "-s", "1", "-l", "2", "-f", "16"]
FILES = ["--features", "F", "--labels", "L", "--split", "S"]


@pytest.mark.parametrize("bad", [FILES + ["--weight-decay", "-1"], FILES + ["--weight-decay", "x"], FILES + ["--weight-decay", "nan"],
                                 FILES + ["--optimizer", "foo"], ["--adamw"], ["--weight-decay", "5e-4"], ["--optimizer", "fused"],
                                 ["--features", "F", "--adamw"]])
def test_cli_rejects_bad_or_partial_options(monkeypatch, dataset, bad):
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    paths = dataset[0]
    argv = [{"F": paths["features"], "L": paths["labels"], "S": paths["split"]}.get(a, a) for a in bad]
    with pytest.raises(SystemExit) as e:
        M.main(BASE + argv)
    assert e.value.code == 2


def test_cli_forwards_the_optimiser_options_and_nothing_else(monkeypatch, dataset):
    M = pkg("PGCN")
    _keep_cli_state(monkeypatch, M)
    paths = dataset[0]
    made, seen = [], []

    class InlineProcess:
        def __init__(self, target, args):
            self.target, self.args, self.exitcode = target, args, None
            made.append(args)

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
    three = {"features": paths["features"], "labels": paths["labels"], "split": paths["split"]}
    pos = (0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo")
    # without the new options: exactly the argument tuples of before, in all three forms
    M.main(BASE)
    M.main(BASE + ["--dropout", "0.5"])
    M.main(BASE + files + ["--epochs", "9"])
    head = (0, 1, M.run, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo", None)
    assert made[0] == head
    assert made[1] == head + (0.5, 0)
    assert made[2] == head + (0.0, 0, paths["features"], paths["labels"], paths["split"], None, 9, None, None, None)
    assert seen == [(pos, {}), (pos, {"dropout": 0.5, "dropout_seed": 0}), (pos, dict(three, epochs=9))]
    # with them: appended, and only what was given reaches run
    del made[:], seen[:]
    M.main(BASE + files + ["--weight-decay", "5e-4"])
    M.main(BASE + files + ["--adamw", "--weight-decay", "0.01", "--optimizer", "fused"])
    M.main(BASE + files + ["--optimizer", "torch"])
    assert made[0] == head + (0.0, 0, paths["features"], paths["labels"], paths["split"], None, None, None, None, None, 5e-4, None, None)
    assert seen == [(pos, dict(three, weight_decay=5e-4)),
                    (pos, dict(three, weight_decay=0.01, decoupled_decay=True, optimizer="fused")),
                    (pos, dict(three, optimizer="torch"))]
    # init_process itself, called the old way and with the new keywords
    del seen[:]
    M.init_process(0, 1, M.run, 2, 16, "A", "pv", "gloo")
    M.init_process(0, 1, M.run, 2, 16, "A", "pv", "gloo", weight_decay=5e-4, optimizer="fused")
    assert seen == [((0, 1, 2, 16, "A", "pv", "gloo"), {}), ((0, 1, 2, 16, "A", "pv", "gloo"), {"weight_decay": 5e-4, "optimizer": "fused"})]
