"""Gradient clipping, learning-rate schedules and early stopping (optim.py: lr_at, adam_step_ctl_composed, FlatAdam(max_norm=, schedule=);
nodeloss.Control; run(clip_norm=, lr_schedule=, lr_warmup=, lr_min=, lr_step=, lr_gamma=, lr_horizon=, patience=) and the options of
PGCN.py / PGAT.py) -- the CPU side: the definition at named points, the framework composition against float64, the entry points'
refusals (nothing launches: no device needed), the data loop over gloo with the checker-backed kernels against a float64 restatement,
early stopping, exact resume and the command line.  The kernels are held in test_train_control_gpu.py.

Tolerances are those of test_fused_adam.py (F.errors_and_bound; W.check_against_reference), the yardstick being torch's fp32 Adam with
torch.nn.utils.clip_grad_norm_ and the learning rate set by hand."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _fused_adam_workers as F
import _nodeclass_workers as W
import _train_control_workers as T
from conftest import gpath, pkg

LR_ULPS = 16 * 2.0 ** -53        # the rate formed by tensor operations (another cos / pow) against Python's: a few roundings


# ---- the definition ----------------------------------------------------------------------------------------------------------------

def test_lr_at_named_points():
    optim = pkg("optim")
    base, lr_min, Wm, Tm = 0.02, 0.002, 4, 20
    cos = ("cosine", base, Wm, Tm, lr_min, 1, 1.0)
    assert optim.lr_at(0, cos) == pytest.approx(base / Wm, rel=2 ** -50)              # the first update of the warm-up
    assert optim.lr_at(0, ("constant", base, Wm, 0, 0.0, 1, 1.0)) == base * 1 / Wm
    assert optim.lr_at(Wm - 1, ("constant", base, Wm, 0, 0.0, 1, 1.0)) == base
    assert optim.lr_at(Wm, cos) == pytest.approx(base, rel=2 ** -50)
    assert optim.lr_at(Wm, ("cosine", base, Wm, Tm, 0.0, 1, 1.0)) == base             # (no rounding of base - lr_min: exact)
    assert optim.lr_at((Wm + Tm) // 2, cos) == pytest.approx((base + lr_min) / 2, rel=2 ** -50)
    for t in (Tm, Tm + 1, 10 * Tm):
        assert optim.lr_at(t, cos) == lr_min                                          # exactly
    step = ("step", base, Wm, 0, 0.0, 5, 0.5)
    assert optim.lr_at(Wm + 5 - 1, step) == base and optim.lr_at(Wm + 5, step) == base * 0.5
    assert optim.lr_at(Wm + 10 - 1, step) == base * 0.5 and optim.lr_at(Wm + 10, step) == base * 0.25
    assert optim.lr_at(1, step) == base * 2 / Wm                                      # warm-up scales whatever the kind gives
    for t in range(30):
        for s in (cos, step, ("constant", base, 0, 0, 0.0, 1, 1.0)):
            assert optim.lr_at(t, s) == T.lr64(t, s)                                  # the tests' restatement, bit for bit
            got = float(optim.lr_at_composed(torch.tensor([t]), s))
            assert abs(got - T.lr64(t, s)) <= LR_ULPS * T.lr64(t, s)
    for bad in (("linear", base, 0, 0, 0.0, 1, 1.0), ("cosine", base, 4, 4, 0.0, 1, 1.0), ("cosine", base, 0, 9, 2 * base, 1, 1.0),
                ("step", base, 0, 0, 0.0, 0, 0.5), ("step", base, 0, 0, 0.0, 5, 0.0), ("step", base, 0, 0, 0.0, 5, 1.5),
                ("constant", -1.0, 0, 0, 0.0, 1, 1.0), ("constant", float("nan"), 0, 0, 0.0, 1, 1.0), ("constant", base, -1, 0, 0.0, 1, 1.0),
                ("constant", base, 0.5, 0, 0.0, 1, 1.0), ("constant", base, 0, 0, float("inf"), 1, 1.0), ("constant", base), None):
        with pytest.raises(ValueError):
            optim.lr_at(0, bad)
    w = torch.nn.Parameter(torch.zeros(3))
    for kw in (dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=float("nan")), dict(schedule=("cosine", 0.1, 4, 4, 0.0, 1, 1.0))):
        with pytest.raises(ValueError):
            optim.FlatAdam([w], **kw)


# ---- the composition ----------------------------------------------------------------------------------------------------------------

SCHEDS = [("cosine", F.LR, 2, 4, 1e-3, 1, 1.0), ("step", F.LR, 1, 0, 0.0, 1, 0.5)]


def _composed(optim, p0, grads, sched, max_norm, wd, decoupled, grad_scale=1.0, ctl_call=True):
    n = p0.size
    p, m, v = torch.from_numpy(p0.copy()), torch.zeros(n), torch.zeros(n)
    step, ctl, recs = torch.zeros(1, dtype=torch.int64), torch.zeros(4, dtype=torch.float64), []
    for g in grads:
        gt = torch.from_numpy(g.copy())
        if ctl_call:
            optim.adam_step_ctl_composed(p, gt, m, v, step, sched, max_norm, ctl, F.BETAS, F.EPS, wd, decoupled, grad_scale, True)
            recs.append(ctl.tolist())
        else:
            optim.adam_step_composed(p, gt, m, v, step, sched[1], F.BETAS, F.EPS, wd, decoupled, grad_scale, True)
        assert not gt.any()
        step.add_(1)
    return (p, m, v), recs


@pytest.mark.parametrize("n", [1, 5, 1025, 4099])
@pytest.mark.parametrize("wd,decoupled", [(F.WD, False), (F.WD, True)])
def test_composed_ctl_step_against_float64(n, wd, decoupled):
    optim = pkg("optim")
    p0, grads = F.make_case(n, 3, seed=n)
    norms = [T.clip64([g], None, F.THIRD)[1] for g in grads]
    max_norm = 0.5 * (min(norms) + max(norms)) if n > 1 else 0.5 * max(norms)          # some steps clip, some do not
    for sched in SCHEDS:
        hyper = dict(weight_decay=wd, decoupled=decoupled, grad_scale=F.THIRD)
        ref, recs = T.reference_steps(p0, grads, sched, max_norm, **hyper)
        assert any(r[2] < 1.0 for r in recs) and (n == 1 or any(r[2] == 1.0 for r in recs))
        yard = T.torch_steps(p0, grads, "cpu", sched, max_norm, **hyper)
        got, ctls = _composed(optim, p0, grads, sched, max_norm, wd, decoupled, F.THIRD)
        for name, a, y, r in zip("pmv", got, yard, ref):
            e, e_torch, bound = F.errors_and_bound(a.numpy(), y, r)
            print("n %d %s wd %g decoupled %s: %s e_composed %.3g e_torch %.3g bound %.3g" % (n, sched[0], wd, decoupled, name, e, e_torch, bound))
            assert e <= bound
        for c, r in zip(ctls, recs):
            assert abs(c[0] - r[0]) <= n * 2.0 ** -52 * r[0] and abs(c[1] - r[1]) <= n * 2.0 ** -52 * r[1]
            assert abs(c[2] - r[2]) <= n * 2.0 ** -51 * r[2] and (c[2] == 1.0) == (r[2] == 1.0)
            assert abs(c[3] - r[3]) <= LR_ULPS * r[3]


@pytest.mark.parametrize("wd,decoupled", [(F.WD, False), (F.WD, True)])
def test_composed_ctl_step_bit_equalities(wd, decoupled):
    """Neutral options: the bits of adam_step_composed.  max_norm above every norm (coef == 1): the bits of the unclipped step."""
    optim = pkg("optim")
    n = 1025
    p0, grads = F.make_case(n, 3, seed=3)
    plain, _ = _composed(optim, p0, grads, ("constant", F.LR), None, wd, decoupled, F.THIRD, ctl_call=False)
    neutral, recs = _composed(optim, p0, grads, optim.constant_schedule(F.LR), None, wd, decoupled, F.THIRD)
    assert all(r == [0.0, 0.0, 1.0, F.LR] for r in recs)
    for a, b in zip(plain, neutral):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    sched = SCHEDS[0]
    loose, recs = _composed(optim, p0, grads, sched, 1e6, wd, decoupled, F.THIRD)
    unclipped, _ = _composed(optim, p0, grads, sched, None, wd, decoupled, F.THIRD)
    assert all(r[2] == 1.0 and r[1] > 0.0 for r in recs)
    for a, b in zip(loose, unclipped):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_flat_adam_under_control_and_its_record():
    """FlatAdam(max_norm=, schedule=) on CPU tensors: the composition; control() returns the record; without either option step()
    makes today's call and control() answers None."""
    optim = pkg("optim")
    calls = []

    class Takes:
        def adam_step(self, *a):
            calls.append(a)
            return True

    w = torch.nn.Parameter(torch.ones(5))
    opt = optim.FlatAdam([w], lr=0.1, kernels=Takes())
    w.grad.fill_(1.0)
    opt.step()
    assert len(calls) == 1 and len(calls[0]) == 12 and calls[0][5] == 0.1 and opt.control() is None and opt.ctl is None and opt.partial is None
    sched = ("cosine", 0.1, 2, 6, 0.0, 1, 1.0)
    w = torch.nn.Parameter(torch.ones(5))
    opt = optim.FlatAdam([w], lr=0.5, max_norm=1.0, schedule=sched)
    assert opt.lr == 0.1                                            # the schedule's base replaces lr
    for t in range(3):
        w.grad.fill_(3.0)
        opt.step()
        rec = opt.control()
        assert rec["sumsq"] == 45.0 and rec["gnorm"] == math.sqrt(45.0) and rec["clip"] == 1.0 / (math.sqrt(45.0) + 1e-6)
        assert abs(rec["lr"] - optim.lr_at(t, sched)) <= LR_ULPS * rec["lr"]
        assert not opt.flat_g.any() and not opt.flat_p[5:].any()   # cleared; the padding stays zero under the clip
    assert int(opt.step_count) == 3


# ---- the entry points without a device ----------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_refuse_bad_arguments_without_a_device():
    _lib = pkg("_lib")
    L = _lib.lib()
    for name in ("pgcn_grad_sumsq_parts", "pgcn_grad_sumsq_f32", "pgcn_adam_step_ctl_f32"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.pgcn_abi_version() == 3
    parts = L.pgcn_grad_sumsq_parts
    assert [parts(n) for n in (-1, 0, 1, 1024, 1025, 2048, 2049, 256 * 1024, 256 * 1024 + 1, 1 << 33)] == [0, 0, 1, 1, 2, 2, 3, 256, 256, 256]
    buf = (ctypes.c_float * 16)()
    dbl = (ctypes.c_double * 8)()
    step = (ctypes.c_int64 * 1)()
    a, d, s = ctypes.addressof(buf), ctypes.addressof(dbl), ctypes.addressof(step)
    ok = dict(n=4, kind=0, base=1e-3, W=0.0, T=0.0, lr_min=0.0, S=1.0, gamma=1.0, max_norm=0.0, partial=d, parts=1, ctl=d + 32, b1=0.9,
              b2=0.999, eps=1e-8, wd=0.0, gs=1.0, p=a, g=a + 16, m=a + 32, v=a + 48, st=s)

    def call(**kw):
        h = dict(ok, **kw)
        return L.pgcn_adam_step_ctl_f32(h["p"], h["g"], h["m"], h["v"], h["n"], h["kind"], h["base"], h["W"], h["T"], h["lr_min"], h["S"],
                                        h["gamma"], h["max_norm"], h["partial"], h["parts"], h["ctl"], h["b1"], h["b2"], h["eps"], h["wd"], 0,
                                        h["gs"], 1, h["st"], None)

    EINVAL = -1
    assert call(n=0) == _lib.PGCN_OK and call(n=0, p=None, partial=None) == _lib.PGCN_OK            # nothing to do, nothing launched
    nan, inf = float("nan"), float("inf")
    bad = [dict(kind=3), dict(kind=-1)]
    bad += [{k: x} for k in ("base", "W", "T", "lr_min", "S", "gamma") for x in (nan, inf, -1.0)]    # a schedule value
    bad += [dict(kind=1, W=4.0, T=4.0), dict(kind=1, W=4.0, T=3.0), dict(kind=1, T=9.0, lr_min=1.0)]  # cosine: T <= W; lr_min > base
    bad += [dict(S=0.0), dict(S=0.5), dict(kind=2, S=0.0), dict(kind=2, gamma=0.0), dict(kind=2, gamma=1.5)]
    bad += [dict(max_norm=-1.0), dict(max_norm=nan)]
    bad += [dict(ctl=None), dict(ctl=d + 36), dict(st=None), dict(st=s + 4)]                          # null or misaligned
    bad += [dict(max_norm=1.0, partial=None), dict(max_norm=1.0, partial=d + 4), dict(max_norm=1.0, parts=2), dict(max_norm=1.0, parts=0)]
    bad += [dict(n=1025, max_norm=1.0, parts=1), dict(n=-1), dict(p=None), dict(g=None), dict(m=None), dict(v=None)]
    bad += [dict(b1=1.0), dict(b2=1.0), dict(eps=-1e-8), dict(wd=nan), dict(gs=inf)]                  # what pgcn_adam_step_f32 refuses
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert b"pgcn_adam_step_ctl_f32" in L.pgcn_last_error()
    sumsq = lambda g=a, n=4, partial=d, parts=1: L.pgcn_grad_sumsq_f32(g, n, partial, parts, None)
    assert sumsq(n=0, parts=0) == _lib.PGCN_OK and sumsq(g=None, n=0, partial=None, parts=0) == _lib.PGCN_OK
    for kw in (dict(n=-1), dict(parts=2), dict(parts=0), dict(n=1025, parts=1), dict(g=None), dict(partial=None), dict(partial=d + 4), dict(g=a + 2)):
        assert sumsq(**kw) == EINVAL, kw
        assert b"pgcn_grad_sumsq_f32" in L.pgcn_last_error()
    assert not any(buf) and not any(dbl)                            # and nothing was written


def test_bindings_answer_none_for_what_the_kernels_do_not_cover():
    """HipKernels.grad_sumsq / adam_step_ctl on a box without a GPU: every tensor is a CPU tensor -> None, before the library is
    touched."""
    kernels, optim = pkg("kernels"), pkg("optim")
    k = object.__new__(kernels.HipKernels)
    k.device, k.lib = torch.device("cuda:0"), None
    z = torch.zeros(8)
    assert k.grad_sumsq(z) is None
    assert k.adam_step_ctl(z, z.clone(), z.clone(), z.clone(), torch.zeros(1, dtype=torch.int64), optim.constant_schedule(1e-3), 1.0,
                           torch.zeros(1, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), (0.9, 0.999), 1e-8, 0.0, False, 1.0,
                           True) is None


# ---- the stop rule ---------------------------------------------------------------------------------------------------------------------

def test_stop_rule_counts_reports_after_the_best_by_strict_greater():
    nodeloss = pkg("nodeloss")
    c = nodeloss.Control({"patience": 2}, 0.01)
    h = lambda *vals: [{"epoch": 2 * i, "val": v} for i, v in enumerate(vals)]
    assert not c.stop([]) and not c.stop(h(0.5)) and not c.stop(h(0.5, 0.5)) and c.stop(h(0.5, 0.5, 0.5))         # a tie does not beat
    assert not c.stop(h(0.5, 0.4, 0.6)) and not c.stop(h(0.5, 0.4, 0.6, 0.6)) and c.stop(h(0.5, 0.4, 0.6, 0.6, 0.1))
    assert c.stop(h(float("nan"), 0.5, 0.6))                        # report keeps a first NaN as the best: nothing beats it
    assert not nodeloss.Control({"clip_norm": 1.0}, 0.01).stop(h(0.5, 0.5, 0.5, 0.5))
    for vals in ((0.1, 0.2, 0.2, 0.15, 0.3), (0.3, 0.1, 0.1), (0.1, 0.2, 0.3)):
        hist = h(*vals)
        stops = [e["epoch"] for i, e in enumerate(hist) if c.stop(hist[:i + 1])]
        assert (stops[0] if stops else None) == T.stop_epoch(vals, [e["epoch"] for e in hist], 2)


# ---- the data loop over gloo -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("train_control")))


WIDTHS = [W.FIN, W.HIDDEN, W.CLASSES]
WARMUP, LR_MIN = 3, 0.002
SCHED = ("cosine", W.LR, WARMUP, W.EPOCHS, LR_MIN, 1, 1.0)
CONTROL = dict(lr_schedule="cosine", lr_warmup=WARMUP, lr_min=LR_MIN)


@pytest.fixture(scope="module")
def clipped(dataset):
    """max_norm halfway between the smallest and the largest gradient norm of the float64 run under the schedule, and the float64 run
    under schedule and clip: at least one epoch clips, at least one does not, none within 1e-3 of the threshold."""
    data = dataset[1]
    norms = [c[0] for c in T.float64_reference(data, WIDTHS, sched=SCHED, weight_decay=F.WD)[3]]
    max_norm = 0.5 * (min(norms) + max(norms))
    reference = T.float64_reference(data, WIDTHS, sched=SCHED, max_norm=max_norm, weight_decay=F.WD)
    coefs = [c[1] for c in reference[3]]
    print("max_norm %.6g; float64 norms %s" % (max_norm, " ".join("%.4f" % c[0] for c in reference[3])))
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs)
    assert all(abs(c[0] - max_norm) > 1e-3 * max_norm for c in reference[3])
    return max_norm, reference


def check_control_history(optim, res, reference, exact_lr):
    for r in res:
        assert [h["epoch"] for h in r["history"]] == list(range(W.EPOCHS))
        for h, (norm, coef, lr) in zip(r["history"], reference[3]):
            assert sorted(h) == sorted(["epoch", "loss", "train", "val", "test", "losses", "correct", "rows", "lr", "gnorm", "clip"])
            assert lr == optim.lr_at(h["epoch"], SCHED)
            assert h["lr"] == lr if exact_lr else abs(h["lr"] - lr) <= LR_ULPS * lr
            assert abs(h["gnorm"] - norm) <= 1e-4 * norm, (h["epoch"], h["gnorm"], norm)
            assert (h["clip"] < 1.0) == (coef < 1.0) and abs(h["clip"] - coef) <= 1e-4, (h["epoch"], h["clip"], coef)
    assert any(h["clip"] < 1.0 for h in res[0]["history"]) and any(h["clip"] == 1.0 for h in res[0]["history"])


@pytest.mark.parametrize("P", [1, 2])
def test_runs_under_clip_warmup_and_cosine_over_gloo_against_float64(dataset, clipped, P):
    """run(clip_norm=, lr_schedule="cosine", lr_warmup=, lr_min=) with both optimisers (fused: the composition -- the checker-backed
    provider has no adam_step_ctl) against the float64 loop under the same clip and schedule; torch's run is the yardstick of the
    trained weights and held to the same loss bound."""
    optim = pkg("optim")
    paths, data = dataset
    max_norm, reference = clipped
    opts = dict(weight_decay=F.WD, control=dict(CONTROL, clip_norm=max_norm))
    yard = F.spawn_run(P, paths, False, optimizer="torch", **opts)
    W.check_against_reference(yard, reference[0], reference[1], data)
    check_control_history(optim, yard, reference, True)
    res = F.spawn_run(P, paths, False, optimizer="fused", **opts)
    worst = W.check_against_reference(res, reference[0], reference[1], data)
    check_control_history(optim, res, reference, False)
    e, e_torch, bound = F.weight_errors(res, yard, reference[2])
    print("P = %d: largest relative loss error %.3g; trained weights e_run %.3g e_torch %.3g bound %.3g" % (P, worst, e, e_torch, bound))
    assert e <= bound
    assert all(np.array_equal(r["weights"][0], res[0]["weights"][0]) for r in res)
    lines = res[0]["stdout"].strip().splitlines()                   # the printed lines are those of a run without the options
    assert lines[-1].startswith("Best Val ") and len([l for l in lines if l.startswith("Epoch ")]) == W.EPOCHS and "Stopped" not in res[0]["stdout"]


STOP_LR, STOP_EPOCHS, STOP_EVERY, PATIENCE = 0.1, 16, 2, 2


def test_early_stopping_on_two_ranks_and_the_checkpoint(dataset, tmp_path):
    """patience with eval_every = 2: the run stops at the epoch the float64 history predicts, on both ranks; the checkpoint counts the
    epochs completed.  A run without any new option writes the fields and optimiser state keys of before."""
    paths, data = dataset
    ref = F.float64_reference(data, WIDTHS, epochs=STOP_EPOCHS, lr=STOP_LR)[0]
    epochs = T.reported(STOP_EPOCHS, STOP_EVERY)
    vals = [ref[e]["correct"]["val"] / ref[e]["rows"]["val"] for e in epochs]
    stop = T.stop_epoch(vals, epochs, PATIENCE)
    print("float64 Val at the reported epochs: %s; stop at %s" % (" ".join("%.4f" % v for v in vals), stop))
    assert stop is not None and stop < STOP_EPOCHS - 2
    # the prediction does not hang on a near tie: the best report beats every other by more than the rows that may fall either way
    at = int(np.argmax(vals))
    near = [ref[e]["near"]["val"] for e in epochs]
    assert all(abs(vals[at] - v) * ref[0]["rows"]["val"] > near[at] + near[i] for i, v in enumerate(vals) if i != at and epochs[i] <= stop)
    ck = str(tmp_path / "stopped.pt")
    res = F.spawn_run(2, paths, False, optimizer="fused", lr=STOP_LR, epochs=STOP_EPOCHS, eval_every=STOP_EVERY, save=ck,
                      control=dict(patience=PATIENCE))
    for r in res:                                                   # both ranks
        assert [h["epoch"] for h in r["history"]] == [e for e in epochs if e <= stop]
        assert sorted(r["history"][0]) == sorted(["epoch", "loss", "train", "val", "test", "losses", "correct", "rows"])      # patience adds nothing
    out = res[0]["stdout"]
    assert "Stopped early at epoch %05d: no better Val in %d reports" % (stop, PATIENCE) in out
    assert len([l for l in out.splitlines() if l.startswith("Epoch ")]) == len(res[0]["history"])
    saved = torch.load(ck, map_location="cpu", weights_only=True)
    assert saved["epochs"] == stop + 1 and saved["optimizer"]["state"]["step"] == stop + 1
    assert saved["best"]["entry"]["epoch"] == epochs[at] == res[0]["best"]["epoch"]
    # without the options: the file of before
    plain = str(tmp_path / "plain.pt")
    F.spawn_run(1, paths, False, optimizer="fused", epochs=2, save=plain)
    saved = torch.load(plain, map_location="cpu", weights_only=True)
    assert sorted(saved) == sorted(["format", "launcher", "arch", "model", "optimizer", "epochs", "dropout_step", "history", "best"])
    assert saved["format"] == 1 and sorted(saved["optimizer"]) == ["kind", "state"] and sorted(saved["optimizer"]["state"]) == ["state", "step"]
    assert sorted(saved["optimizer"]["state"]["state"][0]) == ["exp_avg", "exp_avg_sq"]
    assert sorted(saved["history"][0]) == sorted(["epoch", "loss", "train", "val", "test", "losses", "correct", "rows"])


@pytest.mark.parametrize("optimizer", ["torch", "fused"])
def test_exact_resume_under_the_schedule(dataset, clipped, tmp_path, optimizer):
    """6 epochs straight against 3 (lr_horizon = 6) + 3 resumed, cosine + warm-up + clip: weights, moments and history bit for bit."""
    paths = dataset[0]
    control = dict(lr_schedule="cosine", lr_warmup=2, lr_min=LR_MIN, clip_norm=clipped[0])
    files = {k: str(tmp_path / (k + ".pt")) for k in ("straight", "half", "resumed")}
    opts = dict(optimizer=optimizer, weight_decay=F.WD)
    F.spawn_run(1, paths, False, epochs=6, save=files["straight"], control=control, **opts)
    F.spawn_run(1, paths, False, epochs=3, save=files["half"], control=dict(control, lr_horizon=6), **opts)
    F.spawn_run(1, paths, False, epochs=3, load=files["half"], save=files["resumed"], control=control, **opts)     # horizon: 3 + 3
    a, b = (torch.load(files[k], map_location="cpu", weights_only=True) for k in ("straight", "resumed"))
    assert a["epochs"] == b["epochs"] == 6

    def same(x, y):
        if isinstance(x, torch.Tensor):
            return x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.dtype is torch.float32 else x, y.view(torch.int32) if y.dtype is torch.float32 else y)
        if isinstance(x, dict):
            return sorted(x, key=str) == sorted(y, key=str) and all(same(x[k], y[k]) for k in x)
        if isinstance(x, (list, tuple)):
            return len(x) == len(y) and all(same(u, w) for u, w in zip(x, y))
        return x == y or (x != x and y != y)

    assert same(a["model"], b["model"]) and same(a["optimizer"], b["optimizer"])
    assert same(a["history"], b["history"]) and same(a["best"], b["best"])
    assert [h["epoch"] for h in a["history"]] == list(range(6)) and "lr" in a["history"][0] and "clip" in a["history"][0]


def test_run_refuses_bad_control_options(dataset):
    M = pkg("PGCN")
    paths = dataset[0]
    three = dict(features=paths["features"], labels=paths["labels"], split=paths["split"])
    base = (0, 1, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo")
    for kw in (dict(clip_norm=1.0), dict(lr_schedule="cosine"), dict(lr_warmup=2), dict(patience=3)):
        with pytest.raises(ValueError, match="need features, labels and split"):
            M.run(*base, **kw)
    for kw, text in ((dict(clip_norm=0.0), "clip_norm takes"), (dict(clip_norm=float("nan")), "clip_norm takes"), (dict(clip_norm="x"), "clip_norm takes"),
                     (dict(lr_schedule="linear"), "lr_schedule takes"), (dict(lr_warmup=-1), "lr_warmup takes"), (dict(lr_warmup=1.5), "lr_warmup takes"),
                     (dict(lr_schedule="cosine", lr_min=-1.0), "lr_min takes"), (dict(lr_schedule="cosine", lr_min=1.0), "lr_min takes"),
                     (dict(lr_schedule="step", lr_step=0), "lr_step takes"), (dict(lr_schedule="step", lr_step=2, lr_gamma=0.0), "lr_gamma takes"),
                     (dict(lr_schedule="step", lr_step=2, lr_gamma=1.5), "lr_gamma takes"), (dict(lr_schedule="cosine", lr_horizon=0), "lr_horizon takes"),
                     (dict(patience=0), "patience takes"), (dict(lr_min=1e-4), "lr_min needs lr_schedule=cosine"),
                     (dict(lr_step=2), "lr_step needs lr_schedule=step"), (dict(lr_schedule="step"), "needs lr_step"),
                     (dict(lr_schedule="cosine", lr_warmup=4, epochs=4), "must be above lr_warmup"),
                     (dict(lr_schedule="cosine", lr_warmup=4, lr_horizon=3), "must be above lr_warmup")):
        with pytest.raises(ValueError, match=text):
            M.run(*base, **dict(three, **kw))
    with pytest.raises(TypeError):
        M.run(*base, clip=1.0, **three)


# ---- the command line ------------------------------------------------------------------------------------------------------------------

def _keep_cli_state(monkeypatch, M):
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        if k in os.environ:
            monkeypatch.setenv(k, os.environ[k])
        else:
            monkeypatch.delenv(k, raising=False)
    for name in ("path_A", "path_partvec", "mode", "heads"):
        if hasattr(M, name) or name.startswith("path"):
            monkeypatch.setattr(M, name, getattr(M, name, None), raising=False)


BASE = ["-a", gpath("karate.mtx"), "-p", gpath("karate.mtx.1.rp"), "-b", "gloo", "-s", "1", "-l", "2", "-f", "16"]
FILES = ["--features", "F", "--labels", "L", "--split", "S"]
BAD = [(FILES + ["--clip-norm", "0"], "--clip-norm takes"), (FILES + ["--clip-norm", "x"], "--clip-norm takes"),
       (FILES + ["--clip-norm", "inf"], "--clip-norm takes"), (FILES + ["--lr-schedule", "linear"], "--lr-schedule takes"),
       (FILES + ["--lr-warmup", "-1"], "--lr-warmup takes"), (FILES + ["--lr-warmup", "1.5"], "--lr-warmup takes"),
       (FILES + ["--lr-schedule", "cosine", "--lr-min", "-1"], "--lr-min takes"), (FILES + ["--lr-schedule", "cosine", "--lr-min", "1"], "--lr-min takes"),
       (FILES + ["--lr-schedule", "step", "--lr-step", "0"], "--lr-step takes"), (FILES + ["--lr-schedule", "step", "--lr-step", "2", "--lr-gamma", "0"], "--lr-gamma takes"),
       (FILES + ["--lr-schedule", "cosine", "--lr-horizon", "0"], "--lr-horizon takes"), (FILES + ["--patience", "0"], "--patience takes"),
       (FILES + ["--patience", "two"], "--patience takes"), (FILES + ["--lr-min", "1e-4"], "--lr-min needs --lr-schedule cosine"),
       (FILES + ["--lr-schedule", "step"], "needs --lr-step"), (FILES + ["--lr-schedule", "cosine", "--lr-warmup", "4", "--epochs", "4"], "must be above --lr-warmup"),
       (["--clip-norm", "1"], "need them"), (["--lr-schedule", "cosine"], "need them"), (["--lr-warmup", "2"], "need them"), (["--lr-min", "0"], "need them"),
       (["--lr-step", "2"], "need them"), (["--lr-gamma", "0.5"], "need them"), (["--lr-horizon", "9"], "need them"), (["--patience", "3"], "need them"),
       (["--features", "F", "--patience", "3"], "need them")]


@pytest.mark.parametrize("launcher", ["PGCN", "PGAT"])
@pytest.mark.parametrize("bad,text", BAD)
def test_cli_rejects_bad_or_partial_options(monkeypatch, capsys, dataset, launcher, bad, text):
    M = pkg(launcher)
    _keep_cli_state(monkeypatch, M)
    if launcher == "PGAT":
        monkeypatch.setattr(M, "mode", "standard")                 # (a module global that an earlier test's --mode may have left)
    paths = dataset[0]
    argv = [{"F": paths["features"], "L": paths["labels"], "S": paths["split"]}.get(a, a) for a in bad]
    with pytest.raises(SystemExit) as e:
        M.main(BASE + argv)
    out = capsys.readouterr().out
    assert e.value.code == 2 and text in out, out
    if text == "need them":
        assert bad[-2] in out.split("got")[1]
        assert ("--norm, --residual, --root-weight, --bias need them" in out) if launcher == "PGCN" else ("--patience need them); got" in out)


def test_pgat_reference_mode_refuses_the_options(monkeypatch, capsys, dataset):
    M = pkg("PGAT")
    _keep_cli_state(monkeypatch, M)
    paths = dataset[0]
    with pytest.raises(SystemExit) as e:
        M.main(BASE + ["--mode", "reference", "--features", paths["features"], "--labels", paths["labels"], "--split", paths["split"], "--clip-norm", "1"])
    assert e.value.code == 2 and "--mode reference" in capsys.readouterr().out
    monkeypatch.setattr(M, "mode", "reference")
    with pytest.raises(ValueError, match="reference layer"):
        M.run(0, 1, 1, 4, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo", features=paths["features"], labels=paths["labels"],
              split=paths["split"], clip_norm=1.0)
    with pytest.raises(ValueError, match="need them"):
        M.run(0, 1, 1, 4, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo", patience=2)


def test_cli_forwards_the_control_options_and_nothing_else(monkeypatch, dataset):
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
    head = (0, 1, M.run, 2, 16, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), "gloo", None)
    M.main(BASE + files + ["--epochs", "9"])                        # without the options: the argument tuple of before
    assert made[0] == head + (0.0, 0, paths["features"], paths["labels"], paths["split"], None, 9, None, None, None)
    M.main(BASE + files + ["--epochs", "9", "--clip-norm", "2.5", "--lr-schedule", "cosine", "--lr-warmup", "3", "--lr-min", "1e-4",
                           "--lr-horizon", "20", "--patience", "4"])
    M.main(BASE + files + ["--lr-schedule", "step", "--lr-step", "30", "--lr-gamma", "0.5", "--optimizer", "fused"])
    control = dict(clip_norm=2.5, lr_schedule="cosine", lr_warmup=3, lr_min=1e-4, lr_horizon=20, patience=4)
    assert made[1][-1] == control and made[1][:-1] == made[0] + (None,) * 11
    assert seen[1] == (pos, dict(three, epochs=9, **control))
    assert seen[2] == (pos, dict(three, optimizer="fused", lr_schedule="step", lr_step=30, lr_gamma=0.5))
    assert all(type(control[k]) is int for k in ("lr_warmup", "lr_horizon", "patience"))
