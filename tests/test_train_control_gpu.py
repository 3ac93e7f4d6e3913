"""pgcn_grad_sumsq_f32 and pgcn_adam_step_ctl_f32 on the GPU (csrc/pgcn_optim.hip) against the float64 definitions
(tests/_train_control_workers.py): every size at which the float4 body, the scalar tail, the block edge and the grid-stride wrap meet,
both decay modes, both schedules with warm-up, a gradient scale, three launches with the step advanced on the device; sentinels round
every buffer; the bit-equalities the definitions promise; gradients of 1e25; non-finite gradients as ordinary inputs; the binding's
refusals; one captured training step replayed; run(optimizer="fused", clip_norm=, lr_schedule=) end to end.

Tolerances: p / m / v as in test_fused_adam_gpu.py (F.errors_and_bound), the yardstick being torch's fp32 Adam with
torch.nn.utils.clip_grad_norm_ and the rate set by hand, on the same device.  The record: sumsq within n 2^-52 (relative) of the float64
sum -- two orders of summing n exact products differ by no more --, the coefficient rounded to fp32 within one fp32 ulp of the
definition's, the rate within 16 x 2^-53 of lr_at (the 4-ulp class of the device's double cos / pow plus the expression's roundings)."""
import math

import numpy as np
import pytest
import torch

import _fused_adam_workers as F
import _nodeclass_workers as W
import _train_control_workers as T
from conftest import pkg

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 1023, 1024, 1025, 4099, 300000]       # as test_fused_adam_gpu.SIZES; 300 000 floats: 293 chunks of 1024 > 256 partial sums
SCHEDS = [("cosine", F.LR, 2, 4, 1e-3, 1, 1.0), ("step", F.LR, 1, 0, 0.0, 1, 0.5)]
SENTINEL, GUARD = 12345.0, 64
LR_ULPS = 16 * 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def K(dev):
    return pkg("kernels").HipKernels(dev)


def _window(dev, n, dtype, offset):
    buf = torch.full((offset + n + GUARD + 1,), SENTINEL, device=dev, dtype=dtype)
    return buf, buf[offset:offset + n]


def _launches(K, dev, p0, grads, sched, max_norm, wd=0.0, decoupled=False, grad_scale=1.0, offset=GUARD, plain=False):
    """grad_sumsq (when clipping) + adam_step_ctl over windows of sentinel-filled allocations, one pair of launches per gradient, the
    step advanced on the device (``plain``: adam_step with lr = the schedule's base instead).  Returns (p, m, v, g after the last
    launch, the records [steps, 4], the last partial sums); asserts the 64 elements on either side of every window."""
    n = p0.size
    parts = K.grad_sumsq_parts(n)
    bufs, (p, g, m, v) = zip(*[_window(dev, n, torch.float32, offset) for _ in range(4)])
    cbuf, ctl = _window(dev, 4, torch.float64, GUARD)
    pbuf, partial = _window(dev, parts, torch.float64, GUARD)
    assert all(w.data_ptr() % 16 == 4 * (offset % 4) for w in (p, g, m, v))
    p.copy_(torch.from_numpy(p0))
    m.zero_()
    v.zero_()
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    recs = []
    for gr in grads:
        g.copy_(torch.from_numpy(gr))
        if plain:
            assert K.adam_step(p, g, m, v, step, sched[1], F.BETAS, F.EPS, wd, decoupled, grad_scale, True) is True
        else:
            if max_norm:
                assert K.grad_sumsq(g, partial) is partial
            assert K.adam_step_ctl(p, g, m, v, step, sched, max_norm, partial if max_norm else None, ctl, F.BETAS, F.EPS, wd, decoupled,
                                   grad_scale, True) is True
            recs.append(ctl.clone())
        step.add_(1)
    torch.cuda.synchronize()
    for b, w in zip(bufs + (cbuf, pbuf), (p, g, m, v, ctl, partial)):
        lo = (w.data_ptr() - b.data_ptr()) // b.element_size()
        assert bool((b[:lo] == SENTINEL).all()) and bool((b[lo + w.numel():] == SENTINEL).all())
    if not max_norm and not plain:
        assert bool((partial == SENTINEL).all())                    # no clip: the partial sums are not touched
    assert int(step) == len(grads)
    return p.clone(), m.clone(), v.clone(), g.clone(), (torch.stack(recs).cpu() if recs else None), partial.clone()


def _bits(t):
    return t.view(torch.int32) if t.dtype is torch.float32 else t.view(torch.int64)


def _max_norm(grads, grad_scale, n):
    norms = [T.clip64([g], None, grad_scale)[1] for g in grads]
    return 0.5 * (min(norms) + max(norms)) if n > 1 else 0.5 * max(norms)


@pytest.mark.parametrize("n", SIZES)
def test_kernels_against_float64_at_every_size(K, dev, n):
    p0, grads = F.make_case(n, 3, seed=n)
    max_norm = _max_norm(grads, F.THIRD, n)
    assert max_norm > 0.0
    for sched, (wd, decoupled) in zip(SCHEDS * 2, ((F.WD, False), (F.WD, True), (F.WD, True), (F.WD, False))):
        hyper = dict(weight_decay=wd, decoupled=decoupled, grad_scale=F.THIRD)
        ref, recs = T.reference_steps(p0, grads, sched, max_norm, **hyper)
        yard = T.torch_steps(p0, grads, dev, sched, max_norm, **hyper)
        got = _launches(K, dev, p0, grads, sched, max_norm, wd, decoupled, F.THIRD)
        assert not got[3].any()                                     # the gradient was cleared
        for name, a, y, r in zip("pmv", got, yard, ref):
            e, e_torch, bound = F.errors_and_bound(a.cpu().numpy(), y, r)
            print("n %d %s wd %g decoupled %s: %s e_kernel %.3g e_torch %.3g bound %.3g" % (n, sched[0], wd, decoupled, name, e, e_torch, bound))
            assert e <= bound, (n, sched[0], wd, decoupled, name)
        for t, (c, r) in enumerate(zip(got[4].tolist(), recs)):
            print("n %d %s step %d: sumsq %.17g (float64 %.17g) norm %.9g coef %.9g (%.9g) lr %.17g (%.17g)" % (n, sched[0], t, c[0], r[0], c[1], c[2], r[2], c[3], r[3]))
            assert abs(c[0] - r[0]) <= n * 2.0 ** -52 * r[0]
            assert abs(c[1] - r[1]) <= n * 2.0 ** -52 * r[1]
            assert abs(float(np.float32(c[2])) - float(np.float32(r[2]))) <= float(np.spacing(np.float32(r[2])))
            assert abs(c[3] - r[3]) <= LR_ULPS * r[3]
        assert any(r[2] < 1.0 for r in recs) and (n == 1 or any(r[2] == 1.0 for r in recs))       # steps that clip, steps that do not


@pytest.mark.parametrize("n", [5, 1025, 4099, 300000])
def test_bit_equalities(K, dev, n):
    optim = pkg("optim")
    p0, grads = F.make_case(n, 3, seed=7 * n)
    max_norm = _max_norm(grads, F.THIRD, n)
    for wd, decoupled in ((F.WD, False), (F.WD, True)):
        # neutral options: the bits of pgcn_adam_step_f32
        plain = _launches(K, dev, p0, grads, ("constant", F.LR), None, wd, decoupled, F.THIRD, plain=True)
        neutral = _launches(K, dev, p0, grads, optim.constant_schedule(F.LR), None, wd, decoupled, F.THIRD)
        assert neutral[4].tolist() == [[0.0, 0.0, 1.0, F.LR]] * 3
        for a, b in zip(plain[:4], neutral[:4]):
            assert torch.equal(_bits(a), _bits(b))
        # coef == 1 (max_norm above every norm): the bits of the unclipped ctl step
        sched = SCHEDS[0]
        loose = _launches(K, dev, p0, grads, sched, 1e6, wd, decoupled, F.THIRD)
        unclipped = _launches(K, dev, p0, grads, sched, None, wd, decoupled, F.THIRD)
        assert bool((loose[4][:, 2] == 1.0).all()) and bool((loose[4][:, 1] > 0.0).all())
        for a, b in zip(loose[:4], unclipped[:4]):
            assert torch.equal(_bits(a), _bits(b))
        # two runs from the same state; bases 4 bytes off (scalar loads throughout) against aligned bases
        a = _launches(K, dev, p0, grads, sched, max_norm, wd, decoupled, F.THIRD)
        again = _launches(K, dev, p0, grads, sched, max_norm, wd, decoupled, F.THIRD)
        odd = _launches(K, dev, p0, grads, sched, max_norm, wd, decoupled, F.THIRD, offset=GUARD + 1)
        assert bool((a[4][:, 2] < 1.0).any())
        for x, y, z in zip(a, again, odd):
            assert torch.equal(_bits(x), _bits(y))
            assert torch.equal(_bits(x), _bits(z))


def test_gradients_of_1e25_have_a_finite_norm(K, dev):
    n = 4099
    p0, _ = F.make_case(n, 1, seed=5)
    g = (np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * 1e25).astype(np.float32)
    with np.errstate(over="ignore"):
        assert not np.isfinite((g * g).sum())                       # an fp32 square overflows
    got = _launches(K, dev, p0, [g], SCHEDS[0], 1.0, F.WD, False, 1.0)
    sumsq, norm, coef, _ = got[4][0].tolist()
    want = math.sqrt(float((g.astype(np.float64) ** 2).sum()))
    assert math.isfinite(norm) and abs(norm - want) <= n * 2.0 ** -52 * want
    assert abs(coef - 1.0 / norm) <= 1e-12 * coef and 0.0 < coef < 1e-25
    for a in got[:3]:
        assert bool(torch.isfinite(a).all())
    assert not torch.equal(got[0].cpu(), torch.from_numpy(p0))      # and the parameters moved
    assert not got[3].any()


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_non_finite_gradients_are_ordinary_inputs(K, dev, value):
    """One NaN element: norm and coefficient are NaN and so is every parameter (clip_grad_norm_ with error_if_nonfinite off).  One inf
    element: coef = 0.  Both as the composition does it, element for element: the same NaN pattern, the finite elements within
    2 e_composed + 2^-23 max(1, max |ref|) of the float64 definition (F.errors_and_bound with the composition as the yardstick)."""
    optim = pkg("optim")
    n = 4099
    p0, grads = F.make_case(n, 1, seed=11)
    bad = grads[0].copy()
    bad[1030] = value
    sched = SCHEDS[0]
    got = _launches(K, dev, p0, [bad], sched, 1.0, F.WD, False, 1.0)
    sumsq, norm, coef, lr = got[4][0].tolist()
    p, m, v = torch.from_numpy(p0.copy()), torch.zeros(n), torch.zeros(n)
    ctl = torch.zeros(4, dtype=torch.float64)
    optim.adam_step_ctl_composed(p, torch.from_numpy(bad.copy()), m, v, torch.zeros(1, dtype=torch.int64), sched, 1.0, ctl, F.BETAS, F.EPS,
                                 F.WD, False, 1.0, True)
    if math.isnan(value):
        assert math.isnan(norm) and math.isnan(coef) and math.isnan(sumsq)
        assert bool(torch.isnan(got[0]).all())                      # every parameter
    else:
        assert math.isinf(norm) and coef == 0.0
    assert [math.isnan(x) for x in ctl.tolist()] == [math.isnan(x) for x in (sumsq, norm, coef, lr)]      # the composition's record
    assert math.isnan(coef) or ctl[2].item() == coef
    fine = np.ones(n, dtype=bool)
    fine[1030] = False
    zero = np.zeros(n, dtype=np.float32)
    ref, _ = T.reference_steps(p0, [zero], sched, None, weight_decay=F.WD)          # coef = 0: the step of a zero gradient
    for name, a, c, r in zip("pmv", got[:3], (p, m, v), ref):
        a = a.cpu()
        assert torch.equal(torch.isnan(a), torch.isnan(c)), name
        if not math.isnan(value):
            assert bool(torch.isnan(a[1030])) and bool(torch.isfinite(a[torch.from_numpy(fine)]).all())      # inf * 0
            e, e_comp, bound = F.errors_and_bound(a.numpy()[fine], c.numpy()[fine], r[fine])
            print("inf: %s e_kernel %.3g e_composed %.3g bound %.3g" % (name, e, e_comp, bound))
            assert e <= bound
    assert not got[3].any()                                         # the gradient arena, NaN / inf included, was cleared


def test_bindings_answer_none_for_what_the_kernels_do_not_cover(K, dev):
    optim = pkg("optim")
    z = lambda **kw: torch.zeros(64, device=dev, **kw)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    ctl, partial = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    sched = optim.constant_schedule(1e-3)
    tail = ((0.9, 0.999), 1e-8, 0.0, False, 1.0, True)
    d = dict(dtype=torch.float64)
    assert K.adam_step_ctl(z(**d), z(**d), z(**d), z(**d), step, sched, 1.0, partial, ctl, *tail) is None
    assert K.adam_step_ctl(torch.zeros(128, device=dev)[::2], z(), z(), z(), step, sched, 1.0, partial, ctl, *tail) is None      # non-contiguous
    assert K.adam_step_ctl(z(), z().cpu(), z(), z(), step, sched, 1.0, partial, ctl, *tail) is None                              # another device
    assert K.adam_step_ctl(z().cpu(), z().cpu(), z().cpu(), z().cpu(), step.cpu(), sched, 1.0, partial.cpu(), ctl.cpu(), *tail) is None
    assert K.adam_step_ctl(z(), z(), z(), z(), step, sched, 1.0, partial, ctl.cpu(), *tail) is None
    assert K.adam_step_ctl(z(), z(), z(), z(), step, sched, 1.0, None, ctl, *tail) is None                                       # clipping without partial sums
    assert K.grad_sumsq(z(**d)) is None and K.grad_sumsq(torch.zeros(128, device=dev)[::2]) is None and K.grad_sumsq(z().cpu()) is None
    assert K.grad_sumsq(z(), torch.zeros(2, dtype=torch.float64, device=dev)) is None                                            # another number of parts
    p = torch.ones(64, device=dev)
    g = torch.full((64,), 2.0, device=dev)
    assert K.grad_sumsq(g, partial) is partial and partial.item() == 256.0
    assert K.adam_step_ctl(p, g, z(), z(), step, sched, 1.0, partial, ctl, *tail) is True and bool((p < 1).all())
    assert ctl.tolist() == [256.0, 16.0, 1.0 / (16.0 + 1e-6), 1e-3]
    assert K.adam_step_ctl(p, g, z(), z(), step, sched, None, None, ctl, *tail) is True and ctl.tolist() == [0.0, 0.0, 1.0, 1e-3]
    with pytest.raises(pkg("_lib").PgcnError):
        K.adam_step_ctl(z(), z(), z(), z(), step, ("cosine", 1e-3, 4, 4, 0.0, 1, 1.0), None, None, ctl, *tail)                   # refused by the entry point


# ---- one captured training step ------------------------------------------------------------------------------------------------------

def test_captured_training_step_reads_rate_and_clip_from_device_memory(K, dev, tmp_path, monkeypatch):
    """The model of test_fused_adam_gpu's captured step under warm-up 2 + cosine to a horizon of 4 + a clip: three replays of the
    captured step leave the bits of three eager steps, and the record afterwards holds the rate of update 2 -- the schedule is read
    from device memory, not baked in."""
    P, partition, engine, optim = pkg("PGCN"), pkg("partition"), pkg("engine"), pkg("optim")
    n = 600
    _, data = W.make_dataset(str(tmp_path), n=n, nnz=7200, community=60)
    row, col, val = P._coo_tensors(data["A"])
    part = partition.build_partition(row, col, val, n, torch.zeros(n, dtype=torch.int64), 0, 1, normalize="sym")
    eng = engine.AggregationEngine(part, K, dev)
    for name, value in (("device", dev), ("myrank", 0), ("world_size", 1), ("_engine_current", eng), ("_kernel_provider", K)):
        monkeypatch.setattr(P, name, value)
    own = part.owned.numpy()
    H = torch.from_numpy(data["X"][own]).to(dev)
    y = torch.from_numpy(data["labels"][own]).to(dev)
    s = torch.from_numpy(data["split"][own]).to(dev)
    n_train = int((data["split"] == 1).sum())
    torch.manual_seed(W.WEIGHT_SEED)
    model = torch.nn.Sequential(P.PGCN(eng, W.FIN, W.HIDDEN), P.PGCN(eng, W.HIDDEN, W.CLASSES, relu=False)).to(dev)
    sched = ("cosine", W.LR, 2, 4, 0.002, 1, 1.0)
    opt = optim.FlatAdam(model.parameters(), lr=W.LR, weight_decay=F.WD, kernels=K, max_norm=1e9, schedule=sched)
    start = opt.flat_p.clone()

    def restart():
        opt.flat_p.copy_(start)
        for t in (opt.flat_g, opt.exp_avg, opt.exp_avg_sq, opt.step_count):
            t.zero_()

    def one_step():
        loss, _ = P.masked_loss(model(H), y, s, n_train)
        loss.backward()
        opt.reduce_gradients(average=False)
        opt.step()
        return loss

    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):                                   # everything on one side stream: warm-up, eager steps, capture
        for _ in range(2):
            one_step()
        opt.set_control(0.75 * opt.control()["gnorm"], sched)       # a clip of the size of the gradients: the record and the partial
        restart()                                                   # sums are allocated here, before the capture
        recs = []
        for _ in range(3):
            one_step()
            recs.append(opt.control())
        eager, eager_ctl = opt.flat_p.clone(), opt.ctl.clone()
        print("eager records: %s" % recs)
        assert int(opt.step_count) == 3 and not torch.equal(eager, start)
        assert [abs(r["lr"] - optim.lr_at(t, sched)) <= LR_ULPS * r["lr"] for t, r in enumerate(recs)] == [True] * 3
        assert recs[0]["lr"] != recs[2]["lr"]                       # the rate of the update a capture would bake in is not the last one
        restart()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            one_step()
    torch.cuda.synchronize()
    assert int(opt.step_count) == 0 and torch.equal(opt.flat_p, start)      # a capture runs nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(opt.step_count) == 3
    assert torch.equal(opt.flat_p.view(torch.int32), eager.view(torch.int32))
    assert torch.equal(opt.ctl.view(torch.int64), eager_ctl.view(torch.int64))
    assert abs(opt.control()["lr"] - optim.lr_at(2, sched)) <= LR_ULPS * optim.lr_at(2, sched) and optim.lr_at(2, sched) != optim.lr_at(0, sched)
    assert not opt.flat_g.any()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------

def test_fused_run_under_control_on_one_gpu_against_float64(tmp_path):
    optim = pkg("optim")
    paths, data = W.make_dataset(str(tmp_path))
    widths = [W.FIN, W.HIDDEN, W.CLASSES]
    sched = ("cosine", W.LR, 3, W.EPOCHS, 0.002, 1, 1.0)
    norms = [c[0] for c in T.float64_reference(data, widths, sched=sched, weight_decay=F.WD)[3]]
    max_norm = 0.5 * (min(norms) + max(norms))
    ref, final, weights, ctl = T.float64_reference(data, widths, sched=sched, max_norm=max_norm, weight_decay=F.WD)
    assert any(c[1] < 1.0 for c in ctl) and any(c[1] == 1.0 for c in ctl) and all(abs(c[0] - max_norm) > 1e-3 * max_norm for c in ctl)
    opts = dict(weight_decay=F.WD, control=dict(lr_schedule="cosine", lr_warmup=3, lr_min=0.002, clip_norm=max_norm))
    yard = F.spawn_run(1, paths, True, optimizer="torch", **opts)
    res = F.spawn_run(1, paths, True, optimizer="fused", **opts)
    assert res[0]["hip"] == yard[0]["hip"] == "HipKernels"
    W.check_against_reference(yard, ref, final, data)
    worst = W.check_against_reference(res, ref, final, data)
    e, e_torch, bound = F.weight_errors(res, yard, weights)
    print("fused under control on one GPU: largest relative loss error %.3g; trained weights e_run %.3g e_torch %.3g bound %.3g" % (worst, e, e_torch, bound))
    assert e <= bound
    for h, (norm, coef, lr) in zip(res[0]["history"], ctl):
        assert abs(h["lr"] - optim.lr_at(h["epoch"], sched)) <= LR_ULPS * lr and lr == optim.lr_at(h["epoch"], sched)
        assert abs(h["gnorm"] - norm) <= 1e-4 * norm and (h["clip"] < 1.0) == (coef < 1.0) and abs(h["clip"] - coef) <= 1e-4
    assert [sorted(h) for h in res[0]["history"]] == [sorted(h) for h in yard[0]["history"]]
