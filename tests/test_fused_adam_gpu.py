"""pgcn_adam_step_f32 on the GPU (csrc/pgcn_optim.hip) against the float64 definition (tests/_fused_adam_workers.py: adam64): every size at
which the float4 body, the scalar tail, the block edge and the grid-stride wrap meet, both decay modes, a gradient scale, three
launches with the step advanced on the device; canaries round every buffer, zeroing, misaligned bases, repeatability, non-finite
gradients as ordinary inputs, one captured training step replayed, and run(optimizer="fused") end to end.

Tolerance (F.errors_and_bound): against float64 the kernel may be twice as far as torch.optim.Adam / AdamW in fp32 on the same device
with the same inputs and steps, plus one rounding of the value: e_kernel <= 2 e_torch + 2^-23 max(1, max |p|).  Both errors are
printed before the assertion."""
import itertools

import numpy as np
import pytest
import torch

import _fused_adam_workers as F
import _nodeclass_workers as W
from conftest import pkg

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 1023, 1024, 1025, 4099, 300000]       # 300 000: 75 000 float4 chunks > 256 blocks x 256 lanes, the loop wraps
SETTINGS = list(itertools.product((0.0, F.WD), (False, True), (1.0, F.THIRD)))
SENTINEL, GUARD = 12345.0, 64


@pytest.fixture(scope="module")
def dev():
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def K(dev):
    return pkg("kernels").HipKernels(dev)


def _launches(K, dev, p0, grads, wd=0.0, decoupled=False, grad_scale=1.0, zero_grad=True, offset=GUARD, start=None):
    """The kernel over windows of four sentinel-filled allocations, one launch per gradient, the step advanced on the device.
    Returns (p, m, v, g after the last launch) as device tensors; asserts the 64 floats on either side of every window."""
    n = p0.size
    bufs = [torch.full((offset + n + GUARD + 1,), SENTINEL, device=dev) for _ in range(4)]
    p, g, m, v = (b[offset:offset + n] for b in bufs)
    assert all(w.data_ptr() % 16 == (0 if offset % 4 == 0 else 4 * (offset % 4)) for w in (p, g, m, v))
    p.copy_(torch.from_numpy(p0))
    m.zero_()
    v.zero_()
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    if start is not None:
        m.copy_(start[0])
        v.copy_(start[1])
        step.fill_(start[2])
    for gr in grads:
        g.copy_(torch.from_numpy(gr))
        assert K.adam_step(p, g, m, v, step, F.LR, F.BETAS, F.EPS, wd, decoupled, grad_scale, zero_grad) is True
        step.add_(1)
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[:offset] == SENTINEL).all()) and bool((b[offset + n:] == SENTINEL).all())
    assert int(step) == len(grads) + (start[2] if start is not None else 0)
    return p.clone(), m.clone(), v.clone(), g.clone()


@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_float64_at_every_size(K, dev, n):
    p0, grads = F.make_case(n, 3, seed=n)
    for wd, decoupled, gs in SETTINGS:
        hyper = dict(weight_decay=wd, decoupled=decoupled, grad_scale=gs)
        ref = F.reference_steps(p0, grads, **hyper)
        yard = F.torch_steps(p0, grads, dev, **hyper)
        got = _launches(K, dev, p0, grads, wd, decoupled, gs)
        assert not got[3].any()                                     # the gradient was cleared
        for name, a, y, r in zip("pmv", got, yard, ref):
            e, e_torch, bound = F.errors_and_bound(a.cpu().numpy(), y, r)
            print("n %d wd %g decoupled %s scale %.3g: %s e_kernel %.3g e_torch %.3g bound %.3g" % (n, wd, decoupled, gs, name, e, e_torch, bound))
            assert e <= bound, (n, wd, decoupled, gs, name)


@pytest.mark.parametrize("n", [5, 1025, 4099])
def test_zeroing_misaligned_bases_and_repeatability(K, dev, n):
    p0, grads = F.make_case(n, 3, seed=7 * n)
    for wd, decoupled, gs in ((F.WD, False, F.THIRD), (F.WD, True, 1.0)):
        a = _launches(K, dev, p0, grads, wd, decoupled, gs, zero_grad=True)
        again = _launches(K, dev, p0, grads, wd, decoupled, gs, zero_grad=True)
        keep = _launches(K, dev, p0, grads, wd, decoupled, gs, zero_grad=False)
        odd = _launches(K, dev, p0, grads, wd, decoupled, gs, zero_grad=True, offset=GUARD + 1)      # bases 4 bytes off: the scalar loop
        assert torch.equal(a[3], torch.zeros_like(a[3]))            # exactly zero
        assert torch.equal(keep[3].view(torch.int32), torch.from_numpy(grads[-1]).to(dev).view(torch.int32))    # bit for bit its input
        for x, y, z, w in zip(a[:3], again[:3], keep[:3], odd[:3]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))      # two runs from the same state: the same bits
            assert torch.equal(x.view(torch.int32), z.view(torch.int32))      # zeroing changes nothing else
            assert torch.equal(x.view(torch.int32), w.view(torch.int32))      # the scalar path: the same values


def test_non_finite_gradients_stay_in_their_elements(K, dev):
    n = 4099
    p0, grads = F.make_case(n, 1, seed=11)
    clean = _launches(K, dev, p0, grads, F.WD, False, 1.0)
    bad = grads[0].copy()
    bad[7], bad[1030], bad[4098] = np.nan, np.inf, np.nan          # float4 body (two blocks) and the scalar tail
    got = _launches(K, dev, p0, [bad], F.WD, False, 1.0)
    hit = torch.zeros(n, dtype=torch.bool, device=dev)
    hit[[7, 1030, 4098]] = True
    for a, c in zip(got[:3], clean[:3]):
        assert not bool(torch.isfinite(a[hit]).any())
        assert torch.equal(a[~hit].view(torch.int32), c[~hit].view(torch.int32))
    assert not got[3].any()                                         # and the gradient, NaN included, was cleared


def test_binding_answers_none_for_what_the_kernel_does_not_cover(K, dev):
    z = lambda **kw: torch.zeros(64, device=dev, **kw)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    tail = (1e-3, (0.9, 0.999), 1e-8, 0.0, False, 1.0, True)
    assert K.adam_step(z(dtype=torch.float64), z(dtype=torch.float64), z(dtype=torch.float64), z(dtype=torch.float64), step, *tail) is None
    assert K.adam_step(torch.zeros(128, device=dev)[::2], z(), z(), z(), step, *tail) is None            # non-contiguous
    assert K.adam_step(z(), z().cpu(), z(), z(), step, *tail) is None                                    # another device
    assert K.adam_step(z().cpu(), z().cpu(), z().cpu(), z().cpu(), step.cpu(), *tail) is None             # CPU tensors
    p = torch.ones(64, device=dev)
    assert K.adam_step(p, torch.ones(64, device=dev), z(), z(), step, *tail) is True and bool((p < 1).all())
    with pytest.raises(pkg("_lib").PgcnError):
        K.adam_step(z(), z(), z(), z(), step, 1e-3, (1.0, 0.999), 1e-8, 0.0, False, 1.0, True)             # refused by the entry point


# ---- one captured training step ------------------------------------------------------------------------------------------------------

def test_captured_training_step_replays_like_eager_steps(K, dev, tmp_path, monkeypatch):
    """forward, masked_loss, backward, reduce_gradients, step() and the step increment of a 2-layer model on the planted graph at 600
    vertices, one rank: three replays of the captured step leave the bits of three eager steps from the same start, and the device
    step count at 3 -- the bias correction of a replay is read from memory, not baked in."""
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
    opt = optim.FlatAdam(model.parameters(), lr=W.LR, weight_decay=F.WD, kernels=K)
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
        restart()
        losses = [float(one_step()) for _ in range(3)]
        eager = opt.flat_p.clone()
        assert int(opt.step_count) == 3 and not torch.equal(eager, start) and losses[2] < losses[0]
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
    assert not opt.flat_g.any()
    for p, o in zip(opt.params, opt.offsets):                       # the model's parameters ARE the arena
        assert p.data_ptr() == opt.flat_p.data_ptr() + 4 * o


# ---- end to end ------------------------------------------------------------------------------------------------------------------------

def test_fused_run_on_one_gpu_against_float64(tmp_path):
    paths, data = W.make_dataset(str(tmp_path))
    ref, final, weights = F.float64_reference(data, [W.FIN, W.HIDDEN, W.CLASSES], weight_decay=F.WD)
    yard = F.spawn_run(1, paths, True, weight_decay=F.WD, optimizer="torch")
    res = F.spawn_run(1, paths, True, weight_decay=F.WD, optimizer="fused")
    assert res[0]["hip"] == yard[0]["hip"] == "HipKernels"
    W.check_against_reference(yard, ref, final, data)
    worst = W.check_against_reference(res, ref, final, data)
    e, e_torch, bound = F.weight_errors(res, yard, weights)
    print("fused on one GPU: largest relative loss error %.3g; trained weights e_run %.3g e_torch %.3g bound %.3g" % (worst, e, e_torch, bound))
    assert e <= bound
    assert [sorted(h) for h in res[0]["history"]] == [sorted(h) for h in yard[0]["history"]]
    assert sorted(res[0]["history"][0]) == sorted(["epoch", "loss", "train", "val", "test", "losses", "correct", "rows"])
