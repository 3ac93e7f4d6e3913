"""Fused dropout on the GPU (gemm/pgcn_dense.hip: the pgcn_dropout_* entry points of include/pgcn_gemm.h): the kernels against the
host statement of the keep function (dropout.keep_mask) and today's kernels, the device-resident step under a replayed graph, the
layers end to end -- fused against unfused against float64, P real-kernel ranks on one GPU against one."""
import numpy as np
import pytest
import torch

from conftest import gpath, pkg
from test_dropout import BOUND, check_against_float64, float64_run, gather_global, spawn_layers

pytestmark = pytest.mark.gpu

SHAPES = [(77, 128, 128), (32, 64, 64), (100, 36, 128), (65, 128, 40), (5, 8, 4), (33, 4, 4), (1, 128, 128), (64, 16, 100), (0, 128, 128),
          (232965, 128, 128), (100003, 64, 64), (4097, 128, 44)]          # test_zz_dense_fused.SHAPES + the large ones


def _dev():
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return dev


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _host_keep(D, seed, step, layer, ids, width, thr, dev):
    return D.keep_mask(seed, step, layer, ids, width, thr).to(dev)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n,fin,fout", SHAPES)
def test_forward_kernel_equals_the_host_masks(n, fin, fout, p):
    P, D = pkg("PGCN"), pkg("dropout")
    dev = _dev()
    L, s = P._dense_lib(), _stream(dev)
    g0 = torch.Generator().manual_seed(n + fin)
    x = torch.randn(n, fin, generator=g0).to(dev)
    w = (torch.randn(fout, fin, generator=g0) / 8).to(dev)
    thr, scale = D.threshold(p)
    state = D.DropoutState(21, dev)
    state.step.fill_(5)
    zero = torch.zeros((), device=dev)
    y0 = P.linear_relu_call(L, x, w, True, s)
    # no ids: the row index
    y, mask = P.dropout_linear_relu_call(L, x, w, None, state.seed, state.step, 1, thr, s)
    keep = _host_keep(D, 21, 5, 1, np.arange(n), fout, thr, dev)
    assert torch.equal(y, torch.where(keep, y0 * scale, zero))
    assert torch.equal(mask, D.pack_words(keep & (y0 > 0)))
    ya, ma = P.dropout_linear_relu_call(L, x, w, torch.arange(n, device=dev), state.seed, state.step, 1, thr, s)
    assert torch.equal(ya, y) and torch.equal(ma, mask)
    # rows fed in another order with their ids: the same result row for row; ids above 2^32
    perm = torch.randperm(n, generator=g0)
    ids = (perm * 7 + (torch.arange(n) % 3 == 0) * (2 ** 33 + 11)).to(torch.int64)
    yp, mp_ = P.dropout_linear_relu_call(L, x, w, ids.to(dev), state.seed, state.step, 1, thr, s)
    keep_p = _host_keep(D, 21, 5, 1, ids, fout, thr, dev)
    assert torch.equal(yp, torch.where(keep_p, y0 * scale, zero)) and torch.equal(mp_, D.pack_words(keep_p & (y0 > 0)))
    inv = torch.argsort(perm).to(dev)
    yq, _ = P.dropout_linear_relu_call(L, x[perm.to(dev)].contiguous(), w, (perm * 7).to(dev), state.seed, state.step, 1, thr, s)
    yr, _ = P.dropout_linear_relu_call(L, x, w, (torch.arange(n) * 7).to(dev), state.seed, state.step, 1, thr, s)
    assert torch.equal(yq[inv], yr)
    assert torch.equal(P.dropout_keep_words_call(L, ids.to(dev), n, fout, state.seed, state.step, 1, thr, s), D.pack_words(keep_p))
    assert torch.equal(P.dropout_keep_words_call(L, None, n, fout, state.seed, state.step, 1, thr, s), D.pack_words(keep))
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,fin,fout", SHAPES)
def test_input_gradient_kernel(n, fin, fout):
    P, D = pkg("PGCN"), pkg("dropout")
    dev = _dev()
    L, s = P._dense_lib(), _stream(dev)
    g0 = torch.Generator().manual_seed(n + fout)
    w = (torch.randn(fout, fin, generator=g0) / 8).to(dev)
    g = torch.randn(n, fout, generator=g0).to(dev)
    bits = torch.rand(n, fout, generator=g0).to(dev) < 0.3
    mask = D.pack_words(bits)
    _, scale = D.threshold(0.5 if n % 2 else 0.1)
    gm, gx = P.dropout_grad_input_call(L, g, mask, scale, w, s)
    want = torch.where(bits, g * scale, torch.zeros((), device=dev))
    assert torch.equal(gm, want)
    if n:
        den = want.double().abs() @ w.double().abs() + 1e-30
        e = float(((gx.double() - want.double() @ w.double()).abs() / den).max())
        print("dX: %.3g of sum |a||b|" % e)
        assert e <= BOUND
    g2 = g.clone()
    gm2, gx2 = P.dropout_grad_input_call(L, g2, mask, scale, w, s, gm=g2)                # in place
    assert torch.equal(g2, want) and torch.equal(gx2, gx)
    torch.cuda.synchronize()


def test_padded_leading_dimensions():
    P, D = pkg("PGCN"), pkg("dropout")
    dev = _dev()
    L, s = P._dense_lib(), _stream(dev)
    torch.manual_seed(4)
    x = torch.randn(5000, 256, device=dev)[:, :128]
    w = torch.randn(64, 136, device=dev)[:, :128] / 8
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(2, dev)
    y, mask = P.dropout_linear_relu_call(L, x, w, None, state.seed, state.step, 0, thr, s)
    keep = _host_keep(D, 2, 0, 0, np.arange(5000), 64, thr, dev)
    y0 = P.linear_relu_call(L, x, w, True, s)
    assert torch.equal(y, torch.where(keep, y0 * scale, torch.zeros((), device=dev)))
    g = torch.randn(5000, 128, device=dev)[:, :64]
    gm, gx = P.dropout_grad_input_call(L, g, mask, scale, w, s)
    assert torch.equal(gm, torch.where(keep & (y0 > 0), g * scale, torch.zeros((), device=dev)))
    assert P.dropout_linear_relu_fused(torch.randn(64, 132, device=dev), torch.randn(8, 132, device=dev), None, 0, state.step, 0, thr) is None


def test_step_lives_on_the_device_and_graphs_replay_new_masks():
    P, D = pkg("PGCN"), pkg("dropout")
    dev = _dev()
    torch.manual_seed(6)
    n, f = 4097, 128
    x, w = torch.randn(n, f, device=dev), torch.randn(f, f, device=dev) / 8
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(9, dev)
    y0 = P.linear_relu_fused(x, w)
    want = lambda step: torch.where(_host_keep(D, 9, step, 3, np.arange(n), f, thr, dev), y0 * scale, torch.zeros((), device=dev))
    assert torch.equal(P.dropout_linear_relu_fused(x, w, None, state.seed, state.step, 3, thr)[0], want(0))
    state.advance()
    assert torch.equal(P.dropout_linear_relu_fused(x, w, None, state.seed, state.step, 3, thr)[0], want(1))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):                     # one stream: forward, then the step moves on
            out, _ = P.dropout_linear_relu_fused(x, w, None, state.seed, state.step, 3, thr)
            state.advance()
    torch.cuda.synchronize()
    state.step.fill_(10)
    graph.replay()
    torch.cuda.synchronize()
    first = out.clone()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, want(10)) and torch.equal(out, want(11)) and state.host_step() == 12


def test_node_fused_against_unfused_and_repeatable(monkeypatch):
    P, D, tuning = pkg("PGCN"), pkg("dropout"), pkg("tuning")
    dev = _dev()
    torch.manual_seed(2)
    n, f = 30011, 128
    x0, w0, coef = torch.randn(n, f, device=dev), torch.randn(f, f, device=dev) / 11, torch.randn(n, f, device=dev)
    ids = torch.randperm(n, device=dev)
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(4, dev)
    out = {}
    for fused in (1, 1, 0):
        monkeypatch.setattr(tuning.T, "dropout_fused", fused)
        x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        y = P._LinearReluDropoutNoBias.apply(x, w, ids, state, 1, thr, scale)
        (y * coef).sum().backward()
        torch.cuda.synchronize()
        if fused in out:                                              # the same (seed, step): bit-equal
            assert all(torch.equal(a, b) for a, b in zip(out[fused], (y.detach(), x.grad, w.grad)))
        out[fused] = (y.detach(), x.grad, w.grad)
    keep = _host_keep(D, 4, 0, 1, ids, f, thr, dev)
    assert torch.equal(out[1][0] == 0, out[0][0] == 0) or float(((out[1][0] == 0) != (out[0][0] == 0)).float().mean()) < 1e-5
    assert bool((out[1][0][~keep] == 0).all()) and bool((out[0][0][~keep] == 0).all())
    for a, b in zip(out[1], out[0]):
        assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max())


def test_layers_fused_unfused_float64_and_ranks_on_one_gpu():
    """3 layers, dropout 0.5, two training steps on karate with the real kernels: P = 1 fused and unfused and P = 2, 3 processes on the
    one GPU against float64 with the host masks; eval() equals a model without dropout."""
    f, nlayers, p_drop, dseed, seed, steps = 16, 3, 0.5, 7, 3, 2
    ref = float64_run(gpath("karate.mtx"), f, nlayers, p_drop, dseed, seed, steps)
    n = ref[0]["hidden"][0].shape[0]
    runs = {}
    for pv, fused in (("karate.mtx.1.rp", 1), ("karate.mtx.1.rp", 0), ("karate.mtx.2.rp", 1), ("karate.mtx.3.hp", 1)):
        P = int(pv.split(".")[-2])
        res = spawn_layers(P, gpath("karate.mtx"), gpath(pv), f, nlayers, p_drop, dseed, seed, steps, True, fused=fused)
        check_against_float64(res, P, ref, n, nlayers)
        runs[(P, fused)] = res
    again = spawn_layers(1, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), f, nlayers, p_drop, dseed, seed, steps, True, fused=1)
    for s in range(steps):
        for l in range(nlayers):
            assert np.array_equal(gather_global(again, n, "hidden", s, l), gather_global(runs[(1, 1)], n, "hidden", s, l))
    plain = spawn_layers(1, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), f, nlayers, 0.0, dseed, seed, 0, True)
    for r in plain:                                                   # a model without dropout, the same initial weights
        r["steps"] = []
    zero_steps = spawn_layers(1, gpath("karate.mtx"), gpath("karate.mtx.1.rp"), f, nlayers, p_drop, dseed, seed, 0, True)
    assert np.array_equal(zero_steps[0]["eval"], plain[0]["eval"])
