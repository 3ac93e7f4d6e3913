"""The weight gradient on the raw gradient and the sign mask (gemm/pgcn_wgrad.hip: pgcn_linear_weight_grad_masked_f32) against the
kernel of before on the Gm it no longer reads -- bit for bit -- and the side stream it runs on in a layer's backward
(tuning.wgrad_lane; engine.AggregationEngine.wgrad_lane / join_wgrad): lane on against lane off, eager and under a replayed graph."""
import ctypes

import pytest
import torch
import torch.nn as nn

from conftest import pkg

pytestmark = pytest.mark.gpu

ROWS = [1, 17, 1000, 4099]                      # below a 16-row step, ragged steps, several workgroups' ranges plus a ragged tail
WIDTHS = [(128, 128), (72, 40), (4, 4)]         # (fout, fin): full 2 x 2 tiles, ragged widths with a tile's second block cut, one block


def _dev():
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return dev


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _pack(bits, pad_ones=False):
    """int32 words of the sign-mask layout from bool [n, width]; pad_ones: the bits beyond the width set (the kernel must ignore them)."""
    n, width = bits.shape
    mw = (width + 31) // 32
    full = torch.full((n, mw * 32), bool(pad_ones), dtype=torch.bool, device=bits.device)
    full[:, :width] = bits
    w = (full.view(n, mw, 32).to(torch.int64) << torch.arange(32, device=bits.device)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()


def _reference(P, L, g, bits, scale, x, s):
    """The kernel of before on Gm = bit ? g * scale : 0 (scale 1: no product, as the plain input gradient writes it)."""
    gm = torch.where(bits, g if scale == 1.0 else g * scale, torch.zeros((), device=g.device))
    return P.weight_grad_call(L, gm, x, s)


@pytest.mark.parametrize("fout,fin", WIDTHS)
@pytest.mark.parametrize("n", ROWS)
def test_masked_kernel_equals_the_kernel_on_gm(n, fout, fin):
    P = pkg("PGCN")
    dev = _dev()
    L, s = P._dense_lib(), _stream(dev)
    assert L.pgcn_has_wgrad_masked and L.pgcn_wgrad_masked_abi_version() == 1
    gen = torch.Generator().manual_seed(1000 * n + fout)
    g = torch.randn(n, fout, generator=gen).to(dev)
    x = torch.randn(n, fin, generator=gen).to(dev)
    rnd = (torch.rand(n, fout, generator=gen) < 0.5).to(dev)
    rnd[0, 0] = False                                              # (at least one cleared bit, for the planted values below)
    zeros, ones = torch.zeros_like(rnd), torch.ones_like(rnd)
    for scale in (1.0, float(torch.tensor(1.0 / (1.0 - 0.3), dtype=torch.float32))):
        for bits, pad in ((rnd, False), (zeros, False), (ones, True)):
            got = P.weight_grad_masked_call(L, g, _pack(bits, pad), scale, x, s)
            assert got is not None and _bits_equal(got, _reference(P, L, g, bits, scale, x, s)), (scale, pad)
        # a cleared mask: an exact (+0) zero matrix
        assert not P.weight_grad_masked_call(L, g, _pack(zeros), scale, x, s).view(torch.int32).any()
        # NaN and +-Inf under cleared bits only contribute +0: a select, not a product
        bad = g.clone()
        planted = torch.tensor([float("nan"), float("inf"), float("-inf")], device=dev)[torch.arange(n * fout, device=dev) % 3].view(n, fout)
        bad[~rnd] = planted[~rnd]
        assert _bits_equal(P.weight_grad_masked_call(L, bad, _pack(rnd), scale, x, s), _reference(P, L, g, rnd, scale, x, s))
        # no mask: every bit set
        assert _bits_equal(P.weight_grad_masked_call(L, g, None, scale, x, s), _reference(P, L, g, ones, scale, x, s))
    assert _bits_equal(P.weight_grad_masked_call(L, g, None, 1.0, x, s), P.weight_grad_call(L, g, x, s))     # the old entry point itself
    torch.cuda.synchronize()


def test_padded_leading_dimensions():
    P = pkg("PGCN")
    dev = _dev()
    L, s = P._dense_lib(), _stream(dev)
    gen = torch.Generator().manual_seed(3)
    n, fout, fin = 1000, 72, 40
    G = torch.randn(n, 96, generator=gen).to(dev)
    X = torch.randn(n, 52, generator=gen).to(dev)
    g, x = G[:, :fout], X[:, 4:4 + fin]
    bits = (torch.rand(n, fout, generator=gen) < 0.5).to(dev)
    assert _bits_equal(P.weight_grad_masked_call(L, g, _pack(bits), 1.25, x, s), _reference(P, L, g.contiguous(), bits, 1.25, x.contiguous(), s))
    torch.cuda.synchronize()


def test_refused_operands_return_minus_two_and_write_nothing():
    P = pkg("PGCN")
    dev = _dev()
    L, s = P._dense_lib(), _stream(dev)
    ws = torch.empty(int(L.pgcn_linear_weight_grad_ws_elems()), device=dev)

    def call(g, mask_ptr, x, dw, ldg=None):
        return L.pgcn_linear_weight_grad_masked_f32(g.data_ptr(), g.stride(0) if ldg is None else ldg, mask_ptr, ctypes.c_float(1.5), x.data_ptr(),
                                                    x.stride(0), g.shape[0], g.shape[1], x.shape[1], dw.data_ptr(), dw.stride(0), ws.data_ptr(),
                                                    ws.numel(), s)
    n = 100
    x = torch.randn(n, 64, device=dev)
    for fout in (160, 64):
        g = torch.randn(n, fout, device=dev)
        mask = torch.full((n, (fout + 31) // 32 + 1), -1, dtype=torch.int32, device=dev)
        dw = torch.full((fout, 64), 7.0, device=dev)
        if fout == 160:                                            # widths above 128: the library product's
            assert call(g, mask.data_ptr(), x, dw) == -2
        else:                                                      # mask words off their alignment; a stride beyond the 32-bit lane offsets
            assert call(g, mask.data_ptr() + 2, x, dw) == -2
            assert call(g, mask.data_ptr(), x, dw, ldg=1 << 25) == -2
        torch.cuda.synchronize()
        assert bool((dw == 7.0).all())
    assert b"" != L.pgcn_wgrad_last_error()


# ---- the side stream in a model's backward --------------------------------------------------------------------------------------
N, NNZ, F = 4096, 60000, 128
_model = {}


def _setup():
    """One engine, three layers' weights, features and labels, built once and left unchanged."""
    if not _model:
        P, synth, partition, engine, kernels = pkg("PGCN"), pkg("synth"), pkg("partition"), pkg("engine"), pkg("kernels")
        dev = _dev()
        _, row, col, val = synth.make_graph(N, NNZ, seed=11)
        part = partition.build_partition(row, col, val, N, torch.zeros(N, dtype=torch.int64), 0, 1)
        eng = engine.AggregationEngine(part, kernels.HipKernels(dev), dev)
        P.device, P.myrank, P.world_size = dev, 0, 1
        P.init_stats()
        torch.manual_seed(5)
        weights = [(torch.randn(F, F) / 8).to(dev) for _ in range(3)]
        H = torch.rand(N, F, generator=torch.Generator().manual_seed(6)).to(dev)
        _model.update(P=P, dev=dev, eng=eng, weights=weights, H=H, labels=part.owned.to(dev) % F, T=pkg("tuning").T)
    return _model


def _fresh(m, h_grad, dropout=0.0):
    P = m["P"]
    state = pkg("dropout").DropoutState(3, m["dev"]) if dropout else None
    model = nn.Sequential(*[P.PGCN(m["eng"], F, F, dropout=dropout if i < 2 else 0.0, layer=i, state=state) for i in range(3)]).to(m["dev"])
    with torch.no_grad():
        for layer, w in zip(model, m["weights"]):
            layer.linear.weight.copy_(w)
    return model, m["H"].clone().requires_grad_(h_grad)


def _backward(m, model, H):
    m["P"].local_loss(model(H), m["labels"], N).backward()


def _grads(model, H):
    torch.cuda.synchronize()
    return [p.grad.clone() for p in model.parameters()] + ([H.grad.clone()] if H.grad is not None else [])


def _eager(m, lane, h_grad, dropout, monkeypatch=None):
    P = m["P"]
    made = []
    if monkeypatch is not None:
        real = P.weight_grad_masked_call

        def spy(*a):
            out = real(*a)
            made.append((out.data_ptr(), a[-1]))
            return out
        monkeypatch.setattr(P, "weight_grad_masked_call", spy)
    old = m["T"].wgrad_lane
    m["T"].wgrad_lane = lane
    try:
        model, H = _fresh(m, h_grad, dropout)
        _backward(m, model, H)
        assert m["eng"]._wgrad_parked == []                        # every weight gradient was joined inside the backward
        return _grads(model, H), model, made
    finally:
        m["T"].wgrad_lane = old


@pytest.mark.parametrize("dropout", [0.0, 0.3])
@pytest.mark.parametrize("h_grad", [True, False])
def test_lane_on_and_off_give_the_same_bits(h_grad, dropout, monkeypatch):
    m = _setup()
    off, _, _ = _eager(m, 0, h_grad, dropout)
    on, model, made = _eager(m, 1, h_grad, dropout, monkeypatch)
    assert len(on) == len(off) == 3 + int(h_grad)
    for a, b in zip(on, off):
        assert _bits_equal(a, b)
    # the masked route ran for every layer, on the engine's side stream -- not the current one, not a launch lane of the aggregation
    side = m["eng"]._wgrad_stream.cuda_stream
    assert len(made) == 3 and all(s == side for _, s in made)
    assert side != torch.cuda.current_stream(m["dev"]).cuda_stream and side not in [s.cuda_stream for s in m["eng"].k.sides]
    # ... and autograd adopted each result as the parameter's gradient instead of reading it (on the current stream) before the join
    assert sorted(p.grad.data_ptr() for p in model.parameters()) == sorted(ptr for ptr, _ in made)


def test_lane_under_graph_capture_and_replay(monkeypatch):
    m = _setup()
    off, _, _ = _eager(m, 0, True, 0.0)
    monkeypatch.setattr(m["T"], "wgrad_lane", 1)
    model, H = _fresh(m, True)
    side = torch.cuda.Stream(device=m["dev"])
    side.wait_stream(torch.cuda.current_stream(m["dev"]))
    with torch.cuda.stream(side):                                  # (warm-up off the default stream, as torch.cuda.graph asks)
        _backward(m, model, H)
    torch.cuda.current_stream(m["dev"]).wait_stream(side)
    torch.cuda.synchronize()
    for p in list(model.parameters()) + [H]:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _backward(m, model, H)
    assert m["eng"]._wgrad_parked == [] and m["eng"]._wgrad_stream is not None
    for _ in range(2):
        for p in list(model.parameters()) + [H]:
            p.grad.zero_()
        graph.replay()
        for a, b in zip(_grads(model, H), off):
            assert _bits_equal(a, b)


def test_backward_that_stops_short_of_the_aggregation_still_joins():
    """torch.autograd.grad for the last layer's weight alone: its dense backward defers the join to a PSpMM.backward that this
    backward pass never runs -- the callback at the end of the pass joins instead, before grad() returns."""
    m = _setup()
    off, _, _ = _eager(m, 0, True, 0.0)
    old = m["T"].wgrad_lane
    m["T"].wgrad_lane = 1
    try:
        model, H = _fresh(m, True)
        loss = m["P"].local_loss(model(H), m["labels"], N)
        (gw,) = torch.autograd.grad(loss, [model[2].linear.weight])
        assert m["eng"]._wgrad_parked == []
        torch.cuda.current_stream(m["dev"]).synchronize()          # (the CURRENT stream alone: it has to have waited for the side stream)
        assert _bits_equal(gw, off[2])
    finally:
        m["T"].wgrad_lane = old
