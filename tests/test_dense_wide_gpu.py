"""The dense-layer kernels for widths above 128 (gemm/pgcn_dense_wide.hip, include/pgcn_dense_wide.h) against float64: the three
products with and without masks at the shapes where the chunking can go wrong, row independence, dropout, refusals, the layers."""
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

CASES = [(132, 8), (8, 132), (192, 256), (260, 132), (1024, 36)]   # one column past a panel, exact / ragged chunks, the largest K
NS = [1, 257, 300]                                                 # ... a second row panel with one row
EPS = 1e-6                                                         # of sum |a||b| in float64: the narrow kernels' bound


def _dev():
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return dev


def _padded(t, dev):
    """t as a column slice of a wider NaN-filled buffer: ld > width, 16-byte aligned base, poison around it"""
    buf = torch.full((t.shape[0], t.shape[1] + 8), float("nan"), device=dev)
    buf[:, 4:4 + t.shape[1]] = t.to(dev)
    return buf[:, 4:4 + t.shape[1]]


def _operands(n, fin, fout, dev):
    torch.manual_seed(1000 * fin + fout + n)
    x, g, w = torch.randn(n, fin), torch.randn(n, fout), torch.randn(fout, fin) / 8
    bits = torch.rand(n, fout) < 0.6
    return _padded(x, dev), _padded(g, dev), w.to(dev), bits.to(dev)


def _close(got, ref, a, b):
    """every element of got within EPS * (|a| . |b|) of ref (float64)"""
    bound = EPS * (a.double().abs() @ b.double().abs())
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all() and bool((err <= bound).all()), "max excess %g" % float((err - bound).max())


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("fin,fout", CASES)
def test_products_against_float64(fin, fout, n):
    P, D = pkg("PGCN"), pkg("dropout")
    dev = _dev()
    x, g, w, bits = _operands(n, fin, fout, dev)
    ref = x.double() @ w.double().t()
    for relu in (True, False):
        y, mask = P.wide_linear_relu_fused(x, w, relu, True)
        _close(y, ref.clamp_min(0) if relu else ref, x, w.t())
        assert torch.equal(mask, D.pack_words(y > 0))               # (pack_words leaves the bits of columns >= fout 0)
        assert torch.equal(P.wide_linear_relu_fused(x, w, relu, False), y)
    words = D.pack_words(bits)
    g[~bits] = float("nan")                                         # NaN under every cleared bit: a select must give +0
    for m, scale in ((words, 2.0), (None, 1.0)):
        gg = g if m is not None else torch.nan_to_num(g)
        gm_ref = torch.where(bits, gg * scale, torch.zeros((), device=dev)) if m is not None else gg
        gm, gx = P.wide_grad_input_fused(gg, m, scale, w, True)
        assert torch.equal(gm, gm_ref)
        _close(gx, gm_ref.double() @ w.double(), gm_ref, w)
        assert torch.equal(P.wide_grad_input_fused(gg, m, scale, w, False)[1], gx)
        gw = P.wide_weight_grad_masked_fused(gg, m, scale, x)
        _close(gw, gm_ref.double().t() @ x.double(), gm_ref.t(), x)
        assert torch.equal(P.wide_weight_grad_masked_fused(gg, m, scale, x), gw)        # two repeats: the same bits
    torch.cuda.synchronize()


@pytest.mark.parametrize("fin,fout", CASES)
def test_rows_do_not_depend_on_n(fin, fout):
    P, D = pkg("PGCN"), pkg("dropout")
    dev = _dev()
    x, g, w, bits = _operands(300, fin, fout, dev)
    words = D.pack_words(bits)
    y, mask = P.wide_linear_relu_fused(x, w, True, True)
    y33, mask33 = P.wide_linear_relu_fused(x[:33], w, True, True)
    assert torch.equal(y[:33], y33) and torch.equal(mask[:33], mask33)
    gx = P.wide_grad_input_fused(g, words, 1.0, w, False)[1]
    assert torch.equal(gx[:33], P.wide_grad_input_fused(g[:33], words[:33].contiguous(), 1.0, w, False)[1])


def test_dropout_equals_the_keep_words():
    P, D = pkg("PGCN"), pkg("dropout")
    dev = _dev()
    n, fin, fout = 300, 192, 256
    x, _, w, _ = _operands(n, fin, fout, dev)
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(21, dev)
    state.step.fill_(5)
    ids = torch.arange(n, dtype=torch.int64) * 7
    ids[41] = 2 ** 33 + 11
    ids = ids.to(dev)
    y0 = P.wide_linear_relu_fused(x, w, True, False)
    y, mask = P.wide_linear_relu_fused(x, w, True, True, dropout=(ids, state.seed, state.step, 3, thr))
    words = P.dropout_keep_words_call(P._dense_lib(), ids, n, fout, state.seed, state.step, 3, thr, torch.cuda.current_stream(dev).cuda_stream)
    keep = P.unpack_sign_mask(words, fout)
    assert 0.4 < float(keep.float().mean()) < 0.6
    assert torch.equal(y, torch.where(keep, y0 * scale, torch.zeros((), device=dev)))
    assert torch.equal(mask, D.pack_words(keep & (y0 > 0)))
    # no ids: the row index
    y1, _ = P.wide_linear_relu_fused(x, w, True, True, dropout=(None, state.seed, state.step, 3, thr))
    assert torch.equal(y1, P.wide_linear_relu_fused(x, w, True, True, dropout=(torch.arange(n, device=dev), state.seed, state.step, 3, thr))[0])


def test_raw_entry_points_and_refusals():
    P = pkg("PGCN")
    dev = _dev()
    L, s = P._dense_lib(), torch.cuda.current_stream(dev).cuda_stream
    n, fin, fout = 257, 260, 132
    x, g, w, _ = _operands(n, fin, fout, dev)
    y = torch.empty(n, fout, device=dev)
    ws = torch.empty(int(L.pgcn_wide_image_ws_bytes(fin, fout)), dtype=torch.uint8, device=dev)

    def forward(xx, ws_bytes, fin_=fin, fout_=fout):
        return L.pgcn_wide_linear_relu_f32(xx.data_ptr(), xx.stride(0), n, fin_, w.data_ptr(), w.stride(0), fout_, y.data_ptr(), y.stride(0), 1,
                                           None, None, 0, None, 0, 0, ws.data_ptr(), ws_bytes, s)
    assert forward(x, ws.numel()) == 0
    assert torch.equal(y, P.wide_linear_relu_fused(x, w, True, False))
    assert forward(x, ws.numel() - 1) == -2                         # a short work-space
    assert forward(x[:, 1:], ws.numel(), fin - 4) == -2             # a misaligned base
    assert forward(x, ws.numel(), 130, 130) == -2                   # a width that is no multiple of 4
    assert forward(x, ws.numel(), 128, 128) == -2                   # both widths up to 128: the narrow kernels' shape
    dx, dw = torch.empty(n, fin, device=dev), torch.empty(fout, fin, device=dev)
    ws2 = torch.empty(int(L.pgcn_wide_image_ws_bytes(fout, fin)), dtype=torch.uint8, device=dev)
    assert L.pgcn_wide_grad_input_f32(g.data_ptr(), g.stride(0), None, 1.0, None, 0, n, fout, w.data_ptr(), w.stride(0), fin, dx.data_ptr(),
                                      dx.stride(0), ws2.data_ptr(), ws2.numel(), s) == 0
    assert torch.equal(dx, P.wide_grad_input_fused(g, None, 1.0, w, False)[1])
    ws3 = torch.empty(int(L.pgcn_wide_weight_grad_ws_elems(n, fout, fin)), device=dev)
    for elems, rc in ((ws3.numel(), 0), (ws3.numel() - 1, -2)):
        assert L.pgcn_wide_weight_grad_f32(g.data_ptr(), g.stride(0), None, 1.0, x.data_ptr(), x.stride(0), n, fout, fin, dw.data_ptr(),
                                           dw.stride(0), ws3.data_ptr(), elems, s) == rc
    assert torch.equal(dw, P.wide_weight_grad_masked_fused(g, None, 1.0, x))
    # the fused functions answer None where the entry points refuse, and the narrow ones keep refusing the wide shapes
    x128, w128 = torch.randn(n, 128, device=dev), torch.randn(128, 128, device=dev)
    assert P.wide_linear_relu_fused(x128, w128, True, False) is None and P.wide_grad_input_fused(x128, None, 1.0, w128, False) is None
    assert P.wide_weight_grad_masked_fused(x128, None, 1.0, x128) is None
    assert P.wide_linear_relu_fused(x[:, 1:], w[:, 1:], True, False) is None
    assert P.linear_relu_fused(x, w, True) is None
    torch.cuda.synchronize()


@pytest.mark.parametrize("wide", [1, 0])
@pytest.mark.parametrize("x_grad", [True, False])
@pytest.mark.parametrize("drop", [False, True])
def test_layers(monkeypatch, drop, x_grad, wide):
    P, D, T = pkg("PGCN"), pkg("dropout"), pkg("tuning")
    dev = _dev()
    monkeypatch.setattr(T.T, "dense_wide", wide)
    n, f = 300, 256
    x, g, w, _ = _operands(n, f, f, dev)
    x, g = x.contiguous().requires_grad_(x_grad), g.contiguous()
    w = w.requires_grad_(True)
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(9, dev)
    state.step.fill_(2)
    ids = torch.arange(n, dtype=torch.int64, device=dev) + 1000
    keep = D.keep_mask(9, 2, 1, ids.cpu(), f, thr).to(dev) if drop else torch.ones(n, f, dtype=torch.bool, device=dev)
    sc = scale if drop else 1.0
    y = P._LinearReluDropoutNoBias.apply(x, w, ids, state, 1, thr, scale) if drop else P._LinearReluNoBias.apply(x, w)
    y.backward(g)
    zero = torch.zeros((), device=dev)
    if wide:                                                        # against float64 autograd
        x64, w64 = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
        y64 = (x64 @ w64.t()).clamp_min(0) * keep * sc
        y64.backward(g.double())
        gm = torch.where(keep & (y64 > 0), g * sc, zero)
        bound = EPS * sc * (x.detach().double().abs() @ w.detach().double().abs().t())
        assert bool(((y.double() - y64).abs() <= bound).all())
        _close(w.grad, w64.grad, gm.t(), x.detach())
        if x_grad:
            _close(x.grad, x64.grad, gm, w.detach())
    else:                                                           # the library route called directly: the same bits
        y0 = P.mm_nt(x.detach(), w.detach()).clamp_min_(0.0)
        yl = torch.where(keep, y0 * sc, zero) if drop else y0
        gm = torch.where(keep & (y0 > 0), g * sc, zero) if drop else torch.ops.aten.threshold_backward(g, y0, 0.0)
        assert torch.equal(y, yl) and torch.equal(w.grad, P._LinearNoBias.weight_grad(gm, x.detach()))
        if x_grad:
            assert torch.equal(x.grad, P.mm_nn(gm, w.detach()))
    assert (x.grad is not None) == x_grad
    torch.cuda.synchronize()
