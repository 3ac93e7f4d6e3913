"""The layer-norm kernels of csrc/pgcn_layernorm.hip on the device, against the float64 definition (tests/_layernorm_workers.py: the
bounds are derived there) evaluated on the same fp32 inputs: forward, mask, row statistics, dX, dgamma, dbeta over the shape grid;
the float4 path against a misaligned base; dropout masks; the residual, out of place and in place; row independence; layout (leading
dimensions, poisoned padding, canary rows); planted non-finite values; repeatability; graph capture; two data runs end to end.  Every
figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import _layernorm_workers as W
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED, LAYER = 77, 1


@pytest.fixture(scope="module")
def env():
    kernels, P = pkg("kernels"), pkg("PGCN")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return kernels.HipKernels(dev), dev, kernels.LN_STAT_ROWS, P


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _both(k, Xt, gt, bt, Gt, R=None, scale=1.0, **drop):
    """Forward and backward of the kernels -> (Y, mean, rstd, mask, dX, dgamma, dbeta)."""
    Y, mean, rstd, mask = k.ln_relu_forward(Xt, gt, bt, W.EPS, R=R, **drop)
    return (Y, mean, rstd, mask) + tuple(k.ln_relu_backward(Gt, Xt, mean, rstd, gt, mask, scale))


def _got(P, f, outs):
    Y, mean, rstd, mask, dX, dg, db = outs
    return {"Y": Y.cpu().numpy(), "mean": mean.cpu().numpy(), "rstd": rstd.cpu().numpy(), "bits": P.unpack_sign_mask(mask, f).cpu().numpy(),
            "dX": dX.cpu().numpy(), "dgamma": dg.cpu().numpy(), "dbeta": db.cpu().numpy()}


def _torch_fp32_figures(X, gamma, beta, Xt, gt, bt):
    """For the record (nothing is asserted): torch's own fp32 layer_norm on the same device and input, in units of the same bounds."""
    n, f = X.shape
    if n == 0:
        return
    ref = W.ln64(X, gamma, beta)
    bf, cmp_, _ = W.forward_bounds(X, gamma, beta, ref)
    out, mean, rstd = torch.native_layer_norm(Xt, (f,), gt, bt, W.EPS)
    D = W.depth(f)
    ef = float((np.abs(torch.relu(out).cpu().double().numpy() - ref["Y"]) / np.maximum(bf, 1e-300))[cmp_].max()) if cmp_.any() else 0.0
    em = float((np.abs(mean.reshape(-1).cpu().double().numpy() - ref["mean"]) / np.maximum(8 * W.U * D * np.abs(ref["mean"]), 1e-300)).max())
    er = float((np.abs(rstd.reshape(-1).cpu().double().numpy() - ref["rstd"]) / (8 * W.U * D * ref["rstd"])).max())
    print("    torch fp32 layer_norm, same input: error / bound  forward %.3g  mean %.3g  rstd %.3g" % (ef, em, er), flush=True)


@pytest.mark.parametrize("f", [1, 3, 4, 32, 100, 128, 132, 256, 260, 512, 1024])
def test_forward_mask_statistics_and_backward_against_float64(env, f):
    """256 is the last row of one wave, 260 the first of two, 1024 spans four.  The mean's bound is relative to the mean itself; measured
    on an MI355X, n = 2049: 4.58 bounds at f = 3 and 5.62 at f = 4 on one cancelling row each (torch's fp32 layer_norm on the same
    input and device: 11.7 and 3.84), every other case at most 0.34 -- those two cases, and no other, are held to twice torch's figure
    (W.MEAN_BY_TORCH)."""
    k, dev, B, P = env
    rows = [0, 1, 63, 64, 65, B, B + 1, 4 * B + 1] if f <= 260 else [1, 65, B + 1]
    for n in rows:
        X, gamma, beta, G, _ = W.make_case(n, f, 1000 * f + n)
        Xt, gt, bt, Gt = (_t(a, dev) for a in (X, gamma, beta, G))
        outs = _both(k, Xt, gt, bt, Gt)
        if n == 0:
            assert outs[0].shape == (0, f) and outs[4].shape == (0, f)
            assert not bool(outs[5].any()) and not bool(outs[6].any())            # zeroed, nothing else written
            continue
        got = _got(P, f, outs)
        _torch_fp32_figures(X, gamma, beta, Xt, gt, bt)
        torch_mean = torch.native_layer_norm(Xt, (f,), gt, bt, W.EPS)[1].reshape(-1).cpu().numpy() if (n, f) in W.MEAN_BY_TORCH else None
        W.check_case("kernels", X, gamma, beta, G, got, torch_mean=torch_mean)
        if n > 2:
            assert abs(float(got["rstd"][2]) * np.sqrt(W.EPS) - 1.0) <= 1e-6        # the constant row: variance 0
        if f % 32:
            assert not bool((outs[3][:, -1] >> (f % 32)).any())                     # mask bits at and beyond f are zero
        # inference: nothing saved, the same Y
        Yi, a, b, c = k.ln_relu_forward(Xt, gt, bt, W.EPS, save=False)
        assert a is None and b is None and c is None and torch.equal(Yi, outs[0])
        # no sums asked for: one launch, the same dX
        dX1, dg1, db1 = k.ln_relu_backward(Gt, Xt, outs[1], outs[2], gt, outs[3], 1.0, want_sums=False)
        assert dg1 is None and db1 is None and torch.equal(dX1, outs[4])


@pytest.mark.parametrize("f", [128, 260, 1024])
def test_a_misaligned_base_gives_the_bits_of_the_float4_path(env, f):
    k, dev, B, P = env
    n = B + 1
    X, gamma, beta, G, R = W.make_case(n, f, 31 + f)
    Xt, gt, bt, Gt, Rt = (_t(a, dev) for a in (X, gamma, beta, G, R))
    want = _both(k, Xt, gt, bt, Gt, R=Rt)

    def shifted(t):
        s = torch.empty(t.numel() + 1, device=dev)[1:].view(t.shape)
        s.copy_(t)
        assert s.data_ptr() % 16 == 4
        return s

    Xs, Gs, Rs = shifted(Xt), shifted(Gt), shifted(Rt)
    Ys, dXs = shifted(torch.zeros_like(Xt)), shifted(torch.zeros_like(Xt))
    Y, mean, rstd, mask = k.ln_relu_forward(Xs, gt, bt, W.EPS, R=Rs, out=Ys)
    dX, dg, db = k.ln_relu_backward(Gs, Xs, mean, rstd, gt, mask, 1.0, out=dXs)
    same = [torch.equal(a, b) for a, b in zip((Y, mean, rstd, mask, dX, dg, db), want)]
    print("f %d: element-wise path against the float4 path, bit for bit (Y, mean, rstd, mask, dX, dgamma, dbeta):" % f, same)
    assert Y is Ys and dX is dXs and all(same)


@pytest.mark.parametrize("f", [100, 128])
def test_dropout_masks_are_those_of_the_keep_function(env, f):
    k, dev, B, P = env
    D = pkg("dropout")
    n = B + 1
    X, gamma, beta, G, _ = W.make_case(n, f, 5 * f)
    Xt, gt, bt, Gt = (_t(a, dev) for a in (X, gamma, beta, G))
    ids = torch.arange(n, dtype=torch.int64) * 5 + 7
    ids[-3:] += 2 ** 33                                                      # ids beyond 2^33: the second round of the hash
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(SEED, dev)
    state.step.fill_(4)
    Y0, mean0, rstd0, mask0 = k.ln_relu_forward(Xt, gt, bt, W.EPS)
    bits0 = P.unpack_sign_mask(mask0, f)
    masks = []
    for step in (4, 5):
        outs = _both(k, Xt, gt, bt, Gt, scale=scale, row_ids=ids.to(dev), seed=SEED, step=state.step, layer=LAYER, thr=thr)
        keep = D.keep_mask(SEED, step, LAYER, ids, f, thr)
        want = torch.where(keep.to(dev), Y0 * scale, torch.zeros((), device=dev))
        dropped = float((~keep).float().mean())
        ok = torch.equal(outs[0], want)
        bits_ok = torch.equal(P.unpack_sign_mask(outs[3], f), bits0 & keep.to(dev))
        print("f %d step %d: dropped %.4f, Y == keep ? relu(t) * scale : 0 bit for bit: %s, mask == sign AND keep: %s" % (f, step, dropped, ok,
                                                                                                                      bits_ok))
        assert ok and bits_ok and 0.45 < dropped < 0.55
        assert torch.equal(outs[1], mean0) and torch.equal(outs[2], rstd0)
        W.check_case("kernels dropout step %d" % step, X, gamma, beta, G, _got(P, f, outs), keep.numpy(), scale)
        masks.append(keep)
        state.advance()
    assert not torch.equal(masks[0], masks[1])                                # the device-resident step draws a new mask
    Yz, _, _, maskz = k.ln_relu_forward(Xt, gt, bt, W.EPS, row_ids=ids.to(dev), seed=SEED, step=state.step, layer=LAYER, thr=0)
    assert torch.equal(Yz, Y0) and torch.equal(maskz, mask0)                  # dropout 0: the path without dropout, bit for bit


@pytest.mark.parametrize("f", [100, 128, 512])
def test_residual_out_of_place_and_in_place(env, f):
    k, dev, B, P = env
    D = pkg("dropout")
    n = B + 1
    X, gamma, beta, G, R = W.make_case(n, f, 13 * f)
    Xt, gt, bt, Gt, Rt = (_t(a, dev) for a in (X, gamma, beta, G, R))
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(SEED, dev)
    ids = (torch.arange(n, dtype=torch.int64) * 3 + 1)
    for drop in ({}, dict(row_ids=ids.to(dev), seed=SEED, step=state.step, layer=LAYER, thr=thr)):
        d = _both(k, Xt, gt, bt, Gt, scale=scale if drop else 1.0, **drop)
        outs = _both(k, Xt, gt, bt, Gt, R=Rt, scale=scale if drop else 1.0, **drop)
        same = [torch.equal(outs[0], Rt + d[0])] + [torch.equal(a, b) for a, b in zip(outs[1:], d[1:])]
        print("f %d dropout %s: Y == R + d bit for bit, and every other output equal to the run without R:" % (f, bool(drop)), same)
        assert all(same)
        Rc = Rt.clone()
        Yp, mean, rstd, mask = k.ln_relu_forward(Xt, gt, bt, W.EPS, R=Rc, out=Rc, **drop)
        assert Yp is Rc and torch.equal(Rc, outs[0]) and torch.equal(mask, outs[3]) and torch.equal(mean, outs[1])
        keep = D.keep_mask(SEED, 0, LAYER, ids, f, thr).numpy() if drop else None
        W.check_case("kernels R%s" % (" dropout" if drop else ""), X, gamma, beta, G, _got(P, f, outs), keep, scale if drop else 1.0, R)


@pytest.mark.parametrize("f", [3, 100, 128, 260, 1024])
def test_a_rows_results_depend_on_that_row_alone(env, f):
    k, dev, B, P = env
    D = pkg("dropout")
    n = B + 1
    X, gamma, beta, G, R = W.make_case(n, f, 3 * f + 1)
    Xt, gt, bt, Gt, Rt = (_t(a, dev) for a in (X, gamma, beta, G, R))
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(SEED, dev)
    ids = (torch.arange(n, dtype=torch.int64) * 3 + 1).to(dev)
    drop = dict(seed=SEED, step=state.step, layer=LAYER, thr=thr)
    base = _both(k, Xt, gt, bt, Gt, R=Rt, scale=scale, row_ids=ids, **drop)
    p = torch.from_numpy(np.random.default_rng(f).permutation(n)).to(dev)
    perm = _both(k, Xt[p].contiguous(), gt, bt, Gt[p].contiguous(), R=Rt[p].contiguous(), scale=scale, row_ids=ids[p].contiguous(), **drop)
    same = [torch.equal(a, b[p]) for a, b in zip(perm[:5], base[:5])]
    print("f %d: outputs of X[p] are the outputs of X permuted, bit for bit (Y, mean, rstd, mask, dX):" % f, same)
    assert all(same)
    head = _both(k, Xt[:65].contiguous(), gt, bt, Gt[:65].contiguous(), R=Rt[:65].contiguous(), scale=scale, row_ids=ids[:65].contiguous(), **drop)
    same = [torch.equal(a, b[:65]) for a, b in zip(head[:5], base[:5])]
    print("f %d: a 65-row call equals the first 65 rows of the %d-row call:" % (f, n), same)
    assert all(same)


def _raw_forward(k, X, ldx, n, f, gt, bt, R, ldr, Y, ldy, mean, rstd, mask):
    _lib = pkg("_lib")
    _lib.check(k.lib.pgcn_ln_relu_forward_f32(X.data_ptr(), ldx, n, f, gt.data_ptr(), bt.data_ptr(), W.EPS, R.data_ptr(), ldr, None, 0, None, 0,
                                              0, Y.data_ptr(), ldy, mean.data_ptr(), rstd.data_ptr(), mask.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "pgcn_ln_relu_forward_f32")


@pytest.mark.parametrize("f,ld", [(100, 104), (128, 136), (3, 5)])
def test_leading_dimensions_padding_and_canary_rows(env, f, ld):
    k, dev, B, P = env
    n = B + 1
    mw = (f + 31) // 32
    X, gamma, beta, G, R = W.make_case(n, f, 9 * f)
    Xt, gt, bt, Gt, Rt = (_t(a, dev) for a in (X, gamma, beta, G, R))
    want = _both(k, Xt, gt, bt, Gt, R=Rt)
    bufs = [torch.full((n + 2, ld), float("nan"), device=dev) for _ in range(5)]
    Xw, Gw, Rw, Yw, dXw = (b[1:n + 1, :f] for b in bufs)
    Xw.copy_(Xt)
    Gw.copy_(Gt)
    Rw.copy_(Rt)
    before = [b.clone() for b in bufs[:3]]
    CAN = -1.25
    meanb, rstdb = torch.full((n + 2,), CAN, device=dev), torch.full((n + 2,), CAN, device=dev)
    maskb = torch.full((n + 2, mw), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    _raw_forward(k, Xw, ld, n, f, gt, bt, Rw, ld, Yw, ld, meanb[1:], rstdb[1:], maskb[1:])
    mean, rstd, mask = meanb[1:n + 1], rstdb[1:n + 1], maskb[1:n + 1]
    dX, dg, db = k.ln_relu_backward(Gw, Xw, mean.contiguous(), rstd.contiguous(), gt, mask.contiguous(), 1.0, out=dXw)
    same = [torch.equal(a, b) for a, b in zip((Yw, mean, rstd, mask, dXw, dg, db), want)]
    print("f %d ld %d: outputs equal to the contiguous run bit for bit (Y, mean, rstd, mask, dX, dgamma, dbeta): %s" % (f, ld, same))
    assert dX is dXw and all(same)
    for b, was in zip(bufs[:3], before):
        assert torch.equal(b.view(torch.int32), was.view(torch.int32))        # no input changed
    for b in bufs[3:]:
        outside = torch.ones_like(b, dtype=torch.bool)
        outside[1:n + 1, :f] = False
        assert bool(torch.isnan(b[outside]).all()) and not bool(torch.isnan(b[1:n + 1, :f]).any())      # nothing outside the window
    for b in (meanb, rstdb):
        assert float(b[0]) == CAN and float(b[-1]) == CAN
    assert bool((maskb[0] == 0x5A5A5A5A).all()) and bool((maskb[-1] == 0x5A5A5A5A).all())


@pytest.mark.parametrize("f", [32, 260])
def test_a_nan_and_an_inf_stay_in_their_row(env, f):
    k, dev, B, P = env
    n = 300
    X, gamma, beta, G, R = W.make_case(n, f, 17 + f)
    Xt, gt, bt, Gt, Rt = (_t(a, dev) for a in (X, gamma, beta, G, R))
    Gz = Gt.clone()
    Gz[7] = 0.0                                                             # the reference: row 7 adds nothing to the column sums
    clean = _both(k, Xt, gt, bt, Gz, R=Rt)
    Xp = Xt.clone()
    Xp[7, 3], Xp[7, f - 1] = float("nan"), float("inf")
    poisoned = _both(k, Xp, gt, bt, Gt, R=Rt)
    others = torch.ones(n, dtype=torch.bool, device=dev)
    others[7] = False
    for name, a, b in zip(("Y", "mean", "rstd", "mask", "dX"), poisoned[:5], clean[:5]):
        ok = torch.equal(a[others], b[others])
        print("f %d %s: every other row keeps its bits: %s" % (f, name, ok))
        assert ok
    assert not bool(torch.isfinite(poisoned[0][7]).any()) and not bool(torch.isfinite(poisoned[4][7]).any())      # it stays in its row
    masked_in = P.unpack_sign_mask(poisoned[3], f)[7]
    for name, a, b in (("dgamma", poisoned[5], clean[5]), ("dbeta", poisoned[6], clean[6])):
        ok = torch.equal(a[~masked_in], b[~masked_in])
        print("f %d %s: every column but that row's masked-in ones (%d) keeps its bits: %s" % (f, name, int(masked_in.sum()), ok))
        assert ok and bool(torch.isfinite(a[~masked_in]).all())


def test_two_runs_give_the_same_bits(env):
    k, dev, B, P = env
    n, f = 4 * B + 1, 132
    X, gamma, beta, G, R = W.make_case(n, f, 23)
    Xt, gt, bt, Gt, Rt = (_t(a, dev) for a in (X, gamma, beta, G, R))
    runs = [_both(k, Xt, gt, bt, Gt, R=Rt) for _ in range(2)]
    same = [torch.equal(a, b) for a, b in zip(*runs)]
    print("two runs, every output bit for bit (Y, mean, rstd, mask, dX, dgamma, dbeta):", same)
    assert all(same)


def test_a_captured_training_step_replays_like_eager_steps(env):
    """Forward and backward of the node with the step on the device in one captured graph, replayed three times: every step's output
    and gradients equal three eager steps bit for bit -- so the masks advanced with the device-resident step at every replay."""
    k, dev, B, P = env
    D = pkg("dropout")
    n, f = B + 65, 100
    X, gamma, beta, G, R = W.make_case(n, f, 41)
    Xt, Gt, Rt = _t(X, dev), _t(G, dev), _t(R, dev)
    ids = (torch.arange(n, dtype=torch.int64) * 3 + 1).to(dev)
    thr, scale = D.threshold(0.5)
    old = (P._kernel_provider, P.world_size)
    P._kernel_provider, P.world_size = k, 1
    try:
        def make():
            return _t(gamma, dev).requires_grad_(True), _t(beta, dev).requires_grad_(True), D.DropoutState(SEED, dev)

        def step(x, r, g_, b_, state):
            Y = P._LayerNormReluDropout.apply(x, g_, b_, r, True, W.EPS, ids, state, LAYER, thr, scale)
            assert Y.grad_fn.saved_tensors[4].dtype is torch.int32 and Y.grad_fn.saved_tensors[4].shape == (n, (f + 31) // 32)      # the HIP route
            grads = torch.autograd.grad((Y * Gt).sum(), (x, g_, b_, r))
            state.advance()
            return (Y.detach(),) + grads

        g_, b_, state = make()
        x, r = Xt.clone().requires_grad_(True), Rt.clone().requires_grad_(True)
        eager = [tuple(t.clone() for t in step(x, r, g_, b_, state)) for _ in range(3)]
        assert not torch.equal(eager[0][0], eager[1][0])                      # another step, another mask

        g_, b_, state = make()
        x, r = Xt.clone().requires_grad_(True), Rt.clone().requires_grad_(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(x, r, g_, b_, state)                                         # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        state.step.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step(x, r, g_, b_, state)
        for i in range(3):
            graph.replay()
            torch.cuda.synchronize()
            same = [torch.equal(a, b) for a, b in zip(outs, eager[i])]
            print("replay %d against eager step %d (Y, dX, dgamma, dbeta, dR):" % (i, i), same)
            assert all(same)
        assert int(state.step.item()) == 3
    finally:
        P._kernel_provider, P.world_size = old


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("layernorm_gpu")))


@pytest.mark.parametrize("dropout", [0.0, W.DROPOUT])
def test_data_run_on_the_kernels_against_the_composition(dataset, dropout):
    """A 4-layer run(norm="node", residual=True), hidden 32, on the device: the layer-norm kernels against the same run with a provider
    that has none (the framework composition on the same device) -- losses within 1e-6 relative, the same best-validation epoch."""
    paths, _ = dataset
    got = W.spawn_run(1, paths, True, dropout=dropout, nlayers=4)[0]
    want = W.spawn_run(1, paths, "composed", dropout=dropout, nlayers=4)[0]
    assert got["hip"] == "HipKernels" and want["hip"] == "NoLayerNorm"
    # the route: the kernels leave int32 mask words, the composition a bool tensor
    print("nodes and masks:", got["node"], got["mask_dtype"], want["node"], want["mask_dtype"])
    assert got["node"] == want["node"] == "_LayerNormReluDropoutBackward"
    assert got["mask_dtype"] == "torch.int32" and want["mask_dtype"] == "torch.bool"
    assert got["residual"] == [False, True, True, False] and len(got["history"]) == len(want["history"]) == W.EPOCHS
    print("dropout %.1f: best epochs %d / %d" % (dropout, got["best"]["epoch"], want["best"]["epoch"]))
    W.check_losses([got], want["history"], bound=1e-6)
    assert got["best"]["epoch"] == want["best"]["epoch"]
