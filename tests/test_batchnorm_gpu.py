"""The batch-norm kernels of csrc/pgcn_norm.hip on the device, against the float64 definition (tests/_batchnorm_workers.py) evaluated
on the same fp32 inputs: column sums, the forward and backward bounds, dropout masks, layout (leading dimensions, poisoned padding,
canary rows, a misaligned base), column independence, repeatability, graph capture and a data run end to end.  Every figure is
printed before it is asserted."""
import numpy as np
import pytest
import torch

import _batchnorm_workers as W
from conftest import pkg

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SEED, LAYER = 77, 1


@pytest.fixture(scope="module")
def env():
    kernels, P = pkg("kernels"), pkg("PGCN")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return kernels.HipKernels(dev), dev, kernels.BN_STAT_ROWS, P


def _inputs(n, f, seed):
    """X with a column of mean 1000 and std 1, one of mean 0 and std 1e-3, a constant one (where f allows), the rest spread."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, f)) * rng.uniform(0.1, 3.0, f) + rng.uniform(-2.0, 2.0, f)
    X[:, 0] = 1000.0 + rng.standard_normal(n)
    if f > 1:
        X[:, 1] = 1e-3 * rng.standard_normal(n)
    if f > 2:
        X[:, 2] = 0.75
    return (X.astype(np.float32), rng.uniform(0.5, 1.5, f).astype(np.float32), rng.uniform(-0.5, 0.5, f).astype(np.float32),
            rng.standard_normal((n, f)).astype(np.float32))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _forward(k, X, gamma, beta, rm=None, rv=None, training=True, **drop):
    f = X.shape[1]
    sums = k.bn_colstats(X) if training else None
    mean, invstd = k.bn_prepare(sums, f, W.EPS, W.MOMENTUM, training, rm, rv)
    return sums, mean, invstd, k.bn_relu_apply(X, mean, invstd, gamma, beta, **drop)


def _backward(k, G, Y, X, mean, invstd, gamma, n_global, scale=1.0):
    sums, dg, db = k.bn_backward_stats(G, Y, X, mean, invstd, scale)
    return sums, dg, db, k.bn_relu_backward(G, Y, X, mean, invstd, gamma, sums, n_global, scale)


def _check_forward(Y, X, gamma, beta, scale=1.0, keep=None):
    Xd, gd, bd = X.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64)
    Y64, mean, invstd = W.bn64(Xd, gd, bd, keep=keep, scale=scale)
    bound = 4 * U * scale * (np.abs(gd) * invstd * (np.abs(Xd) + np.abs(mean)) + np.abs(bd))
    err = np.abs(Y.astype(np.float64) - Y64)
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0, mean, invstd


def _check_backward(dX, dg, db, G, Y, X, gamma, mean, invstd, scale, n):
    """The three error / bound ratios, the kernel's own Y as the mask on both sides."""
    Xd, Gd, gd = X.astype(np.float64), G.astype(np.float64), gamma.astype(np.float64)
    dX64, dg64, db64, S1, S2 = W.bn_backward64(Gd, Y, Xd, mean, invstd, gd, scale)
    gm = np.abs(np.where(Y > 0, Gd * scale, 0.0))
    xh, R = np.abs((Xd - mean) * invstd), np.abs(mean) * invstd
    bx = 16 * U * np.abs(gd) * invstd * (gm + np.abs(S1) / n + (xh + R) * np.abs(S2) / n)
    bg, bb = 4 * U * (gm * (xh + R)).sum(0), 2 * U * gm.sum(0)

    def ratio(got, want, bound):
        e = np.abs(got.astype(np.float64) - want)
        return float(np.where(e > 0, e / np.maximum(bound, 1e-300), 0.0).max())

    return ratio(dX, dX64, bx), ratio(dg, dg64, bg), ratio(db, db64, bb)


@pytest.mark.parametrize("f", [1, 3, 4, 32, 100, 128, 132, 1024])
def test_statistics_forward_and_backward_against_float64(env, f):
    k, dev, B, _ = env
    rows = [0, 1, 63, 64, 65, B, B + 1, 4 * B + 1] if f < 1024 else [1, 65, B + 1]
    for n in rows:
        X, gamma, beta, G = _inputs(n, f, 1000 * f + n)
        Xt, gt, bt, Gt = (_t(a, dev) for a in (X, gamma, beta, G))
        rm, rv = torch.zeros(f, device=dev), torch.ones(f, device=dev)
        sums, mean, invstd, Y = _forward(k, Xt, gt, bt, rm, rv)
        s = sums.cpu().numpy()
        Xd = X.astype(np.float64)
        e1 = np.abs(s[:f] - Xd.sum(0)) / np.maximum(np.abs(Xd).sum(0), 1e-300)
        e2 = np.abs(s[f:2 * f] - (Xd * Xd).sum(0)) / np.maximum((Xd * Xd).sum(0), 1e-300)
        print("f %d n %d: column sums %.3g, sums of squares %.3g (relative)" % (f, n, e1.max() if n else 0, e2.max() if n else 0))
        assert s[2 * f] == n
        if n == 0:
            assert not s.any() and Y.shape == (0, f)
            assert torch.equal(rm, torch.zeros_like(rm)) and torch.equal(rv, torch.ones_like(rv))      # no vertex: no record
            continue
        assert e1.max() <= 1e-12 and e2.max() <= 1e-12
        Yn = Y.cpu().numpy()
        rf, mean64, invstd64 = _check_forward(Yn, X, gamma, beta)
        m64, var64, _ = W.stats64(Xd)
        wm, wv = W.running64(np.zeros(f), np.ones(f), m64, var64, n)
        er = max(np.abs(rm.cpu().numpy() - wm).max() / max(1.0, np.abs(wm).max()), np.abs(rv.cpu().numpy() - wv).max() / max(1.0, np.abs(wv).max()))
        if f > 2:
            assert abs(float(invstd[2]) * np.sqrt(W.EPS) - 1.0) <= 1e-6            # the constant column: var = 0
        _, dg, db, dX = _backward(k, Gt, Y, Xt, mean, invstd, gt, n)
        rx, rg, rb = _check_backward(dX.cpu().numpy(), dg.cpu().numpy(), db.cpu().numpy(), G, Yn, X, gamma, mean64, invstd64, 1.0, n)
        print("f %d n %d: error / bound forward %.3g, dX %.3g, dgamma %.3g, dbeta %.3g; running statistics %.3g" % (f, n, rf, rx, rg, rb, er))
        assert rf <= 1.0 and rx <= 1.0 and rg <= 1.0 and rb <= 1.0 and er <= 1e-6


@pytest.mark.parametrize("f", [100, 128])
def test_dropout_masks_are_those_of_the_keep_function(env, f):
    k, dev, B, _ = env
    D = pkg("dropout")
    n = B + 1
    X, gamma, beta, G = _inputs(n, f, 5 * f)
    Xt, gt, bt, Gt = (_t(a, dev) for a in (X, gamma, beta, G))
    ids = torch.arange(n, dtype=torch.int64) * 5 + 7
    ids[-3:] += 2 ** 33                                                      # ids beyond 2^32: the second round of the hash
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(SEED, dev)
    state.step.fill_(4)
    _, mean, invstd, Y0 = _forward(k, Xt, gt, bt)
    masks = []
    for step in (4, 5):
        Y1 = k.bn_relu_apply(Xt, mean, invstd, gt, bt, row_ids=ids.to(dev), seed=SEED, step=state.step, layer=LAYER, thr=thr)
        keep = D.keep_mask(SEED, step, LAYER, ids, f, thr)
        want = torch.where(keep.to(dev), Y0 * scale, torch.zeros((), device=dev))
        dropped = float((~keep).float().mean())
        print("f %d step %d: dropped %.4f, output equal to keep ? y * scale : 0 bit for bit: %s" % (f, step, dropped, torch.equal(Y1, want)))
        assert torch.equal(Y1, want) and 0.45 < dropped < 0.55
        assert torch.equal((Y1 == 0).cpu(), ~keep | (Y0 == 0).cpu())            # zeros exactly where the keep function drops
        masks.append(keep)
        state.advance()
    assert not torch.equal(masks[0], masks[1])                                # the device-resident step draws a new mask
    rf, mean64, invstd64 = _check_forward(Y1.cpu().numpy(), X, gamma, beta, scale, masks[1].numpy())
    _, dg, db, dX = _backward(k, Gt, Y1, Xt, mean, invstd, gt, n, scale)
    rx, rg, rb = _check_backward(dX.cpu().numpy(), dg.cpu().numpy(), db.cpu().numpy(), G, Y1.cpu().numpy(), X, gamma, mean64, invstd64, scale, n)
    print("f %d with dropout: error / bound forward %.3g, dX %.3g, dgamma %.3g, dbeta %.3g" % (f, rf, rx, rg, rb))
    assert rf <= 1.0 and rx <= 1.0 and rg <= 1.0 and rb <= 1.0
    Yz = k.bn_relu_apply(Xt, mean, invstd, gt, bt, row_ids=ids.to(dev), seed=SEED, step=state.step, layer=LAYER, thr=0)
    assert torch.equal(Yz, Y0)                                                # dropout 0: the path without dropout, bit for bit


def _windows(n, f, ld, dev, count):
    """`count` (buffer, window) pairs: (n + 2) x ld buffers of NaN whose rows 1 .. n, columns 0 .. f - 1 are the window."""
    bufs = [torch.full((n + 2, ld), float("nan"), device=dev) for _ in range(count)]
    return bufs, [b[1:n + 1, :f] for b in bufs]


@pytest.mark.parametrize("f,ld", [(100, 104), (128, 136), (3, 5)])
def test_leading_dimensions_padding_and_canary_rows(env, f, ld):
    k, dev, B, _ = env
    n = B + 1
    X, gamma, beta, G = _inputs(n, f, 9 * f)
    Xt, gt, bt, Gt = (_t(a, dev) for a in (X, gamma, beta, G))
    _, mean, invstd, Y = _forward(k, Xt, gt, bt)
    bs, dg, db, dX = _backward(k, Gt, Y, Xt, mean, invstd, gt, n)
    bufs, (Xw, Gw, Yw, dXw) = _windows(n, f, ld, dev, 4)
    Xw.copy_(Xt)
    Gw.copy_(Gt)
    before = [b.clone() for b in bufs]
    sums_w = k.bn_colstats(Xw)
    mean_w, invstd_w = k.bn_prepare(sums_w, f, W.EPS, W.MOMENTUM, True, None, None)
    assert k.bn_relu_apply(Xw, mean_w, invstd_w, gt, bt, out=Yw) is Yw
    bs_w, dg_w, db_w = k.bn_backward_stats(Gw, Yw, Xw, mean_w, invstd_w, 1.0)
    assert k.bn_relu_backward(Gw, Yw, Xw, mean_w, invstd_w, gt, bs_w, n, 1.0, out=dXw) is dXw
    same = [torch.equal(a, b) for a, b in ((mean_w, mean), (invstd_w, invstd), (Yw, Y), (bs_w, bs), (dg_w, dg), (db_w, db), (dXw, dX))]
    print("f %d ld %d: outputs equal to the contiguous run bit for bit: %s" % (f, ld, same))
    assert all(same)
    for b, was in zip(bufs[:2], before[:2]):
        assert torch.equal(b.view(torch.int32), was.view(torch.int32))        # no input changed
    for b in bufs[2:]:
        outside = torch.ones_like(b, dtype=torch.bool)
        outside[1:n + 1, :f] = False
        assert bool(torch.isnan(b[outside]).all()) and not bool(torch.isnan(b[1:n + 1, :f]).any())      # nothing outside the window


def test_a_misaligned_base_gives_the_bits_of_the_aligned_run(env):
    k, dev, B, _ = env
    n, f = B + 1, 128
    X, gamma, beta, G = _inputs(n, f, 31)
    Xt, gt, bt, Gt = (_t(a, dev) for a in (X, gamma, beta, G))
    sums, mean, invstd, Y = _forward(k, Xt, gt, bt)
    bs, dg, db, dX = _backward(k, Gt, Y, Xt, mean, invstd, gt, n)

    def shifted(t):
        s = torch.empty(t.numel() + 1, device=dev)[1:].view(t.shape)
        s.copy_(t)
        assert s.data_ptr() % 16 == 4
        return s

    Xs, Gs = shifted(Xt), shifted(Gt)
    Ys, dXs = shifted(torch.zeros_like(Xt)), shifted(torch.zeros_like(Xt))
    sums_s = k.bn_colstats(Xs)
    mean_s, invstd_s = k.bn_prepare(sums_s, f, W.EPS, W.MOMENTUM, True, None, None)
    k.bn_relu_apply(Xs, mean_s, invstd_s, gt, bt, out=Ys)
    bs_s, dg_s, db_s = k.bn_backward_stats(Gs, Ys, Xs, mean_s, invstd_s, 1.0)
    k.bn_relu_backward(Gs, Ys, Xs, mean_s, invstd_s, gt, bs_s, n, 1.0, out=dXs)
    same = [torch.equal(a, b) for a, b in ((sums_s, sums), (mean_s, mean), (invstd_s, invstd), (Ys, Y), (bs_s, bs), (dg_s, dg), (db_s, db),
                                           (dXs, dX))]
    print("element-wise path against the float4 path, bit for bit:", same)
    assert all(same)


def test_a_nan_and_an_inf_stay_in_their_columns(env):
    k, dev, B, _ = env
    n, f = 300, 32
    X, gamma, beta, G = _inputs(n, f, 17)
    Xt, gt, bt, Gt = (_t(a, dev) for a in (X, gamma, beta, G))
    sums, mean, invstd, Y = _forward(k, Xt, gt, bt)
    bs, dg, db, dX = _backward(k, Gt, Y, Xt, mean, invstd, gt, n)
    Xp = Xt.clone()
    Xp[5, 3], Xp[7, 9] = float("nan"), float("inf")
    sums_p, mean_p, invstd_p, Yp = _forward(k, Xp, gt, bt)
    bs_p, dg_p, db_p, dXp = _backward(k, Gt, Yp, Xp, mean_p, invstd_p, gt, n)
    clean = torch.ones(f, dtype=torch.bool, device=dev)
    clean[[3, 9]] = False
    for name, a, b in (("mean", mean_p, mean), ("invstd", invstd_p, invstd), ("Y", Yp, Y), ("dX", dXp, dX), ("dgamma", dg_p, dg),
                       ("dbeta", db_p, db), ("sums", sums_p[:2 * f].view(2, f), sums[:2 * f].view(2, f)), ("bsums", bs_p.view(2, f), bs.view(2, f))):
        ok = torch.equal(a[..., clean], b[..., clean])
        print("%s: the other columns keep their bits: %s" % (name, ok))
        assert ok
    assert not bool(torch.isfinite(sums_p[[3, 9]]).any()) and not bool(torch.isfinite(Yp[:, [3, 9]]).any())
    assert not bool(torch.isfinite(mean_p[[3, 9]]).any()) and not bool(torch.isfinite(dXp[:, [3, 9]]).any())


def test_two_runs_give_the_same_bits(env):
    k, dev, B, _ = env
    n, f = 4 * B + 1, 132
    X, gamma, beta, G = _inputs(n, f, 23)
    Xt, gt, bt, Gt = (_t(a, dev) for a in (X, gamma, beta, G))
    runs = []
    for _ in range(2):
        sums, mean, invstd, Y = _forward(k, Xt, gt, bt)
        runs.append((sums, mean, invstd, Y) + _backward(k, Gt, Y, Xt, mean, invstd, gt, n))
    same = [torch.equal(a, b) for a, b in zip(*runs)]
    print("two runs, every output bit for bit:", same)
    assert all(same)


def test_a_captured_training_step_replays_like_eager_steps(env):
    """Statistics, prepare, apply and the backward of the node in one captured graph, replayed three times: the running statistics and
    every step's output and gradients equal three eager steps bit for bit -- so the masks advanced with the device-resident step and
    the running statistics were updated from device memory at every replay."""
    k, dev, B, P = env
    D = pkg("dropout")
    n, f = B + 65, 100
    X, gamma, beta, G = _inputs(n, f, 41)
    Xt, Gt = _t(X, dev), _t(G, dev)
    ids = (torch.arange(n, dtype=torch.int64) * 3 + 1).to(dev)
    thr, scale = D.threshold(0.5)
    old = (P._kernel_provider, P.world_size)
    P._kernel_provider, P.world_size = k, 1
    try:
        def make():
            return (_t(gamma, dev).requires_grad_(True), _t(beta, dev).requires_grad_(True), torch.zeros(f, device=dev),
                    torch.ones(f, device=dev), D.DropoutState(SEED, dev))

        def step(x, g_, b_, rm, rv, state):
            Y = P._BatchNormReluDropout.apply(x, g_, b_, (rm, rv), True, W.MOMENTUM, W.EPS, n, ids, state, LAYER, thr, scale)
            grads = torch.autograd.grad((Y * Gt).sum(), (x, g_, b_))
            state.advance()
            return (Y.detach(),) + grads

        g_, b_, rm, rv, state = make()
        x = Xt.clone().requires_grad_(True)
        eager = [tuple(t.clone() for t in step(x, g_, b_, rm, rv, state)) for _ in range(3)]
        assert not torch.equal(eager[0][0] == 0, eager[1][0] == 0)
        want_rm, want_rv = rm.clone(), rv.clone()

        g_, b_, rm, rv, state = make()
        x = Xt.clone().requires_grad_(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(x, g_, b_, rm, rv, state)                                    # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        rm.zero_()
        rv.fill_(1.0)
        state.step.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step(x, g_, b_, rm, rv, state)
        for i in range(3):
            graph.replay()
            torch.cuda.synchronize()
            same = [torch.equal(a, b) for a, b in zip(outs, eager[i])]
            print("replay %d against eager step %d (Y, dX, dgamma, dbeta):" % (i, i), same)
            assert all(same)
        assert torch.equal(rm, want_rm) and torch.equal(rv, want_rv) and int(state.step.item()) == 3
    finally:
        P._kernel_provider, P.world_size = old


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return W.make_dataset(str(tmp_path_factory.mktemp("batchnorm_gpu")))


@pytest.mark.parametrize("dropout,optimizer", [(0.0, None), (W.DROPOUT, "fused")])
def test_data_run_on_the_kernels_against_the_composition(dataset, dropout, optimizer):
    """A 3-layer run(norm="batch") on the device: the batch-norm kernels against the same run with a provider that has none (the
    framework composition on the same device) -- losses within 1e-5 (relative, floor 1), the same best-validation epoch."""
    paths, _ = dataset
    got = W.spawn_run(1, paths, True, dropout=dropout, optimizer=optimizer)[0]
    want = W.spawn_run(1, paths, "composed", dropout=dropout, optimizer=optimizer)[0]
    assert got["hip"] == "HipKernels" and want["hip"] == "NoNorm"
    worst = 0.0
    for a, b in zip(got["history"], want["history"]):
        for name in W.SETS:
            worst = max(worst, abs(a["losses"][name] - b["losses"][name]) / max(1.0, abs(b["losses"][name])))
    print("dropout %.1f optimizer %s: largest loss difference %.3g; best epochs %d / %d" % (dropout, optimizer, worst, got["best"]["epoch"],
                                                                                         want["best"]["epoch"]))
    assert len(got["history"]) == len(want["history"]) == W.EPOCHS and worst <= 1e-5
    assert got["best"]["epoch"] == want["best"]["epoch"]
    for (rm, rv), (wm, wv) in zip(got["running"], want["running"]):
        assert np.abs(rm - wm).max() <= 1e-5 * max(1.0, np.abs(wm).max()) and np.abs(rv - wv).max() <= 1e-5 * max(1.0, np.abs(wv).max())
