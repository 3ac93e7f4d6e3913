"""The GAT tail kernels of csrc/pgcn_gat_tail.hip on the device against their fp32 statement in numpy (tests/_gat_tail_workers.py) and
float64 column sums: every width class in both head modes, the ELU bound, the band boundaries, dropout masks, layout (leading
dimensions, canary rows, in place, a misaligned base), non-finite operands, repeatability, refusals, graph capture and data runs end
to end against a dense float64 GAT.  Every figure is printed before it is asserted.

The ELU bound: where expm1 is involved the output may be 3 ulp from float64 expm1 rounded to fp32 (the accuracy class of expm1 in the
OpenCL profile the device math library is written to), plus 1 ulp when the dropout scale multiplies it (one more rounding)."""
import itertools

import numpy as np
import pytest
import torch

import _gat_tail_workers as W
from conftest import held_to_fixture, pkg

pytestmark = pytest.mark.gpu

SEED, LAYER = 77, 1
EINVAL, ENOMEM = -1, -4


@pytest.fixture(scope="module")
def env():
    kernels, M = pkg("kernels"), pkg("PGAT")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return kernels.HipKernels(dev), dev, kernels.GAT_TAIL_SUM_ROWS, M


def _inputs(n, K, d, mean, seed):
    rng = np.random.default_rng(seed)
    fout = d if mean else K * d
    x = rng.standard_normal((n, K * d)).astype(np.float32)
    return x, rng.standard_normal(fout).astype(np.float32), rng.standard_normal((n, fout)).astype(np.float32)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(k, dev, n, K, d, seed):
    """Both head modes x bias present / absent x act 0 / 1 at one shape, without dropout; returns (largest ELU distance in ulp,
    largest dbias error / bound)."""
    worst_ulp, worst_db = 0.0, 0.0
    for mean in (False, True):
        x, b, G = _inputs(n, K, d, mean, seed + int(mean))
        Xt, Bt, Gt = (_t(a, dev) for a in (x, b, G))
        fout = d if mean else K * d
        for present, act in itertools.product((True, False), (0, 1)):
            case = (n, K, d, mean, present, act)
            Y = k.gat_tail_forward(Xt, K, d, mean, Bt if present else None, act)
            want, exact = W.tail32(x, K, d, mean, b if present else None, act)
            Yn = Y.cpu().numpy()
            assert Yn.shape == (n, fout) and np.array_equal(_bits(Yn[exact]), _bits(want[exact])), case
            if act and n:
                u = float(W.ulps(Yn, want).max())
                worst_ulp = max(worst_ulp, u)
                assert u <= 3, (case, u)
            dX, db = k.gat_tail_backward(Gt, Y if act else None, K, d, mean, act)
            dx32, gm32 = W.tail_backward32(G, Yn, K, d, mean, act)
            assert dX.shape == (n, K * d) and np.array_equal(_bits(dX.cpu().numpy()), _bits(dx32)), case
            err, bound = W.dbias_error_and_bound(db.cpu().numpy(), gm32)
            if n == 0:
                assert not db.cpu().numpy().any()
            else:
                worst_db = max(worst_db, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), case
            only, db2 = k.gat_tail_backward(Gt, Y if act else None, K, d, mean, act, want_dx=False)
            assert only is None and torch.equal(db2, db), case                       # sums only (dX == NULL): the same bits
            dX3, none = k.gat_tail_backward(Gt, Y if act else None, K, d, mean, act, want_dbias=False)
            assert none is None and torch.equal(dX3, dX), case                       # no sums: one launch, the same bits
    return worst_ulp, worst_db


@pytest.mark.parametrize("K,d", [(1, 1), (1, 3), (3, 1), (4, 8), (4, 33), (2, 50), (8, 32), (4, 64), (1, 1024)])
def test_kernels_against_the_fp32_statement_and_the_elu_bound(env, K, d):
    k, dev, B, _ = env
    u, worst = _check(k, dev, B + 65, K, d, 1000 + 10 * K + d)
    print("heads %d d %d n %d: forward bit-equal off the expm1 branch, dX bit-equal; ELU at most %.3g ulp from fp32(expm1 in double) "
          "(bound 3); dbias error / bound %.3g" % (K, d, B + 65, u, worst))


@pytest.mark.parametrize("n", [0, 1, 2 * 512 + 1])
def test_kernels_at_the_band_boundaries(env, n):
    k, dev, B, _ = env
    assert B == 512
    u, worst = _check(k, dev, n, 2, 50, 2000 + n)
    print("heads 2 d 50 n %d: bit-equal; ELU %.3g ulp; dbias error / bound %.3g" % (n, u, worst))


@pytest.mark.parametrize("K,d,mean", [(4, 8, False), (2, 50, True), (4, 64, True)])
def test_dropout_masks_are_those_of_the_keep_function(env, K, d, mean):
    k, dev, B, _ = env
    D = pkg("dropout")
    n = B + 65
    fout = d if mean else K * d
    x, b, G = _inputs(n, K, d, mean, 5 * d)
    Xt, Bt, Gt = (_t(a, dev) for a in (x, b, G))
    ids = torch.arange(n, dtype=torch.int64) * 3 + 1
    ids[-1] += 2 ** 32                                                       # an id beyond 2^32: the second round of the hash
    idt = ids.to(dev)
    thr, scale = D.threshold(0.5)
    state = D.DropoutState(SEED, dev)
    state.step.fill_(4)
    a0, _ = W.tail32(x, K, d, mean, b, 1)
    masks = []
    for step in (4, 5):
        Y = k.gat_tail_forward(Xt, K, d, mean, Bt, 1, row_ids=idt, seed=SEED, step=state.step, layer=LAYER, thr=thr)
        Yn = Y.cpu().numpy()
        keep = D.keep_mask(SEED, step, LAYER, ids, fout, thr).numpy()
        want, exact = W.tail32(x, K, d, mean, b, 1, keep, scale)
        dropped = float((~keep).mean())
        zero_ok = np.array_equal(Yn == 0, ~keep | (a0 == 0))
        exact_ok = np.array_equal(_bits(Yn[exact]), _bits(want[exact]))
        u = float(W.ulps(Yn, want).max())
        dX, db = k.gat_tail_backward(Gt, Y, K, d, mean, 1, row_ids=idt, seed=SEED, step=state.step, layer=LAYER, thr=thr)
        dx32, gm32 = W.tail_backward32(G, Yn, K, d, mean, 1, keep, scale)
        dXn = dX.cpu().numpy()
        back_ok = np.array_equal(_bits(dXn), _bits(dx32))
        back_zero_ok = np.array_equal(dXn == 0, np.tile(~keep, (1, K) if mean else (1, 1)) | (dx32 == 0)) and \
            not dXn[np.tile(~keep, (1, K) if mean else (1, 1))].any()
        err, bound = W.dbias_error_and_bound(db.cpu().numpy(), gm32)
        print("heads %d d %d mean %s step %d: dropped %.4f; zeros exactly where dropped or a == 0: %s; kept elements off the expm1 branch "
              "bit-equal: %s; ELU * scale at most %.3g ulp (bound 4); dX bit-equal: %s; dX zero exactly on the dropped: %s"
              % (K, d, mean, step, dropped, zero_ok, exact_ok, u, back_ok, back_zero_ok))
        assert zero_ok and exact_ok and u <= 4 and back_ok and back_zero_ok and 0.45 < dropped < 0.55 and (err <= bound).all()
        masks.append(keep)
        state.advance()
    assert not np.array_equal(masks[0], masks[1])                             # the device-resident step draws a new mask
    Y0 = k.gat_tail_forward(Xt, K, d, mean, Bt, 1, row_ids=idt, seed=SEED, step=state.step, layer=LAYER, thr=0)
    Yp = k.gat_tail_forward(Xt, K, d, mean, Bt, 1)
    assert torch.equal(Y0, Yp)                                                # thr 0: the path without dropout, bit for bit
    b0 = k.gat_tail_backward(Gt, Y0, K, d, mean, 1, row_ids=idt, seed=SEED, step=state.step, layer=LAYER, thr=0)
    bp = k.gat_tail_backward(Gt, Yp, K, d, mean, 1)
    assert torch.equal(b0[0], bp[0]) and torch.equal(b0[1], bp[1])


def _windows(n, widths, lds, dev):
    """(buffer, window) pairs: (n + 2) x ld buffers of NaN whose rows 1 .. n, columns 0 .. width - 1 are the window."""
    bufs = [torch.full((n + 2, ld), float("nan"), device=dev) for ld in lds]
    return bufs, [b[1:n + 1, :w] for b, w in zip(bufs, widths)]


def _outside_untouched(buf, n, w):
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[1:n + 1, :w] = False
    return bool(torch.isnan(buf[outside]).all()) and not bool(torch.isnan(buf[1:n + 1, :w]).any())


@pytest.mark.parametrize("K,d,mean,pad", [(2, 50, False, 4), (2, 50, True, 2), (4, 32, True, 8), (3, 1, False, 2)])
def test_leading_dimensions_canary_rows_and_in_place(env, K, d, mean, pad):
    k, dev, B, _ = env
    n = B + 65
    fin, fout = K * d, d if mean else K * d
    x, b, G = _inputs(n, K, d, mean, 9 * d + K)
    Xt, Bt, Gt = (_t(a, dev) for a in (x, b, G))
    Y = k.gat_tail_forward(Xt, K, d, mean, Bt, 1)
    dX, db = k.gat_tail_backward(Gt, Y, K, d, mean, 1)
    bufs, (Xw, Gw, Yw, dXw) = _windows(n, (fin, fout, fout, fin), (fin + pad, fout + pad, fout + pad, fin + pad), dev)
    Xw.copy_(Xt)
    Gw.copy_(Gt)
    before = [v.clone() for v in bufs]
    assert k.gat_tail_forward(Xw, K, d, mean, Bt, 1, out=Yw) is Yw
    dX_w, db_w = k.gat_tail_backward(Gw, Yw, K, d, mean, 1, out=dXw)
    same = [torch.equal(a, c) for a, c in ((Yw, Y), (dX_w, dX), (db_w, db))]
    print("heads %d d %d mean %s ld + %d: outputs equal to the contiguous run bit for bit: %s" % (K, d, mean, pad, same))
    assert dX_w is dXw and all(same)
    for v, was in zip(bufs[:2], before[:2]):
        assert torch.equal(v.view(torch.int32), was.view(torch.int32))            # no input changed
    assert _outside_untouched(bufs[2], n, fout) and _outside_untouched(bufs[3], n, fin)      # nothing outside the windows
    if not mean:                                                                  # in place: the bits of the out-of-place run
        assert k.gat_tail_forward(Xw, K, d, mean, Bt, 1, out=Xw) is Xw
        assert torch.equal(Xw, Y) and _outside_untouched(bufs[0], n, fin)
        Xc = Xt.clone()
        assert torch.equal(k.gat_tail_forward(Xc, K, d, mean, Bt, 1, out=Xc), Y)
        Gc = Gt.clone()
        assert torch.equal(k.gat_tail_backward(Gc, Y, K, d, mean, 1, out=Gc)[0], dX)


@pytest.mark.parametrize("K,d,mean", [(4, 32, False), (4, 32, True)])
def test_a_misaligned_base_gives_the_bits_of_the_aligned_run(env, K, d, mean):
    k, dev, B, _ = env
    D = pkg("dropout")
    n = B + 65
    x, b, G = _inputs(n, K, d, mean, 31)
    Xt, Bt, Gt = (_t(a, dev) for a in (x, b, G))
    thr, _ = D.threshold(0.5)
    state = D.DropoutState(SEED, dev)
    kw = dict(seed=SEED, step=state.step, layer=LAYER, thr=thr)
    Y = k.gat_tail_forward(Xt, K, d, mean, Bt, 1, **kw)
    dX, db = k.gat_tail_backward(Gt, Y, K, d, mean, 1, **kw)

    def shifted(t):
        s = torch.empty(t.numel() + 1, device=dev)[1:].view(t.shape)
        s.copy_(t)
        assert s.data_ptr() % 16 == 4
        return s

    Ys, dXs = shifted(torch.zeros_like(Y)), shifted(torch.zeros_like(dX))
    k.gat_tail_forward(shifted(Xt), K, d, mean, Bt, 1, out=Ys, **kw)
    dX_s, db_s = k.gat_tail_backward(shifted(Gt), Ys, K, d, mean, 1, out=dXs, **kw)
    same = [torch.equal(a, c) for a, c in ((Ys, Y), (dX_s, dX), (db_s, db))]
    print("mean %s: element-wise path against the float4 path, bit for bit: %s" % (mean, same))
    assert all(same)


def test_a_nan_and_an_inf_stay_in_their_own_elements(env):
    k, dev, B, _ = env
    n, K, d = 300, 4, 8
    x, b, G = _inputs(n, K, d, True, 17)
    Xt, Bt, Gt = (_t(a, dev) for a in (x, b, G))
    Y = k.gat_tail_forward(Xt, K, d, True, Bt, 1)
    Xp = Xt.clone()
    Xp[5, 2 * d + 3], Xp[7, 1] = float("nan"), float("inf")                   # head 2 of output (5, 3); head 0 of output (7, 1)
    Yp = k.gat_tail_forward(Xp, K, d, True, Bt, 1)
    clean = torch.ones_like(Y, dtype=torch.bool)
    clean[5, 3] = clean[7, 1] = False
    ok = torch.equal(Yp[clean], Y[clean])
    print("forward: every other element keeps its bits: %s; Y[5, 3], Y[7, 1] = %r, %r" % (ok, float(Yp[5, 3]), float(Yp[7, 1])))
    assert ok and bool(torch.isnan(Yp[5, 3])) and bool(torch.isinf(Yp[7, 1]))
    dX, db = k.gat_tail_backward(Gt, Y, K, d, True, 1)
    Gp = Gt.clone()
    Gp[11, 3], Gp[290, 6] = float("nan"), float("inf")
    dXp, dbp = k.gat_tail_backward(Gp, Y, K, d, True, 1)
    cols = torch.ones(d, dtype=torch.bool, device=dev)
    cols[[3, 6]] = False
    cleanx = torch.ones_like(dX, dtype=torch.bool)
    for h in range(K):
        cleanx[11, h * d + 3] = cleanx[290, h * d + 6] = False
    ok = torch.equal(dbp[cols], db[cols]) and torch.equal(dXp[cleanx], dX[cleanx])
    print("backward: the other elements and columns keep their bits: %s; dbias[3], dbias[6] = %r, %r" % (ok, float(dbp[3]), float(dbp[6])))
    assert ok and bool(torch.isnan(dbp[3])) and bool(torch.isinf(dbp[6])) and bool(torch.isnan(dXp[~cleanx][:K]).all()) and \
        bool(torch.isinf(dXp[~cleanx][K:]).all())


def test_two_runs_give_the_same_bits(env):
    k, dev, B, _ = env
    D = pkg("dropout")
    n, K, d = 2 * B + 1, 4, 33
    x, b, G = _inputs(n, K, d, True, 23)
    Xt, Bt, Gt = (_t(a, dev) for a in (x, b, G))
    thr, _ = D.threshold(0.5)
    state = D.DropoutState(SEED, dev)
    kw = dict(seed=SEED, step=state.step, layer=LAYER, thr=thr)
    runs = []
    for _ in range(2):
        Y = k.gat_tail_forward(Xt, K, d, True, Bt, 1, **kw)
        runs.append((Y,) + k.gat_tail_backward(Gt, Y, K, d, True, 1, **kw))
    same = [torch.equal(a, c) for a, c in zip(*runs)]
    print("two runs, every output bit for bit:", same)
    assert all(same)


def test_refusals_write_nothing(env):
    k, dev, B, _ = env
    _lib = pkg("_lib")
    L = _lib.lib()
    n, ld = 8, 9220
    wide = torch.full((n + 2, ld), float("nan"), device=dev)
    out = torch.full((n + 2, ld), float("nan"), device=dev)
    db = torch.full((1028,), float("nan"), device=dev)
    ws = torch.full((1028,), float("nan"), device=dev, dtype=torch.float64)
    aux = torch.zeros(n + 2, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    X, Y = wide[1].data_ptr(), out[1].data_ptr()

    def fwd(heads=2, d=50, mean=0, x=X, y=Y, ldx=ld, ldy=ld, rows=n, step=None, ids=None, act=1):
        return L.pgcn_gat_tail_forward_f32(x, ldx, rows, heads, d, mean, None, act, ids, 0, step, 0, 0, y, ldy, s)

    def bwd(heads=2, d=50, mean=0, g=X, y=X, dx=Y, ldg=ld, lddx=ld, rows=n, step=None, ids=None, w=ws.data_ptr(), ws_bytes=1 << 13, act=1):
        return L.pgcn_gat_tail_backward_f32(g, ldg, y, ld, rows, heads, d, mean, act, ids, 0, step, 0, 0, dx, lddx, db.data_ptr(), w, ws_bytes, s)

    einval = {
        "forward X null": fwd(x=None), "forward Y null": fwd(y=None), "forward nrows < 0": fwd(rows=-1), "forward heads 0": fwd(heads=0),
        "forward d 0": fwd(d=0), "forward act 2": fwd(act=2), "forward ldx < heads d": fwd(ldx=99), "forward ldy < fout": fwd(ldy=99),
        "forward ldy < d (mean)": fwd(mean=1, ldy=49), "forward step misaligned": fwd(step=aux.data_ptr() + 4),
        "forward row_ids misaligned": fwd(ids=aux.data_ptr() + 4), "forward in place with mean": fwd(mean=1, y=X),
        "forward in place, other ld": fwd(y=X, ldy=ld - 4),
        "backward G null": bwd(g=None), "backward Y null with ELU": bwd(y=None), "backward nrows < 0": bwd(rows=-1),
        "backward ldg < fout": bwd(ldg=99), "backward lddx < heads d": bwd(lddx=99), "backward lddx < heads d (mean)": bwd(mean=1, lddx=99),
        "backward ws null": bwd(w=None), "backward ws misaligned": bwd(w=ws.data_ptr() + 4),
        "backward step misaligned": bwd(step=aux.data_ptr() + 4), "backward row_ids misaligned": bwd(ids=aux.data_ptr() + 4),
        "backward in place with mean": bwd(mean=1, dx=X),
    }
    unsupported = {"forward fout 1028": fwd(heads=1, d=1028), "forward heads d 9216 (mean)": fwd(heads=9, d=1024, mean=1),
                   "backward fout 1028": bwd(heads=1, d=1028), "backward heads d 9216 (mean)": bwd(heads=9, d=1024, mean=1)}
    nomem = {"backward short ws": bwd(ws_bytes=100 * 8 - 1)}
    torch.cuda.synchronize()
    print("PGCN_EINVAL:", einval)
    print("PGCN_EUNSUPPORTED:", unsupported)
    print("PGCN_ENOMEM:", nomem)
    assert all(v == EINVAL for v in einval.values()) and all(v == _lib.PGCN_EUNSUPPORTED for v in unsupported.values())
    assert all(v == ENOMEM for v in nomem.values())
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(db).all()) and bool(torch.isnan(ws).all()) and bool(torch.isnan(wide).all())
    assert L.pgcn_gat_tail_ws_bytes(n, 1028) == -1 and L.pgcn_gat_tail_ws_bytes(513, 100) == 2 * 100 * 8
    assert k.gat_tail_forward(wide[1:n + 1, :1028], 1, 1028, False, None, 1) is None          # the binding answers None above 1024 columns


def test_a_captured_forward_and_backward_replay_like_eager(env):
    """Forward and backward of the node captured on one stream and replayed twice: every output equals the eager steps bit for bit --
    so the masks advanced with the device-resident step at every replay."""
    k, dev, B, M = env
    D = pkg("dropout")
    n, K, d = B + 65, 4, 8
    x, b, G = _inputs(n, K, d, True, 41)
    Gt = _t(G, dev)
    ids = (torch.arange(n, dtype=torch.int64) * 3 + 1).to(dev)
    thr, scale = D.threshold(0.5)
    old = M._kernel_provider
    M._kernel_provider = k
    try:
        def make():
            return _t(x, dev).requires_grad_(True), _t(b, dev).requires_grad_(True), D.DropoutState(SEED, dev)

        def step(a, bias, state):
            Y = M._GatTail.apply(a, bias, K, d, True, 1, ids, state, LAYER, thr, scale)
            grads = torch.autograd.grad((Y * Gt).sum(), (a, bias))
            state.advance()
            return (Y.detach(),) + grads

        a, bias, state = make()
        eager = [tuple(t.clone() for t in step(a, bias, state)) for _ in range(2)]
        assert not torch.equal(eager[0][0] == 0, eager[1][0] == 0)
        keep = D.keep_mask(SEED, 0, LAYER, ids.cpu(), d, thr).to(dev)
        assert not bool(eager[0][0][~keep].any())

        a, bias, state = make()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(a, bias, state)                                              # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        state.step.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step(a, bias, state)
        for i in range(2):
            graph.replay()
            torch.cuda.synchronize()
            same = [torch.equal(u, v) for u, v in zip(outs, eager[i])]
            print("replay %d against eager step %d (Y, dX, dbias):" % (i, i), same)
            assert all(same)
        assert int(state.step.item()) == 2
    finally:
        M._kernel_provider = old


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------

EPOCHS, LR = 3, 0.01


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return W.make_datasets(str(tmp_path_factory.mktemp("gat_tail_gpu")))


_refs = {}


def _reference(data, opts):
    key = W.tag(opts)
    if key not in _refs:
        _refs[key] = W.reference(data, opts, 0, EPOCHS, LR)
    return _refs[key]


@pytest.mark.parametrize("hidden,Ko,P", [(32, 1, 1), (32, 2, 1), (32, 1, 2), (32, 2, 2), (256, 1, 1)])
def test_data_run_on_the_device_against_the_float64_model(datasets, hidden, Ko, P):
    """PGAT.run on the planted problem: 2 layers, 4 heads, dropout 0.5, bias, 3 epochs of Adam; hidden 256 = 4 x 64 is the recomputing
    kernels' shape.  P = 2: two processes on the one device."""
    paths, data = datasets
    opts = W.options(K=4, hidden=hidden, Ko=Ko, bias=True, elu=True, dropout=W.DROPOUT)
    ref = _reference(data["single"], opts)
    params = {k: v.numpy() for k, v in ref["params"].items()}
    res = W.spawn(W.run_worker, P, paths, True, opts=opts, params=params, epochs=EPOCHS, lr=LR)
    n = W.GW.N
    r0 = res[0]
    print("hidden %d Ko %d on %d ranks: provider %s, two-pass route per layer %s" % (hidden, Ko, P, r0["hip"], r0["fused"]))
    assert r0["hip"] == "HipKernels" and r0["widths"] == [W.GW.FIN, hidden, W.GW.CLASSES] and len(r0["history"]) == EPOCHS
    assert r0["fused"][0] == (hidden == 256)
    where = "gat_tail-gpu/h%dKo%d/P%d" % (hidden, Ko, P)
    held = W.hold_steps(where, res, ref, n, EPOCHS)
    held_to_fixture(where, "eval logits", W.rows(res, lambda r: r["eval_logits"], n), ref["twin"]["eval"][-1].numpy(),
                    ref["m64"]["eval"][-1].numpy())
    for e, h in enumerate(r0["history"]):
        a64, a32 = W.accuracy(ref["m64"]["eval"][e], data["single"]), W.accuracy(ref["twin"]["eval"][e], data["single"])
        held_to_fixture("%s/epoch%d" % (where, e), "losses", np.array([h["losses"][s] for s in W.SETS]),
                        np.array([a32[s][0] for s in W.SETS]), np.array([a64[s][0] for s in W.SETS]))
    print("%s: %d tensors held; reported losses %s" % (where, held + 1 + EPOCHS, [round(h["loss"], 4) for h in r0["history"]]))
